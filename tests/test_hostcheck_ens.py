"""What the ensemble launchers (cloudsc2_nl_launch_ens, cloudsc2_tl_launch_ens, cloudsc2_vjp_launch_ens) run besides the column sweeps,
compiled for the HOST in both precisions: the derivation of a member's constants from its row of the parameter table must give the
BYTES the host's make_consts + make_parlin give for a parameter block holding that row (the promise that a member is the bits of the
single-parameter-set call rests on it), a member's argument block is the template with every pointer advanced by member x its stride,
and the workgroup -> (member, column) mapping visits every column of every member once without a wave of 64 spanning two members.
No tolerance anywhere: bytes and counts."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.hostbuild import host_lib
from tests.util import PARAM_NAMES, c2, make_params

KBLOCK = 128  # kBlock of cloudsc2_sweep_kernels.hpp
# the shapes of the GPU test: (a) 72 padded columns, less than one workgroup; (b) 256, two workgroups per member
SHAPES = {"a": (24, 70), "b": (64, 200)}


@pytest.fixture(params=["fp64", "fp32"])
def lib(request):
    single = request.param == "fp32"
    lib = host_lib("ens", single)
    assert lib.hostcheck_ens_real_bytes() == (4 if single else 8)
    return lib


def dvec(values):
    return (C.c_double * 4)(*[float(v) for v in values])


def rows_of(prm) -> list:
    """parameter rows: prm's own, hand-picked values whose reciprocals and hundredths are inexact, and random ones around prm's"""
    own = [getattr(prm, n) for n in PARAM_NAMES]
    rows = [own,
            [1.7e-4, 3.0e-4, 266.0 + 1.0 / 3.0, 5.44e-4 / 3.0],
            [own[0] * (1.0 + 2.0 ** -52), own[1] * (1.0 - 2.0 ** -53), own[2] + 1e-9, own[3] * 3.0],
            [1.0 / 7000.0, 1.0 / 3333.0, 250.7, 1.0 / 1837.0]]
    rng = np.random.default_rng(7)
    rows += [[v * f for v, f in zip(own, rng.uniform(0.5, 1.5, 4))] for _ in range(8)]
    return rows


FLAGS = [dict(lregcl=r, **e) for r in (False, True) for e in (dict(), dict(levapls2=True), dict(ldrain1d=True))]


@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: "-".join(k for k, v in f.items() if v) or "plain")
def test_constants_derived_from_a_parameter_row_are_the_hosts_bytes(lib, flags):
    prm = make_params(c2.synthetic_table(), **flags)
    for ptsphy in (3600.0, 1234.5):
        for row in rows_of(prm):
            tangents = [0.01 * v / 3.0 for v in row]
            assert lib.hostcheck_ens_consts(C.byref(prm), ptsphy, dvec(row), dvec(tangents)) == 0, (flags, ptsphy, row, "tangents given")
            assert lib.hostcheck_ens_consts(C.byref(prm), ptsphy, dvec(row), None) == 0, (flags, ptsphy, row, "tangents NULL")


@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True)], ids=["plain", "evap-regcl"])
def test_a_members_argument_block_is_the_template_advanced(lib, flags):
    prm = make_params(c2.synthetic_table(), **flags)
    for shape, (nproma, ngptot) in SHAPES.items():
        ncols_pad = -(-ngptot // nproma) * nproma
        for row in rows_of(prm)[:4]:
            for member in (0, 1, 2, 40000):
                rc = lib.hostcheck_ens_member_args(C.byref(prm), 3600.0, dvec(row), dvec([1.0, 2.0, 3.0, 4.0]), member, ncols_pad)
                assert rc == 0, (flags, shape, row, member, "check", rc)


@pytest.mark.parametrize("members", [1, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_column_of_every_member_is_visited_once_and_no_wave_spans_two_members(lib, shape, members):
    nproma, ngptot = SHAPES[shape]
    ncols_pad = -(-ngptot // nproma) * nproma
    wgs = -(-ncols_pad // KBLOCK)
    n = members * wgs * KBLOCK
    member, column = np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.full(n, -1, dtype=np.int64)
    lib.hostcheck_ens_locate(members, wgs, KBLOCK, member.ctypes.data, column.ctypes.data)
    assert np.all(member < members) and np.all(column >= 0)
    live = column < ncols_pad  # (the others find no column and leave: lane_setup)
    visits = np.zeros((members, ncols_pad), dtype=np.int64)
    np.add.at(visits, (member[live], column[live]), 1)
    assert np.all(visits == 1), (shape, members, "columns not visited exactly once", np.argwhere(visits != 1)[:5])
    waves = member.reshape(-1, 64)
    assert np.all(waves == waves[:, :1]), "a wave holds two members"
    # consecutive lanes, consecutive columns (coalescing), and a workgroup starts at a multiple of the block
    cols = column.reshape(-1, KBLOCK)
    assert np.all(np.diff(cols, axis=1) == 1) and np.all(cols[:, 0] % KBLOCK == 0)
    if shape == "b":
        assert wgs == 2 and int(live.reshape(-1, KBLOCK)[1].sum()) == KBLOCK  # 256 padded columns: both workgroups have columns (the second's last 56 are the padded tail)
    else:
        assert wgs == 1 and int(live.reshape(-1, KBLOCK)[0].sum()) == 72  # a partly idle workgroup
