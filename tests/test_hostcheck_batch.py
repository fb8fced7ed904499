"""The batched TL and reverse sweeps (tl_batch_column, vjp_batch_column: what cloudsc2_tl_launch_batch / cloudsc2_vjp_launch_batch
run) compiled for the HOST against K runs of their single-direction twins (tl_column, ad_reverse_column<F | C2F_ASSIGN | C2F_VJP>):
every direction's results bit for bit, the output adjoints left as they were, the padded tail untouched, every active element
written."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.util import (FLAGS, B, block_array, c2, flat_block, flat_fields, host_qsat, host_traj_blocks, hostcheck, increments_of,
                        make_params, same_bits, tail_checks)


def test_batch_max_of_the_host_build_is_the_librarys():
    assert host_lib("batch").hostcheck_batch_max() == B.lib.cloudsc2_batch_max()


@pytest.mark.parametrize("flags", FLAGS)
def test_batched_columns_equal_single_direction_columns(precise, flags):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, nproma, ngptot)
    nb = st.nblocks
    qsat = host_qsat(st)
    inc = increments_of(st, qsat)
    hc, hv, hb = hostcheck(), host_lib("vjp"), host_lib("batch")
    kmax = hb.hostcheck_batch_max()
    assert 2 <= kmax <= 8

    # kmax distinct seeded tangents: the drivers' 0.01 x scaled point by point, another draw per direction
    rng = np.random.default_rng(2024)
    tangents = [{n: np.ascontiguousarray(a * rng.uniform(-1.5, 1.5, a.shape).astype(B.REAL)) for n, a in inc.items()} for _ in range(kmax)]

    # K single TL sweeps (they also write the trajectory outputs, PFPLSL5 / PFPLSN5 among them)
    traj = st.copy()
    i, o = host_traj_blocks(traj, qsat)
    tl_single = []
    for v in tangents:
        dy = flat_fields("out", nb, nlev, nproma, fill=np.nan)
        assert hc.hostcheck_tl(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o), C.byref(flat_block("in", v)),
                               C.byref(flat_block("out", dy))) == 0
        tl_single.append(dy)
    # the cover checkpoints of the trajectory pass; read with the evaporation branch only
    scratch = np.zeros((nb, nlev, nproma), dtype=B.REAL)
    fwd = st.copy()
    fi, fo = host_traj_blocks(fwd, qsat)
    assert hv.hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(fi), C.byref(fo), None, None,
                                  scratch.ctypes.data, 1, 0) == 0
    # K single reverse sweeps in the vector-Jacobian form; the cotangents are the TL results (zero in the padded tail)
    cotangents = [{n: np.nan_to_num(a, nan=0.0) for n, a in dy.items()} for dy in tl_single]
    vjp_single = []
    for u in cotangents:
        xa = flat_fields("in", nb, nlev, nproma, fill=np.nan)
        y = {n: a.copy() for n, a in u.items()}
        assert hv.hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o), C.byref(flat_block("in", xa)),
                                      C.byref(flat_block("out", y)), scratch.ctypes.data, 2, 1) == 0
        vjp_single.append(xa)

    for K in sorted({1, min(3, kmax), kmax}):
        dys = [flat_fields("out", nb, nlev, nproma, fill=np.nan) for _ in range(K)]
        assert hb.hostcheck_tl_batch(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), K, block_array("in", tangents[:K]),
                                     block_array("out", dys)) == 0
        for k in range(K):
            tail_checks(dys[k], nproma, ngptot, f"TL batch K={K} direction {k}")
            for n in dys[k]:
                assert same_bits(dys[k][n], tl_single[k][n]), ("batched TL != single TL", K, k, n)

        xas = [flat_fields("in", nb, nlev, nproma, fill=np.nan) for _ in range(K)]
        ys = [{n: a.copy() for n, a in u.items()} for u in cotangents[:K]]
        assert hb.hostcheck_vjp_batch(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o), K, block_array("in", xas),
                                      block_array("out", ys), scratch.ctypes.data) == 0
        for k in range(K):
            tail_checks(xas[k], nproma, ngptot, f"VJP batch K={K} direction {k}")
            for n in ys[k]:
                assert same_bits(ys[k][n], cotangents[k][n]), ("batched VJP changed an output adjoint", K, k, n)
            for n in xas[k]:
                assert same_bits(xas[k][n], vjp_single[k][n]), ("batched VJP != single VJP", K, k, n)
