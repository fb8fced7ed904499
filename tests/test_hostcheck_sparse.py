"""The sparse TL and reverse sweeps (tl_column / ad_reverse_column with C2F_SPARSE: what cloudsc2_tl_launch_sparse and
cloudsc2_vjp_launch_sparse run) compiled for the HOST against their dense twins given zero planes for what is absent: every present
plane has the twin's bits, every active element of it is written, the padded tail is left alone, and what is read is unchanged.
Absent planes are NULL pointers: a missing guard in the column functions is a segmentation fault here, on the CPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.sparse_patterns import in_names, patterns
from tests.util import B, c2, flat_block, flat_fields, host_qsat, host_traj_blocks, increments_of, make_params, same_bits


def check_written(got: dict, want: dict, nb: int, nproma: int, ngptot: int, what) -> None:
    """every present written plane: the dense bits on the active columns, NaN (untouched) in the padded tail"""
    for n, g in got.items():
        for ibl in range(nb):
            icend = min(nproma, ngptot - ibl * nproma)
            act = g[ibl][:, :icend]
            assert not np.any(np.isnan(act)), (what, n, "an active element was not written")
            assert same_bits(act, want[n][ibl][:, :icend]), (what, n, "differs from the dense twin")
            assert np.all(np.isnan(g[ibl][:, icend:])), (what, n, "the padded tail was touched")


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True), dict(ldrain1d=True), dict(lregcl=True)])
def test_sparse_sweeps_have_the_dense_bits(precise, flags, satur):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)  # nonzero PSUPSAT
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, nproma, ngptot)
    nb = st.nblocks
    qsat = None if satur else host_qsat(st)
    ins = in_names(satur)
    lib = host_lib("sparse")
    geom = (C.byref(prm), st.ptsphy, nproma, nlev, ngptot)

    # the trajectory: complete in every launch (PFPLSL5 / PFPLSN5 and the cover checkpoints from the trajectory pass)
    traj = st.copy()
    i, o = host_traj_blocks(traj, qsat)
    scratch = np.zeros((nb, nlev, nproma), dtype=B.REAL)
    assert lib.hostcheck_sparse_forward(*geom, C.byref(i), C.byref(o), scratch.ctypes.data) == 0

    inc = increments_of(st, host_qsat(st))  # v = 0.01 x
    dx = {n: inc[n] for n in ins}

    def tl(sparse: int, present_in, present_out, fill):
        dy = {n: a for n, a in flat_fields("out", nb, nlev, nproma, fill=fill).items() if n in present_out}
        din = {n: dx[n].copy() for n in present_in}
        assert lib.hostcheck_sparse_tl(*geom, int(satur), sparse, C.byref(i), C.byref(flat_block("in", din)), C.byref(flat_block("out", dy))) == 0
        for n in din:
            assert same_bits(din[n], dx[n]), ("TL changed a tangent", n)
        return dy

    zero_in = {n: np.zeros_like(dx[n]) for n in ins}
    for name, pin, pout in patterns(satur, tl=True):
        # the dense twin on zero planes for the absent tangents (its inputs are the given ones and zeros)
        saved = {n: dx[n] for n in ins}
        for n in ins:
            if n not in pin:
                dx[n] = zero_in[n]
        want = tl(0, ins, B.OUT_NAMES, np.nan)
        got = tl(1, pin, pout, np.nan)
        dx.update(saved)
        assert set(got) == set(pout)
        check_written(got, want, nb, nproma, ngptot, ("TL", name))

    # cotangents: u = TL v of the full tangent
    u = tl(0, ins, B.OUT_NAMES, 0.0)

    def vjp(sparse: int, present_in, y: dict):
        xa = {n: a for n, a in flat_fields("in", nb, nlev, nproma, fill=np.nan).items() if n in present_in}
        yc = {n: a.copy() for n, a in y.items()}
        assert lib.hostcheck_sparse_vjp(*geom, int(satur), sparse, C.byref(i), C.byref(o), C.byref(flat_block("in", xa)),
                                        C.byref(flat_block("out", yc)), scratch.ctypes.data) == 0
        for n in yc:
            assert same_bits(yc[n], y[n]), ("the reverse sweep changed a cotangent", n)
        return xa

    for name, pin, pout in patterns(satur):
        want = vjp(0, ins, {n: (u[n] if n in pout else np.zeros_like(u[n])) for n in B.OUT_NAMES})
        got = vjp(1, pin, {n: u[n] for n in pout})
        assert set(got) == set(pin)
        check_written(got, want, nb, nproma, ngptot, ("VJP", name))
