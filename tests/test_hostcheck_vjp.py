"""The vector-Jacobian form of the adjoint's reverse sweep (ad_reverse_column<F | C2F_ASSIGN | C2F_VJP>, what cloudsc2_vjp_launch
runs) compiled for the HOST against the assign form (<F | C2F_ASSIGN>, cloudsc2_ad_launch_reverse with assign = 1): the same input
adjoints except PSUPSAT, which is the true derivative, the output adjoints left as they were, and the dot-product identity
<TL v, u> = <v, VJP u> with a nonzero PSUPSAT tangent -- which the assign form (CLOUDSC2AD's PSUPSAT = PTSPHY*zqp1) fails."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.util import B, c2, flat_block, flat_fields, host_qsat, host_traj_blocks, hostcheck, increments_of, make_params


@pytest.mark.skipif(B.SINGLE, reason="the 1e-12 identity is an fp64 statement")
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True), dict(ldrain1d=True), dict(lregcl=True)])
def test_vjp_sweep_against_assign_form(precise, flags):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)  # nonzero PSUPSAT
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, nproma, ngptot)
    nb = st.nblocks
    qsat = host_qsat(st)
    inc = increments_of(st, qsat)  # v = 0.01 x, PSUPSAT's included (nonzero)
    assert np.any(inc["supsat"] != 0.0)
    hc, hv = hostcheck(), host_lib("vjp")

    # u = TL v (and the trajectory outputs, PFPLSL5 / PFPLSN5 among them, written by the same sweep)
    got = st.copy()
    i, o = host_traj_blocks(got, qsat)
    tl = flat_fields("out", nb, nlev, nproma)
    assert hc.hostcheck_tl(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o), C.byref(flat_block("in", inc)),
                           C.byref(flat_block("out", tl))) == 0
    # the cover checkpoints of the trajectory pass (cloudsc2_ad_launch_forward); read with the evaporation branch only
    scratch = np.zeros((nb, nlev, nproma))
    fwd = st.copy()
    fi, fo = host_traj_blocks(fwd, qsat)
    assert hv.hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(fi), C.byref(fo), None, None,
                                  scratch.ctypes.data, 1, 0) == 0
    assert np.array_equal(fwd.PFPLSL, got.PFPLSL) and np.array_equal(fwd.PFPLSN, got.PFPLSN)

    def reverse(vjp: int, fill: float):
        x = flat_fields("in", nb, nlev, nproma, fill=fill)
        y = {n: a.copy() for n, a in tl.items()}
        assert hv.hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o),
                                      C.byref(flat_block("in", x)), C.byref(flat_block("out", y)), scratch.ctypes.data, 2, vjp) == 0
        return x, y

    xa, ya = reverse(0, 7.25)
    xv, yv = reverse(1, np.nan)

    for n in tl:  # the assign form consumes the output adjoints, the VJP leaves them as they were
        assert np.array_equal(yv[n], tl[n]), ("VJP: output adjoint changed", n)
    for ibl in range(nb):
        icend = min(nproma, ngptot - ibl * nproma)
        for n in xv:
            a, v = xa[n][ibl][:, :icend], xv[n][ibl][:, :icend]
            assert not np.any(np.isnan(v)), ("VJP: active element not written", n)
            assert np.all(np.isnan(xv[n][ibl][:, icend:])), ("VJP touched the padded tail", n)
            if n == "supsat":
                assert np.array_equal(st.ptsphy * v, a), "fl(PTSPHY * VJP supsat) != CLOUDSC2AD's PSUPSAT"
            else:
                assert np.array_equal(a.view(np.int64), v.view(np.int64)), ("VJP != assign form", n)

    # <TL v, u> = <v, VJP u> over the active columns, u = TL v; CLOUDSC2AD's own PSUPSAT adjoint breaks it
    act = np.zeros((nb, 1, nproma), dtype=bool)
    for ibl in range(nb):
        act[ibl, 0, : min(nproma, ngptot - ibl * nproma)] = True
    lhs = sum(float(np.sum(np.where(act, tl[n], 0.0) ** 2)) for n in tl)
    rhs_v = sum(float(np.sum(np.where(act, inc[n] * xv[n], 0.0))) for n in inc)
    rhs_a = sum(float(np.sum(np.where(act, inc[n] * xa[n], 0.0))) for n in inc)
    assert abs(lhs - rhs_v) / abs(lhs) <= 1e-12, (lhs, rhs_v)
    assert abs(lhs - rhs_a) / abs(lhs) > 1e-9, "the assign form's PSUPSAT term should break the identity"
