"""SATUR differentiated (satur_lin_point) and the sweeps that carry its derivative inside (C2F_SATLIN: what cloudsc2_tl_launch_satur
and cloudsc2_vjp_launch_satur run), compiled for the HOST.  The reference ships no SATURTL / SATURAD, so the new derivative code is
tied to the reference by three routes: central differences of the reference's SATUR, the reference's CLOUDSC2TL fed the composed
qsat tangent, and a Taylor test of the composite function pap, t -> SATUR -> CLOUDSC2 run by the reference alone.

Tolerances: 1e-12 (host dot-product identity) and 1e-11 of a field's maximum over the active columns are the project's own numbers
for TL / AD statements; 1e-8 for the partials against central differences of relative step 1e-6 (the differences themselves reach
5.2e-10 / 2.8e-10 against an analytic restatement); 5e-6 for the composite Taylor test (the reference-composed TL reaches 4.6e-7,
a 1e-3 relative error in dqs/dt gives 1.2e-4)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.host_sweeps import field_err, increments15, run_tl_satur, run_vjp_satur, trajectory_for_reverse
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.satur_lin_ref import satur_numpy, satur_partials_numpy
from tests.util import (FLAG_SETS, B, bits, blocks_of, c2, flat_block, flat_fields, fp64_only, hfld, host_qsat, host_traj_blocks,
                        hostcheck, increments_of, make_params, refcall, set_lib_params, the_tables)

SAT_NAMES = tuple(n for n in B.IN_NAMES if n != "qsat")
TLAD_TOL = 1e-11


@pytest.fixture(scope="module")
def ref():
    """the reference itself where it is built, else its C restatement"""
    return refcall.RefLib() if refcall.have_ref() else refcall.OracleLib()


def one_block(a2d: np.ndarray) -> np.ndarray:
    """(nlev, ncol) table plane -> (1, nlev, ncol): the table as one NPROMA block"""
    return np.ascontiguousarray(a2d[None], dtype=B.REAL)


def hc_satur_lin(prm, pap: np.ndarray, t: np.ndarray, want_qsat: bool = True):
    nb, nlev, nproma = pap.shape
    q, dp, dt = (np.full_like(pap, np.nan) for _ in range(3))
    assert host_lib("satur_lin").hostcheck_satur_lin(C.byref(prm), nproma, nlev, nb * nproma, hfld(pap), hfld(t),
                                                     hfld(q) if want_qsat else B.Field(), hfld(dp), hfld(dt)) == 0
    return q, dp, dt


def hc_satur(prm, pap: np.ndarray, t: np.ndarray) -> np.ndarray:
    nb, nlev, nproma = pap.shape
    q = np.full_like(pap, np.nan)
    assert hostcheck().hostcheck_satur(C.byref(prm), nproma, nlev, nb * nproma, hfld(pap), hfld(t), hfld(q)) == 0
    return q


@pytest.mark.parametrize("which", [0, 1])
def test_qsat_of_satur_lin_has_the_bits_of_satur(precise, which):
    name, tab = the_tables()[which]
    prm = make_params(tab)
    pap, t = one_block(tab["PAP"]), one_block(tab["PT"])
    q, dp, dt = hc_satur_lin(prm, pap, t)
    assert np.array_equal(bits(q), bits(hc_satur(prm, pap, t))), name
    _, dp2, dt2 = hc_satur_lin(prm, pap, t, want_qsat=False)  # partials only
    assert np.array_equal(bits(dp), bits(dp2)) and np.array_equal(bits(dt), bits(dt2))
    assert not np.any(np.isnan(dp)) and not np.any(np.isnan(dt))


def check_partials_against_reference_differences(ref, prm, pap2, t2, dp, dt, label):
    """dp, dt (nlev, ncol) against central differences of the reference's SATUR, relative step 1e-6.  Returns the clamped mask."""
    h = 1e-6
    set_lib_params(ref, prm)
    c = np.ascontiguousarray
    fd_t = (ref.satur(pap2, c(t2 * (1 + h))) - ref.satur(pap2, c(t2 * (1 - h)))) / (2 * h * t2)
    fd_p = (ref.satur(c(pap2 * (1 + h)), t2) - ref.satur(c(pap2 * (1 - h)), t2)) / (2 * h * pap2)
    # stencils that straddle a kink are left out: t within two steps of RTICE / RTWAT, or zqs crossing 0.5 inside a stencil
    near = (np.abs(t2 - prm.rtice) <= 2 * h * t2) | (np.abs(t2 - prm.rtwat) <= 2 * h * t2)
    side = [satur_numpy(prm, p_, t_)[1] > 0.5 for p_, t_ in ((pap2, t2), (pap2, t2 * (1 + h)), (pap2, t2 * (1 - h)),
                                                               (pap2 * (1 + h), t2), (pap2 * (1 - h), t2))]
    crossing = np.zeros_like(near)
    for s in side[1:]:
        crossing |= s != side[0]
    out = near | crossing
    assert out.sum() <= 0.01 * out.size, (label, "points left out", int(out.sum()), out.size)
    clamped = side[0] & ~out
    free = ~side[0] & ~out
    assert np.all(dp[clamped] == 0.0) and np.all(dt[clamped] == 0.0), (label, "partials on clamped points must be exactly 0")
    assert np.all(fd_p[clamped] == 0.0) and np.all(fd_t[clamped] == 0.0), (label, "reference differences on clamped points")
    err_t = float(np.max(np.abs(dt[free] - fd_t[free]) / np.abs(fd_t[free])))
    err_p = float(np.max(np.abs(dp[free] - fd_p[free]) / np.abs(fd_p[free])))
    print(f"{label}: left out {int(out.sum())} of {out.size}, clamped {int(clamped.sum())}, rel diff dqs/dt {err_t:.3e}, dqs/dpap {err_p:.3e}")
    assert err_t <= 1e-8 and err_p <= 1e-8, (label, err_t, err_p)
    return clamped


@fp64_only
@pytest.mark.parametrize("which", [0, 1])
def test_partials_against_central_differences_of_the_reference(precise, ref, which):
    name, tab = the_tables()[which]
    prm = make_params(tab)
    pap2, t2 = np.ascontiguousarray(tab["PAP"]), np.ascontiguousarray(tab["PT"])
    _, dp, dt = hc_satur_lin(prm, one_block(pap2), one_block(t2))
    clamped = check_partials_against_reference_differences(ref, prm, pap2, t2, dp[0], dt[0], name)
    if name == "seed5":
        assert clamped.sum() == 3 and np.all(np.nonzero(clamped)[0] == 0), "seed 5 clamps three points, all on level 0"
    # the numpy restatement the other tests use is the same function
    ndp, ndt, _ = satur_partials_numpy(prm, pap2, t2)
    assert np.allclose(ndp, dp[0], rtol=1e-9, atol=0.0) and np.allclose(ndt, dt[0], rtol=1e-9, atol=0.0)


@fp64_only
@pytest.mark.parametrize("which", [0, 1])
def test_the_clamp_on_purpose(precise, ref, which):
    """pap of the top five levels divided by 100: clamped and unclamped lanes side by side in one level"""
    name, tab = the_tables()[which]
    prm = make_params(tab)
    pap2, t2 = np.ascontiguousarray(tab["PAP"]).copy(), np.ascontiguousarray(tab["PT"])
    pap2[:5] /= 100.0
    q, dp, dt = hc_satur_lin(prm, one_block(pap2), one_block(t2))
    assert np.array_equal(bits(q), bits(hc_satur(prm, one_block(pap2), one_block(t2)))), name
    clamped = check_partials_against_reference_differences(ref, prm, pap2, t2, dp[0], dt[0], name + " top/100")
    n = int(clamped[:5].sum())
    assert 450 <= n < 500, (name, "clamped of the 500 points of the top five levels", n)
    assert clamped[:3].sum() >= 299


@fp64_only
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_fused_tl_against_the_reference_tl_fed_the_composed_qsat_tangent(precise, ref, flags):
    nlev, nproma, ngptot = 137, 16, 30  # padded tail
    tab = c2.random_table(nlev, 30, seed=11)
    prm = make_params(tab, **flags)
    set_lib_params(ref, prm)
    st = c2.state_from_table(tab, nproma, ngptot)
    inc = increments15(st)
    tl = run_tl_satur(prm, st, inc)
    want = {n: [] for n in B.OUT_NAMES}
    got = {n: [] for n in B.OUT_NAMES}
    for ibl, icend in blocks_of(st):
        pap, t = np.ascontiguousarray(st.PAP[ibl]), np.ascontiguousarray(st.PT[ibl])
        qs = ref.satur(pap, t, kfdia=icend)
        dp, dt, _ = satur_partials_numpy(prm, pap[:, :icend], t[:, :icend])
        dinp = {n: np.ascontiguousarray(a[ibl]) for n, a in inc.items()}
        dinp["qsat"] = np.zeros_like(pap)
        dinp["qsat"][:, :icend] = dp * dinp["pap"][:, :icend] + dt * dinp["t"][:, :icend]
        _, dout = ref.cloudsc2tl(st.ptsphy, refcall.block_inputs(st, ibl, qs), dinp, ldrain1d=bool(prm.ldrain1d), kfdia=icend)
        for n in B.OUT_NAMES:
            want[n].append(dout[n][:, :icend])
            got[n].append(tl[n][ibl][:, :icend])
            assert np.all(np.isnan(tl[n][ibl][:, icend:])), ("the fused TL touched the padded tail", n)
    for n in B.OUT_NAMES:
        e = field_err(want[n], got[n])
        print(f"{flags} {n}: {e:.3e}")
        assert e <= TLAD_TOL, (n, e)


LAMBDAS = (1e-4, 1e-5, 1e-6, 1e-7, 1e-8)
ERROR_NORM_ORDER = ("tent", "tenq", "tenl", "teni", "clc", "fplsl", "fplsn", "fhpsl", "fhpsn", "covptot")


def composite_taylor_ratios(ref, prm, st, tl: dict) -> list:
    """The driver's Taylor ratios (ERROR_NORM, cloudsc_driver_tl_mod.F90:21-31,233-252) of the composite function: the reference's
    SATUR recomputed at x + lambda * 0.01 x, the reference's CLOUDSC2, against the tangent `tl`."""
    set_lib_params(ref, prm)
    ld = bool(prm.ldrain1d)

    def nl(ibl, icend, lam):
        x = refcall.block_inputs(st, ibl)
        x = {n: np.ascontiguousarray(a + lam * (a * 0.01)) for n, a in x.items()}
        x["qsat"] = ref.satur(x["pap"], x["t"], kfdia=icend)  # SATUR of the perturbed pap, t: the composite function
        return ref.cloudsc2(st.ptsphy, x, ldrain1d=ld, kfdia=icend)

    base = {ibl: nl(ibl, icend, 0.0) for ibl, icend in blocks_of(st)}
    ratios = []
    for lam in LAMBDAS:
        worst = 0.0
        for ibl, icend in blocks_of(st):
            f5 = nl(ibl, icend, lam)
            znorm = zcount = 0.0
            for n in ERROR_NORM_ORDER:
                den = float(np.sum(tl[n][ibl][:, :icend] * lam))
                if abs(den) > np.finfo(np.float64).eps:
                    zcount += 1.0
                    znorm += abs(float(np.sum(base[ibl][n][:, :icend] - f5[n][:, :icend])) / den)
            assert zcount > 0.0
            worst = max(worst, znorm / zcount)
        ratios.append(worst)
    return ratios


@fp64_only
@pytest.mark.parametrize("case", ["synthetic", "seed5", "synthetic-levapls2"])
def test_composite_taylor_test_by_the_reference(precise, ref, case):
    tab = c2.random_table(137, 100, seed=5) if case == "seed5" else c2.synthetic_table()
    prm = make_params(tab, lregcl=False, levapls2=case.endswith("levapls2"))
    st = c2.state_from_table(tab, 32, 100)
    tl = run_tl_satur(prm, st, increments15(st))
    ratios = composite_taylor_ratios(ref, prm, st, tl)
    off = [abs(1.0 - r) for r in ratios]
    print(f"{case}: fused TL ratios {ratios}")
    assert min(off) <= 5e-6, (case, ratios)
    assert off[2] < off[0], ("the ratios must approach 1", case, ratios)

    # the motivation: today's TL with qsat as an independent input and no qsat tangent is not the derivative of the composite
    qsat = hc_satur(prm, np.ascontiguousarray(st.PAP), np.ascontiguousarray(st.PT))
    qsat[np.isnan(qsat)] = 0.0  # (padded tail: not written)
    inc = increments_of(st, qsat)
    inc["qsat"][...] = 0.0
    got = st.copy()
    i, o = host_traj_blocks(got, qsat)
    tl0 = flat_fields("out", st.nblocks, st.nlev, st.nproma)
    assert hostcheck().hostcheck_tl(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(i), C.byref(o),
                                    C.byref(flat_block("in", inc)), C.byref(flat_block("out", tl0))) == 0
    r0 = composite_taylor_ratios(ref, prm, st, tl0)
    print(f"{case}: TL with dqsat = 0 ratios {r0}")
    assert min(abs(1.0 - r) for r in r0) > 1.0, (case, r0)


@fp64_only
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_dot_product_identity_of_the_fused_sweeps(precise, flags):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)  # nonzero PSUPSAT
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, nproma, ngptot)
    v = increments15(st)
    assert np.any(v["supsat"] != 0.0)
    u = run_tl_satur(prm, st, v)
    fwd, scratch = trajectory_for_reverse(prm, st, host_qsat(st))
    # (the padded tail of u is NaN: what the reverse sweep must neither read into its results nor change)
    xa, y = run_vjp_satur(prm, st, fwd, scratch, u)
    for n in u:
        assert np.array_equal(bits(y[n]), bits(u[n])), ("output adjoint changed", n)
    act = np.zeros((st.nblocks, 1, nproma), dtype=bool)
    for ibl, icend in blocks_of(st):
        act[ibl, 0, :icend] = True
        for n in xa:
            assert not np.any(np.isnan(xa[n][ibl][:, :icend])), ("active element not written", n)
            assert np.all(np.isnan(xa[n][ibl][:, icend:])), ("the padded tail was touched", n)
    lhs = sum(float(np.sum(np.where(act, u[n], 0.0) ** 2)) for n in u)
    rhs = sum(float(np.sum(np.where(act, v[n] * xa[n], 0.0))) for n in v)
    print(f"{flags}: <TL v, u> = {lhs!r}, <v, VJP u> = {rhs!r}, rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) / abs(lhs) <= 1e-12, (lhs, rhs)


@fp64_only
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_fused_vjp_against_the_existing_vjp_composed_with_the_partials(precise, flags):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, nproma, ngptot)
    nb = st.nblocks
    qsat = host_qsat(st)
    u = run_tl_satur(prm, st, increments15(st))
    for n in u:
        u[n][np.isnan(u[n])] = 0.0
    fwd, scratch = trajectory_for_reverse(prm, st, qsat)
    xs, _ = run_vjp_satur(prm, st, fwd, scratch, u)

    i, _ = host_traj_blocks(st, qsat)
    _, o = host_traj_blocks(fwd, qsat)
    xv = flat_fields("in", nb, nlev, nproma, fill=np.nan)
    y = {n: a.copy() for n, a in u.items()}
    assert host_lib("vjp").hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o), C.byref(flat_block("in", xv)),
                                               C.byref(flat_block("out", y)), scratch.ctypes.data, 2, 1) == 0
    _, dp, dt = hc_satur_lin(prm, np.ascontiguousarray(st.PAP), np.ascontiguousarray(st.PT))
    want = {"pap": xv["pap"] + dp * xv["qsat"], "t": xv["t"] + dt * xv["qsat"]}
    for n in SAT_NAMES:
        if n in want:
            e = field_err([want[n][ibl][:, :ic] for ibl, ic in blocks_of(st)], [xs[n][ibl][:, :ic] for ibl, ic in blocks_of(st)])
            print(f"{flags} {n}: {e:.3e}")
            assert e <= TLAD_TOL, (n, e)
        else:
            for ibl, ic in blocks_of(st):
                assert np.array_equal(bits(xs[n][ibl][:, :ic]), bits(xv[n][ibl][:, :ic])), ("not the bits of the existing VJP", n)
