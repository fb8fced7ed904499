"""The derivative with respect to the tunable parameters rkconv, rclcrit, rlptrc, rpecons (C2F_PARLIN: what cloudsc2_tl_launch_par and
cloudsc2_vjp_launch_par run), compiled for the HOST.  The reference has no parameter derivative; the new code is tied to it by central
differences of the reference's NL kernel with respect to each parameter, and to the existing sweeps by the dot-product identity, by
bit equality of the field adjoints and by linearity.

Bounds.  Against the differences: 1e-5 of a field's maximum at relative step 1e-6, a column left out when the differences at 1e-5 and
1e-6 disagree by more than 1e-5 of the field's maximum, at most 2 of 100 columns per case -- all three from the reference alone (its
two step sizes agree to 1.7e-6 on the kept columns; a wrong factor, 1.9 for 2 or a missing PTSPHY, gives 1e-3 and more).  Measured
here, worst over the 16 cases and both arithmetics: 1.658e-06 (synthetic, no evaporation, rkconv: the round-off of the smaller step,
the reference's own disagreement between its two steps), the next 8.1e-07 (synthetic, rclcrit); one column left out in one case (seed5,
levapls2, rpecons).  1e-12 for the dot-product identity and for linearity, 1e-13 for dpar = 0 against the existing TL, 1e-11 for the
satur = 1 form against the satur = 0 form: the project's own numbers.  Measured: identity 5.5e-16 at worst (5.3e-4 and more without
the parameter term), linearity 1.4e-14, dpar = 0 against the existing TL 0.0, satur = 1 against satur = 0 fed SATUR's qsat 0.0."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.host_sweeps import (check_against_reference_differences, field_err, increments15, run_tl_par, run_tl_satur, run_vjp_par,
                               run_vjp_satur, trajectory_for_reverse)
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.util import (FLAG_SETS, PARAM_NAMES, B, bits, blocks_of, c2, flat_block, flat_fields, fp64_only, host_qsat,
                        host_traj_blocks, hostcheck, increments_of, make_params, refcall, set_lib_params, the_tables)


@pytest.fixture(scope="module")
def ref():
    """the reference itself where it is built, else its C restatement"""
    return refcall.RefLib() if refcall.have_ref() else refcall.OracleLib()


@fp64_only
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
@pytest.mark.parametrize("which", [0, 1])
def test_parameter_tangent_against_central_differences_of_the_reference(precise, ref, which, flags):
    """Measured (worst over the 16 cases, fast and precise): 1.658e-06 of a field's maximum (synthetic, no evaporation, rkconv)."""
    name, tab = the_tables()[which]
    prm = make_params(tab, lregcl=False, **flags)
    set_lib_params(ref, prm)
    st = c2.state_from_table(tab, 100, 100)
    qs = ref.satur(np.ascontiguousarray(st.PAP[0]), np.ascontiguousarray(st.PT[0]))
    qsat = np.ascontiguousarray(qs[None], dtype=B.REAL)
    zero = {n: np.zeros_like(a) for n, a in increments_of(st, qsat).items()}

    def tl_of(k):
        e = [0.0] * 4
        e[k] = 1.0
        return {n: a[0] for n, a in run_tl_par(prm, st, zero, e, qsat).items()}

    worst = check_against_reference_differences(ref, prm, st, qs, tl_of, f"{name} {flags}")
    print(f"{name} {flags}: worst {worst:.3e}")


def active_mask(st) -> np.ndarray:
    act = np.zeros((st.nblocks, 1, st.nproma), dtype=bool)
    for ibl, icend in blocks_of(st):
        act[ibl, 0, :icend] = True
    return act


def small_state(flags):
    nlev, nproma, ngptot = 137, 16, 30  # padded tail
    tab = c2.random_table(nlev, 30, seed=11)  # nonzero PSUPSAT
    prm = make_params(tab, **flags)
    return prm, c2.state_from_table(tab, nproma, ngptot)


def dp_of(prm) -> list:
    return [0.01 * getattr(prm, n) for n in PARAM_NAMES]


def increments(st, qsat):
    return increments15(st) if qsat is None else increments_of(st, qsat)


@fp64_only
@pytest.mark.parametrize("satur", [0, 1])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_dot_product_identity_with_parameters(precise, flags, satur):
    """<TL(dx, dp), u> = <dx, xa> + dp . par_adj, u = TL(dx, dp) with NaN in its padded tail.  Measured: 5.5e-16 at worst."""
    prm, st = small_state(flags)
    qsat = None if satur else host_qsat(st)
    v, dp = increments(st, qsat), dp_of(prm)
    u = run_tl_par(prm, st, v, dp, qsat)
    fwd, scratch = trajectory_for_reverse(prm, st, host_qsat(st))
    xa, y, par_adj, work = run_vjp_par(prm, st, fwd, scratch, u, qsat)
    for n in u:
        assert np.array_equal(bits(y[n]), bits(u[n])), ("output adjoint changed", n)
    act = active_mask(st)
    assert np.all(np.isfinite(par_adj)), par_adj
    assert np.all(np.isfinite(work[:, :st.ngptot])) and np.all(np.isnan(work[:, st.ngptot:])), "workspace: active columns only"
    for ibl, icend in blocks_of(st):
        for n in xa:
            assert not np.any(np.isnan(xa[n][ibl][:, :icend])), ("active element not written", n)
            assert np.all(np.isnan(xa[n][ibl][:, icend:])), ("the padded tail was touched", n)
    evap = bool(prm.levapls2 or prm.ldrain1d)
    assert (par_adj[3] != 0.0) == evap, ("rpecons acts with the evaporation branch only", par_adj)
    assert np.all(par_adj[:3] != 0.0), par_adj
    lhs = sum(float(np.sum(np.where(act, u[n], 0.0) ** 2)) for n in u)
    rhs = sum(float(np.sum(np.where(act, v[n] * xa[n], 0.0))) for n in v) + float(np.dot(dp, par_adj))
    rhs_fields_only = rhs - float(np.dot(dp, par_adj))
    print(f"{flags} satur={satur}: <TL, u> = {lhs!r}, <dx, xa> + dp.par_adj = {rhs!r}, rel {abs(lhs - rhs) / abs(lhs):.3e}; "
          f"without the parameter term {abs(lhs - rhs_fields_only) / abs(lhs):.3e}")
    assert abs(lhs - rhs) / abs(lhs) <= 1e-12, (lhs, rhs)
    assert abs(lhs - rhs_fields_only) / abs(lhs) > 1e-9, "the parameter term must matter to the identity"


@fp64_only
@pytest.mark.parametrize("satur", [0, 1])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_superset_of_the_existing_sweeps_and_linearity(precise, flags, satur):
    prm, st = small_state(flags)
    nb, nlev, nproma, ngptot = st.nblocks, st.nlev, st.nproma, st.ngptot
    hq = host_qsat(st)
    qsat = None if satur else hq
    v, dp = increments(st, qsat), dp_of(prm)
    blocks = list(blocks_of(st))

    def active(a):
        return [a[ibl][:, :ic] for ibl, ic in blocks]

    # TL with dpar = 0 against the existing host TL
    tl0 = run_tl_par(prm, st, v, [0.0] * 4, qsat)
    if satur:
        old = run_tl_satur(prm, st, v)
    else:
        got = st.copy()
        i, o = host_traj_blocks(got, hq)
        old = flat_fields("out", nb, nlev, nproma)
        assert hostcheck().hostcheck_tl(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o),
                                        C.byref(flat_block("in", v)), C.byref(flat_block("out", old))) == 0
    for n in B.OUT_NAMES:
        e = field_err(active(old[n]), active(tl0[n]))
        print(f"{flags} satur={satur} dpar=0 {n}: {e:.3e}")
        assert e <= 1e-13, (n, e)

    # TL(dx, dp) = TL(dx, 0) + TL(0, dp)
    both = run_tl_par(prm, st, v, dp, qsat)
    only_p = run_tl_par(prm, st, {n: np.zeros_like(a) for n, a in v.items()}, dp, qsat)
    for n in B.OUT_NAMES:
        e = field_err(active(both[n]), [a + b for a, b in zip(active(tl0[n]), active(only_p[n]))])
        print(f"{flags} satur={satur} linearity {n}: {e:.3e}")
        assert e <= 1e-12, (n, e)
    assert any(np.any(a != 0.0) for n in B.OUT_NAMES for a in active(only_p[n]))

    # the field adjoints of the parameter VJP are the bits of the existing VJP sweep
    u = {n: a.copy() for n, a in both.items()}
    fwd, scratch = trajectory_for_reverse(prm, st, hq)
    xp, _, _, _ = run_vjp_par(prm, st, fwd, scratch, u, qsat)
    if satur:
        xo, _ = run_vjp_satur(prm, st, fwd, scratch, u)
    else:
        i, _ = host_traj_blocks(st, hq)
        _, o = host_traj_blocks(fwd, hq)
        xo = flat_fields("in", nb, nlev, nproma, fill=np.nan)
        y = {n: a.copy() for n, a in u.items()}
        assert host_lib("vjp").hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o),
                                                   C.byref(flat_block("in", xo)), C.byref(flat_block("out", y)), scratch.ctypes.data, 2, 1) == 0
    assert set(xp) == set(xo)
    for n in xp:
        assert np.array_equal(bits(xp[n]), bits(xo[n])), ("not the bits of the existing VJP", n)


@fp64_only
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_parameter_gradients_through_satur_equal_those_with_its_qsat(precise, flags):
    """None of the four enters SATUR: the satur = 1 form and the satur = 0 form fed the host SATUR's qsat give the same parameter
    gradients (1e-11 relative).  The cotangent is the satur = 1 tangent of (dx, dp)."""
    prm, st = small_state(flags)
    hq = host_qsat(st)
    u = run_tl_par(prm, st, increments15(st), dp_of(prm), None)
    for n in u:
        u[n][np.isnan(u[n])] = 0.0
    fwd, scratch = trajectory_for_reverse(prm, st, hq)
    _, _, g1, _ = run_vjp_par(prm, st, fwd, scratch, u, None)
    _, _, g0, _ = run_vjp_par(prm, st, fwd, scratch, u, hq)
    for k, n in enumerate(PARAM_NAMES):
        if g0[k] == 0.0:
            assert g1[k] == 0.0, n
            continue
        e = abs(g1[k] - g0[k]) / abs(g0[k])
        print(f"{flags} {n}: satur=1 {g1[k]!r} satur=0 {g0[k]!r} rel {e:.3e}")
        assert e <= 1e-11, (n, e)
