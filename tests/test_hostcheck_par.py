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

import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.test_hostcheck_satur_lin import (FLAG_SETS, bits, blocks_of, field_err, increments15, run_tl_satur, run_vjp_satur,
                                            satlin_lib, the_tables, trajectory_for_reverse)
from tests.test_hostcheck_vjp import host_qsat, vjp_lib
from tests.util import (B, HOSTCHECK_DIR, ROOT, c2, flat_block, flat_fields, host_traj_blocks, hostcheck, increments_of,
                        make_params, refcall, set_lib_params)

PAR_LIB = os.path.join(HOSTCHECK_DIR, "libhostcheck_par_sp.so" if B.SINGLE else "libhostcheck_par.so")
PARAM_NAMES = ("rkconv", "rclcrit", "rlptrc", "rpecons")  # the order of CLOUDSC2_NPAR
fp64_only = pytest.mark.skipif(B.SINGLE, reason="the bounds are fp64 statements")


def build_hostcheck_par() -> str:
    src = os.path.join(HOSTCHECK_DIR, "hostcheck_par.hip")
    deps = [src, os.path.join(HOSTCHECK_DIR, "hostcheck.hip")] + [
        os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "csrc", f) for f in ("cloudsc2_level.hpp", "cloudsc2_column.hpp")]
    if (not os.path.exists(PAR_LIB)) or any(os.path.getmtime(d) > os.path.getmtime(PAR_LIB) for d in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                               "-std=c++17"] + (["-DCLOUDSC2_SINGLE"] if B.SINGLE else []) + ["-o", PAR_LIB, src])
    return PAR_LIB


_lib = None


def par_lib():
    global _lib
    if _lib is None:
        lib = C.CDLL(build_hostcheck_par())
        pp, pi, po, pd = C.POINTER(B.Params), C.POINTER(B.Inputs), C.POINTER(B.Outputs), C.POINTER(C.c_double)
        lib.hostcheck_tl_par.argtypes = [pp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, pi, pi, pd, po]
        lib.hostcheck_vjp_par.argtypes = [pp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, pi, po, pi, po, C.c_void_p, C.c_void_p, pd]
        lib.hostcheck_tl_par.restype = lib.hostcheck_vjp_par.restype = C.c_int
        _lib = lib
    return _lib


@pytest.fixture(params=["fast", "precise"])
def precise(request):
    p = int(request.param == "precise")
    libs = (hostcheck(), vjp_lib(), satlin_lib(), par_lib())
    for lib in libs:
        lib.hostcheck_set_precise(p)
    yield p
    for lib in libs:
        lib.hostcheck_set_precise(0)


@pytest.fixture(scope="module")
def ref():
    """the reference itself where it is built, else its C restatement"""
    return refcall.RefLib() if refcall.have_ref() else refcall.OracleLib()


def dvec(values) -> C.Array:
    return (C.c_double * 4)(*[float(v) for v in values])


def run_tl_par(prm, st, inc: dict, dpar, qsat=None) -> dict:
    """TL(dx, dp) of the host build; qsat given: the satur = 0 form (inc holds 16 fields), None: satur = 1 (15 fields)"""
    nb, nlev, nproma = st.nblocks, st.nlev, st.nproma
    i, _ = host_traj_blocks(st, qsat)
    tl = flat_fields("out", nb, nlev, nproma, fill=np.nan)
    assert par_lib().hostcheck_tl_par(C.byref(prm), st.ptsphy, nproma, nlev, st.ngptot, int(qsat is None), C.byref(i),
                                      C.byref(flat_block("in", inc)), dvec(dpar), C.byref(flat_block("out", tl))) == 0
    return tl


def run_vjp_par(prm, st, fwd, scratch, u: dict, qsat=None):
    """the input adjoints, the (read-only) output adjoints, par_adj[4] and the workspace of the host build's parameter VJP"""
    nb, nlev, nproma = st.nblocks, st.nlev, st.nproma
    i, _ = host_traj_blocks(st, qsat)
    _, o = host_traj_blocks(fwd, qsat)
    xa = flat_fields("in", nb, nlev, nproma, fill=np.nan)
    if qsat is None:
        del xa["qsat"]
    y = {n: a.copy() for n, a in u.items()}
    work = np.full((4, nb * nproma), np.nan)
    par_adj = dvec([np.nan] * 4)
    assert par_lib().hostcheck_vjp_par(C.byref(prm), st.ptsphy, nproma, nlev, st.ngptot, int(qsat is None), C.byref(i), C.byref(o),
                                       C.byref(flat_block("in", xa)), C.byref(flat_block("out", y)), scratch.ctypes.data,
                                       work.ctypes.data, par_adj) == 0
    return xa, y, np.array(par_adj[:]), work


def with_param(prm, name: str, value: float):
    p = copy.copy(prm)
    setattr(p, name, value)
    return p


def reference_difference(ref, prm, st, qs, name: str, h: float) -> dict:
    """(F(p (1 + h)) - F(p (1 - h))) / (2 h p) of the reference's NL kernel, one block"""
    p0 = getattr(prm, name)
    outs = []
    for s in (+1.0, -1.0):
        set_lib_params(ref, with_param(prm, name, p0 * (1.0 + s * h)))
        outs.append(ref.cloudsc2(st.ptsphy, refcall.block_inputs(st, 0, qs), ldrain1d=bool(prm.ldrain1d)))
    set_lib_params(ref, prm)
    return {n: (outs[0][n] - outs[1][n]) / (2.0 * h * p0) for n in B.OUT_NAMES}


def exact_zero_fields(name: str, evap: bool) -> tuple:
    if name == "rpecons" and not evap:
        return tuple(B.OUT_NAMES)
    z = ["clc", "covptot"]
    if name == "rclcrit" and evap:
        z.append("teni")
    return tuple(z)


def check_against_reference_differences(ref, prm, st, qs, tl_of, label: str) -> float:
    """tl_of(k) -> the parameter tangent for dpar = e_k as {field: (nlev[+1], 100)}; returns the worst error of the case"""
    evap = bool(prm.levapls2 or prm.ldrain1d)
    worst = 0.0
    for k, name in enumerate(PARAM_NAMES):
        fd5 = reference_difference(ref, prm, st, qs, name, 1e-5)
        fd6 = reference_difference(ref, prm, st, qs, name, 1e-6)
        tl = tl_of(k)
        out = np.zeros(st.ngptot, dtype=bool)
        for n in B.OUT_NAMES:
            m = float(np.max(np.abs(fd6[n])))
            if m > 0.0:
                out |= np.max(np.abs(fd5[n] - fd6[n]), axis=0) > 1e-5 * m
        assert out.sum() <= 2, (label, name, "columns left out", int(out.sum()))
        keep = ~out
        zeros = exact_zero_fields(name, evap)
        errs = {}
        for n in B.OUT_NAMES:
            got, want = tl[n][:, keep], fd6[n][:, keep]
            assert not np.any(np.isnan(got)), (label, name, n)
            if n in zeros:
                assert np.all(got == 0.0) and np.all(want == 0.0), (label, name, n, "must be exactly zero")
                continue
            m = float(np.max(np.abs(want)))
            if m == 0.0:  # a field the reference does not move at all (tenl under rpecons): nor may the tangent
                assert np.all(got == 0.0), (label, name, n, "the reference's difference vanishes, the tangent does not")
                continue
            errs[n] = float(np.max(np.abs(got - want))) / m
        e = max(errs.values()) if errs else 0.0
        print(f"{label} {name}: left out {int(out.sum())}, worst {e:.3e} " + " ".join(f"{n} {v:.1e}" for n, v in errs.items()))
        for n, v in errs.items():
            assert v <= 1e-5, (label, name, n, v)
        worst = max(worst, e)
    return worst


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
        assert vjp_lib().hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, C.byref(i), C.byref(o),
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
