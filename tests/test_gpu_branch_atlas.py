"""Branch atlas, GPU part: the kernels against the reference on the atmosphere that reaches every branch outcome of the level
physics (tests/branch_atlas.atlas_table), every (field, class) held to the bound tests/branch_atlas.Case measures on the reference
alone.  tests/test_branch_atlas.py proves on the CPU that the atlas reaches the outcomes, that the metric sees what the whole-field
norm misses, and that the host build of the same level functions is inside the same bounds.

NL through the driver (both arithmetic modes, with and without the evaporation branch) and at kernel level with SATUR in the sweep;
TL, AD (accumulating on a background) and VJP for the four flag sets; and, at the plain and the levapls2 + lregcl sets, the sweeps
that wrap the same level functions in other loops (batched, parameter, SATUR differentiated, parameter Jacobian) against the
single-direction sweeps on the atlas state, by the relation their own tests assert at the older states.  Shapes: the atlas at 137 and
at 60 levels, NPROMA 32, 90 columns (a ragged tail).

In an fp32 process (CLOUDSC2_PRECISION=single; tests/test_single.py starts one) the NL, TL, AD and VJP tests hold the kernels of
libcloudsc2_hip_sp.so to the fp32 class bounds (ERR_FACTOR x the error of the reference's own -DSINGLE build inside the class); the
two tests that compare sweeps with each other stay fp64-only, their fp32 contracts are not defined.  The fused fp32 ad_kernel runs
above 400 000 columns only (kAdSplitBelow): at these shapes the fp32 adjoint is the two-kernel form.

Fault discipline as in tests/test_gpu_offset_variants.py: once a launch of this module has ended in an error that is not a failed
comparison, nothing more is launched from it; nothing is retried.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import branch_atlas as A
from tests import offset_variant_checks as ov
from tests.gpu_util import parjac as parjac_launch, rel_err, same_bits, single as parjac_single
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu
fp64_only = pytest.mark.skipif(B.SINGLE, reason="compares sweeps with each other by their fp64 contracts (bits, TLAD_TOL); the fp32 "
                                                "contracts of these sweeps are not defined")

DEV = ov.DEV
NLEVS = [137, 60]
P = c2.PARAM_NAMES
_device_trouble = []  # a launch of this module that ended in an error: nothing more is launched after it


@contextlib.contextmanager
def device_work(what: str):
    if _device_trouble:
        pytest.fail(f"not launched: {_device_trouble[0]}")
    try:
        yield
        torch.cuda.synchronize()
    except AssertionError:
        raise
    except BaseException as e:  # noqa: BLE001  (a HIP error from B.check or from the synchronisation)
        _device_trouble.append(f"{what}: {e!r}")
        raise


def params_of(c, mode: int):
    prm = copy.copy(c.prm)
    prm.math_mode = mode
    return prm


def layout(c):
    return ag.Layout(c.st.nblocks, c.nlev, A.NPROMA, A.NGPTOT)


def device_inputs(c, lay, qsat: bool = True) -> dict:
    """The 16 trajectory inputs as device planes, QSAT the reference's (qsat = False: without it, SATUR in the sweep)."""
    x = {n: torch.from_numpy(a).to(DEV) for n, a in A.blocks_of({n: a for n, a in c.inp.items() if n != "qsat"}).items()}
    if qsat:
        x["qsat"] = torch.from_numpy(c.qsat).to(DEV)
    return ov.packed("in", B.IN_NAMES if qsat else ov.IN15, lay, values=x)


def device_planes(kind: str, d: dict, lay, fill: float = 0.0) -> dict:
    """(NLEVx, NGPTOT) matrices as device planes (packed like DeviceState's), the padded tail `fill`"""
    vals = {n: torch.from_numpy(a).to(DEV) for n, a in A.blocks_of(d, fill).items()}
    return ov.packed(kind, tuple(d), lay, values=vals)


def host_cols(d: dict) -> dict:
    return {n: A.active_cols(np.ascontiguousarray(t.cpu().numpy()), A.NGPTOT) for n, t in d.items()}


def report(c, mode, results):
    failures = []
    for what, (bad, worst, where) in results.items():
        tail = f"ERR_FACTOR {A.ERR_FACTOR:g} DRAWS {A.DRAWS}" if B.SINGLE else f"K_NL {c.K_NL:.2f} K_TLAD {c.K_TLAD:.2f}"
        print(f"{c.nlev} levels {c.flagset} math_mode {mode}: {what:14s} worst err/bound {worst:.3f} at {where}; {tail}")
        failures += [(what,) + b for b in bad]
    assert not failures, failures[:8]


# ---- NL ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("flagset", ["plain", "levapls2"])
@pytest.mark.parametrize("mode", [1, 2])
def test_nl_driver_within_the_class_bounds(nlev, flagset, mode):
    c = A.case(nlev, flagset)
    got = c.st.copy()
    with device_work("cloudsc_driver"):
        c2.run_state(params_of(c, mode), got, "nl")
    report(c, mode, {"nl driver": c.compare("nl", A.state_outputs(got), satur=True)})  # (the driver runs SATUR; fp64 has one set)
    tail = got.PFPLSN[-1][:, A.NGPTOT - (c.st.nblocks - 1) * A.NPROMA:]
    assert np.all(tail == 0.0), "the padded tail was written"


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("flagset", ["plain", "levapls2"])
@pytest.mark.parametrize("mode", [1, 2])
def test_nl_kernel_with_satur_in_the_sweep(nlev, flagset, mode):
    c = A.case(nlev, flagset)
    lay = layout(c)
    with device_work("cloudsc2_nl_launch without qsat"):
        out = ov.nl(device_inputs(c, lay, qsat=False), params_of(c, mode), c.ptsphy, lay)
    report(c, mode, {"nl satur": c.compare("nl", host_cols(out), satur=True)})


# ---- TL, AD, VJP ------------------------------------------------------------------------------------------------------------------------

def background(c) -> dict:
    """a non-zero background for the accumulating adjoint, of the size of the result cell by cell"""
    rng = np.random.default_rng(5)
    return {n: (a * rng.uniform(-1.0, 1.0, size=a.shape)).astype(B.REAL) for n, a in c.ref["ad"].items()}


@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("flagset", list(A.FLAG_SETS))
@pytest.mark.parametrize("mode", [1, 2])
def test_tl_ad_vjp_within_the_class_bounds(nlev, flagset, mode):
    c = A.case(nlev, flagset)
    lay, prm, ptsphy = layout(c), params_of(c, mode), c.ptsphy
    x0 = background(c)
    with device_work("TL, AD, VJP"):
        x = device_inputs(c, lay)
        dx = device_planes("in", c.dinp, lay)
        traj = ov.packed("out", B.OUT_NAMES, lay)
        dy = ov.tl(x, dx, prm, ptsphy, lay, traj=traj)
        # AD accumulating on the background (cloudsc2_ad_launch consumes the output adjoints)
        xa = device_planes("in", x0, lay, fill=float("nan"))
        y = device_planes("out", c.ref["y"], lay, fill=float("nan"))
        tr2, sc = ov.packed("out", B.OUT_NAMES, lay), ov.scratch_of(lay)
        B.check(B.lib.cloudsc2_ad_launch(*ov.geom(prm, ptsphy, lay), ov.blk("in", x, lay), ov.blk("out", tr2, lay), ov.blk("in", xa, lay),
                                         ov.blk("out", y, lay), C.c_void_p(sc.data_ptr()), ov.stream()))
        # VJP (assign) from the trajectory pass
        ftraj, fsc = ov.ad_forward(x, prm, ptsphy, lay)
        u = device_planes("out", c.ref["y"], lay, fill=float("nan"))
        xv = ov.vjp(x, ftraj, fsc, u, prm, ptsphy, lay)
    xv_h = host_cols(xv)
    xv_h["supsat"] = xv_h["supsat"] * ptsphy  # CLOUDSC2AD's PSUPSAT adjoint carries a factor PTSPHY (cloudsc2ad.F90:1733)
    report(c, mode, {"tl": c.compare("tl", host_cols(dy)), "traj": c.compare("traj", host_cols(traj)),
                     "ad accumulate": c.compare("ad", host_cols(xa), A.reference_ad(c, x0)), "vjp": c.compare("ad", xv_h)})
    for n, t in y.items():  # consumed on the active columns, the tail as it was
        assert np.all(A.active_cols(t.cpu().numpy(), A.NGPTOT) == 0.0), ("output adjoint not consumed", n)
        assert bool(torch.all(torch.isnan(t[-1, :, lay.tail:]))), ("padded tail written", n)
    for n, t in xv.items():
        assert bool(torch.all(torch.isnan(t[-1, :, lay.tail:]))), ("padded tail written", n)


# ---- the sweeps that wrap the same level functions in other loops -----------------------------------------------------------------------

def directions(c, lay, x, k):
    """k tangents of the state's own scale (the first: the reference's increments) and k cotangents"""
    dxs = [device_planes("in", c.dinp, lay)] + [ov.packed("in", B.IN_NAMES, lay, values=ov.seeded(B.IN_NAMES, lay, 100 + j, scale=x)) for j in range(1, k)]
    us = [device_planes("out", c.ref["y"], lay)] + [ov.packed("out", B.OUT_NAMES, lay, values=ov.seeded(B.OUT_NAMES, lay, 200 + j)) for j in range(1, k)]
    return dxs, us


@fp64_only
@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("flagset", ["plain", "levapls2+lregcl"])
@pytest.mark.parametrize("mode", [1, 2])
def test_batched_and_parameter_sweeps_equal_the_single_direction_sweeps(nlev, flagset, mode):
    """tl_batch / vjp_batch (3 directions), vjp_par and tl_parjac: the bits of the single-direction launchers, as
    tests/test_gpu_autograd_batch.py, test_gpu_autograd_par.py and test_gpu_autograd_parjac.py hold them to at the older states;
    tl_par with zero parameter increments: 1e-13 of a field's maximum, the bound of tests/test_hostcheck_par.py."""
    c = A.case(nlev, flagset)
    lay, prm, ptsphy = layout(c), params_of(c, mode), c.ptsphy
    evap = c.evap
    with device_work("batched and parameter sweeps"):
        x = device_inputs(c, lay)
        dxs, us = directions(c, lay, x, 3)
        ftraj, fsc = ov.ad_forward(x, prm, ptsphy, lay)
        tl1 = [ov.tl(x, dx, prm, ptsphy, lay) for dx in dxs]
        vjp1 = [ov.vjp(x, ftraj, fsc, u, prm, ptsphy, lay) for u in us]
        tlb = ov.tl_batch(x, dxs, prm, ptsphy, lay)
        vjpb = ov.vjp_batch(x, ftraj, fsc, us, prm, ptsphy, lay)
        tlp = ov.tl_par(x, dxs[0], [0.0] * len(P), prm, ptsphy, lay, 0)
        vjpp, _, par_adj = ov.vjp_par(x, ftraj, fsc, us[0], prm, ptsphy, lay, 0)
        zero = {n: torch.zeros_like(t) for n, t in x.items()}
        sens = parjac_launch(x, prm, ptsphy, lay)
        want = [parjac_single(x, zero, k, prm, ptsphy, lay) if (pname != "rpecons" or evap) else None for k, pname in enumerate(P)]
    for j in range(3):
        for n in B.OUT_NAMES:
            assert same_bits(tlb[j][n], tl1[j][n]), ("TL batch != single", j, n)
        for n in B.IN_NAMES:
            assert same_bits(vjpb[j][n], vjp1[j][n]), ("VJP batch != single", j, n)
    for n in B.IN_NAMES:
        assert same_bits(vjpp[n], vjp1[0][n]), ("vjp_par: not the bits of the plain launcher", n)
    assert bool(torch.all(torch.isfinite(par_adj)))
    for n in B.OUT_NAMES:
        e = rel_err(parjac_active(tlp[n], lay), parjac_active(tl1[0][n], lay))
        print(f"{nlev} levels {flagset} math_mode {mode}: tl_par with dpar = 0 against tl, {n}: {e:.3e}")
        assert e <= 1e-13, ("tl_par with zero parameter increments", n, e)
    for k, pname in enumerate(P):
        for n in B.OUT_NAMES:
            if want[k] is None:
                assert bool(torch.all(torch.isnan(sens[k][n]))), ("the rpecons block was written", n)
            else:
                assert same_bits(sens[k][n], want[k][n]), ("tl_parjac: not the bits of cloudsc2_tl_launch_par", pname, n)
                assert bool(torch.all(torch.isfinite(parjac_active(sens[k][n], lay)))), (pname, n)


def parjac_active(t, lay):
    return t.transpose(0, 1).reshape(t.shape[1], -1)[:, :lay.ngptot]


@fp64_only
@pytest.mark.parametrize("nlev", NLEVS)
@pytest.mark.parametrize("flagset", ["plain", "levapls2+lregcl"])
@pytest.mark.parametrize("mode", [1, 2])
def test_satur_differentiated_in_the_sweep_against_the_chain_rule(nlev, flagset, mode):
    """tl_launch_satur / vjp_launch_satur against the single-direction sweeps with SATUR's tangent and adjoint applied outside
    (the planes of cloudsc2_satur_lin_launch): TLAD_TOL of a field's maximum, the bound tests/test_gpu_autograd_satur.py holds the
    fused route to against the unfused one."""
    c = A.case(nlev, flagset)
    lay, prm, ptsphy = layout(c), params_of(c, mode), c.ptsphy
    with device_work("SATUR differentiated in the sweep"):
        x15 = device_inputs(c, lay, qsat=False)
        qsat, dqp, dqt = ag._satur_planes(prm, lay, x15["pap"], x15["t"])
        x = dict(x15, qsat=qsat)
        dx15 = {n: t for n, t in device_planes("in", c.dinp, lay).items() if n != "qsat"}
        dx = dict(dx15, qsat=dqp * dx15["pap"] + dqt * dx15["t"])
        u = device_planes("out", c.ref["y"], lay)
        straj, ssc = ov.ad_forward(x15, prm, ptsphy, lay)
        got_tl = ov.tl_satur(x15, dx15, prm, ptsphy, lay)
        got_vjp = ov.vjp(x15, straj, ssc, u, prm, ptsphy, lay, satur=True)
        want_tl = ov.tl({n: x[n] for n in B.IN_NAMES}, {n: dx[n] for n in B.IN_NAMES}, prm, ptsphy, lay)
        ftraj, fsc = ov.ad_forward({n: x[n] for n in B.IN_NAMES}, prm, ptsphy, lay)
        xa = ov.vjp({n: x[n] for n in B.IN_NAMES}, ftraj, fsc, u, prm, ptsphy, lay)
        want_vjp = {n: xa[n] for n in ov.IN15}
        want_vjp["pap"] = xa["pap"] + dqp * xa["qsat"]
        want_vjp["t"] = xa["t"] + dqt * xa["qsat"]
    for n in B.OUT_NAMES:
        e = rel_err(parjac_active(got_tl[n], lay), parjac_active(want_tl[n], lay))
        assert e <= A.TLAD_TOL, ("tl_launch_satur", n, e)
    for n in ov.IN15:
        e = rel_err(parjac_active(got_vjp[n], lay), parjac_active(want_vjp[n], lay))
        assert e <= A.TLAD_TOL, ("vjp_launch_satur", n, e)
    assert bool(torch.any(dqt != 0)) and bool(torch.any(parjac_active(dqt, lay) == 0)), "the atlas has clamped and unclamped SATUR cells"
