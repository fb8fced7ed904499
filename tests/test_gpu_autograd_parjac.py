"""The parameter Jacobian in one sweep on the MI355X: cloudsc2_tl_launch_parjac through the C ABI and ``c2.param_jacobian`` through torch.

Contract.  Every direction is the bits of cloudsc2_tl_launch_par (satur = 0) on zero-filled tangent planes with dpar = e_k -- the batched
sweeps' contract, and the reason every direction runs its own straight line in the kernel.  The form with SATUR evaluated in the sweep
(qsat NULL) against the form given cloudsc2_satur_launch's plane: at most 1e-13 of each field's maximum, the project's bound for
"dpar = 0 against the existing TL".  ``param_jacobian`` against ``torch.func.jvp`` of ``cloudsc2(..., params=p)`` with a unit tangent on
one parameter: bits with ``satur=False``; equal as numbers with ``satur=True``, where the fused op multiplies SATUR's partials by zero
tangents and may differ in the sign of a zero.  Against central differences of the reference's NL kernel: the cap and the bound of
tests/test_hostcheck_par.py (2 of 100 columns, 1e-5 of a field's maximum)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, active, new, params, parjac, same_bits, single, state, tail_zero
from tests.host_sweeps import check_against_reference_differences
from tests.util import B, FLAGS, c2, fp64_only, make_params, refcall, set_lib_params
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

P = c2.PARAM_NAMES
NAN = float("nan")
SHAPES = [(32, 100, 1), (32, 100, 2), (128, 16384, 0)]  # lanes, tails and full blocks; the three arithmetic settings


def evap_of(prm) -> bool:
    return bool(prm.levapls2 or prm.ldrain1d)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nproma,ngptot,math_mode", SHAPES)
def test_every_direction_is_the_bits_of_the_single_direction_launcher(nproma, ngptot, math_mode, flags):
    """Measured on the MI355X: see the printed lines (whether the qsat-NULL form came out as the bits of the form given the plane)."""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, 0)
    evap = evap_of(prm)
    x0 = {n: t.clone() for n, t in x.items()}
    zero = {n: torch.zeros_like(t) for n, t in x.items()}
    sens = parjac(x, prm, ptsphy, lay)
    again = parjac(x, prm, ptsphy, lay, null_last=not evap)  # (without the evaporation branch the rpecons block may be NULL)
    fused = parjac({n: t for n, t in x.items() if n != "qsat"}, prm, ptsphy, lay)
    torch.cuda.synchronize()
    for n in B.IN_NAMES:
        assert same_bits(x[n], x0[n]), ("a trajectory input plane changed", n)
    all_bits = True
    for k, pname in enumerate(P):
        if pname == "rpecons" and not evap:
            for n in B.OUT_NAMES:
                assert bool(torch.all(torch.isnan(sens[k][n]))) and bool(torch.all(torch.isnan(fused[k][n]))), ("the rpecons block was written", n)
            continue
        want = single(x, zero, k, prm, ptsphy, lay)
        torch.cuda.synchronize()
        for n in B.OUT_NAMES:
            assert same_bits(sens[k][n], want[n]), ("not the bits of cloudsc2_tl_launch_par (NaN tail included: not written)", pname, n)
            assert same_bits(again[k][n], sens[k][n]), ("two runs differ", pname, n)
            if lay.tail < lay.nproma:
                assert bool(torch.all(torch.isnan(sens[k][n][-1, :, lay.tail:]))), ("the padded tail was written", pname, n)
            a, f = active(sens[k][n], lay), active(fused[k][n], lay)
            assert bool(torch.all(torch.isfinite(a))), (pname, n)
            m = float(torch.max(torch.abs(a)))
            e = float(torch.max(torch.abs(f - a))) / m if m > 0.0 else float(torch.max(torch.abs(f)))
            all_bits = all_bits and same_bits(fused[k][n], sens[k][n])
            assert e <= 1e-13, ("SATUR in the sweep against the plane of cloudsc2_satur_launch", pname, n, e)
            if n in ("clc", "covptot") or (n == "teni" and pname == "rclcrit" and evap):
                assert bool(torch.all(a == 0)), ("must be exactly zero", pname, n)
        assert any(bool(torch.any(active(sens[k][n], lay) != 0)) for n in B.OUT_NAMES), (pname, "a sensitivity that is zero everywhere")
    print(f"{(nproma, ngptot, math_mode)} {flags}: qsat NULL against qsat given: {'the same bits' if all_bits else 'not the same bits'}")


def test_the_runtime_knows_the_new_kernels():
    per_cu = C.c_int(0)
    for f in (0, 1, 2, 3, 4, 5, 6, 7, 32, 39):  # QSAT, PRECISE, EVAP (and OFF32)
        B.check(B.lib.cloudsc2_kernel_occupancy(6, f, C.byref(per_cu)))
        assert per_cu.value >= 1
    for f in (8, 16, 64, 128, 256):
        assert B.lib.cloudsc2_kernel_occupancy(6, f, C.byref(per_cu)) == B.CLOUDSC2_EINVAL


def unit_jvp(x, prm, ptsphy, lay, satur, name, value):
    def f(p):
        return tuple(ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params={name: p}))

    return torch.func.jvp(f, (torch.tensor(value, dtype=torch.float64),), (torch.tensor(1.0, dtype=torch.float64),))[1]


@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("flags", FLAGS)
def test_param_jacobian_is_the_jvp_with_a_unit_tangent_on_each_parameter(flags, satur):
    """Bits with ``satur=False``, equal as numbers with ``satur=True``.  One entry cannot be held to bits: ``rpecons`` without the
    evaporation branch, which is zero tensors by contract (nothing is launched for it), while the jvp's exact zeros there carry signs
    (the single-direction launcher multiplies zero tangents by negative trajectory values: in the host build of these cases 1366 elements
    of clc and 13800 each of fhpsl / fhpsn are -0).  That entry is compared as numbers, like every entry with ``satur=True``."""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)
    xg = {n: t.clone().requires_grad_() for n, t in x.items()}  # (inputs that require a gradient: the result carries no graph)
    sens = c2.param_jacobian(xg, prm, ptsphy, lay.ngptot, satur=satur)
    assert tuple(sens.keys()) == P
    for pname in P:
        tan = unit_jvp(x, prm, ptsphy, lay, satur, pname, getattr(prm, pname))
        torch.cuda.synchronize()
        got = sens[pname]
        assert isinstance(got, ag.Cloudsc2Outputs)
        for k, n in enumerate(B.OUT_NAMES):
            g = getattr(got, n)
            assert not g.requires_grad and g.grad_fn is None and g.is_contiguous() and tuple(g.shape) == lay.shape(n), (pname, n)
            assert tail_zero(g, lay), (pname, n)
            if satur or (pname == "rpecons" and not evap_of(prm)):
                assert torch.equal(g, tan[k]), ("not the jvp's numbers", pname, n)
            else:
                assert same_bits(g, tan[k]), ("not the jvp's bits", pname, n)
        if pname == "rpecons" and not evap_of(prm):
            assert all(bool(torch.all(getattr(got, n) == 0)) for n in B.OUT_NAMES)
        else:
            assert bool(torch.any(got.fplsl != 0)), pname

    # a subset: that entry only, with the overridden value in effect
    value = 0.8 * prm.rclcrit
    for where in ("cpu", DEV):
        sub = c2.param_jacobian(x, prm, ptsphy, lay.ngptot, satur=satur, params={"rclcrit": torch.tensor(value, dtype=torch.float64, device=where)})
        assert tuple(sub.keys()) == ("rclcrit",) and prm.rclcrit != value, "the caller's prm was changed"
        tan = unit_jvp(x, prm, ptsphy, lay, satur, "rclcrit", value)
        torch.cuda.synchronize()
        for k, n in enumerate(B.OUT_NAMES):
            g = getattr(sub["rclcrit"], n)
            assert torch.equal(g, tan[k]) if satur else same_bits(g, tan[k]), ("subset", n)
        assert not same_bits(sub["rclcrit"].fplsl, sens["rclcrit"].fplsl), "the overridden value did not reach the kernel"
    assert c2.param_jacobian(x, prm, ptsphy, lay.ngptot, satur=satur, params={}) == {}


def test_batched_operands_are_refused_and_the_op_refuses_vmap_over_params_as_before():
    tab = c2.synthetic_table()
    prm = params(tab)
    x, ptsphy, lay = state(tab, 32, 64, prm, False)
    T = torch.stack([x["t"], x["t"] + 0.5])
    with pytest.raises(NotImplementedError, match="param_jacobian"):
        torch.func.vmap(lambda t: c2.param_jacobian({**x, "t": t}, prm, ptsphy, lay.ngptot)["rkconv"].fplsl)(T)
    R = torch.tensor([prm.rkconv, 2.0 * prm.rkconv], dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="param_jacobian"):
        torch.func.vmap(lambda r: c2.param_jacobian(x, prm, ptsphy, lay.ngptot, params={"rkconv": r})["rkconv"].fplsl)(R)
    with pytest.raises(NotImplementedError, match="params"):
        torch.func.jacfwd(lambda r: ag.cloudsc2(x, prm, ptsphy, lay.ngptot, params={"rkconv": r}).fplsl)(R[0])


@fp64_only
def test_on_the_device_against_the_reference_differences():
    """seed5, levapls2 (all four directions run), NPROMA 32 x 100 columns."""
    if not refcall.have_ref():
        pytest.fail("the reference build (oracle/_ref) is missing: build() makes it")
    ref = refcall.RefLib()
    tab = c2.random_table(137, 100, seed=5)
    prm = make_params(tab, lregcl=False, levapls2=True)
    set_lib_params(ref, prm)
    one = c2.state_from_table(tab, 100, 100)  # the same columns as one block, for the reference
    qs = ref.satur(np.ascontiguousarray(one.PAP[0]), np.ascontiguousarray(one.PT[0]))
    x, ptsphy, lay = state(tab, 32, 100, prm, 0)
    qsat = np.zeros(lay.shape("qsat"))
    for ibl in range(lay.nblocks):
        icend = min(lay.nproma, lay.ngptot - ibl * lay.nproma)
        qsat[ibl][:, :icend] = qs[:, ibl * lay.nproma:ibl * lay.nproma + icend]
    x["qsat"] = torch.from_numpy(qsat).to(DEV)
    sens = parjac(x, prm, ptsphy, lay)
    torch.cuda.synchronize()

    def tl_of(k):
        return {n: active(sens[k][n], lay).cpu().numpy() for n in B.OUT_NAMES}

    worst = check_against_reference_differences(ref, prm, one, qs, tl_of, "device seed5 levapls2")
    print(f"device seed5 levapls2: worst {worst:.3e}")


def test_a_captured_launch_replays_the_eager_bits():
    tab = c2.random_table(137, 100, seed=31)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = state(tab, 64, 1000, prm, 0)
    eager = parjac(x, prm, ptsphy, lay)  # the eager call a capture needs first: the CETA table
    torch.cuda.synchronize()
    cap = [new(B.OUT_NAMES, lay, fill=NAN) for _ in P]
    on_device = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64, device=DEV)}
    on_host = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64)}
    c2.param_jacobian(x, prm, ptsphy, lay.ngptot, params=on_host)  # (the device probe, before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        parjac(x, prm, ptsphy, lay, sens=cap)
        with pytest.raises(RuntimeError, match="capturing"):  # parameter values on the device would have to be read on the host
            c2.param_jacobian(x, prm, ptsphy, lay.ngptot, params=on_device)
    for s in cap:
        for t in s.values():
            t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for k, pname in enumerate(P):
        for n in B.OUT_NAMES:
            assert same_bits(cap[k][n], eager[k][n]), (pname, n)
