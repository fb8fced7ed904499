"""``cloudsc2_parnormal_launch`` / ``c2.param_normal_equations``: what needs no device.  The launcher reports what is wrong with a call
before it looks for the device (CLOUDSC2_EINVAL with or without a GPU), launches nothing then (the launch log stays empty: it is no
sweep family anyway), and answers CLOUDSC2_ENODEVICE to a well-formed call where there is none; ``check_residual`` raises ``ValueError``
on CPU tensors, and ``param_normal_equations`` reaches the device check only after every other check."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params
from tests.util import B, c2, flat_block, flat_fields, hfld
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

N = NB * NPROMA
LAY = ag.Layout(NB, NLEV, NPROMA, N)
OBS = ("tent", "fplsl")


def test_header_binding_and_package_agree_on_the_new_symbols():
    for name in ("cloudsc2_parnormal_work_doubles", "cloudsc2_parnormal_launch"):
        assert name in B.EXPORTED and hasattr(B.lib, name)
    assert c2.param_normal_equations is ag.param_normal_equations and c2.NormalEquations is ag.NormalEquations
    assert B.NNORMAL == 14
    assert "parnormal" not in B.FAMILIES and len(B.FAMILIES) == 10  # not a sweep family


def test_work_doubles():
    n = C.c_longlong(-1)
    for nproma, ngptot, padded in ((32, 100, 128), (128, 1300, 1408), (128, 16384, 16384), (1, 7, 7), (64, 1, 64)):
        assert B.lib.cloudsc2_parnormal_work_doubles(nproma, ngptot, C.byref(n)) == 0 and n.value == 14 * padded, (nproma, ngptot)
    for nproma, ngptot, res in ((0, 100, C.byref(n)), (32, 0, C.byref(n)), (-1, 100, C.byref(n)), (32, 100, None)):
        assert B.lib.cloudsc2_parnormal_work_doubles(nproma, ngptot, res) == B.CLOUDSC2_EINVAL
        assert B.lib.cloudsc2_last_error()


def tensors(names, device="cpu", dtype=None):
    return {n: torch.ones(LAY.shape(n), dtype=dtype or B.torch_real(), device=device) for n in names}


# ---- the launcher -------------------------------------------------------------------------------------------------------------------
WORK = np.zeros(14 * N)
NORMAL = np.zeros(14)


def host_blocks(qsat=True):
    """a well-formed call's blocks over HOST arrays: only their pointers and strides are looked at here (nothing is launched)"""
    xin = flat_fields("in", NB, NLEV, NPROMA, fill=1.0)
    if not qsat:
        del xin["qsat"]
    out = flat_fields("out", NB, NLEV, NPROMA, fill=1.0)
    return xin, {n: out[n] for n in OBS}, {"fplsl": out["fplsl"].copy()}


def call(prm, xin, resid, weight, nproma=NPROMA, nlev=NLEV, ngptot=N, traj=True, work=True, normal=True):
    """resid / weight: dicts of host arrays, ready-made blocks, or None"""
    def blk(d):
        return None if d is None else C.byref(d if isinstance(d, B.Outputs) else flat_block("out", d))

    return B.lib.cloudsc2_parnormal_launch(C.byref(prm) if prm is not None else None, 3600.0, nproma, nlev, ngptot,
                                           C.byref(flat_block("in", xin)) if traj else None, blk(resid), blk(weight),
                                           WORK.ctypes.data if work else None, NORMAL.ctypes.data if normal else None, None)


def einval_cases():
    xin, r, w = host_blocks()
    ok = dict(xin=xin, resid=r, weight=w)
    yield "params NULL", dict(ok, prm=None)
    yield "traj_in NULL", dict(ok, prm=params(), traj=False)
    yield "resid NULL", dict(ok, prm=params(), resid=None)
    yield "work NULL", dict(ok, prm=params(), work=False)
    yield "normal NULL", dict(ok, prm=params(), normal=False)
    p = params(); p.lphylin = 0
    yield "lphylin = 0", dict(ok, prm=p)
    for flag in ("levapls2", "ldrain1d"):
        p = params(**{flag: True}); p.rpecons = 0.0
        yield f"{flag}, rpecons = 0", dict(ok, prm=p)
    yield "no observed output", dict(ok, prm=params(), resid={}, weight=None)
    yield "a weight for an unobserved output", dict(ok, prm=params(), weight={"tenq": r["tent"]})
    yield "a required input NULL", dict(ok, prm=params(), xin={n: a for n, a in xin.items() if n != "supsat"})
    yield "nproma = 0", dict(ok, prm=params(), nproma=0)
    yield "ngptot = 0", dict(ok, prm=params(), ngptot=0)
    yield "nlev = 1", dict(ok, prm=params(), nlev=1)
    yield "nlev != prm.nlev", dict(ok, prm=params(), nlev=NLEV - 1)
    p = params(); p.math_mode = 3
    yield "math_mode = 3", dict(ok, prm=p)
    # one block stride per layout group: planes of a packed buffer (stride 8 planes) next to contiguous ones
    packed = np.ones((NB, 8, NLEV + 1, NPROMA), dtype=B.REAL)
    big = 8 * (NLEV + 1) * NPROMA
    out = flat_fields("out", NB, NLEV, NPROMA, fill=1.0)
    mixed = flat_block("out", {n: out[n] for n in ("tent", "tenq")})
    mixed.tenq = hfld(packed, 0, big)
    yield "residuals of one group with unequal strides", dict(ok, prm=params(), resid=mixed, weight=None, keep=(packed, out))
    wmixed = flat_block("out", {n: out[n] for n in ("fplsl", "fplsn")})
    wmixed.fplsn = hfld(packed, 0, big)
    yield "weights of one group with unequal strides", dict(ok, prm=params(), resid={n: out[n] for n in ("fplsl", "fplsn")}, weight=wmixed,
                                                            keep=(packed, out))
    wother = B.Outputs()
    wother.fplsl = hfld(packed, 0, big)
    yield "a weight's stride differs from its residual's", dict(ok, prm=params(), weight=wother, keep=(packed,))


@pytest.mark.parametrize("label, kw", list(einval_cases()), ids=[c[0] for c in einval_cases()])
def test_a_bad_call_is_einval_with_or_without_a_device_and_launches_nothing(label, kw):
    kw = dict(kw)
    kw.pop("keep", None)
    B.launch_log_reset()
    assert call(**kw) == B.CLOUDSC2_EINVAL, label
    assert B.lib.cloudsc2_last_error()
    assert B.launch_log() == []


@pytest.mark.parametrize("qsat", [True, False])
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
def test_a_well_formed_call_without_a_device_is_enodevice(flags, weighted, qsat):
    """qsat NULL (SATUR in the sweep), a NULL weight block and weights on a subset of the observed outputs are well-formed.  Where there
    is a device the same call would launch on these host arrays, so it is made only where there is none."""
    if B.lib.cloudsc2_device_available():
        return
    xin, r, w = host_blocks(qsat)
    B.launch_log_reset()
    assert call(params(**flags), xin, r, w if weighted else None) == B.CLOUDSC2_ENODEVICE
    assert b"device" in B.lib.cloudsc2_last_error()
    assert B.launch_log() == []


# ---- check_residual and the entry point ---------------------------------------------------------------------------------------------
def bad_residuals():
    other = torch.float32 if not B.SINGLE else torch.float64
    yield "unknown name", dict(residual={**tensors(OBS), "rain": torch.ones(1)}, weights=None), "unknown name"
    yield "unknown weight name", dict(residual=tensors(OBS), weights={"rain": torch.ones(1)}), "unknown name"
    yield "empty mapping", dict(residual={}, weights=None), "empty"
    yield "not a mapping", dict(residual=[("tent", torch.ones(1))], weights=None), "must map"
    yield "None", dict(residual=None, weights=None), "must map"
    yield "weights not a mapping", dict(residual=tensors(OBS), weights=torch.ones(1)), "must map"
    yield "wrong shape", dict(residual={**tensors(OBS), "fplsn": torch.ones(LAY.shape("tent"), dtype=B.torch_real())}, weights=None), "shape"
    yield "wrong weight shape", dict(residual=tensors(OBS), weights={"tent": torch.ones(LAY.shape("fplsl"), dtype=B.torch_real())}), "shape"
    yield "wrong dtype", dict(residual=tensors(OBS, dtype=other), weights=None), "dtype"
    yield "wrong weight dtype", dict(residual=tensors(OBS), weights=tensors(("tent",), dtype=other)), "dtype"
    yield "not a tensor", dict(residual={"tent": np.ones(LAY.shape("tent"))}, weights=None), "not a tensor"
    yield "weight for an unobserved name", dict(residual=tensors(OBS), weights=tensors(("tenq",))), "not observed"


@pytest.mark.parametrize("label, kw, match", list(bad_residuals()), ids=[c[0] for c in bad_residuals()])
def test_check_residual_refuses(label, kw, match):
    with pytest.raises(ValueError, match=match):
        ag.check_residual(kw["residual"], kw["weights"], LAY)
    with pytest.raises(ValueError, match=match):  # ... and the entry point raises the same before it looks at the device
        c2.param_normal_equations(inputs("cpu"), params(), 3600.0, residual=kw["residual"], weights=kw["weights"])


def test_check_residual_copies_only_the_groups_that_do_not_fit():
    r = tensors(("tent", "tenq", "fplsl", "clc"))
    w = tensors(("tent", "fplsl"))
    r2, w2 = ag.check_residual(r, w, LAY)
    assert tuple(r2) == ("tent", "tenq", "clc", "fplsl") and tuple(w2) == ("tent", "fplsl")  # OUT_NAMES order
    assert all(r2[n] is r[n] for n in r) and all(w2[n] is w[n] for n in w)
    # tendencies as planes of a packed buffer: the residuals agree among themselves, the contiguous weight does not agree with them
    packed = torch.ones((NB, 8, NLEV, NPROMA), dtype=B.torch_real())
    r["tent"], r["tenq"] = packed[:, 0], packed[:, 2]
    r2, w2 = ag.check_residual(r, None, LAY)
    assert r2["tent"] is r["tent"] and r2["tenq"] is r["tenq"] and w2 == {}
    r2, w2 = ag.check_residual(r, w, LAY)
    assert r2["tent"].is_contiguous() and r2["tenq"].is_contiguous() and w2["tent"] is w["tent"]
    assert r2["fplsl"] is r["fplsl"] and w2["fplsl"] is w["fplsl"] and r2["clc"] is r["clc"]
    # members of one group with different strides
    r["tenq"] = torch.ones(LAY.shape("tenq"), dtype=B.torch_real())
    r2, _ = ag.check_residual(r, None, LAY)
    assert r2["tent"].is_contiguous() and torch.equal(r2["tent"], r["tent"])


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_are_refused_as_no_cpu_path_after_every_other_check(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    p64 = torch.tensor(1.0, dtype=torch.float64)
    for p in (None, {"rclcrit": p64}):
        with pytest.raises(ValueError, match="no CPU path"):
            c2.param_normal_equations(x, params(), 3600.0, residual=tensors(OBS), weights=tensors(("tent",)), satur=satur, params=p)
    with pytest.raises(ValueError, match="names"):
        c2.param_normal_equations({n: t for n, t in x.items() if n != "supsat"}, params(), 3600.0, residual=tensors(OBS), satur=satur)
    with pytest.raises(ValueError, match="unknown name"):
        c2.param_normal_equations(x, params(), 3600.0, residual=tensors(OBS), satur=satur, params={"rlmin": p64})
    prm = params()
    prm.lphylin = 0
    with pytest.raises(ValueError, match="lphylin"):
        c2.param_normal_equations(x, prm, 3600.0, residual=tensors(OBS), satur=satur)
