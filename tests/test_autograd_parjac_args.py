"""``cloudsc2_tl_launch_parjac`` / ``c2.param_jacobian``: what needs no device.  The launcher reports what is wrong with a call before it
looks for the device (CLOUDSC2_EINVAL with or without a GPU) and answers CLOUDSC2_ENODEVICE to a well-formed call where there is none;
``param_jacobian`` runs the checks of ``cloudsc2(..., params=...)`` on CPU tensors and raises ``ValueError``, the device check after them."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params
from tests.util import B, c2, flat_block, flat_fields
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

N = NB * NPROMA


def p64(v=1.0):
    return torch.tensor(v, dtype=torch.float64)


def test_header_binding_and_package_agree_on_the_new_symbols():
    assert "cloudsc2_tl_launch_parjac" in B.EXPORTED and hasattr(B.lib, "cloudsc2_tl_launch_parjac")
    assert c2.param_jacobian is ag.param_jacobian
    assert B.lib.cloudsc2_batch_max() >= len(c2.PARAM_NAMES)  # the parameter directions are one launch


def host_blocks(qsat=True):
    """a well-formed call's blocks over HOST arrays: only their pointers and strides are looked at here (nothing is launched)"""
    xin = flat_fields("in", NB, NLEV, NPROMA, fill=1.0)
    if not qsat:
        del xin["qsat"]
    outs = [flat_fields("out", NB, NLEV, NPROMA) for _ in c2.PARAM_NAMES]
    return xin, outs


def call(prm, xin, outs, nproma=NPROMA, nlev=NLEV, ngptot=N, traj=True, pert=True):
    blocks = (B.Outputs * len(outs))(*(flat_block("out", o) for o in outs))
    return B.lib.cloudsc2_tl_launch_parjac(C.byref(prm) if prm is not None else None, 3600.0, nproma, nlev, ngptot,
                                           C.byref(flat_block("in", xin)) if traj else None, blocks if pert else None, None)


def einval_cases():
    xin, outs = host_blocks()
    yield "params NULL", dict(prm=None, xin=xin, outs=outs)
    yield "traj_in NULL", dict(prm=params(), xin=xin, outs=outs, traj=False)
    yield "pert_out NULL", dict(prm=params(), xin=xin, outs=outs, pert=False)
    p = params(); p.lphylin = 0
    yield "lphylin = 0", dict(prm=p, xin=xin, outs=outs)
    for flag in ("levapls2", "ldrain1d"):
        p = params(**{flag: True}); p.rpecons = 0.0
        yield f"{flag}, rpecons = 0", dict(prm=p, xin=xin, outs=outs)
    yield "a required input NULL", dict(prm=params(), xin={n: a for n, a in xin.items() if n != "supsat"}, outs=outs)
    yield "an output NULL in block 0", dict(prm=params(), xin=xin, outs=[{n: a for n, a in outs[0].items() if n != "fhpsn"}] + outs[1:])
    yield "an output NULL in block 2", dict(prm=params(), xin=xin, outs=outs[:2] + [{n: a for n, a in outs[2].items() if n != "clc"}] + outs[3:])
    yield "rpecons block NULL with the evaporation branch", dict(prm=params(levapls2=True), xin=xin, outs=outs[:3] + [{}])
    yield "nproma = 0", dict(prm=params(), xin=xin, outs=outs, nproma=0)
    yield "ngptot = 0", dict(prm=params(), xin=xin, outs=outs, ngptot=0)
    yield "nlev = 1", dict(prm=params(), xin=xin, outs=outs, nlev=1)
    yield "nlev != prm.nlev", dict(prm=params(), xin=xin, outs=outs, nlev=NLEV - 1)
    p = params(); p.math_mode = 3
    yield "math_mode = 3", dict(prm=p, xin=xin, outs=outs)
    # one block stride per layout group, across the blocks too: block 1's tendencies lie in a packed buffer (stride 8 planes)
    packed = np.zeros((NB, 8, NLEV, NPROMA), dtype=B.REAL)
    o1 = dict(outs[1])
    strided = flat_block("out", o1)
    for k, n in enumerate(("tent", "tenq", "tenl", "teni")):
        setattr(strided, n, B.Field(packed.ctypes.data + k * NLEV * NPROMA * B.REAL_BYTES, 8 * NLEV * NPROMA))
    yield "unequal tendency strides across the blocks", dict(prm=params(), xin=xin, outs=outs, replace=(1, strided), keep=packed)
    mixed = flat_block("out", o1)
    mixed.tenq = B.Field(packed.ctypes.data, 8 * NLEV * NPROMA)
    yield "unequal strides inside a group", dict(prm=params(), xin=xin, outs=outs, replace=(1, mixed), keep=packed)


@pytest.mark.parametrize("label, kw", list(einval_cases()), ids=[c[0] for c in einval_cases()])
def test_a_bad_call_is_einval_with_or_without_a_device(label, kw):
    kw = dict(kw)
    replace, _ = kw.pop("replace", None), kw.pop("keep", None)
    if replace is None:
        assert call(**kw) == B.CLOUDSC2_EINVAL, label
    else:
        blocks = (B.Outputs * 4)(*(flat_block("out", o) for o in kw["outs"]))
        blocks[replace[0]] = replace[1]
        assert B.lib.cloudsc2_tl_launch_parjac(C.byref(kw["prm"]), 3600.0, NPROMA, NLEV, N, C.byref(flat_block("in", kw["xin"])),
                                               blocks, None) == B.CLOUDSC2_EINVAL, label
    assert B.lib.cloudsc2_last_error()


@pytest.mark.parametrize("qsat", [True, False])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
def test_a_well_formed_call_without_a_device_is_enodevice(flags, qsat):
    """qsat NULL (SATUR in the sweep) and, without the evaporation branch, a NULL rpecons block are well-formed.  Where there is a
    device the same call would launch on these host arrays, so it is made only where there is none."""
    if B.lib.cloudsc2_device_available():
        return
    xin, outs = host_blocks(qsat)
    if not flags:
        outs[3] = {}
    assert call(params(**flags), xin, outs) == B.CLOUDSC2_ENODEVICE
    assert b"device" in B.lib.cloudsc2_last_error()


@pytest.mark.parametrize("bad, match", [
    ({"rlmin": p64()}, "unknown name"),
    ({"rkconv": p64(), "ptsphy": p64()}, "unknown name"),
    ({"rkconv": torch.tensor(1.0, dtype=torch.float32)}, "dtype"),
    ({"rkconv": torch.tensor(1)}, "dtype"),
    ({"rclcrit": torch.ones(1, dtype=torch.float64)}, "0-d"),
    ({"rclcrit": torch.ones(2, 2, dtype=torch.float64)}, "0-d"),
    ({"rlptrc": 250.0}, "not a tensor"),
    ([("rkconv", p64())], "must map"),
])
def test_bad_params_are_refused_on_cpu_tensors(bad, match):
    with pytest.raises(ValueError, match=match):
        c2.param_jacobian(inputs("cpu"), params(), 3600.0, params=bad)


def test_lphylin_off_is_refused():
    prm = params()
    prm.lphylin = 0
    for p in (None, {"rkconv": p64()}):
        with pytest.raises(ValueError, match="lphylin"):
            c2.param_jacobian(inputs("cpu"), prm, 3600.0, params=p)


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_stop_at_the_device_check_after_the_layout_checks(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    for p in (None, {"rclcrit": p64()}):
        with pytest.raises(ValueError, match="HIP device"):
            c2.param_jacobian(x, params(), 3600.0, satur=satur, params=p)
    with pytest.raises(ValueError, match="names"):
        c2.param_jacobian({n: t for n, t in x.items() if n != "supsat"}, params(), 3600.0, satur=satur)
    with pytest.raises(ValueError, match="qsat"):
        c2.param_jacobian(inputs("cpu"), params(), 3600.0, satur=True)
