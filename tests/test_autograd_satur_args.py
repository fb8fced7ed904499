"""The differentiable op with SATUR inside (``cloudsc2(..., satur=True)``) and the differentiable ``satur``: what needs no device.
The layout checks take 15 names and refuse a ``qsat``; the default path behaves as before; CPU tensors stop at the device check;
the three new launchers answer CLOUDSC2_ENODEVICE where there is no GPU (and CLOUDSC2_EINVAL for a bad call where there is one)."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params, bad_cases
from tests.util import B
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag


def inputs15(device="cpu", **kw):
    x = inputs(device, **kw)
    del x["qsat"]
    return x


def test_the_names_of_the_fused_op():
    assert ag.SAT_NAMES == tuple(n for n in B.IN_NAMES if n != "qsat") and len(ag.SAT_NAMES) == 15
    assert "qsat" not in ag.SAT_GROUPS["full"] and set(sum(ag.SAT_GROUPS.values(), ())) == set(ag.SAT_NAMES)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_fifteen_names_pass_the_layout_checks(device):
    lay = ag.check_layout(inputs15(device), params(), satur=True)
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA) and lay.tail == NPROMA
    lay = ag.check_layout(inputs15(device), params(), ngptot=NB * NPROMA - 5, satur=True)
    assert lay.tail == NPROMA - 5


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_a_qsat_key_is_refused(device):
    with pytest.raises(ValueError, match="qsat"):
        ag.check_layout(inputs(device), params(), satur=True)
    with pytest.raises(ValueError, match="qsat"):
        ag.cloudsc2(inputs(device), params(), 3600.0, satur=True)
    with pytest.raises(ValueError, match="names"):  # and without satur=True the 15 names are not enough, as before
        ag.check_layout(inputs15(device), params())
    x = inputs15(device)
    del x["supsat"]
    with pytest.raises(ValueError, match="names"):
        ag.check_layout(x, params(), satur=True)


@pytest.mark.parametrize("case", [c[0] for c in bad_cases()])
def test_the_default_path_is_unchanged(case):
    """the cases of tests/test_autograd_args.py: satur=False given explicitly raises the very message of the default call"""
    _, x, prm, _ = next(c for c in bad_cases() if c[0] == case)
    ngptot = NB * NPROMA + 1 if case == "ngptot" else None
    with pytest.raises(ValueError) as default:
        ag.check_layout(x, prm, ngptot)
    with pytest.raises(ValueError) as explicit:
        ag.check_layout(x, prm, ngptot, satur=False)
    assert str(default.value) == str(explicit.value)
    with pytest.raises(ValueError) as op:
        ag.cloudsc2(x, prm, 3600.0, ngptot, satur=False)
    assert str(op.value) == str(default.value)
    if case not in ("missing name",) and "qsat" in x:  # the same refusal through the fused op's checks
        x15 = {n: t for n, t in x.items() if n != "qsat"}
        with pytest.raises(ValueError) as fused:
            ag.check_layout(x15, prm, ngptot, satur=True)
        assert str(fused.value) == str(default.value)


def test_cpu_tensors_stop_at_the_device_check():
    x = inputs15("cpu")
    ag.check_layout(x, params(), satur=True)
    with pytest.raises(ValueError, match="HIP device"):
        ag.cloudsc2(x, params(), 3600.0, satur=True)
    with pytest.raises(ValueError, match="HIP device"):
        ag.satur(x["pap"], x["t"], params(), differentiable=True)
    with pytest.raises(ValueError):
        ag.satur(x["pap"], x["t"][:, :-1], params(), differentiable=True)


def test_the_new_launchers_without_a_device():
    """no GPU: CLOUDSC2_ENODEVICE, like every launcher; with one, the same calls (NULL fields) are CLOUDSC2_EINVAL -- never a launch"""
    want = B.CLOUDSC2_EINVAL if B.lib.cloudsc2_device_available() else B.CLOUDSC2_ENODEVICE
    prm = params()
    i, o = B.Inputs(), B.Outputs()
    assert B.lib.cloudsc2_satur_lin_launch(C.byref(prm), NPROMA, NLEV, NB * NPROMA, B.Field(), B.Field(), B.Field(), B.Field(), B.Field(),
                                           None) == want
    assert B.lib.cloudsc2_tl_launch_satur(C.byref(prm), 3600.0, NPROMA, NLEV, NB * NPROMA, C.byref(i), C.byref(i), C.byref(o), None) == want
    assert B.lib.cloudsc2_vjp_launch_satur(C.byref(prm), 3600.0, NPROMA, NLEV, NB * NPROMA, C.byref(i), C.byref(o), C.byref(i), C.byref(o),
                                           None, None) == want
    assert B.lib.cloudsc2_last_error()


def test_header_map_and_binding_agree_on_the_new_symbols():
    for name in ("cloudsc2_satur_lin_launch", "cloudsc2_tl_launch_satur", "cloudsc2_vjp_launch_satur"):
        assert name in B.EXPORTED and hasattr(B.lib, name)
