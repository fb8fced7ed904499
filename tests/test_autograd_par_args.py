"""``cloudsc2(..., params=...)``: what needs no device.  The parameter checks run on CPU tensors and raise ``ValueError``; CPU inputs
stop at the device check after them; the default path (``params=None``) is today's; the new launchers answer CLOUDSC2_ENODEVICE where
there is no GPU (CLOUDSC2_EINVAL for a bad call where there is one, and for a bad ``satur`` everywhere)."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag


def p64(v=1.0, **kw):
    return torch.tensor(v, dtype=torch.float64, **kw)


def test_the_names_and_their_order():
    assert c2.PARAM_NAMES == ag.PARAM_NAMES == B.PARAM_NAMES == ("rkconv", "rclcrit", "rlptrc", "rpecons")
    assert all(hasattr(params(), n) for n in c2.PARAM_NAMES)


def test_any_subset_passes_and_comes_back_in_order():
    prm = params()
    assert ag.check_params({}, prm) == ()
    assert ag.check_params({"rpecons": p64(), "rkconv": p64(requires_grad=True)}, prm) == ("rkconv", "rpecons")
    assert ag.check_params({n: p64() for n in reversed(c2.PARAM_NAMES)}, prm) == c2.PARAM_NAMES


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
        ag.check_params(bad, params())
    with pytest.raises(ValueError, match=match):  # through the op: before the device check
        ag.cloudsc2(inputs("cpu"), params(), 3600.0, params=bad)


def test_params_with_lphylin_off_are_refused():
    prm = params()
    prm.lphylin = 0
    with pytest.raises(ValueError, match="lphylin"):
        ag.check_params({"rkconv": p64()}, prm)
    with pytest.raises(ValueError, match="lphylin"):
        ag.cloudsc2(inputs("cpu"), prm, 3600.0, params={"rkconv": p64()})


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_stop_at_the_device_check(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    with pytest.raises(ValueError, match="HIP device"):
        ag.cloudsc2(x, params(), 3600.0, satur=satur, params={"rkconv": p64(requires_grad=True)})
    with pytest.raises(ValueError, match="names"):  # the layout checks come first, as without params
        ag.cloudsc2({n: t for n, t in x.items() if n != "supsat"}, params(), 3600.0, satur=satur, params={"rkconv": p64()})


def test_the_default_is_no_params():
    with pytest.raises(ValueError) as a:
        ag.cloudsc2(inputs("cpu"), params(), 3600.0)
    with pytest.raises(ValueError) as b:
        ag.cloudsc2(inputs("cpu"), params(), 3600.0, params=None)
    assert str(a.value) == str(b.value) and "HIP device" in str(a.value)


def test_the_workspace_size():
    n = C.c_longlong(-1)
    assert B.lib.cloudsc2_par_work_doubles(128, 160000, C.byref(n)) == 0 and n.value == 4 * 160000
    assert B.lib.cloudsc2_par_work_doubles(16, 30, C.byref(n)) == 0 and n.value == 4 * 32
    assert B.lib.cloudsc2_par_work_doubles(0, 30, C.byref(n)) == B.CLOUDSC2_EINVAL
    assert B.lib.cloudsc2_par_work_doubles(16, 30, None) == B.CLOUDSC2_EINVAL


def test_the_new_launchers_without_a_device():
    """no GPU: CLOUDSC2_ENODEVICE, like every launcher; with one, the same calls (NULL fields) are CLOUDSC2_EINVAL -- never a launch.
    A satur that is neither 0 nor 1 is CLOUDSC2_EINVAL everywhere."""
    want = B.CLOUDSC2_EINVAL if B.lib.cloudsc2_device_available() else B.CLOUDSC2_ENODEVICE
    prm = params()
    i, o = B.Inputs(), B.Outputs()
    dpar = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    n = NB * NPROMA
    for satur in (0, 1):
        assert B.lib.cloudsc2_tl_launch_par(C.byref(prm), 3600.0, NPROMA, NLEV, n, satur, C.byref(i), C.byref(i), dpar, C.byref(o), None) == want
        assert B.lib.cloudsc2_vjp_launch_par(C.byref(prm), 3600.0, NPROMA, NLEV, n, satur, C.byref(i), C.byref(o), C.byref(i), C.byref(o),
                                             None, None, None, None) == want
        assert B.lib.cloudsc2_last_error()
    for satur in (-1, 2):
        assert B.lib.cloudsc2_tl_launch_par(C.byref(prm), 3600.0, NPROMA, NLEV, n, satur, C.byref(i), C.byref(i), dpar, C.byref(o),
                                            None) == B.CLOUDSC2_EINVAL
        assert B.lib.cloudsc2_vjp_launch_par(C.byref(prm), 3600.0, NPROMA, NLEV, n, satur, C.byref(i), C.byref(o), C.byref(i), C.byref(o),
                                             None, None, None, None) == B.CLOUDSC2_EINVAL


def test_header_and_binding_agree_on_the_new_symbols():
    for name in ("cloudsc2_par_work_doubles", "cloudsc2_tl_launch_par", "cloudsc2_vjp_launch_par"):
        assert name in B.EXPORTED and hasattr(B.lib, name)
