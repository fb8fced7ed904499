"""``cloudsc2_ensemble``: what needs no device.  ``check_ensemble`` runs on CPU tensors and raises ``ValueError`` for everything wrong
with the call itself; CPU inputs stop at the device check after it; the workspace query is host arithmetic; the launchers answer
CLOUDSC2_ENODEVICE where there is no GPU and CLOUDSC2_EINVAL for a bad call where there is one."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from tests.gpu_util import (ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, K, arg_inputs as inputs, arg_params as params, bad_params,
                            four_d, pk)
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag



def test_the_entry_points_are_exported():
    assert c2.cloudsc2_ensemble is ag.cloudsc2_ensemble and c2.check_ensemble is ag.check_ensemble


def test_a_valid_call_passes_and_reports_layout_members_and_names():
    prm = params()
    lay, k, names = ag.check_ensemble(inputs(), prm, None, False, {"rpecons": pk(), "rkconv": pk(requires_grad=True)})
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA) and k == K and names == ("rkconv", "rpecons")
    # one member; every name; a padded tail; per-member inputs next to shared ones, any member stride
    assert ag.check_ensemble(inputs(), prm, NB * NPROMA - 5, False, {n: pk(1) for n in c2.PARAM_NAMES})[1:] == (1, c2.PARAM_NAMES)
    x = inputs()
    x["t"] = four_d(x["t"])
    x["paph"] = four_d(x["paph"]).expand(K, -1, -1, -1)
    x["q"] = torch.ones((K, 2, NB, NLEV, NPROMA), dtype=B.torch_real())[:, 1]
    assert ag.check_ensemble(x, prm, None, False, {"rclcrit": pk()})[0].ngptot == NB * NPROMA
    del x["qsat"]
    assert ag.check_ensemble(x, prm, None, True, {"rclcrit": pk()})[1] == K


@pytest.mark.parametrize("bad, match", list(bad_params()))
def test_bad_params_are_refused_on_cpu_tensors(bad, match):
    with pytest.raises(ValueError, match=match):
        ag.check_ensemble(inputs(), params(), None, False, bad)
    with pytest.raises(ValueError, match=match):  # through the op: before the device check
        ag.cloudsc2_ensemble(inputs("cpu"), params(), 3600.0, params=bad)


def test_bad_inputs_are_refused_on_cpu_tensors():
    prm, p = params(), {"rkconv": pk()}
    x = inputs()
    x["t"] = four_d(x["t"], K + 1)
    with pytest.raises(ValueError, match="leading size"):
        ag.check_ensemble(x, prm, None, False, p)
    x = inputs()
    x["t"] = x["t"][0]
    with pytest.raises(ValueError, match="3-D .* or 4-D"):
        ag.check_ensemble(x, prm, None, False, p)
    with pytest.raises(ValueError, match="qsat"):  # qsat given with satur=True
        ag.check_ensemble(inputs(), prm, None, True, p)
    with pytest.raises(ValueError, match="names"):
        ag.check_ensemble({n: t for n, t in inputs().items() if n != "supsat"}, prm, None, False, p)
    # the layout rules of the single op hold for every member: shape, in-block strides, ngptot, nlev
    x = inputs()
    x["q"] = four_d(torch.ones((NB, NLEV - 1, NPROMA), dtype=B.torch_real()))
    with pytest.raises(ValueError, match="shape"):
        ag.check_ensemble(x, prm, None, False, p)
    x = inputs()
    x["mfu"] = torch.ones((K, NB, NPROMA, NLEV), dtype=B.torch_real()).transpose(2, 3)
    with pytest.raises(ValueError, match="column stride"):
        ag.check_ensemble(x, prm, None, False, p)
    with pytest.raises(ValueError, match="ngptot"):
        ag.check_ensemble(inputs(), prm, NB * NPROMA + 1, False, p)
    with pytest.raises(ValueError, match="prm.nlev"):
        ag.check_ensemble(inputs(), params(NLEV - 1), None, False, p)
    off = params()
    off.lphylin = 0
    with pytest.raises(ValueError, match="lphylin"):
        ag.check_ensemble(inputs(), off, None, False, p)


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_stop_at_the_device_check(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    with pytest.raises(ValueError, match="HIP device"):
        ag.cloudsc2_ensemble(x, params(), 3600.0, satur=satur, params={"rkconv": pk(requires_grad=True)})


def test_the_workspace_size():
    """K argument blocks (rounded up to 256 bytes) and K x 4 x the padded column count doubles"""
    f = B.lib.cloudsc2_ens_workspace_bytes
    sums = lambda k, ncols_pad: k * 4 * ncols_pad * 8  # noqa: E731
    one = f(1, 24, 137, 70) - sums(1, 72)
    assert 0 < one <= 4096 and one % 256 == 0  # (an argument block fits the 4 KiB of a kernel-argument segment)
    for k in (1, 3, 8, 65535):
        blocks = f(k, 24, 137, 70) - sums(k, 72)
        assert blocks % 256 == 0 and k * (one - 255) <= blocks <= k * one  # (the blocks are packed, their sum rounded up)
        assert f(k, 64, 137, 200) - sums(k, 256) == blocks and f(k, 128, 137, 160000) - sums(k, 160000) == blocks
    for bad in ((0, 24, 137, 70), (65536, 24, 137, 70), (3, 0, 137, 70), (3, 24, 1, 70), (3, 24, B.CLOUDSC2_MAX_NLEV + 1, 70), (3, 24, 137, 0)):
        assert f(*bad) == B.CLOUDSC2_EINVAL, bad
    assert B.lib.cloudsc2_last_error()


def test_the_new_launchers_without_a_device():
    """no GPU: CLOUDSC2_ENODEVICE, like every launcher; with one, the same calls (NULL fields) are CLOUDSC2_EINVAL -- never a launch.
    Members out of range, a missing parameter array or workspace and a bad satur are CLOUDSC2_EINVAL everywhere."""
    want = B.CLOUDSC2_EINVAL if B.lib.cloudsc2_device_available() else B.CLOUDSC2_ENODEVICE
    prm = params()
    i, o = B.Inputs(), B.Outputs()
    n = NB * NPROMA
    dummy = C.c_void_p(256)  # (never dereferenced: device pointers the kernels alone would read)
    lib = B.lib

    def nl(members=K, par=dummy, work=dummy):
        return lib.cloudsc2_nl_launch_ens(C.byref(prm), 3600.0, NPROMA, NLEV, n, members, par, C.byref(i), None, C.byref(o), None, None, 0, work, None)

    def tl(members=K, par=dummy, work=dummy, satur=0):
        return lib.cloudsc2_tl_launch_ens(C.byref(prm), 3600.0, NPROMA, NLEV, n, satur, members, par, dummy, C.byref(i), None, C.byref(i), None,
                                          C.byref(o), None, work, None)

    def vjp(members=K, par=dummy, work=dummy, satur=0):
        return lib.cloudsc2_vjp_launch_ens(C.byref(prm), 3600.0, NPROMA, NLEV, n, satur, members, par, C.byref(i), None, C.byref(o), None,
                                           C.byref(i), None, C.byref(o), None, None, 0, work, dummy, None)

    for call in (nl, tl, vjp):
        assert call() == want, call.__name__
        assert lib.cloudsc2_last_error()
        assert call(members=0) == B.CLOUDSC2_EINVAL and call(members=65536) == B.CLOUDSC2_EINVAL, call.__name__
        assert call(par=None) == B.CLOUDSC2_EINVAL and call(work=None) == B.CLOUDSC2_EINVAL, call.__name__
    # a field the members write must not be shared by more than one member: refused with or without a device
    shared_out = B.Outputs()
    shared_out.tent.ptr = 256
    assert lib.cloudsc2_nl_launch_ens(C.byref(prm), 3600.0, NPROMA, NLEV, n, K, dummy, C.byref(i), None, C.byref(shared_out), None, None, 0,
                                      dummy, None) == B.CLOUDSC2_EINVAL
    assert b"member stride 0" in lib.cloudsc2_last_error()
    assert lib.cloudsc2_nl_launch_ens(C.byref(prm), 3600.0, NPROMA, NLEV, n, 1, dummy, C.byref(i), None, C.byref(shared_out), None, None, 0,
                                      dummy, None) == want  # (one member shares with nobody)
    for call in (tl, vjp):
        assert call(satur=1) == want and call(satur=2) == B.CLOUDSC2_EINVAL and call(satur=-1) == B.CLOUDSC2_EINVAL, call.__name__


def test_header_and_binding_agree_on_the_new_symbols():
    for name in ("cloudsc2_ens_workspace_bytes", "cloudsc2_nl_launch_ens", "cloudsc2_tl_launch_ens", "cloudsc2_vjp_launch_ens"):
        assert name in B.EXPORTED and hasattr(B.lib, name)


def test_the_sweep_families_are_unchanged():
    """the ensemble kernels are no sweep family: no family number, nothing in the launch log"""
    assert len(B.FAMILIES) == 10 and not any("ens" in f for f in B.FAMILIES)
