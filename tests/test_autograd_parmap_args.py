"""``cloudsc2_param_maps``: what needs no device.  ``check_param_maps`` runs on CPU tensors and raises ``ValueError`` for everything
wrong with the call itself; CPU inputs stop at the device check after it."""
from __future__ import annotations

import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag


def pmap(shape=(NB, NPROMA), dtype=torch.float64, **kw):
    return torch.linspace(1.0, 2.0, int(torch.tensor(shape).prod()) if shape else 1, dtype=torch.float64).reshape(shape).to(dtype).requires_grad_(
        kw.get("requires_grad", False))


def test_the_entry_points_are_exported():
    assert c2.cloudsc2_param_maps is ag.cloudsc2_param_maps and c2.check_param_maps is ag.check_param_maps
    for name in ("cloudsc2_nl_launch_parmap", "cloudsc2_tl_launch_parmap", "cloudsc2_vjp_launch_parmap"):
        assert name in B.EXPORTED and hasattr(B.lib, name)


def test_a_valid_call_passes_and_reports_layout_and_names():
    prm = params()
    lay, names = ag.check_param_maps(inputs(), prm, None, False, {"rpecons": pmap(), "rkconv": pmap(requires_grad=True)})
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA) and names == ("rkconv", "rpecons")
    # every name; a padded tail; SATUR in the op
    assert ag.check_param_maps(inputs(), prm, NB * NPROMA - 5, False, {n: pmap() for n in c2.PARAM_NAMES})[1] == c2.PARAM_NAMES
    x = inputs()
    del x["qsat"]
    assert ag.check_param_maps(x, prm, None, True, {"rclcrit": pmap()})[0].ngptot == NB * NPROMA


BAD = [({}, "empty"),
       (None, "must map"),
       ({"rlmin": pmap()}, "unknown name"),
       ({"rkconv": pmap(), "ptsphy": pmap()}, "unknown name"),
       ({"rkconv": 1.0e-4}, "not a tensor"),
       ({"rkconv": pmap(())}, r"cloudsc2\(\.\.\., params=.*cloudsc2_ensemble"),      # 0-d: the scalar op's form
       ({"rkconv": pmap((3,))}, r"cloudsc2\(\.\.\., params=.*cloudsc2_ensemble"),    # (K,): the ensemble's form
       ({"rkconv": pmap(dtype=torch.float32)}, "dtype"),
       ({"rkconv": pmap(), "rclcrit": pmap(dtype=torch.float32)}, "dtype"),
       ({"rkconv": pmap((NB, NPROMA + 1))}, "shape"),
       ({"rkconv": pmap((NPROMA, NB))}, "shape"),
       ({"rkconv": pmap((1, NB, NPROMA))}, "shape")]


@pytest.mark.parametrize("bad, match", BAD, ids=[m[:24] + f"-{i}" for i, (_, m) in enumerate(BAD)])
def test_bad_params_are_refused_on_cpu_tensors(bad, match):
    with pytest.raises(ValueError, match=match):
        ag.check_param_maps(inputs(), params(), None, False, bad)
    with pytest.raises(ValueError, match=match):  # through the op: before the device check
        ag.cloudsc2_param_maps(inputs("cpu"), params(), 3600.0, params=bad)


def test_bad_inputs_are_refused_on_cpu_tensors():
    prm, p = params(), {"rkconv": pmap()}
    with pytest.raises(ValueError, match="qsat"):  # qsat given with satur=True
        ag.check_param_maps(inputs(), prm, None, True, p)
    with pytest.raises(ValueError, match="names"):
        ag.check_param_maps({n: t for n, t in inputs().items() if n != "supsat"}, prm, None, False, p)
    x = inputs()
    x["q"] = torch.ones((NB, NLEV - 1, NPROMA), dtype=B.torch_real())
    with pytest.raises(ValueError, match="shape"):
        ag.check_param_maps(x, prm, None, False, p)
    with pytest.raises(ValueError, match="ngptot"):
        ag.check_param_maps(inputs(), prm, NB * NPROMA + 1, False, p)
    with pytest.raises(ValueError, match="prm.nlev"):
        ag.check_param_maps(inputs(), params(NLEV - 1), None, False, p)
    off = params()
    off.lphylin = 0
    with pytest.raises(ValueError, match="lphylin"):
        ag.check_param_maps(inputs(), off, None, False, p)


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_stop_at_the_device_check(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    with pytest.raises(ValueError, match="HIP device"):
        ag.cloudsc2_param_maps(x, params(), 3600.0, satur=satur, params={"rkconv": pmap(requires_grad=True)})
