"""The differentiable op (dwarf_p_cloudsc2_tl_ad_amd.autograd) refuses what the kernels cannot take with a ValueError before any
launch: its shape / stride / dtype checks are device-free (CPU and meta tensors), the device check is a step of its own."""
from __future__ import annotations

import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params, bad_cases
from tests.util import B
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag



@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_a_valid_call_passes_the_layout_checks(device):
    lay = ag.check_layout(inputs(device), params())
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA) and lay.tail == NPROMA
    lay = ag.check_layout(inputs(device), params(), ngptot=NB * NPROMA - 5)
    assert lay.tail == NPROMA - 5
    # planes of a packed buffer (block stride 8 planes) are accepted as they are
    buf = torch.ones((NB, 8, NLEV, NPROMA), dtype=B.torch_real(), device=device)
    x = inputs(device)
    for k, n in enumerate(("gtent", "gtenq", "gtenl", "gteni")):
        x[n] = buf[:, k]
    ag.check_layout(x, params())


@pytest.mark.parametrize("case", [c[0] for c in bad_cases()])
def test_bad_arguments_raise_before_any_launch(case):
    _, x, prm, msg = next(c for c in bad_cases() if c[0] == case)
    ngptot = NB * NPROMA + 1 if case == "ngptot" else None
    with pytest.raises(ValueError, match=msg):
        ag.check_layout(x, prm, ngptot)
    with pytest.raises(ValueError, match=msg):  # the op itself: the same error, no launch
        ag.cloudsc2(x, prm, 3600.0, ngptot)


def test_nlev_beyond_the_tables_is_refused_on_meta_tensors():
    with pytest.raises(ValueError, match="nlev"):
        ag.check_layout(inputs("meta", nlev=B.CLOUDSC2_MAX_NLEV + 1), params())


def test_cpu_tensors_are_refused_by_the_device_check():
    x = inputs("cpu")
    ag.check_layout(x, params())  # the layout is fine ...
    with pytest.raises(ValueError, match="HIP device"):
        ag.check_device(x.values())
    with pytest.raises(ValueError, match="HIP device"):  # ... and the op stops at the device check
        ag.cloudsc2(x, params(), 3600.0)
    with pytest.raises(ValueError):
        ag.satur(x["pap"], x["t"], params())


def test_normalize_copies_only_the_groups_that_do_not_fit():
    lay = ag.Layout(NB, NLEV, NPROMA, NB * NPROMA)
    x = inputs()
    buf = torch.zeros((NB, 8, NLEV, NPROMA), dtype=B.torch_real())
    for k, n in enumerate(("gtent", "gtenq", "gtenl", "gteni")):
        x[n] = buf[:, k]
    got = ag.normalize(x, lay, ag.IN_GROUPS)
    assert all(got[n] is x[n] for n in B.IN_NAMES)  # PGTEN* planes share one block stride: no copy
    x["gteni"] = x["gteni"].contiguous()  # one member with another block stride: the whole group is copied
    got = ag.normalize(x, lay, ag.IN_GROUPS)
    assert all(got[n].is_contiguous() and got[n] is not x[n] for n in ("gtent", "gtenq", "gtenl"))
    assert all(got[n] is x[n] for n in ag.IN_GROUPS["full"] + ag.IN_GROUPS["clv"] + ag.IN_GROUPS["half"])
    # a full-level plane of a packed buffer has a block stride the contiguous outputs cannot share: copied
    x["pap"] = buf[:, 5]
    got = ag.normalize(x, lay, ag.IN_GROUPS)
    assert got["pap"].is_contiguous() and got["pap"].stride(0) == NLEV * NPROMA
    # expanded (zero-strided) incoming gradients
    g = {n: torch.ones((), dtype=B.torch_real()).expand(lay.shape(n)) for n in B.OUT_NAMES}
    got = ag.normalize(g, lay, ag.OUT_GROUPS)
    assert all(got[n].is_contiguous() for n in B.OUT_NAMES)
