"""``c2.param_jacobian_column_sums`` / ``c2.param_normal_equations_column_sums``: what needs no device.  ``check_sum_residual`` raises
``ValueError`` on CPU tensors, ``level_weights`` obeys ``check_weights``, and both entry points reach the device check only after every
other check.  (What the two launchers refuse is pinned in tests/test_parcolsum_refusals.py.)"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params
from tests.util import B, ROOT, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

N = NB * NPROMA
LAY = ag.Layout(NB, NLEV, NPROMA, N)
SUMS = ("tent", "fplsl", "fplsn")
OBS = ("tent", "fplsl")


def test_header_binding_and_package_agree_on_the_new_symbols():
    for name in ("cloudsc2_parjac_launch_colsum", "cloudsc2_parnormal_launch_colsum"):
        assert name in B.EXPORTED and hasattr(B.lib, name)
    with open(os.path.join(ROOT, "include", "cloudsc2_hip.h")) as f:
        header = f.read()
    assert "int cloudsc2_parjac_launch_colsum(" in header and "int cloudsc2_parnormal_launch_colsum(" in header
    assert c2.param_jacobian_column_sums is ag.param_jacobian_column_sums
    assert c2.param_normal_equations_column_sums is ag.param_normal_equations_column_sums
    assert c2.check_sum_residual is ag.check_sum_residual
    assert len(B.FAMILIES) == 10 and not any("colsum" in f for f in B.FAMILIES)  # not a sweep family


def level_weights(names=SUMS, dtype=None):
    return {n: torch.ones(LAY.nlevx(n), dtype=dtype or B.torch_real()) for n in names}


def tensors(names, dtype=None, shape=(NB, NPROMA)):
    return {n: torch.ones(shape, dtype=dtype or B.torch_real()) for n in names}


def bad_residuals():
    other = torch.float32 if not B.SINGLE else torch.float64
    yield "unknown name", dict(residual={**tensors(OBS), "rain": torch.ones(1)}, weights=None), "unknown name"
    yield "unknown weight name", dict(residual=tensors(OBS), weights={"rain": torch.ones(1)}), "unknown name"
    yield "empty mapping", dict(residual={}, weights=None), "empty"
    yield "not a mapping", dict(residual=[("tent", torch.ones(1))], weights=None), "must map"
    yield "None", dict(residual=None, weights=None), "must map"
    yield "weights not a mapping", dict(residual=tensors(OBS), weights=torch.ones(1)), "must map"
    yield "a residual without level weights", dict(residual=tensors(("tent", "tenq")), weights=None), "no level weights"
    yield "weight for an unobserved name", dict(residual=tensors(OBS), weights=tensors(("fplsn",))), "not observed"
    yield "a plane instead of a sum", dict(residual={"tent": torch.ones(LAY.shape("tent"), dtype=B.torch_real())}, weights=None), "shape"
    yield "wrong weight shape", dict(residual=tensors(OBS), weights=tensors(("tent",), shape=(NB, NPROMA + 1))), "shape"
    yield "wrong dtype", dict(residual=tensors(OBS, dtype=other), weights=None), "dtype"
    yield "wrong weight dtype", dict(residual=tensors(OBS), weights=tensors(("tent",), dtype=other)), "dtype"
    yield "not a tensor", dict(residual={"tent": np.ones((NB, NPROMA))}, weights=None), "not a tensor"
    yield "weight not a tensor", dict(residual=tensors(OBS), weights={"tent": 1.0}), "not a tensor"


@pytest.mark.parametrize("label, kw, match", list(bad_residuals()), ids=[c[0] for c in bad_residuals()])
def test_check_sum_residual_refuses(label, kw, match):
    with pytest.raises(ValueError, match=match):
        ag.check_sum_residual(kw["residual"], kw["weights"], SUMS, LAY)
    with pytest.raises(ValueError, match=match):  # ... and the entry point raises the same before it looks at the device
        c2.param_normal_equations_column_sums(inputs("cpu"), params(), 3600.0, level_weights=level_weights(), residual=kw["residual"],
                                              weights=kw["weights"])


def test_check_sum_residual_returns_the_names_in_output_order():
    r, w = ag.check_sum_residual(tensors(("fplsn", "tent", "fplsl")), tensors(("fplsl",)), SUMS, LAY)
    assert tuple(r) == ("tent", "fplsl", "fplsn") and tuple(w) == ("fplsl",)
    r, w = ag.check_sum_residual(tensors(("fplsl",)), None, SUMS, LAY)
    assert tuple(r) == ("fplsl",) and w == {}


def bad_level_weights():
    other = torch.float32 if not B.SINGLE else torch.float64
    yield "None", None, "must map"
    yield "empty", {}, "empty"
    yield "unknown name", {"rain": torch.ones(NLEV)}, "unknown name"
    yield "not a tensor", {"tent": [1.0] * NLEV}, "not a tensor"
    yield "two-dimensional", {"tent": torch.ones((NLEV, 1), dtype=B.torch_real())}, "1-D"
    yield "full-level length for a flux", {"fplsl": torch.ones(NLEV, dtype=B.torch_real())}, "length"
    yield "wrong dtype", level_weights(dtype=other), "dtype"
    yield "requires grad", {"tent": torch.ones(NLEV, dtype=B.torch_real(), requires_grad=True)}, "requires grad"


@pytest.mark.parametrize("label, lw, match", list(bad_level_weights()), ids=[c[0] for c in bad_level_weights()])
def test_level_weights_obey_check_weights_in_both_entry_points(label, lw, match):
    with pytest.raises(ValueError, match=match):
        c2.param_jacobian_column_sums(inputs("cpu"), params(), 3600.0, level_weights=lw)
    with pytest.raises(ValueError, match=match):
        c2.param_normal_equations_column_sums(inputs("cpu"), params(), 3600.0, level_weights=lw, residual=tensors(("tent",)))


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_are_refused_as_no_cpu_path_after_every_other_check(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    p64 = torch.tensor(1.0, dtype=torch.float64)
    lw = level_weights()
    calls = (lambda xx, prm, **kw: c2.param_jacobian_column_sums(xx, prm, 3600.0, level_weights=lw, satur=satur, **kw),
             lambda xx, prm, **kw: c2.param_normal_equations_column_sums(xx, prm, 3600.0, level_weights=lw, residual=tensors(OBS),
                                                                         weights=tensors(("tent",)), satur=satur, **kw))
    for call in calls:
        for p in (None, {"rclcrit": p64}):
            with pytest.raises(ValueError, match="no CPU path"):
                call(x, params(), params=p)
        with pytest.raises(ValueError, match="names"):
            call({n: t for n, t in x.items() if n != "supsat"}, params())
        with pytest.raises(ValueError, match="unknown name"):
            call(x, params(), params={"rlmin": p64})
        prm = params()
        prm.lphylin = 0
        with pytest.raises(ValueError, match="lphylin"):
            call(x, prm)
