"""``cloudsc2_column_sums``: what needs no device.  Every ``ValueError`` of ``check_column_sums`` on CPU and meta tensors, each naming the
offending key; the layout checks are ``check_layout``'s with its messages; a CPU call stops at the device check the way ``cloudsc2``
does; the ``lphylin = 0`` refusal is the same; the op is re-exported and the three launchers are declared, exported and bound."""
from __future__ import annotations

import inspect

import pytest
import torch

import dwarf_p_cloudsc2_tl_ad_amd as c2
from tests.gpu_util import (ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params, bad_cases,
                            bad_weights, weights)
from tests.util import B
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

REAL = B.torch_real()
OTHER = torch.float32 if not B.SINGLE else torch.float64


def inputs15(device="cpu"):
    x = inputs(device)
    del x["qsat"]
    return x


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_a_valid_call_passes(device):
    lay, names = ag.check_column_sums(inputs(device), params(), None, False, weights(device, ("tent", "fplsl", "covptot")))
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA) and names == ("tent", "fplsl", "covptot")  # (the order of OUT_NAMES)
    lay, names = ag.check_column_sums(inputs15(device), params(), NB * NPROMA - 5, True, weights(device, B.OUT_NAMES))
    assert lay.tail == NPROMA - 5 and names == tuple(B.OUT_NAMES)
    w = weights(device, ("fplsn",))
    w["fplsn"] = torch.ones(2 * (NLEV + 1), dtype=REAL, device=device)[::2]  # any stride
    assert ag.check_column_sums(inputs(device), params(), None, False, w)[1] == ("fplsn",)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_every_weight_check_raises_and_names_the_key(device):
    seen = 0
    for name, w, text in bad_weights(device):
        with pytest.raises(ValueError) as e:
            ag.check_column_sums(inputs(device), params(), None, False, w)
        assert text in str(e.value), (name, str(e.value))
        with pytest.raises(ValueError) as e2:  # the op raises the same, before any device is asked for
            ag.cloudsc2_column_sums(inputs(device), params(), 3600.0, weights=w)
        assert str(e2.value) == str(e.value), name
        seen += 1
    assert seen >= 9


@pytest.mark.parametrize("case", [c[0] for c in bad_cases()])
def test_check_layout_is_unchanged(case):
    """the cases of tests/test_autograd_args.py: the op raises the very message of check_layout and of cloudsc2 (lphylin = 0 among them)"""
    _, x, prm, _ = next(c for c in bad_cases() if c[0] == case)
    ngptot = NB * NPROMA + 1 if case == "ngptot" else None
    with pytest.raises(ValueError) as layout:
        ag.check_layout(x, prm, ngptot)
    with pytest.raises(ValueError) as sums:
        ag.cloudsc2_column_sums(x, prm, 3600.0, ngptot, weights=weights())
    assert str(layout.value) == str(sums.value)


def test_lphylin_0_and_qsat_with_satur_are_refused_like_cloudsc2():
    prm = params()
    prm.lphylin = 0
    with pytest.raises(ValueError, match="lphylin = 0") as e:
        ag.cloudsc2_column_sums(inputs(), prm, 3600.0, weights=weights())
    with pytest.raises(ValueError) as dense:
        ag.cloudsc2(inputs(), prm, 3600.0)
    assert str(e.value) == str(dense.value)
    with pytest.raises(ValueError, match="must not have a 'qsat'"):
        ag.cloudsc2_column_sums(inputs(), params(), 3600.0, weights=weights(), satur=True)


def test_cpu_tensors_stop_at_the_device_check():
    for satur, x in ((False, inputs("cpu")), (True, inputs15("cpu"))):
        with pytest.raises(ValueError, match="HIP device") as e:
            ag.cloudsc2_column_sums(x, params(), 3600.0, weights=weights(), satur=satur)
        with pytest.raises(ValueError, match="HIP device") as dense:
            ag.cloudsc2(x, params(), 3600.0, satur=satur)
        assert str(e.value) == str(dense.value)


def test_the_signature_and_the_exports():
    sig = inspect.signature(ag.cloudsc2_column_sums)
    assert list(sig.parameters) == ["inputs", "prm", "ptsphy", "ngptot", "weights", "satur"]
    assert sig.parameters["satur"].default is False and sig.parameters["ngptot"].default is None
    assert list(inspect.signature(ag.check_column_sums).parameters) == ["inputs", "prm", "ngptot", "satur", "weights"]
    assert c2.cloudsc2_column_sums is ag.cloudsc2_column_sums and c2.check_column_sums is ag.check_column_sums
    for name in ("cloudsc2_nl_launch_colsum", "cloudsc2_tl_launch_colsum", "cloudsc2_vjp_launch_colsum"):
        assert name in B.EXPORTED and hasattr(B.lib, name)
    assert [len(getattr(B.lib, f"cloudsc2_{k}_launch_colsum").argtypes) for k in ("nl", "tl", "vjp")] == [11, 11, 13]
