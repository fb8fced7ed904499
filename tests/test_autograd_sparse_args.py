"""``cloudsc2(..., sparse=True)``: what needs no device.  ``sparse`` with ``params`` raises; ``sparse=False`` (and the default) reaches
the Function classes of today and ``sparse=True`` the new one, with the same operands; the layout checks are the same function with
the same messages; CPU tensors stop at the device check; the two new launchers are declared, exported and bound."""
from __future__ import annotations

import inspect

import pytest
import torch

from tests.gpu_util import ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, arg_inputs as inputs, arg_params as params, bad_cases
from tests.util import B
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag


def inputs15(device="cpu"):
    x = inputs(device)
    del x["qsat"]
    return x


def test_sparse_with_params_raises_before_anything_else():
    p = {"rkconv": torch.tensor(1e-4, dtype=torch.float64)}
    for satur, x in ((False, inputs("cpu")), (True, inputs15("cpu"))):
        with pytest.raises(NotImplementedError, match="sparse=True with params"):
            ag.cloudsc2(x, params(), 3600.0, satur=satur, params=p, sparse=True)
    with pytest.raises(NotImplementedError):  # (before the layout checks: not even the inputs are looked at)
        ag.cloudsc2({}, params(), 3600.0, params=p, sparse=True)


def test_the_signature():
    sig = inspect.signature(ag.cloudsc2)
    assert list(sig.parameters) == ["inputs", "prm", "ptsphy", "ngptot", "satur", "params", "sparse"]
    assert sig.parameters["sparse"].default is False
    for fn in (ag.cloudsc2_ensemble, ag.param_jacobian, ag.param_normal_equations):  # unchanged: no sparse form
        assert "sparse" not in inspect.signature(fn).parameters


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
def test_which_function_class_the_op_builds(monkeypatch, satur):
    """the op with the device steps stubbed out: sparse=False and the default apply today's class, sparse=True the new one, each
    with the normalized inputs in the order of the names"""
    calls = []

    def recorder(cls):
        def apply(*args):
            calls.append((cls, args))
            return tuple(range(11))
        return apply
    for cls in (ag._Cloudsc2, ag._Cloudsc2Sparse):
        monkeypatch.setattr(cls, "apply", recorder(cls))
    monkeypatch.setattr(ag, "check_device", lambda ts: torch.device("cpu"))
    monkeypatch.setattr(ag, "_prepare", lambda dev: None)
    x = inputs15() if satur else inputs()
    names = ag.SAT_NAMES if satur else B.IN_NAMES
    prm = params()
    for kw in (dict(), dict(sparse=False)):
        calls.clear()
        out = ag.cloudsc2(x, prm, 3600.0, satur=satur, **kw)
        assert isinstance(out, ag.Cloudsc2Outputs) and tuple(out) == tuple(range(10))
        (cls, args), = calls
        assert cls is ag._Cloudsc2 and args[0] is prm and args[1] == 3600.0 and args[3] is satur and len(args) == 4 + len(names)
        assert all(a is x[n] for a, n in zip(args[4:], names))
    calls.clear()
    out = ag.cloudsc2(x, prm, 3600.0, satur=satur, sparse=True)
    assert tuple(out) == tuple(range(10))
    (cls, args), = calls
    assert cls is ag._Cloudsc2Sparse and args[3] is satur and len(args) == 4 + len(names)
    assert all(a is x[n] for a, n in zip(args[4:], names))


@pytest.mark.parametrize("case", [c[0] for c in bad_cases()])
def test_check_layout_is_unchanged(case):
    """the cases of tests/test_autograd_args.py: the sparse op raises the very message of check_layout and of the dense op"""
    _, x, prm, _ = next(c for c in bad_cases() if c[0] == case)
    ngptot = NB * NPROMA + 1 if case == "ngptot" else None
    with pytest.raises(ValueError) as layout:
        ag.check_layout(x, prm, ngptot)
    with pytest.raises(ValueError) as dense:
        ag.cloudsc2(x, prm, 3600.0, ngptot)
    with pytest.raises(ValueError) as sparse:
        ag.cloudsc2(x, prm, 3600.0, ngptot, sparse=True)
    assert str(layout.value) == str(dense.value) == str(sparse.value)


def test_cpu_tensors_stop_at_the_device_check():
    assert list(inspect.signature(ag.check_layout).parameters) == ["inputs", "prm", "ngptot", "satur"]
    lay = ag.check_layout(inputs("cpu"), params())
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA)
    for satur, x in ((False, inputs("cpu")), (True, inputs15("cpu"))):
        with pytest.raises(ValueError, match="HIP device"):
            ag.cloudsc2(x, params(), 3600.0, satur=satur, sparse=True)


def test_header_binding_and_library_agree_on_the_new_symbols():
    for name in ("cloudsc2_tl_launch_sparse", "cloudsc2_vjp_launch_sparse"):
        assert name in B.EXPORTED and hasattr(B.lib, name)
    assert len(B.FAMILIES) == 10 and not any("sparse" in f for f in B.FAMILIES)  # not sweep families
    assert len(B.lib.cloudsc2_tl_launch_sparse.argtypes) == 10 and len(B.lib.cloudsc2_vjp_launch_sparse.argtypes) == 12
