"""``cloudsc2_ensemble_column_sums``: what needs no device.  Its device-free checks are ``check_ensemble`` followed by the weight checks
of ``check_column_sums``, so every ``ValueError`` of the two parents is raised with the parent's own message, on CPU and meta tensors,
before any device is asked for; ``vmap`` and a second differentiation raise ``NotImplementedError`` from the Functions themselves.  The op
is re-exported; the three launchers are declared, exported and bound, and refuse what their parents refuse -- a NULL block, a NULL weight
table, no sum, ``members < 1``, a written field the members share -- before the device is looked for, naming themselves."""
from __future__ import annotations

import ctypes as C
import inspect
import os

import pytest
import torch

import dwarf_p_cloudsc2_tl_ad_amd as c2
from tests.gpu_util import (ARG_NB as NB, ARG_NLEV as NLEV, ARG_NPROMA as NPROMA, K, R_NGPTOT as G_NGPTOT, R_NLEV as G_NLEV,
                            R_NPROMA as G_NPROMA, SumWorld, arg_inputs as inputs, arg_params as params, bad_params, bad_weights, four_d, pk,
                            refusal_params as abi_params, weights)
from tests.util import ROOT, B
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

EINVAL = B.CLOUDSC2_EINVAL
NL, TL, VJP = "cloudsc2_nl_launch_ens_colsum", "cloudsc2_tl_launch_ens_colsum", "cloudsc2_vjp_launch_ens_colsum"


def test_the_signature_and_the_exports():
    sig = inspect.signature(ag.cloudsc2_ensemble_column_sums)
    assert list(sig.parameters) == ["inputs", "prm", "ptsphy", "ngptot", "weights", "params", "satur"]
    assert sig.parameters["satur"].default is False and sig.parameters["ngptot"].default is None
    assert c2.cloudsc2_ensemble_column_sums is ag.cloudsc2_ensemble_column_sums
    assert c2.check_ensemble_column_sums is ag.check_ensemble_column_sums
    for name in (NL, TL, VJP):
        assert name in B.EXPORTED and hasattr(B.lib, name)
    assert [len(getattr(B.lib, n).argtypes) for n in (NL, TL, VJP)] == [18, 18, 22]
    with open(os.path.join(ROOT, "include", "cloudsc2_hip.h")) as f:
        header = f.read()
    assert all(f"int {n}(" in header for n in (NL, TL, VJP))
    assert len(B.FAMILIES) == 10 and not any("ens" in f or "colsum" in f for f in B.FAMILIES)  # not sweep families


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_a_valid_call_reports_layout_members_and_both_sets_of_names(device):
    p = {"rpecons": pk().to(device), "rkconv": pk().to(device)}
    lay, k, pnames, wnames = ag.check_ensemble_column_sums(inputs(device), params(), None, False, p, weights(device, ("tent", "fplsl")))
    assert lay == (NB, NLEV, NPROMA, NB * NPROMA) and k == K and pnames == ("rkconv", "rpecons") and wnames == ("tent", "fplsl")
    x = inputs(device)
    x["t"] = four_d(x["t"])
    x["q"] = torch.ones((K, 2, NB, NLEV, NPROMA), dtype=B.torch_real(), device=device)[:, 1]  # any member stride
    del x["qsat"]
    lay, k, _, wnames = ag.check_ensemble_column_sums(x, params(), NB * NPROMA - 5, True, {"rclcrit": pk().to(device)}, weights(device, B.OUT_NAMES))
    assert lay.tail == NPROMA - 5 and k == K and wnames == tuple(B.OUT_NAMES)


@pytest.mark.parametrize("bad, match", list(bad_params()))
def test_bad_params_raise_the_message_of_cloudsc2_ensemble(bad, match):
    with pytest.raises(ValueError, match=match) as parent:
        ag.check_ensemble(inputs(), params(), None, False, bad)
    with pytest.raises(ValueError) as e:
        ag.check_ensemble_column_sums(inputs(), params(), None, False, bad, weights())
    with pytest.raises(ValueError) as op:  # through the op: before the device check
        ag.cloudsc2_ensemble_column_sums(inputs("cpu"), params(), 3600.0, weights=weights(), params=bad)
    assert str(e.value) == str(parent.value) == str(op.value)


@pytest.mark.parametrize("device", ["cpu", "meta"])
def test_bad_weights_raise_the_message_of_cloudsc2_column_sums(device):
    seen = 0
    p = {"rkconv": pk().to(device)}
    for name, w, text in bad_weights(device):
        with pytest.raises(ValueError) as parent:
            ag.check_column_sums(inputs(device), params(), None, False, w)
        x = inputs(device)
        x["t"] = four_d(x["t"])  # (a per-member input: the weights are checked against member 0's layout)
        with pytest.raises(ValueError) as e:
            ag.check_ensemble_column_sums(x, params(), None, False, p, w)
        with pytest.raises(ValueError) as op:
            ag.cloudsc2_ensemble_column_sums(x, params(), 3600.0, weights=w, params=p)
        assert text in str(e.value) and str(e.value) == str(parent.value) == str(op.value), (name, str(e.value))
        seen += 1
    assert seen >= 9


def test_bad_inputs_raise_the_message_of_cloudsc2_ensemble():
    p, w = {"rkconv": pk()}, weights()
    off = params()
    off.lphylin = 0
    x_members = inputs()
    x_members["t"] = four_d(x_members["t"], K + 1)
    x_dim = inputs()
    x_dim["t"] = x_dim["t"][0]
    for x, prm, ngptot, satur in ((x_members, params(), None, False), (x_dim, params(), None, False), (inputs(), params(), None, True),
                                  (inputs(), params(), NB * NPROMA + 1, False), (inputs(), params(NLEV - 1), None, False),
                                  (inputs(), off, None, False)):
        with pytest.raises(ValueError) as parent:
            ag.check_ensemble(x, prm, ngptot, satur, p)
        with pytest.raises(ValueError) as op:
            ag.cloudsc2_ensemble_column_sums(x, prm, 3600.0, ngptot, weights=w, params=p, satur=satur)
        assert str(op.value) == str(parent.value)


@pytest.mark.parametrize("satur", [False, True])
def test_cpu_inputs_stop_at_the_device_check(satur):
    x = inputs("cpu")
    if satur:
        del x["qsat"]
    with pytest.raises(ValueError, match="HIP device") as e:
        ag.cloudsc2_ensemble_column_sums(x, params(), 3600.0, weights=weights(), params={"rkconv": pk(requires_grad=True)}, satur=satur)
    with pytest.raises(ValueError, match="HIP device") as parent:
        ag.cloudsc2_ensemble(x, params(), 3600.0, satur=satur, params={"rkconv": pk()})
    assert str(e.value) == str(parent.value)


def test_vmap_and_a_second_differentiation_are_refused_by_the_functions():
    for cls in (ag._Cloudsc2EnsColsum, ag._Cloudsc2EnsColsumTl, ag._Cloudsc2EnsColsumVjp):
        with pytest.raises(NotImplementedError, match="cloudsc2_ensemble_column_sums: torch.func.vmap, jacfwd, jacrev and is_grads_batched"):
            cls.vmap(None, ())
    for cls in (ag._Cloudsc2EnsColsumTl, ag._Cloudsc2EnsColsumVjp):
        for again in (cls.backward, cls.jvp):
            with pytest.raises(NotImplementedError, match="cloudsc2_ensemble_column_sums: double backward"):
                again(None)


# ---- the launchers: what they refuse before the device is looked for ---------------------------------------------------------------------

def launcher_cases(W: SumWorld):
    L, r = B.lib, C.byref
    p, pe = abi_params(), abi_params(levapls2=1)
    G = (G_NPROMA, G_NLEV, G_NGPTOT)
    ti, to, scr, tab = W.ins(), W.outs(), W.real("scratch"), W.real("table")
    par, work, adj = W.real("params"), W.real("workspace"), W.real("par_adj")
    own10 = (C.c_longlong * 10)(*([64] * 10))
    own16 = (C.c_longlong * 16)(*([512] * 16))
    ref = lambda b: r(b) if b is not None else None  # noqa: E731

    def nl(q=p, members=2, pr=par, i=ti, w=tab, y="surface", ym=own10, keep=None, km=own10, s=None, sm=64, ws=work):
        y = W.sums("sums") if y == "surface" else y
        return L.cloudsc2_nl_launch_ens_colsum(ref(q), 3600.0, *G, members, pr, ref(i), None, w, ref(y), ym, ref(keep), km, s, sm, ws, None)

    def tl(q=p, members=2, pr=par, dpr=par, i=ti, x="narrow", w=tab, y="surface", ym=own10, ws=work, satur=0):
        x = W.ins("pert", only=("q", "t")) if x == "narrow" else x
        y = W.sums("dsums") if y == "surface" else y
        return L.cloudsc2_tl_launch_ens_colsum(ref(q), 3600.0, *G, satur, members, pr, dpr, ref(i), None, ref(x), None, w, ref(y), ym, ws, None)

    def vjp(q=p, members=2, pr=par, i=ti, o=to, om=own10, x="narrow", xm=own16, w=tab, y="surface", ym=None, s=scr, ws=work, pa=adj, satur=0):
        x = W.ins("adj", only=("q", "t")) if x == "narrow" else x
        y = W.sums("ysums") if y == "surface" else y
        return L.cloudsc2_vjp_launch_ens_colsum(ref(q), 3600.0, *G, satur, members, pr, ref(i), None, ref(o), om, ref(x), xm, w, ref(y), ym, s, 64,
                                                ws, pa, None)

    members = "ensemble: 1 <= members <= 65535 required"
    arrays = "ensemble: the parameter array and the workspace are required"
    shared = "ensemble: a field the members write has member stride 0 (every member needs its own)"
    out = []
    for who, fn in ((NL, nl), (TL, tl), (VJP, vjp)):
        out += [(who, "NULL argument block", lambda fn=fn: fn(q=None)), (who, "NULL argument block", lambda fn=fn: fn(i=None)),
                (who, "NULL argument block", lambda fn=fn: fn(y=None)), (who, members, lambda fn=fn: fn(members=0)),
                (who, members, lambda fn=fn: fn(members=65536)), (who, arrays, lambda fn=fn: fn(pr=None)),
                (who, arrays, lambda fn=fn: fn(ws=None)), (who, "the weight table is NULL", lambda fn=fn: fn(w=None)),
                (who, "ensemble: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)", lambda fn=fn: fn(q=abi_params(lphylin=0)))]
    out += [(NL, "no sum is given (every sums field is NULL)", lambda: nl(y=B.Outputs())),
            (NL, shared, lambda: nl(ym=None)),
            (NL, shared, lambda: nl(keep=W.outs("keep", only=("fplsl", "fplsn")), km=None)),
            (NL, "ensemble: the cover-checkpoint plane has member stride 0", lambda: nl(q=pe, keep=W.outs("keep", only=("fplsl", "fplsn")), s=scr, sm=0)),
            (NL, "keep needs both planes, fplsl and fplsn", lambda: nl(keep=W.outs("keep", only=("fplsl",)))),
            (NL, "keep with LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required",
             lambda: nl(q=pe, keep=W.outs("keep", only=("fplsl", "fplsn")))),
            (TL, "no sum is wanted (every pert_sums field is NULL)", lambda: tl(y=B.Outputs())),
            (TL, shared, lambda: tl(ym=None)),
            (TL, "NULL argument block", lambda: tl(dpr=None)),
            (TL, "NULL argument block", lambda: tl(x=None)),
            (TL, "satur must be 0 (qsat given) or 1 (SATUR differentiated in the sweep)", lambda: tl(satur=2)),
            (VJP, "no cotangent is given (every adj_sums field is NULL)", lambda: vjp(y=B.Outputs())),
            (VJP, shared, lambda: vjp(xm=None)),
            (VJP, "the parameter adjoints' array is required", lambda: vjp(pa=None)),
            (VJP, "traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required", lambda: vjp(o=W.outs(fplsn=None))),
            (VJP, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required", lambda: vjp(q=pe, s=None)),
            (VJP, "satur must be 0 (qsat given) or 1 (SATUR differentiated in the sweep)", lambda: vjp(satur=-1))]
    # one member shares with nobody; no gradient plane at all is a well-formed call of the reverse sweep (the parameter adjoints alone)
    wellformed = [("nl", lambda: nl()), ("nl/one member, strides NULL", lambda: nl(members=1, ym=None)),
                  ("nl/keep", lambda: nl(q=pe, keep=W.outs("keep", only=("fplsl", "fplsn")), s=scr)), ("tl", lambda: tl()),
                  ("tl/no field tangent", lambda: tl(x=B.Inputs())), ("vjp", lambda: vjp()), ("vjp/parameters only", lambda: vjp(x=B.Inputs()))]
    return out, wellformed


def test_the_launchers_refuse_what_their_parents_refuse_and_name_themselves():
    refusals, _ = launcher_cases(SumWorld(False))
    for who, msg, fn in refusals:
        B.lib.cloudsc2_debug_launch_log_reset()
        rc = fn()
        text = B.lib.cloudsc2_last_error().decode()
        assert (rc, text) == (EINVAL, f"{who}: {msg}"), (who, msg, rc, text)
        assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0, (who, msg, "the launch log is not empty after a refusal")


def test_a_well_formed_call_needs_a_device():
    if B.device_available():
        pytest.skip("a device is present: the well-formed calls would launch on dummy pointers")
    _, wellformed = launcher_cases(SumWorld(False))
    for name, fn in wellformed:
        assert fn() == B.CLOUDSC2_ENODEVICE, (name, B.lib.cloudsc2_last_error().decode())


def test_the_workspace_covers_the_larger_blocks():
    """one query serves the six ensemble launchers: K blocks of at most 4 KiB (a kernel-argument segment) and K x 4 x ncols_pad doubles"""
    f = B.lib.cloudsc2_ens_workspace_bytes
    one = f(1, 24, 137, 70) - 4 * 72 * 8
    assert 0 < one <= 4096 and one % 256 == 0
    blocks = f(8, 128, 137, 160000) - 8 * 4 * 160000 * 8
    assert blocks % 256 == 0 and 8 * (one - 255) <= blocks <= 8 * one
