"""What every route of the differentiable op hands to which launcher, pinned on the CPU: ``autograd_launch_trace.json`` holds, route
by route, every call the op makes across the ctypes boundary -- the entry point, its scalars, the four parameter values of ``prm``,
and for every block, by-value field and raw pointer whether it is NULL, its block stride and a label for the pointer; member-stride
and ``double[4]`` arrays by value.  The file is recorded once from a known-good tree and compared call for call ever after, so a
change to ``autograd.py`` that moves anything at that boundary -- another launcher, a plane more or less, a zero plane no longer
shared, another stride -- fails here without a device.

No device is touched: ``check_device``, ``_prepare``, ``_stream``, ``torch.cuda.device`` and
``torch.cuda.is_current_stream_capturing`` are stubbed, ``binding.lib`` is a recorder that returns 0 and answers the size queries
with fixed numbers, and the tensors live on the CPU.  The kernels do not run, so what the op returns is uninitialised memory; only
the calls are looked at.

Labels.  A pointer into a tensor the test itself holds at the time of the call (inputs, outputs already returned, cotangents,
tangents) is ``name+element offset``; every other pointer is ``#k``, numbered by first appearance within that one call, which pins
aliasing inside a call (the one shared zero plane of ``_zero_filled``) without depending on what the allocator reuses between calls.
A field is ``"label|block stride"``; absent fields are left out.

Geometry: NPROMA 8, NLEV 4, NGPTOT 12 -- two blocks, the second with a padded tail -- and NGPTOT 16 where full blocks change the
route (a batch of states under ``vmap`` folds into the block dimension only then).

``python -m tests.test_autograd_launch_trace record`` writes the file."""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "autograd_launch_trace.json")
NPROMA, NLEV, TAIL, FULL = 8, 4, 12, 16
PTSPHY = 3600.0
NDIR = 5    # directions of jacfwd / jacrev: more than the stub's cloudsc2_batch_max() = 4
NSTATE = 2  # states of a vmap over the op
NMEMBER = 3
HALF = ag.HALF_IN + ag.HALF_OUT
BYREF = type(C.byref(C.c_int()))
REAL_LIB = B.lib
SIZES = {"cloudsc2_par_work_doubles": 24, "cloudsc2_ens_workspace_bytes": 4096, "cloudsc2_batch_max": 4}
F64 = torch.float64


class Trace:
    """the calls of one route and the tensors the test holds"""

    def __init__(self):
        self.calls, self.held = [], []

    def hold(self, prefix: str, ts: dict) -> dict:
        self.held += [(f"{prefix}.{n}", t) for n, t in ts.items() if t is not None]
        return ts

    def label(self, ptr: int, local: dict) -> str:
        inside = None
        for name, t in self.held:
            if not t.numel():
                continue
            lo, size = t.data_ptr(), t.element_size()
            if ptr == lo:
                return name + "+0"
            extent = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
            if inside is None and lo < ptr < lo + extent * size:
                inside = f"{name}+{(ptr - lo) // size}"
        return inside or "#%d" % local.setdefault(ptr, len(local))

    def arg(self, a, local: dict):
        if a is None or isinstance(a, (int, float)):
            return a
        if isinstance(a, BYREF):
            return self.arg(a._obj, local)
        if isinstance(a, B.Params):
            return {"prm": [getattr(a, n) for n in B.PARAM_NAMES]}
        if isinstance(a, (B.Inputs, B.Outputs)):
            return {n: self.arg(getattr(a, n), local) for n, _ in a._fields_ if getattr(a, n).ptr}
        if isinstance(a, B.Field):
            return f"{self.label(a.ptr, local)}|{a.block_stride}" if a.ptr else None
        if isinstance(a, C.c_void_p):
            return self.label(a.value, local) if a.value else None
        if isinstance(a, C.c_longlong):
            return "result"
        assert isinstance(a, C.Array), type(a)
        return [self.arg(e, local) for e in a]

    def record(self, name: str, args: tuple):
        local = {}
        self.calls.append([name] + [self.arg(a, local) for a in args])
        if name == "cloudsc2_par_work_doubles":
            args[2]._obj.value = SIZES[name]
            return 0
        return SIZES.get(name, 0)


class Lib:
    """``binding.lib`` of a route: launchers and size queries are recorded, everything else (``cloudsc2_params_default``) is real"""

    def __init__(self, trace: Trace):
        self._trace = trace

    def __getattr__(self, name: str):
        if "launch" not in name and name not in SIZES:
            return getattr(REAL_LIB, name)
        return lambda *args: self._trace.record(name, args)


def stub(mp, trace: Trace) -> None:
    mp.setattr(ag, "check_device", lambda ts: (list(ts), torch.device("cpu"))[1])
    mp.setattr(ag, "_prepare", lambda dev: None)
    mp.setattr(ag, "_stream", lambda dev: C.c_void_p(None))
    mp.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    mp.setattr(B, "lib", Lib(trace))


def fields(names, nb: int, seed: int, batch: tuple = ()) -> dict:
    g = torch.Generator().manual_seed(seed)
    return {n: torch.rand(batch + (nb, NLEV + (n in HALF), NPROMA), generator=g, dtype=B.torch_real()) for n in names}


def setup(T: Trace, satur: bool, ngptot: int = TAIL, evap: bool = False, grad=(), views: bool = False, members=()):
    """names, the held inputs ``x.*``, prm.  views: the PGTEN* group as planes of two packed buffers with different block strides;
    members: the inputs that are 4-D, one state per member of an ensemble"""
    nb = -(-ngptot // NPROMA)
    names = ag.SAT_NAMES if satur else B.IN_NAMES
    x = fields(names, nb, 1)
    if views:
        two, three = (torch.rand((nb, k, NLEV, NPROMA), generator=torch.Generator().manual_seed(7), dtype=B.torch_real()) for k in (2, 3))
        x.update(gtent=two[:, 0], gtenq=two[:, 1], gtenl=three[:, 0], gteni=three[:, 2])
    x.update(fields(members, nb, 8, batch=(NMEMBER,)))
    for n in grad:
        x[n].requires_grad_()
    return names, T.hold("x", x), c2.default_params(np.linspace(0.01, 1.0, NLEV), levapls2=evap), nb


class _Drop(torch.autograd.Function):
    """identity whose backward hands on no gradient at all"""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return None


def r_backward(T, satur, sparse=False, evap=True, wanted=("t", "q"), cot=("fplsl", "tent"), views=False, drop=False):
    names, x, prm, nb = setup(T, satur, evap=evap, grad=names_or(wanted, satur), views=views)
    out = ag.cloudsc2(x, prm, PTSPHY, TAIL, satur=satur, sparse=sparse)
    T.hold("out", out._asdict())
    if not wanted:
        assert not out.tent.requires_grad  # (nothing to differentiate: the forward launch is the whole route)
        return
    cot = B.OUT_NAMES if cot == "all" else cot
    g = T.hold("g", fields(cot, nb, 2))
    ys = [_Drop.apply(getattr(out, n)) if drop else getattr(out, n) for n in cot]
    torch.autograd.grad(ys, [x[n] for n in names_or(wanted, satur)], [g[n] for n in cot], allow_unused=drop)


def names_or(wanted, satur):
    return (ag.SAT_NAMES if satur else B.IN_NAMES) if wanted == "all" else wanted


def r_forward_ad(T, satur, sparse=False, evap=False):
    names, x, prm, nb = setup(T, satur, evap=evap)
    dx = T.hold("dx", fields(("t", "q"), nb, 3))
    with fwAD.dual_level():
        ag.cloudsc2({**x, **{n: fwAD.make_dual(x[n], d) for n, d in dx.items()}}, prm, PTSPHY, TAIL, satur=satur, sparse=sparse)


def r_jacfwd(T, satur, sparse=False):
    names, x, prm, nb = setup(T, satur)
    basis = T.hold("basis", fields(("t",), nb, 4, batch=(NDIR,)))["t"]
    f = lambda s: ag.cloudsc2({**x, "t": x["t"] + torch.tensordot(s, basis, 1)}, prm, PTSPHY, TAIL, satur=satur, sparse=sparse).tent  # noqa: E731
    torch.func.jacfwd(f)(torch.zeros(NDIR, dtype=B.torch_real()))


def r_jacrev(T, satur, sparse=False):
    names, x, prm, nb = setup(T, satur, evap=True)
    w = T.hold("w", fields(("tent",), nb, 5, batch=(NDIR,)))["tent"]
    f = lambda t: torch.tensordot(w, ag.cloudsc2({**x, "t": t}, prm, PTSPHY, TAIL, satur=satur, sparse=sparse).tent, 3)  # noqa: E731
    torch.func.jacrev(f)(x["t"])


def r_vmap_states(T, satur, sparse=False, ngptot=FULL, evap=False):
    names, x, prm, nb = setup(T, satur, ngptot, evap=evap)
    xb = T.hold("xb", fields(("t", "q"), nb, 6, batch=(NSTATE,)))
    f = lambda t, q: tuple(ag.cloudsc2({**x, "t": t, "q": q}, prm, PTSPHY, ngptot, satur=satur, sparse=sparse))  # noqa: E731
    torch.func.vmap(f)(xb["t"], xb["q"])


def r_vmap_states_jvp(T, satur, sparse=False, ngptot=FULL):
    names, x, prm, nb = setup(T, satur, ngptot)
    xb, db = T.hold("xb", fields(("t",), nb, 6, batch=(NSTATE,))), T.hold("dxb", fields(("t",), nb, 9, batch=(NSTATE,)))
    f = lambda t: tuple(ag.cloudsc2({**x, "t": t}, prm, PTSPHY, ngptot, satur=satur, sparse=sparse))  # noqa: E731
    torch.func.vmap(lambda t, dt: torch.func.jvp(f, (t,), (dt,))[1])(xb["t"], db["t"])


def r_vmap_states_vjp(T, satur, sparse=False, ngptot=FULL, evap=True):
    names, x, prm, nb = setup(T, satur, ngptot, evap=evap)
    xb, gb = T.hold("xb", fields(("t",), nb, 6, batch=(NSTATE,))), T.hold("gb", fields(("tent",), nb, 10, batch=(NSTATE,)))
    f = lambda t: ag.cloudsc2({**x, "t": t}, prm, PTSPHY, ngptot, satur=satur, sparse=sparse).tent  # noqa: E731
    torch.func.vmap(lambda t, g: torch.func.vjp(f, t)[1](g))(xb["t"], gb["tent"])


def r_params(T, satur, mode="grad_p"):
    names, x, prm, nb = setup(T, satur, evap=True, grad=("t",))
    p = T.hold("p", {"rkconv": torch.tensor(1.5e-4, dtype=F64), "rpecons": torch.tensor(6e-5, dtype=F64)})
    if mode == "jvp":
        dx = T.hold("dx", fields(("t",), nb, 3))
        with fwAD.dual_level():
            pd = {**p, "rkconv": fwAD.make_dual(p["rkconv"], torch.tensor(2.0, dtype=F64))}
            ag.cloudsc2({**x, "t": fwAD.make_dual(x["t"].detach(), dx["t"])}, prm, PTSPHY, TAIL, satur=satur, params=pd)
        return
    if mode == "grad_p":
        p["rkconv"].requires_grad_()
    out = ag.cloudsc2(x, prm, PTSPHY, TAIL, satur=satur, params=p)
    T.hold("out", out._asdict())
    g = T.hold("g", fields(("tent",), nb, 2))
    torch.autograd.grad([out.tent], [x["t"]] + ([p["rkconv"]] if mode == "grad_p" else []), [g["tent"]])


def r_param_jacobian(T, satur, given=False, evap=False):
    names, x, prm, nb = setup(T, satur, evap=evap)
    ag.param_jacobian(x, prm, PTSPHY, TAIL, satur=satur, params={"rclcrit": torch.tensor(0.5, dtype=F64)} if given else None)


def r_param_normal(T, satur, given=False, evap=False):
    names, x, prm, nb = setup(T, satur, evap=evap)
    r, w = T.hold("r", fields(("tent", "fplsl"), nb, 11)), T.hold("w", fields(("tent",), nb, 12))
    ag.param_normal_equations(x, prm, PTSPHY, TAIL, residual=r, weights=w if given else None, satur=satur,
                              params={"rclcrit": torch.tensor(0.5, dtype=F64), "rpecons": torch.tensor(6e-5, dtype=F64)} if given else None)


def r_ensemble(T, satur, per_member=False, mode="backward"):
    members = ("t", "q") if per_member else ()
    names, x, prm, nb = setup(T, satur, evap=True, grad=("t", "pap") if mode == "backward" else (), members=members)
    p = T.hold("p", {n: torch.linspace(1e-4, 2e-4, NMEMBER, dtype=F64) for n in ("rkconv", "rclcrit")})
    if mode == "jvp":
        dx = T.hold("dx", fields(("t",), nb, 3, batch=(NMEMBER,) if per_member else ()))
        with fwAD.dual_level():
            pd = {**p, "rkconv": fwAD.make_dual(p["rkconv"], torch.ones(NMEMBER, dtype=F64))}
            ag.cloudsc2_ensemble({**x, "t": fwAD.make_dual(x["t"], dx["t"])}, prm, PTSPHY, TAIL, satur, pd)
        return
    p["rkconv"].requires_grad_()
    out = ag.cloudsc2_ensemble(x, prm, PTSPHY, TAIL, satur, p)
    T.hold("out", out._asdict())
    g = T.hold("g", fields(("tent",), nb, 2, batch=(NMEMBER,)))
    torch.autograd.grad([out.tent], [x["t"], x["pap"], p["rkconv"]], [g["tent"]])


def r_column_sums(T, satur, mode="backward"):
    names, x, prm, nb = setup(T, satur, evap=True, grad=("t", "q") if mode == "backward" else ())
    g = torch.Generator().manual_seed(13)
    w = T.hold("w", {n: torch.rand(NLEV + (n in HALF), generator=g, dtype=B.torch_real()) for n in ("tent", "fplsl")})
    if mode == "jvp":
        dx = T.hold("dx", fields(("t",), nb, 3))
        with fwAD.dual_level():
            ag.cloudsc2_column_sums({**x, "t": fwAD.make_dual(x["t"], dx["t"])}, prm, PTSPHY, TAIL, weights=w, satur=satur)
        return
    out = ag.cloudsc2_column_sums(x, prm, PTSPHY, TAIL, weights=w, satur=satur)
    T.hold("out", out._asdict())
    if mode == "backward":
        gy = T.hold("g", {"tent": torch.rand((nb, NPROMA), generator=g, dtype=B.torch_real())})
        torch.autograd.grad([out.tent], [x["t"], x["q"]], [gy["tent"]])


def r_satur(T, satur, differentiable=False):
    names, x, prm, nb = setup(T, True, grad=("t",) if differentiable else ())
    q = ag.satur(x["pap"], x["t"], prm, TAIL, differentiable=differentiable)
    if differentiable:
        torch.autograd.grad([q], [x["t"]], [T.hold("g", fields(("qsat",), nb, 2))["qsat"]])


def routes() -> dict:
    """id -> (route, satur, keywords); every route with ``satur`` off and on but :func:`satur` itself"""
    out = {}

    def add(name, fn, both=True, **kw):
        for satur in (False, True) if both else (False,):
            key = f"{name}/{'satur' if satur else 'qsat'}" if both else name
            assert key not in out, key
            out[key] = (fn, satur, kw)

    add("dense/backward_narrow", r_backward)
    add("dense/backward_narrow_no_evap", r_backward, evap=False)
    add("dense/no_gradient_wanted", r_backward, wanted=())
    add("dense/backward_copied_views", r_backward, views=True)
    add("sparse/backward_narrow", r_backward, sparse=True)
    add("sparse/backward_everything", r_backward, sparse=True, wanted="all", cot="all")
    add("sparse/backward_no_cotangent", r_backward, sparse=True, drop=True)
    add("dense/forward_ad", r_forward_ad, evap=True)
    add("sparse/forward_ad_missing_tangents", r_forward_ad, sparse=True)
    add("dense/jacfwd", r_jacfwd)
    add("dense/jacrev", r_jacrev)
    add("sparse/jacfwd", r_jacfwd, sparse=True)
    add("sparse/jacrev", r_jacrev, sparse=True)
    add("dense/vmap_states_full", r_vmap_states, evap=True)
    add("dense/vmap_states_tail", r_vmap_states, ngptot=TAIL)
    add("sparse/vmap_states_full", r_vmap_states, sparse=True)
    add("sparse/vmap_states_tail", r_vmap_states, sparse=True, ngptot=TAIL, evap=True)
    add("dense/vmap_states_jvp_full", r_vmap_states_jvp)
    add("dense/vmap_states_jvp_tail", r_vmap_states_jvp, ngptot=TAIL)
    add("dense/vmap_states_vjp_full", r_vmap_states_vjp)
    add("dense/vmap_states_vjp_tail", r_vmap_states_vjp, ngptot=TAIL, evap=False)
    add("sparse/vmap_states_jvp_full", r_vmap_states_jvp, sparse=True)
    add("sparse/vmap_states_vjp_full", r_vmap_states_vjp, sparse=True)
    add("params/backward_parameter_wanted", r_params)
    add("params/backward_fields_only", r_params, mode="grad_x")
    add("params/forward_ad", r_params, mode="jvp")
    add("param_jacobian/prm", r_param_jacobian, evap=True)
    add("param_jacobian/given", r_param_jacobian, given=True)
    add("param_normal_equations/prm", r_param_normal)
    add("param_normal_equations/given_weighted", r_param_normal, given=True, evap=True)
    add("ensemble/shared_backward", r_ensemble)
    add("ensemble/shared_forward_ad", r_ensemble, mode="jvp")
    add("ensemble/per_member_backward", r_ensemble, per_member=True)
    add("ensemble/per_member_forward_ad", r_ensemble, per_member=True, mode="jvp")
    add("column_sums/backward", r_column_sums)
    add("column_sums/untracked", r_column_sums, mode="untracked")
    add("column_sums/forward_ad", r_column_sums, mode="jvp")
    add("satur/plain", r_satur, both=False)
    add("satur/differentiable", r_satur, both=False, differentiable=True)
    return out


def run(mp, key: str) -> list:
    fn, satur, kw = routes()[key]
    T = Trace()
    stub(mp, T)
    fn(T, satur, **kw)
    return json.loads(json.dumps(T.calls))


_recorded = None


def recorded() -> dict:
    global _recorded
    if _recorded is None:
        with open(JSON) as f:
            _recorded = json.load(f)
    return _recorded


def test_the_recorded_file_matches_the_routes():
    assert sorted(recorded()) == sorted(routes())
    assert all(calls and all(c[0].startswith("cloudsc2_") for c in calls) for calls in recorded().values())


@pytest.mark.parametrize("key", list(routes()))
def test_route_makes_the_recorded_calls(monkeypatch, key):
    got, want = run(monkeypatch, key), recorded()[key]
    assert [c[0] for c in got] == [c[0] for c in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (key, k, g[0], [(j, a, b) for j, (a, b) in enumerate(zip(g, w)) if a != b])


if __name__ == "__main__":
    assert sys.argv[1:] == ["record"], "usage: python -m tests.test_autograd_launch_trace record"
    rec = {}
    for key in routes():
        with pytest.MonkeyPatch.context() as mp:
            rec[key] = run(mp, key)
        print(f"{key}: {[c[0].replace('cloudsc2_', '') for c in rec[key]]}")
    with open(os.environ.get("CLOUDSC2_LAUNCH_TRACE_OUT", JSON), "w") as f:  # one call per line
        body = [json.dumps(k) + ": [\n" + ",\n".join(" " + json.dumps(c, separators=(",", ":")) for c in calls) + "\n]" for k, calls in rec.items()]
        f.write("{\n" + ",\n".join(body) + "\n}\n")
    print(f"{len(rec)} routes, {sum(len(c) for c in rec.values())} calls recorded")
