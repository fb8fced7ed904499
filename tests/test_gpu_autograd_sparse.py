"""The sparse derivative sweeps on the MI355X: ``cloudsc2_tl_launch_sparse`` / ``cloudsc2_vjp_launch_sparse`` through the C ABI (children
running tests/sparse_variant_checks.py, one per addressing form and precision) and ``cloudsc2(..., sparse=True)`` through torch.

Contract: every plane the sparse route returns has the bits of the dense route; what it does not need it neither allocates nor moves.
The shapes are the suite's small ones: ``random_table(137, 100)`` (non-zero supsat), NPROMA 32 x 100 columns (four blocks, a padded
tail of 28), one case at NPROMA 128 x 128 (in the children)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, make_inputs, params, same_bits, seeded
from tests.util import ROOT, B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

FAULT_CODES = (124, 134, 137, 139, -6, -9, -11)
_device_trouble = []  # a child that faulted, aborted or ran into its time limit: this module launches nothing more after it
NARROW_IN, NARROW_OUT = ("q", "t"), ("fplsl", "fplsn")


@pytest.fixture(autouse=True)
def need_a_sound_device():
    if _device_trouble:
        pytest.fail(f"not launched: {_device_trouble[0]}")


# ---- checks 1 and 2: the C ABI, in children ---------------------------------------------------------------------------------------------

def run_children(d, env: dict, *args):
    """tests/sparse_variant_checks.py for CLOUDSC2_OFF32 = 0, 1, one after the other, each under its own time limit, no retry; the
    second is not started if the first did not end well"""
    runs = []
    for mode in ("0", "1"):
        f = str(d / f"off32_{mode}.npz")
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sparse_variant_checks.py"), f, *args],
                               env={**os.environ, **env, "CLOUDSC2_OFF32": mode}, capture_output=True, text=True, timeout=240)
            rc, text = r.returncode, r.stdout + r.stderr
        except subprocess.TimeoutExpired as e:
            rc, text = 124, f"time limit: {e}"
        print(f"{env} CLOUDSC2_OFF32={mode}: return code {rc}\n{text[-3000:]}")
        z = None
        if rc == 0:
            with np.load(f) as data:
                z = {k: data[k] for k in data.files}
        runs.append((rc, text, z))
        if rc != 0:
            if rc in FAULT_CODES:
                _device_trouble.append(f"tests/sparse_variant_checks.py with {env} CLOUDSC2_OFF32={mode} ended with {rc}")
            break
    return runs


def check_children(runs, ncases: int):
    for mode, (rc, text, _) in zip("01", runs):
        assert rc == 0, (f"CLOUDSC2_OFF32={mode}", text[-4000:])  # every present plane the dense bits, tails and inputs untouched, log empty
    assert len(runs) == 2
    z64, z32 = runs[0][2], runs[1][2]
    assert len(z64["cases"]) == ncases and list(z64["cases"]) == list(z32["cases"])
    assert list(z64["keys"]) == list(z32["keys"]) and len(z64["keys"]) > 100 * ncases
    assert np.array_equal(z64["sums"], z32["sums"]), "the two addressing forms differ in a plane"


def test_sparse_launchers_have_the_dense_bits_in_both_addressing_forms(tmp_path):
    check_children(run_children(tmp_path, {}), 17)


def test_sparse_launchers_of_the_fp32_library(tmp_path):
    """the fp32 library packs pairs of operations (v_pk_*_f32), and which pairs it packs decides which products fuse: the bits hold only
    with the pins of the stored values in the order and in the blocks of the dense sweep's stores (DESIGN.md 3.6 has the history)"""
    check_children(run_children(tmp_path, {"CLOUDSC2_PRECISION": "single"}, "small"), 16)


# ---- checks 3 to 6: through torch -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def state():
    tab = c2.random_table(137, 100, seed=21)
    return tab


def setup(tab, satur: bool, **flags):
    prm = params(tab, **flags)
    x, ptsphy, lay = make_inputs(tab, 32, 100, prm)
    names = ag.SAT_NAMES if satur else B.IN_NAMES
    return prm, {n: x[n] for n in names}, ptsphy, lay, names


def leaves(x, wanted):
    return {n: (t.clone().requires_grad_() if n in wanted else t) for n, t in x.items()}


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True)], ids=["plain", "evap"])
def test_narrow_gradients_are_the_dense_bits(state, flags, satur):
    prm, x, ptsphy, lay, names = setup(state, satur, **flags)
    u = seeded(B.OUT_NAMES, lay, seed=6)
    # the dense op, all gradients, zero cotangents for the other outputs
    xd = leaves(x, names)
    out = ag.cloudsc2(xd, prm, ptsphy, lay.ngptot, satur=satur)
    want = dict(zip(names, torch.autograd.grad([out.fplsl, out.fplsn], [xd[n] for n in names], [u["fplsl"], u["fplsn"]])))
    # torch.autograd.grad of the narrow case
    xs = leaves(x, NARROW_IN)
    out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, sparse=True)
    g = dict(zip(NARROW_IN, torch.autograd.grad([out.fplsl, out.fplsn], [xs[n] for n in NARROW_IN], [u["fplsl"], u["fplsn"]])))
    for n in NARROW_IN:
        assert same_bits(g[n], want[n]), n
    # .backward() on a loss over two outputs: the same, and no other input gets a .grad
    xs = leaves(x, names)
    for n in names:
        if n not in NARROW_IN:
            xs[n].requires_grad_(False)
    out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, sparse=True)
    (torch.sum(u["fplsl"] * out.fplsl) + torch.sum(u["fplsn"] * out.fplsn)).backward()
    xd2 = leaves(x, names)
    outd = ag.cloudsc2(xd2, prm, ptsphy, lay.ngptot, satur=satur)
    (torch.sum(u["fplsl"] * outd.fplsl) + torch.sum(u["fplsn"] * outd.fplsn)).backward()
    for n in names:
        if n in NARROW_IN:
            assert same_bits(xs[n].grad, xd2[n].grad), n
        else:
            assert xs[n].grad is None, n
    # every gradient wanted and every cotangent given: the dense sweep, the same bits
    xa = leaves(x, names)
    out = ag.cloudsc2(xa, prm, ptsphy, lay.ngptot, satur=satur, sparse=True)
    ga = torch.autograd.grad(list(out), [xa[n] for n in names], [u[n] for n in B.OUT_NAMES])
    xb = leaves(x, names)
    outb = ag.cloudsc2(xb, prm, ptsphy, lay.ngptot, satur=satur)
    gb = torch.autograd.grad(list(outb), [xb[n] for n in names], [u[n] for n in B.OUT_NAMES])
    assert all(same_bits(a, b) for a, b in zip(ga, gb))


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
def test_forward_mode_with_two_tangents(state, satur):
    prm, x, ptsphy, lay, names = setup(state, satur, levapls2=True)
    v = {n: 0.01 * x[n] for n in NARROW_IN}

    def f(sparse):
        def g(q, t):
            xs = dict(x)
            xs.update(q=q, t=t)
            return tuple(ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, sparse=sparse))
        return g
    _, dy_d = torch.func.jvp(f(False), (x["q"], x["t"]), (v["q"], v["t"]))
    _, dy_s = torch.func.jvp(f(True), (x["q"], x["t"]), (v["q"], v["t"]))
    assert all(same_bits(a, b) for a, b in zip(dy_s, dy_d))
    import torch.autograd.forward_ad as fwad
    with fwad.dual_level():
        xs = dict(x)
        xs.update(q=fwad.make_dual(x["q"], v["q"]), t=fwad.make_dual(x["t"], v["t"]))
        out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, sparse=True)
        dy_f = [fwad.unpack_dual(o).tangent for o in out]
    assert all(same_bits(a, b) for a, b in zip(dy_f, dy_d))


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
def test_torch_func_transforms_agree_with_the_dense_op(state, satur):
    prm, x, ptsphy, lay, names = setup(state, satur)
    u = seeded(NARROW_OUT, lay, seed=7)
    u2 = [torch.stack([u[n], 0.5 * u[n]]) for n in NARROW_OUT]
    v2 = [torch.stack([0.01 * x[n], -0.02 * x[n]]) for n in NARROW_IN]

    def f(sparse):
        def g(q, t):
            xs = dict(x)
            xs.update(q=q, t=t)
            out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, sparse=sparse)
            return out.fplsl, out.fplsn
        return g

    def loss(sparse):
        return lambda q, t: sum(torch.sum(w * o) for w, o in zip((u["fplsl"], u["fplsn"]), f(sparse)(q, t)))
    res = {}
    for sparse in (False, True):
        _, pull = torch.func.vjp(f(sparse), x["q"], x["t"])
        r = list(pull((u["fplsl"], u["fplsn"])))
        r += list(torch.func.grad(loss(sparse), argnums=(0, 1))(x["q"], x["t"]))
        r += list(torch.func.vmap(pull)((u2[0], u2[1])))  # two cotangents over one state
        jv = torch.func.vmap(lambda a, b: torch.func.jvp(f(sparse), (x["q"], x["t"]), (a, b))[1])(v2[0], v2[1])  # two tangents
        r += list(jv)
        res[sparse] = r
    assert len(res[True]) == len(res[False]) == 8
    for k, (a, b) in enumerate(zip(res[True], res[False])):
        assert same_bits(a, b), k
    # jacrev over two output elements' worth of directions: a reduced function keeps the Jacobian small
    def two_sums(sparse):
        return lambda q, t: torch.stack([torch.sum(o * w) for o, w in zip(f(sparse)(q, t), (u["fplsl"], u["fplsn"]))])
    jd = torch.func.jacrev(two_sums(False), argnums=(0, 1))(x["q"], x["t"])
    js = torch.func.jacrev(two_sums(True), argnums=(0, 1))(x["q"], x["t"])
    assert all(same_bits(a, b) for a, b in zip(js, jd))


def test_a_batch_of_two_states_under_vmap(state):
    prm, x, ptsphy, lay, names = setup(state, False)
    x128 = {n: t for n, t in make_inputs(state, 128, 128, prm)[0].items()}  # full blocks: the batch folds into the blocks
    lay128 = ag.Layout(1, 137, 128, 128)
    u = seeded(NARROW_OUT, lay128, seed=8)
    q2 = torch.stack([x128["q"], 1.01 * x128["q"]])
    t2 = torch.stack([x128["t"], x128["t"] + 0.5])

    def g(sparse):
        def loss(q, t):
            xs = dict(x128)
            xs.update(q=q, t=t)
            out = ag.cloudsc2(xs, prm, ptsphy, 128, sparse=sparse)
            return torch.sum(u["fplsl"] * out.fplsl) + torch.sum(u["fplsn"] * out.fplsn)
        return torch.func.vmap(torch.func.grad(loss, argnums=(0, 1)))
    gd, gs = g(False)(q2, t2), g(True)(q2, t2)
    assert all(same_bits(a, b) for a, b in zip(gs, gd))


def test_backward_allocates_only_the_wanted_gradients(state):
    """four blocks (plane = 4 x 137 x 32 elements), only t and q require grad, grad_outputs for fplsl and fplsn only"""
    prm, x, ptsphy, lay, names = setup(state, False)
    plane = 4 * 137 * 32 * x["t"].element_size()
    u = seeded(NARROW_OUT, lay, seed=9)
    rise = {}
    for sparse in (True, False):
        xs = leaves(x, NARROW_IN)
        out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, sparse=sparse)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        before = torch.cuda.max_memory_allocated(DEV)
        g = torch.autograd.grad([out.fplsl, out.fplsn], [xs[n] for n in NARROW_IN], [u["fplsl"], u["fplsn"]])
        torch.cuda.synchronize()
        rise[sparse] = torch.cuda.max_memory_allocated(DEV) - before
        del g, out, xs
    print("peak memory rise across torch.autograd.grad, in planes: sparse", rise[True] / plane, "dense", rise[False] / plane)
    assert rise[True] <= 3 * plane, rise[True] / plane   # 2 wanted, one plane of slack for rounding
    assert rise[False] >= 16 * plane, rise[False] / plane


def test_graph_capture_replays_the_eager_bits(state):
    prm, x, ptsphy, lay, names = setup(state, False, levapls2=True)
    xs = {n: (t.clone().requires_grad_() if n in NARROW_IN else t.clone()) for n, t in x.items()}
    u = seeded(NARROW_OUT, lay, seed=10)

    def step():
        out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, sparse=True)
        grads = torch.autograd.grad([out.fplsl, out.fplsn], [xs[n] for n in NARROW_IN], [u["fplsl"], u["fplsn"]])
        return [t.detach() for t in out], list(grads)

    def eager():
        o, g = step()
        return [t.clone() for t in o + g]
    first = eager()  # the eager call: device probe and CETA table before the capture
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_out, cap_g = step()
    for t in cap_out + cap_g:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip(first, cap_out + cap_g))
    with torch.no_grad():  # the inputs overwritten in place: the replay gives the new eager bits
        xs["t"].add_(0.25)
        xs["q"].mul_(1.01)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in cap_out + cap_g]
    second = eager()
    assert all(same_bits(a, b) for a, b in zip(second, replayed))
    assert not all(same_bits(a, b) for a, b in zip(first, second))


@pytest.mark.skipif(B.SINGLE, reason="the 1e-12 identity is an fp64 statement")
def test_dot_product_identity_of_the_two_sparse_sweeps(state):
    """<TL dx, y> = <dx, VJP y> on the narrow masks, satur=True, to the bound the dense pair is held to"""
    prm, x, ptsphy, lay, names = setup(state, True, lregcl=True)
    dx = {n: 0.01 * x[n] for n in NARROW_IN}
    y = seeded(NARROW_OUT, lay, seed=11)
    fwd = ag._Cloudsc2Sparse.apply(prm, ptsphy, lay, True, *(x[n] for n in names))
    saved = [x[n] for n in names] + [fwd[B.OUT_NAMES.index("fplsl")], fwd[B.OUT_NAMES.index("fplsn")], fwd[-1]]
    dy = ag._Cloudsc2SparseTl.apply(prm, ptsphy, lay, True, *(x[n] for n in names), *(dx.get(n) for n in names))
    xa = ag._Cloudsc2SparseVjp.apply(prm, ptsphy, lay, True, NARROW_IN, *saved, *(y.get(n) for n in B.OUT_NAMES))
    lhs = sum(float(torch.sum(dy[B.OUT_NAMES.index(n)].double() * y[n].double())) for n in NARROW_OUT)
    rhs = sum(float(torch.sum(dx[n].double() * a.double())) for n, a in zip(NARROW_IN, xa))
    assert abs(lhs - rhs) / abs(lhs) <= 1e-12, (lhs, rhs)
