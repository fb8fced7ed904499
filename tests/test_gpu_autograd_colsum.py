"""Column sums formed in the sweeps, on the MI355X: ``cloudsc2_column_sums`` through torch and the three launchers through the C ABI
(children running tests/colsum_variant_checks.py, one per addressing form and precision).

Contract: a sum is the bits of the fold ``acc = 0; acc = acc + w[k] * out[k]`` -- separate ``mul`` and ``add``, a Python loop over the
levels -- over the outputs of ``cloudsc2``; tangent sums are the fold over the dense jvp's planes; gradients are the bits of
``cloudsc2(..., sparse=True)`` differentiated through that fold with the same cotangents.  The shapes are the suite's small ones:
``random_table(137, 100, seed=21)``, NPROMA 32 x 100 columns (four blocks, a padded tail of 28), one case at NPROMA 128 x 128."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, make_inputs, params, same_bits
from tests.util import ROOT, B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

FAULT_CODES = (124, 134, 137, 139, -6, -9, -11)
_device_trouble = []  # a child that faulted, aborted or ran into its time limit: this module launches nothing more after it
NARROW_IN, NARROW_OUT = ("q", "t"), ("fplsl", "fplsn")
REAL = B.torch_real()


@pytest.fixture(autouse=True)
def need_a_sound_device():
    if _device_trouble:
        pytest.fail(f"not launched: {_device_trouble[0]}")


# ---- the C ABI, in children ------------------------------------------------------------------------------------------------------------

def run_children(d, env: dict, *args):
    """tests/colsum_variant_checks.py for CLOUDSC2_OFF32 = 0, 1, one after the other, each under its own time limit, no retry; the
    second is not started if the first did not end well"""
    runs = []
    for mode in ("0", "1"):
        f = str(d / f"off32_{mode}.npz")
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "colsum_variant_checks.py"), f, *args],
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
                _device_trouble.append(f"tests/colsum_variant_checks.py with {env} CLOUDSC2_OFF32={mode} ended with {rc}")
            break
    return runs


def check_children(runs, ncases: int):
    for mode, (rc, text, _) in zip("01", runs):
        assert rc == 0, (f"CLOUDSC2_OFF32={mode}", text[-4000:])
    assert len(runs) == 2
    z64, z32 = runs[0][2], runs[1][2]
    assert len(z64["cases"]) == ncases and list(z64["cases"]) == list(z32["cases"])
    assert list(z64["keys"]) == list(z32["keys"]) and len(z64["keys"]) > 50 * ncases
    assert np.array_equal(z64["sums"], z32["sums"]), "the two addressing forms differ"


def test_colsum_launchers_hold_the_bit_contracts_in_both_addressing_forms(tmp_path):
    check_children(run_children(tmp_path, {}), 9)


def test_colsum_launchers_of_the_fp32_library(tmp_path):
    check_children(run_children(tmp_path, {"CLOUDSC2_PRECISION": "single"}, "small"), 8)


# ---- through torch ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def state():
    return c2.random_table(137, 100, seed=21)


def setup(tab, satur: bool, nproma=32, ngptot=100, **flags):
    prm = params(tab, **flags)
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    names = ag.SAT_NAMES if satur else B.IN_NAMES
    return prm, {n: x[n] for n in names}, ptsphy, lay, names


def leaves(x, wanted):
    return {n: (t.clone().requires_grad_() if n in wanted else t) for n, t in x.items()}


def all_weights(lay, seed=31) -> dict:
    """seeded weights with negative entries, exact zeros and non-zero entries at both ends"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for n in B.OUT_NAMES:
        w = 2 * torch.rand(lay.nlevx(n), generator=g, dtype=REAL, device=DEV) - 1
        w[torch.rand(lay.nlevx(n), generator=g, device=DEV) < 0.2] = 0
        w[0], w[-1] = -0.75, 0.625
        out[n] = w
    return out


def surface_weights(lay) -> dict:
    w = torch.zeros(lay.nlev + 1, dtype=REAL, device=DEV)
    w[-1] = 1
    return {"fplsl": w, "fplsn": w.clone()}


def fold(w, plane):
    acc = torch.zeros((plane.shape[0], plane.shape[2]), dtype=plane.dtype, device=plane.device)
    for k in range(plane.shape[1]):
        acc = torch.add(acc, torch.mul(plane[:, k, :], w[k]))
    return acc


def folded(out, weights) -> dict:
    return {n: fold(weights[n], getattr(out, n)) for n in weights}


def ybars(names, lay, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for n in names:
        t = torch.randn((lay.nblocks, lay.nproma), generator=g, dtype=REAL, device=DEV)
        if lay.tail < lay.nproma:
            t[-1, lay.tail:] = 0
        out[n] = t
    return out


def tail_zero(t, lay):
    return lay.tail == lay.nproma or bool(torch.all(t[-1, lay.tail:] == 0))


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True)], ids=["plain", "evap"])
def test_sums_and_gradients_are_the_bits_of_the_fold(state, flags, satur):
    prm, x, ptsphy, lay, names = setup(state, satur, **flags)
    for weights, wanted in ((surface_weights(lay), NARROW_IN), (all_weights(lay), names)):
        wn = tuple(n for n in B.OUT_NAMES if n in weights)
        u = ybars(wn, lay, seed=6)
        # the reference: the sparse op differentiated through the torch fold
        xr = leaves(x, wanted)
        ref = folded(ag.cloudsc2(xr, prm, ptsphy, lay.ngptot, satur=satur, sparse=True), weights)
        gref = dict(zip(wanted, torch.autograd.grad([ref[n] for n in wn], [xr[n] for n in wanted], [u[n] for n in wn])))
        # forward without grad: the lean form
        with torch.no_grad():
            ys = ag.cloudsc2_column_sums(x, prm, ptsphy, lay.ngptot, weights=weights, satur=satur)
        assert isinstance(ys, ag.Cloudsc2Outputs)
        for n in B.OUT_NAMES:
            y = getattr(ys, n)
            if n not in weights:
                assert y is None, n
                continue
            assert y.shape == (lay.nblocks, lay.nproma) and tail_zero(y, lay), n
            assert same_bits(y[:-1], ref[n][:-1].detach()) and same_bits(y[-1, :lay.tail], ref[n][-1, :lay.tail].detach()), n
        # torch.autograd.grad of the grad-tracking forward: the same sums, the reference's gradients, None for what is not wanted
        xs = leaves(x, wanted)
        ys2 = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights, satur=satur)
        for n in wn:
            assert same_bits(getattr(ys2, n).detach(), getattr(ys, n)), n
        g = dict(zip(wanted, torch.autograd.grad([getattr(ys2, n) for n in wn], [xs[n] for n in wanted], [u[n] for n in wn])))
        for n in wanted:
            assert same_bits(g[n], gref[n]), n
        # .backward() on a loss: only the wanted inputs get a .grad
        xb = leaves(x, names)
        for n in names:
            if n not in wanted:
                xb[n].requires_grad_(False)
        yb = ag.cloudsc2_column_sums(xb, prm, ptsphy, lay.ngptot, weights=weights, satur=satur)
        sum(torch.sum(u[n] * getattr(yb, n)) for n in wn).backward()
        for n in names:
            if n in wanted:
                assert same_bits(xb[n].grad, gref[n]), n
            else:
                assert xb[n].grad is None, n
    # a sum without a cotangent contributes nothing: only fplsl's cotangent is given
    weights = surface_weights(lay)
    u = ybars(NARROW_OUT, lay, seed=7)
    xs, xr = leaves(x, NARROW_IN), leaves(x, NARROW_IN)
    ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights, satur=satur)
    ref = folded(ag.cloudsc2(xr, prm, ptsphy, lay.ngptot, satur=satur, sparse=True), weights)
    g = torch.autograd.grad([ys.fplsl], [xs[n] for n in NARROW_IN], [u["fplsl"]])
    gr = torch.autograd.grad([ref["fplsl"]], [xr[n] for n in NARROW_IN], [u["fplsl"]])
    assert all(same_bits(a, b) for a, b in zip(g, gr))


def test_one_block_of_128_columns(state):
    prm, x, ptsphy, lay, names = setup(state, True, nproma=128, ngptot=128, levapls2=True)
    weights = all_weights(lay)
    u = ybars(B.OUT_NAMES, lay, seed=8)
    xs, xr = leaves(x, NARROW_IN), leaves(x, NARROW_IN)
    ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, 128, weights=weights, satur=True)
    ref = folded(ag.cloudsc2(xr, prm, ptsphy, 128, satur=True, sparse=True), weights)
    for n in B.OUT_NAMES:
        assert same_bits(getattr(ys, n).detach(), ref[n].detach()), n
    g = torch.autograd.grad(list(ys), [xs[n] for n in NARROW_IN], [u[n] for n in B.OUT_NAMES])
    gr = torch.autograd.grad([ref[n] for n in B.OUT_NAMES], [xr[n] for n in NARROW_IN], [u[n] for n in B.OUT_NAMES])
    assert all(same_bits(a, b) for a, b in zip(g, gr))


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
def test_forward_mode_sums_are_the_fold_over_the_dense_jvp(state, satur):
    import torch.autograd.forward_ad as fwad

    prm, x, ptsphy, lay, names = setup(state, satur, levapls2=True)
    weights = all_weights(lay)
    wn = tuple(B.OUT_NAMES)
    for tangent_names in (NARROW_IN, names):  # only the tangents of t and q; every tangent
        v = {n: 0.01 * x[n] for n in tangent_names}

        def dense(*ts):
            xs = dict(x)
            xs.update(zip(tangent_names, ts))
            return tuple(ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur))

        def sums(*ts):
            xs = dict(x)
            xs.update(zip(tangent_names, ts))
            return tuple(ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights, satur=satur))
        primals, tangents = tuple(x[n] for n in tangent_names), tuple(v[n] for n in tangent_names)
        _, dy = torch.func.jvp(dense, primals, tangents)
        want = {n: fold(weights[n], d) for n, d in zip(B.OUT_NAMES, dy)}
        ys, dys = torch.func.jvp(sums, primals, tangents)
        for n, d in zip(wn, dys):
            assert same_bits(d, want[n]) and tail_zero(d, lay), n
        with fwad.dual_level():
            xs = dict(x)
            xs.update({n: fwad.make_dual(x[n], v[n]) for n in tangent_names})
            out = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights, satur=satur)
            for n in wn:
                assert same_bits(fwad.unpack_dual(getattr(out, n)).tangent, want[n]), n


def test_torch_func_grad_and_vjp(state):
    prm, x, ptsphy, lay, names = setup(state, False)
    weights = surface_weights(lay)
    u = ybars(NARROW_OUT, lay, seed=9)

    def sums(q, t):
        xs = dict(x)
        xs.update(q=q, t=t)
        ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights)
        return ys.fplsl, ys.fplsn

    def ref(q, t):
        xs = dict(x)
        xs.update(q=q, t=t)
        out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, sparse=True)
        return fold(weights["fplsl"], out.fplsl), fold(weights["fplsn"], out.fplsn)

    def loss(f):
        return lambda q, t: sum(torch.sum(w * o) for w, o in zip((u["fplsl"], u["fplsn"]), f(q, t)))
    res = {}
    for f in (sums, ref):
        _, pull = torch.func.vjp(f, x["q"], x["t"])
        res[f] = list(pull((u["fplsl"], u["fplsn"]))) + list(torch.func.grad(loss(f), argnums=(0, 1))(x["q"], x["t"]))
    assert all(same_bits(a, b) for a, b in zip(res[sums], res[ref]))


def test_what_is_refused(state):
    prm, x, ptsphy, lay, names = setup(state, False)
    weights = surface_weights(lay)
    u = ybars(NARROW_OUT, lay, seed=10)

    def sums(q, t):
        xs = dict(x)
        xs.update(q=q, t=t)
        ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights)
        return ys.fplsl, ys.fplsn
    q2, t2 = torch.stack([x["q"], x["q"]]), torch.stack([x["t"], x["t"]])
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.func.vmap(sums)(q2, t2)
    with pytest.raises(NotImplementedError):
        torch.func.jacrev(lambda q, t: torch.stack([torch.sum(s) for s in sums(q, t)]), argnums=(0, 1))(x["q"], x["t"])
    with pytest.raises(NotImplementedError):
        torch.func.jacfwd(lambda q: torch.stack([torch.sum(s) for s in sums(q, x["t"])]))(x["q"])
    xs = leaves(x, NARROW_IN)
    ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad([ys.fplsl], [xs["q"]], [torch.stack([u["fplsl"], u["fplsl"]])], is_grads_batched=True)
    ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights)
    g, = torch.autograd.grad([ys.fplsl], [xs["q"]], [u["fplsl"]], create_graph=True)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad([g.sum()], [xs["t"]])
    w = dict(weights)
    w["fplsl"] = w["fplsl"].clone().requires_grad_(True)
    with pytest.raises(ValueError, match=r"weights\['fplsl'\] requires grad"):
        ag.cloudsc2_column_sums(x, prm, ptsphy, lay.ngptot, weights=w)
    with pytest.raises(ValueError, match=r"weights\['fplsn'\] is on cpu"):
        ag.cloudsc2_column_sums(x, prm, ptsphy, lay.ngptot, weights=dict(weights, fplsn=weights["fplsn"].cpu()))


def test_graph_capture_replays_the_eager_bits(state):
    prm, x, ptsphy, lay, names = setup(state, False, levapls2=True)
    xs = {n: (t.clone().requires_grad_() if n in NARROW_IN else t.clone()) for n, t in x.items()}
    weights = surface_weights(lay)
    u = ybars(NARROW_OUT, lay, seed=11)

    def step():
        ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights)
        grads = torch.autograd.grad([ys.fplsl, ys.fplsn], [xs[n] for n in NARROW_IN], [u["fplsl"], u["fplsn"]])
        return [ys.fplsl.detach(), ys.fplsn.detach()], list(grads)

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
    with torch.no_grad():  # an input overwritten in place: the replay gives the new eager bits
        xs["t"].copy_(xs["t"] + 0.25)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in cap_out + cap_g]
    second = eager()
    assert all(same_bits(a, b) for a, b in zip(second, replayed))
    assert not all(same_bits(a, b) for a, b in zip(first, second))


def test_no_plane_is_allocated_that_the_route_does_not_need(state):
    """four blocks (a full-level plane = 4 x 137 x 32 elements): peak memory across the calls, the dense route printed next to each"""
    weights_of = surface_weights
    for flags, kept in ((dict(), 2), (dict(levapls2=True, lregcl=True), 3)):
        prm, x, ptsphy, lay, names = setup(state, False, **flags)
        weights = weights_of(lay)
        plane = lay.nblocks * lay.nlev * lay.nproma * x["t"].element_size()
        u = ybars(NARROW_OUT, lay, seed=12)

        def rise_of(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(DEV)
            before = torch.cuda.memory_allocated(DEV)
            keep = fn()
            torch.cuda.synchronize()
            return (torch.cuda.max_memory_allocated(DEV) - before) / plane, keep

        def dense_forward(xs):
            out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, sparse=True)
            return torch.einsum("k,bkc->bc", weights["fplsl"], out.fplsl), torch.einsum("k,bkc->bc", weights["fplsn"], out.fplsn)
        # the route's own small arrays: the table and the sums (warm-up, so that no first-use allocation of the library is counted)
        with torch.no_grad():
            ag.cloudsc2_column_sums(x, prm, ptsphy, lay.ngptot, weights=weights)
            lean, _ = rise_of(lambda: ag.cloudsc2_column_sums(x, prm, ptsphy, lay.ngptot, weights=weights))
            lean_dense, _ = rise_of(lambda: dense_forward(x))
        xs = leaves(x, NARROW_IN)
        tracking, ys = rise_of(lambda: ag.cloudsc2_column_sums(xs, prm, ptsphy, lay.ngptot, weights=weights))
        back, g = rise_of(lambda: torch.autograd.grad([ys.fplsl, ys.fplsn], [xs[n] for n in NARROW_IN], [u["fplsl"], u["fplsn"]]))
        xd = leaves(x, NARROW_IN)
        tracking_dense, yd = rise_of(lambda: dense_forward(xd))
        back_dense, gd = rise_of(lambda: torch.autograd.grad(list(yd), [xd[n] for n in NARROW_IN], [u["fplsl"], u["fplsn"]]))
        print(f"{flags}: peak memory rise in full-level planes: no-grad forward {lean:.3f} (dense route {lean_dense:.2f}), grad-tracking "
              f"forward {tracking:.3f} ({tracking_dense:.2f}), narrow backward {back:.3f} ({back_dense:.2f})")
        half = (lay.nlev + 1) / lay.nlev  # a kept flux plane has nlev + 1 levels
        assert lean < 1.0, lean
        assert tracking < (2 * half + (kept - 2)) + 1.0, tracking
        assert back < 2.0 + 1.0, back
        del ys, g, yd, gd
