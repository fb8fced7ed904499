"""Batched tangents and cotangents on the MI355X: cloudsc2_tl_launch_batch / cloudsc2_vjp_launch_batch against K single launches bit
for bit (a chunk, a split, a ragged split; the paced size; the 64-bit-offset variants), and the op under torch.func.vmap / jacfwd /
jacrev against Python loops over the unbatched op."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, make_inputs, new, params, same_bits, seeded, stream, tail_zero, tl_launch
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

KMAX = B.lib.cloudsc2_batch_max()
FLAGS = [dict(), dict(levapls2=True), dict(ldrain1d=True), dict(lregcl=True)]
NAN = float("nan")


def forward_launch(x, prm, ptsphy, lay):
    """the trajectory pass: PFPLSL5 / PFPLSN5 and the cover checkpoints"""
    traj = new(B.OUT_NAMES, lay)
    scratch = torch.zeros((lay.nblocks, lay.nlev, lay.nproma), dtype=B.torch_real(), device=DEV)
    B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                             C.byref(ag._block("out", traj, lay)), C.c_void_p(scratch.data_ptr()), stream()))
    return ag._block("out", {"fplsl": traj["fplsl"], "fplsn": traj["fplsn"]}, lay), scratch, traj


def vjp_launch(x, traj_out, scratch, y, prm, ptsphy, lay, fill=NAN):
    xa = new(B.IN_NAMES, lay, fill=fill)
    B.check(B.lib.cloudsc2_vjp_launch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                      C.byref(traj_out), C.byref(ag._block("in", xa, lay)), C.byref(ag._block("out", y, lay)),
                                      C.c_void_p(scratch.data_ptr()), stream()))
    return xa


def tl_launch_nan(x, dx, prm, ptsphy, lay):
    dy = new(B.OUT_NAMES, lay, fill=NAN)
    B.check(B.lib.cloudsc2_tl_launch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                     C.byref(B.Outputs()), C.byref(ag._block("in", dx, lay)), C.byref(ag._block("out", dy, lay)),
                                     stream()))
    return dy


def blocks(kind, per_direction, lay):
    return ag._block_array(kind, per_direction, lay)


def tl_batch_rc(x, dxs, dys, prm, ptsphy, lay):
    return B.lib.cloudsc2_tl_launch_batch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                          len(dxs), blocks("in", dxs, lay), blocks("out", dys, lay), stream())


def vjp_batch_rc(x, traj_out, scratch, xas, ys, prm, ptsphy, lay):
    return B.lib.cloudsc2_vjp_launch_batch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                           C.byref(traj_out), len(ys), blocks("in", xas, lay), blocks("out", ys, lay),
                                           C.c_void_p(scratch.data_ptr()), stream())


def tangents(x, lay, k, seed=100):
    """K distinct seeded tangents of the state's own scale"""
    return [{n: x[n] * r for n, r in seeded(B.IN_NAMES, lay, seed + j, scale=0.01).items()} for j in range(k)]


def check_batches_against_singles(x, prm, ptsphy, lay, ks):
    kall = max(ks)
    dxs = tangents(x, lay, kall)
    us = [seeded(B.OUT_NAMES, lay, 200 + j) for j in range(kall)]
    traj_out, scratch, _ = forward_launch(x, prm, ptsphy, lay)
    tl_single = [tl_launch_nan(x, dx, prm, ptsphy, lay) for dx in dxs]
    vjp_single = [vjp_launch(x, traj_out, scratch, u, prm, ptsphy, lay) for u in us]
    for k in ks:
        dys = [new(B.OUT_NAMES, lay, fill=NAN) for _ in range(k)]
        B.check(tl_batch_rc(x, dxs[:k], dys, prm, ptsphy, lay))
        xas = [new(B.IN_NAMES, lay, fill=NAN) for _ in range(k)]
        ys = [{n: t.clone() for n, t in u.items()} for u in us[:k]]
        B.check(vjp_batch_rc(x, traj_out, scratch, xas, ys, prm, ptsphy, lay))
        torch.cuda.synchronize()
        for j in range(k):
            for n in B.OUT_NAMES:  # (NaN-filled before: equal bits include the untouched tail)
                assert same_bits(dys[j][n], tl_single[j][n]), ("TL batch != single", k, j, n)
                assert same_bits(ys[j][n], us[j][n]), ("output adjoint changed", k, j, n)
                assert bool(torch.all(torch.isfinite(dys[j][n][-1, :, :lay.tail]))), ("active element not written", k, j, n)
                assert lay.tail == lay.nproma or bool(torch.all(torch.isnan(dys[j][n][-1, :, lay.tail:]))), ("tail written", k, j, n)
            for n in B.IN_NAMES:
                assert same_bits(xas[j][n], vjp_single[j][n]), ("VJP batch != single", k, j, n)
                assert bool(torch.all(torch.isfinite(xas[j][n][-1, :, :lay.tail]))), ("active element not written", k, j, n)
                assert lay.tail == lay.nproma or bool(torch.all(torch.isnan(xas[j][n][-1, :, lay.tail:]))), ("tail written", k, j, n)


def test_batch_max():
    assert 2 <= KMAX <= 8


@pytest.mark.parametrize("math_mode", [1, 2])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nproma,ngptot", [(32, 100), (100, 1000), (128, 16384)])
def test_batched_launches_equal_single_launches(nproma, ngptot, flags, math_mode):
    tab = c2.random_table(137, 100, seed=21)
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    check_batches_against_singles(x, prm, ptsphy, lay, sorted({1, 2, KMAX, KMAX + 1, 2 * KMAX + 1}))


def test_batched_launches_at_the_paced_size():
    tab = c2.random_table(137, 100, seed=22)
    prm = params(tab)
    x, ptsphy, lay = make_inputs(tab, 128, 160000, prm)
    check_batches_against_singles(x, prm, ptsphy, lay, [KMAX])


@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
def test_batched_launches_with_64_bit_offsets(flags):
    """a layout group whose block stride x nblocks x element size reaches 4 GiB takes the launch off the 32-bit byte offsets (finish()
    in cloudsc2_launch.hip): PL / PI as planes of one packed buffer with a large block stride, for the single launches alike"""
    tab = c2.random_table(137, 100, seed=23)
    prm = params(tab, **flags)
    nproma, ngptot = 128, 16384
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    esize = torch.empty((), dtype=B.torch_real()).element_size()
    planes = -(-(1 << 32) // (esize * lay.nblocks * lay.nlev * nproma))  # block stride = planes x nlev x nproma elements
    packed = torch.zeros((lay.nblocks, planes, lay.nlev, nproma), dtype=B.torch_real(), device=DEV)
    assert packed.stride(0) * lay.nblocks * esize >= 1 << 32
    packed[:, 0] = x["l"]
    packed[:, planes - 1] = x["i"]
    x = dict(x, l=packed[:, 0], i=packed[:, planes - 1])
    check_batches_against_singles(x, prm, ptsphy, lay, [KMAX, KMAX + 1])


def test_batched_launches_refuse_what_they_cannot_take():
    tab = c2.random_table(137, 100, seed=24)
    prm = params(tab)
    x, ptsphy, lay = make_inputs(tab, 32, 100, prm)
    dxs = tangents(x, lay, 2)
    dys = [new(B.OUT_NAMES, lay) for _ in range(2)]
    traj_out, scratch, _ = forward_launch(x, prm, ptsphy, lay)
    us = [seeded(B.OUT_NAMES, lay, 300 + j) for j in range(2)]
    xas = [new(B.IN_NAMES, lay) for _ in range(2)]
    B.check(tl_batch_rc(x, dxs, dys, prm, ptsphy, lay))
    B.check(vjp_batch_rc(x, traj_out, scratch, xas, us, prm, ptsphy, lay))
    # the second direction's PGTEN* planes with another block stride than the first's
    wide = torch.zeros((lay.nblocks, 2, lay.nlev, lay.nproma), dtype=B.torch_real(), device=DEV)
    odd = dict(dxs[1], gtent=wide[:, 0], gtenq=wide[:, 1], gtenl=wide[:, 0], gteni=wide[:, 1])
    assert tl_batch_rc(x, [dxs[0], odd], dys, prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    assert b"same block stride" in B.lib.cloudsc2_last_error()
    odd = dict(xas[1], gtent=wide[:, 0], gtenq=wide[:, 1], gtenl=wide[:, 0], gteni=wide[:, 1])
    assert vjp_batch_rc(x, traj_out, scratch, [xas[0], odd], us, prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    # no directions, no qsat, a NULL field
    assert tl_batch_rc(x, [], [], prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    assert vjp_batch_rc(x, traj_out, scratch, [], [], prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    noq = {n: (None if n == "qsat" else t) for n, t in x.items()}
    assert tl_batch_rc(noq, dxs, dys, prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    assert vjp_batch_rc(noq, traj_out, scratch, xas, us, prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    hole = dict(dxs[1], t=None)
    assert tl_batch_rc(x, [dxs[0], hole], dys, prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    hole = dict(us[1], clc=None)
    assert vjp_batch_rc(x, traj_out, scratch, xas, [us[0], hole], prm, ptsphy, lay) == B.CLOUDSC2_EINVAL
    torch.cuda.synchronize()


def test_batched_kernels_have_an_occupancy_and_a_pacing_verdict():
    B.check(B.lib.cloudsc2_device_prepare())
    for kernel in (4, 5):
        for flags in (1, 3, 5, 7, 33, 35, 37, 39):
            per_cu = C.c_int(0)
            B.check(B.lib.cloudsc2_kernel_occupancy(kernel, flags + 64 * KMAX, C.byref(per_cu)))  # (built per direction count)
            assert per_cu.value >= 1
            nap, pacing = C.c_int(-2), C.c_int(-2)
            B.check(B.lib.cloudsc2_device_rules(per_cu.value, C.byref(nap), C.byref(pacing)))
            assert pacing.value in (0, 1), (kernel, flags, per_cu.value)  # probed: this occupancy is in device_prepare's list
        assert B.lib.cloudsc2_kernel_occupancy(kernel, 64 * KMAX, C.byref(per_cu)) == B.CLOUDSC2_EINVAL  # no variant without qsat
        assert B.lib.cloudsc2_kernel_occupancy(kernel, 1 + 64 * (KMAX + 1), C.byref(per_cu)) == B.CLOUDSC2_EINVAL


# ---- through torch ------------------------------------------------------------------------------------------------------------

KEYS = list(B.IN_NAMES)


def op(prm, ptsphy, lay):
    def f(*xs):
        return tuple(ag.cloudsc2(dict(zip(KEYS, xs)), prm, ptsphy, lay.ngptot))
    return f


@pytest.mark.parametrize("flags", [dict(lregcl=True), dict(levapls2=True)])
def test_vmap_of_jvp_and_vjp_equal_python_loops(flags):
    tab = c2.random_table(137, 100, seed=25)
    prm = params(tab, **flags)
    x, ptsphy, lay = make_inputs(tab, 64, 1000, prm)  # a padded tail
    f = op(prm, ptsphy, lay)
    xs = tuple(x[n] for n in KEYS)
    K = 2 * KMAX + 1
    dxs = tangents(x, lay, K)

    # tangents for every input
    V = tuple(torch.stack([d[n] for d in dxs]) for n in KEYS)
    got = torch.func.vmap(lambda *v: torch.func.jvp(f, xs, v)[1])(*V)
    for j in range(K):
        want = torch.func.jvp(f, xs, tuple(dxs[j][n] for n in KEYS))[1]
        for k, n in enumerate(B.OUT_NAMES):
            assert same_bits(got[k][j], want[k]), ("vmap(jvp)", j, n)
            assert tail_zero(got[k][j], lay), n
    # tangents for a subset of the inputs only (the others have none: shared zero planes)
    sub = lambda t, q: f(*[t if n == "t" else q if n == "q" else x[n] for n in KEYS])  # noqa: E731
    Vt, Vq = V[KEYS.index("t")], V[KEYS.index("q")]
    got = torch.func.vmap(lambda vt, vq: torch.func.jvp(sub, (x["t"], x["q"]), (vt, vq))[1])(Vt, Vq)
    for j in range(K):
        dx0 = {n: (dxs[j][n] if n in ("t", "q") else torch.zeros_like(x[n])) for n in KEYS}
        want = tl_launch(x, dx0, prm, ptsphy, lay)
        for k, n in enumerate(B.OUT_NAMES):
            assert same_bits(got[k][j], want[n]), ("vmap(jvp), partial tangents", j, n)

    # cotangents for every output
    us = [seeded(B.OUT_NAMES, lay, 400 + j) for j in range(K)]
    U = tuple(torch.stack([u[n] for u in us]) for n in B.OUT_NAMES)
    _, pullback = torch.func.vjp(f, *xs)
    got = torch.func.vmap(pullback)(U)
    for j in range(K):
        want = pullback(tuple(us[j][n] for n in B.OUT_NAMES))
        for k, n in enumerate(KEYS):
            assert same_bits(got[k][j], want[k]), ("vmap(vjp)", j, n)
            assert tail_zero(got[k][j], lay), n
    # cotangents for two outputs only: the op's backward sees None for the others
    two = lambda *a: (lambda o: (o[B.OUT_NAMES.index("tent")], o[B.OUT_NAMES.index("fplsl")]))(f(*a))  # noqa: E731
    _, pullback2 = torch.func.vjp(two, *xs)
    U2 = (U[B.OUT_NAMES.index("tent")], U[B.OUT_NAMES.index("fplsl")])
    got = torch.func.vmap(pullback2)(U2)
    for j in range(K):
        want = pullback2((us[j]["tent"], us[j]["fplsl"]))
        for k, n in enumerate(KEYS):
            assert same_bits(got[k][j], want[k]), ("vmap(vjp), None cotangents", j, n)
    torch.cuda.synchronize()


@pytest.mark.skipif(B.SINGLE, reason="the 1e-11 agreement of TL and AD is an fp64 statement")
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True)])
def test_jacfwd_and_jacrev_agree(flags):
    """The adjoint identity, K directions at a time: the Jacobian of ten weighted field sums with respect to a handful of input
    elements (a one-hot basis), forward mode through the batched TL sweep against reverse mode through the batched reverse sweep,
    to the TL / AD tolerance of 1e-11 relative in max norm, per Jacobian block (output field, input field)."""
    tab = c2.random_table(137, 100, seed=26)
    prm = params(tab, **flags)
    x, ptsphy, lay = make_inputs(tab, 32, 64, prm)
    f = op(prm, ptsphy, lay)
    # fixed positive weights: a plain sum of a flux-form tendency is a conserved quantity whose derivative is all cancellation
    w = [0.5 + torch.rand(lay.shape(n), generator=torch.Generator(device=DEV).manual_seed(500 + k), dtype=B.torch_real(), device=DEV)
         for k, n in enumerate(B.OUT_NAMES)]
    fields = ("t", "q", "l", "i", "supsat", "pap")
    spots = [(0, 90, 3), (1, 110, 17), (1, 125, 30)]  # (block, level, column) of the selected elements, cloud levels
    basis = {n: torch.zeros((len(spots),) + lay.shape(n), dtype=B.torch_real(), device=DEV) for n in fields}
    for n in fields:
        for j, s in enumerate(spots):
            basis[n][(j,) + s] = 1.0

    def g(z):  # z: (fields, spots)
        xs = [x[n] + torch.tensordot(z[fields.index(n)], basis[n], dims=1) if n in fields else x[n] for n in KEYS]
        return torch.stack([torch.sum(wk * o) for wk, o in zip(w, f(*xs))])

    z0 = torch.zeros((len(fields), len(spots)), dtype=B.torch_real(), device=DEV)
    jf = torch.func.jacfwd(g)(z0)  # (10, fields, spots)
    jr = torch.func.jacrev(g)(z0)
    torch.cuda.synchronize()
    assert jf.shape == jr.shape == (10, len(fields), len(spots))
    assert bool(torch.any(jf != 0))
    worst = 0.0
    for k, on in enumerate(B.OUT_NAMES):
        for i, n in enumerate(fields):
            a, b = jf[k, i], jr[k, i]
            scale = float(torch.max(torch.abs(a)))
            diff = float(torch.max(torch.abs(a - b)))
            rel = 0.0 if diff == 0.0 else diff / scale if scale > 0.0 else float("inf")
            print(f"jacobian block d {on} / d {n}: max |entry| {scale:.3e}, max |jacfwd - jacrev| {diff:.3e}, relative {rel:.3e}")
            worst = max(worst, rel)
            assert rel <= 1e-11, (on, n, rel)
    print("worst block:", worst)


@pytest.mark.parametrize("nproma,ngptot", [(32, 128), (32, 100)])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
def test_vmap_over_states_equals_separate_calls(nproma, ngptot, flags):
    prms, states = None, []
    for seed in (27, 28, 29):
        tab = c2.random_table(137, 100, seed=seed)
        prms = prms or params(tab, **flags)  # (one vertical grid: CETA comes from the first table)
        x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prms)
        states.append(x)
    f = op(prms, ptsphy, lay)
    X = tuple(torch.stack([s[n] for s in states]) for n in KEYS)
    got = torch.func.vmap(f)(*X)
    # a batch of states with a batch of cotangents: vmap over grad
    loss = lambda *xs: sum(torch.sum(o) for o in f(*xs))  # noqa: E731
    ggot = torch.func.vmap(torch.func.grad(loss, argnums=(KEYS.index("t"), KEYS.index("q"))))(*X)
    for j, s in enumerate(states):
        want = f(*(s[n] for n in KEYS))
        for k, n in enumerate(B.OUT_NAMES):
            assert same_bits(got[k][j], want[k]), ("vmap(f)", j, n)
            assert tail_zero(got[k][j], lay), ("padded tail", j, n)
        gwant = torch.func.grad(loss, argnums=(KEYS.index("t"), KEYS.index("q")))(*(s[n] for n in KEYS))
        for a, b in zip(ggot, gwant):
            assert same_bits(a[j], b), ("vmap(grad)", j)
            assert tail_zero(a[j], lay)
    # only some inputs batched: the others are expanded
    part = torch.func.vmap(lambda t: f(*[t if n == "t" else states[0][n] for n in KEYS]))(X[KEYS.index("t")])
    for j, s in enumerate(states):
        want = f(*[s["t"] if n == "t" else states[0][n] for n in KEYS])
        for k, n in enumerate(B.OUT_NAMES):
            assert same_bits(part[k][j], want[k]), ("vmap(f), one batched input", j, n)
    torch.cuda.synchronize()


def test_nested_vmap_and_batched_grads_are_refused():
    tab = c2.random_table(137, 100, seed=30)
    prm = params(tab)
    x, ptsphy, lay = make_inputs(tab, 32, 64, prm)
    f = op(prm, ptsphy, lay)
    T = torch.stack([x["t"], x["t"]]).unsqueeze(0)
    with pytest.raises(NotImplementedError):
        torch.func.vmap(torch.func.vmap(lambda t: f(*[t if n == "t" else x[n] for n in KEYS])))(T)
    xt = x["t"].clone().requires_grad_()
    out = f(*[xt if n == "t" else x[n] for n in KEYS])
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(out[0], xt, torch.ones((2,) + tuple(out[0].shape), dtype=B.torch_real(), device=DEV), is_grads_batched=True)
    torch.cuda.synchronize()


def test_graph_capture_of_a_batched_jvp_replays_the_eager_bits():
    tab = c2.random_table(137, 100, seed=31)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = make_inputs(tab, 64, 1000, prm)
    f = op(prm, ptsphy, lay)
    xs = tuple(x[n] for n in KEYS)
    K = KMAX + 1
    dxs = tangents(x, lay, K)
    V = tuple(torch.stack([d[n] for d in dxs]) for n in KEYS)

    def step():
        return list(torch.func.vmap(lambda *v: torch.func.jvp(f, xs, v)[1])(*V))

    eager = [t.clone() for t in step()]  # the eager call: device probe and CETA table before the capture
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = step()
    for t in cap:
        t.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, cap):
        assert same_bits(a, b)
