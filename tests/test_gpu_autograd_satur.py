"""The differentiable op with SATUR inside (``cloudsc2(..., satur=True)``: cloudsc2_tl_launch_satur / cloudsc2_vjp_launch_satur) and the
differentiable ``satur`` (cloudsc2_satur_lin_launch) on the MI355X.  The fused op against the unfused route -- ``satur(pap, t,
differentiable=True)`` fed to the plain op, torch's chain rule in between -- to 1e-11 of a field's maximum (the project's TL / AD
tolerance); the forward bit for bit against the NL sweep with SATUR fused; the dot-product identity to 1e-12; batches; graph capture."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, make_inputs, new, nl_launch, params, rel_err, same_bits, seeded, stream, tail_zero
from tests.satur_lin_ref import satur_partials_numpy
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

KEYS = list(ag.SAT_NAMES)
FLAGS = [dict(), dict(levapls2=True, lregcl=True), dict(ldrain1d=True), dict(lregcl=True)]
TLAD_TOL = 1e-11
fp64_only = pytest.mark.skipif(B.SINGLE, reason="the 1e-11 / 1e-12 bounds are fp64 statements")


def inputs15(tab, nproma, ngptot, prm):
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    return {n: x[n] for n in KEYS}, ptsphy, lay


def fused(prm, ptsphy, lay):
    def f(*xs):
        return tuple(ag.cloudsc2(dict(zip(KEYS, xs)), prm, ptsphy, lay.ngptot, satur=True))
    return f


def unfused(prm, ptsphy, lay):
    """what a user would otherwise write: the differentiable SATUR, the plain op, torch's chain rule"""
    def f(*xs):
        x = dict(zip(KEYS, xs))
        x["qsat"] = ag.satur(x["pap"], x["t"], prm, lay.ngptot, differentiable=True)
        return tuple(ag.cloudsc2(x, prm, ptsphy, lay.ngptot))
    return f


@pytest.mark.parametrize("nproma,ngptot", [(32, 100), (128, 16384), (4096, 4096)])
def test_forward_is_the_nl_sweep_with_satur_fused(nproma, ngptot):
    tab = c2.synthetic_table()
    prm = params(tab)
    x, ptsphy, lay = inputs15(tab, nproma, ngptot, prm)
    out = ag.cloudsc2(x, prm, ptsphy, ngptot, satur=True)
    want = nl_launch(x, prm, ptsphy, lay)  # no qsat in the block: SATUR fused
    torch.cuda.synchronize()
    assert isinstance(out, ag.Cloudsc2Outputs)
    for n in B.OUT_NAMES:
        assert same_bits(getattr(out, n), want[n]), n
        assert tail_zero(getattr(out, n), lay), n


@pytest.mark.parametrize("math_mode", [1, 2])
def test_satur_lin_launch(math_mode):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode)
    x, _, lay = inputs15(tab, 32, 100, prm)
    f = lambda t, n="pap": ag._field(t, lay, n)  # noqa: E731
    q0, q1, dp, dt, dp2, dt2 = (torch.full(lay.shape("pap"), float("nan"), dtype=B.torch_real(), device=DEV) for _ in range(6))
    B.check(B.lib.cloudsc2_satur_launch(C.byref(prm), lay.nproma, lay.nlev, lay.ngptot, f(x["pap"]), f(x["t"]), f(q0), stream()))
    B.check(B.lib.cloudsc2_satur_lin_launch(C.byref(prm), lay.nproma, lay.nlev, lay.ngptot, f(x["pap"]), f(x["t"]), f(q1), f(dp), f(dt),
                                            stream()))
    B.check(B.lib.cloudsc2_satur_lin_launch(C.byref(prm), lay.nproma, lay.nlev, lay.ngptot, f(x["pap"]), f(x["t"]), B.Field(), f(dp2),
                                            f(dt2), stream()))  # partials only
    torch.cuda.synchronize()
    assert same_bits(q0, q1), "qsat of cloudsc2_satur_lin_launch != cloudsc2_satur_launch (NaN tail included: not written)"
    assert same_bits(dp, dp2) and same_bits(dt, dt2)
    act = torch.zeros(lay.shape("pap"), dtype=torch.bool, device=DEV)
    act[:-1] = True
    act[-1, :, :lay.tail] = True
    assert bool(torch.all(torch.isnan(dp[~act]))) and bool(torch.all(torch.isnan(dt[~act]))), "padded tail written"
    if not B.SINGLE:
        pap, t = x["pap"].cpu().numpy(), x["t"].cpu().numpy()
        a = act.cpu().numpy()
        ndp, ndt, clamped = satur_partials_numpy(prm, np.where(a, pap, 1.0), np.where(a, t, 250.0))
        gp, gt = dp.cpu().numpy(), dt.cpu().numpy()
        assert clamped[a].sum() > 0 and np.all(gp[a & clamped] == 0.0) and np.all(gt[a & clamped] == 0.0)
        free = a & ~clamped
        ep = float(np.max(np.abs(gp[free] - ndp[free]) / np.abs(ndp[free])))
        et = float(np.max(np.abs(gt[free] - ndt[free]) / np.abs(ndt[free])))
        print(f"math_mode {math_mode}: partials against the numpy restatement: dqs/dpap {ep:.3e}, dqs/dt {et:.3e}")
        assert ep <= 1e-8 and et <= 1e-8


@fp64_only
@pytest.mark.parametrize("math_mode", [1, 2])
@pytest.mark.parametrize("flags", FLAGS)
def test_backward_and_jvp_against_the_unfused_route(math_mode, flags):
    tab = c2.random_table(137, 100, seed=5)  # nonzero PSUPSAT
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = inputs15(tab, 32, 100, prm)  # a padded tail
    u = seeded(B.OUT_NAMES, lay, seed=1)
    v = {n: 0.01 * t for n, t in x.items()}
    grads, tans, prims = [], [], []
    for route in (fused, unfused):
        f = route(prm, ptsphy, lay)
        xs = [x[n].clone().requires_grad_() for n in KEYS]
        out = f(*xs)
        grads.append(torch.autograd.grad(list(out), xs, [u[n] for n in B.OUT_NAMES]))
        prim, tan = torch.func.jvp(f, tuple(x[n] for n in KEYS), tuple(v[n] for n in KEYS))
        tans.append(tan)
        prims.append(prim)
    import torch.autograd.forward_ad as fwAD

    with fwAD.dual_level():
        out = ag.cloudsc2({n: fwAD.make_dual(x[n], v[n]) for n in KEYS}, prm, ptsphy, lay.ngptot, satur=True)
        tan2 = [fwAD.unpack_dual(o).tangent for o in out]
    torch.cuda.synchronize()
    bit_equal = []
    for k, n in enumerate(KEYS):
        e = rel_err(grads[0][k], grads[1][k])
        assert tail_zero(grads[0][k], lay), n
        assert e <= TLAD_TOL, ("gradient", n, e)
        if n not in ("pap", "t"):
            bit_equal.append(same_bits(grads[0][k], grads[1][k]))
    assert bool(torch.any(grads[0][KEYS.index("t")] != 0)) and bool(torch.any(grads[0][KEYS.index("supsat")] != 0))
    print(f"math_mode {math_mode} {flags}: {sum(bit_equal)} of {len(bit_equal)} gradients other than pap, t are the bits of the unfused op")
    for k, n in enumerate(B.OUT_NAMES):
        e = rel_err(tans[0][k], tans[1][k])
        assert e <= TLAD_TOL, ("tangent", n, e)
        assert same_bits(tan2[k], tans[0][k]), ("forward_ad != torch.func.jvp", n)
        assert same_bits(prims[0][k], prims[1][k]), ("primal", n)
        assert tail_zero(tans[0][k], lay), n


@fp64_only
@pytest.mark.parametrize("table", ["synthetic", "random"])
def test_adjoint_identity_through_the_torch_apis(table):
    tab = c2.synthetic_table() if table == "synthetic" else c2.random_table(137, 100, seed=8)
    prm = params(tab, lregcl=True)
    x, ptsphy, lay = inputs15(tab, 128, 16384, prm)
    v = {n: 0.01 * t for n, t in x.items()}
    v["supsat"] = 1e-3 * x["q"]
    f = fused(prm, ptsphy, lay)
    _, u = torch.func.jvp(f, tuple(x[n] for n in KEYS), tuple(v[n] for n in KEYS))
    _, pullback = torch.func.vjp(f, *(x[n] for n in KEYS))
    xa = pullback(u)
    lhs = sum(float(torch.sum(t.double() * t.double())) for t in u)
    rhs = sum(float(torch.sum(v[n].double() * a.double())) for n, a in zip(KEYS, xa))
    print(f"{table}: <TL v, u> = {lhs!r}, <v, VJP u> = {rhs!r}, relative {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) / abs(lhs) <= 1e-12, (lhs, rhs)


@fp64_only
@pytest.mark.parametrize("flags", [dict(lregcl=True), dict(levapls2=True)])
@pytest.mark.parametrize("K", [1, 4, 5])
def test_batched_directions_against_a_python_loop(K, flags):
    """vmap(jvp) and vmap(vjp_fn) of the fused op run by composition (one cloudsc2_satur_lin_launch, the batched sweeps with qsat as a
    plane, the chain rule in torch): 1e-11 against a loop over the unbatched fused op, not its bits"""
    tab = c2.random_table(137, 100, seed=25)
    prm = params(tab, **flags)
    x, ptsphy, lay = inputs15(tab, 64, 1000, prm)  # a padded tail
    f = fused(prm, ptsphy, lay)
    xs = tuple(x[n] for n in KEYS)
    dxs = [{n: x[n] * r for n, r in seeded(KEYS, lay, 100 + j, scale=0.01).items()} for j in range(K)]
    V = tuple(torch.stack([d[n] for d in dxs]) for n in KEYS)
    got = torch.func.vmap(lambda *v: torch.func.jvp(f, xs, v)[1])(*V)
    for j in range(K):
        want = torch.func.jvp(f, xs, tuple(dxs[j][n] for n in KEYS))[1]
        for k, n in enumerate(B.OUT_NAMES):
            e = rel_err(got[k][j], want[k])
            assert e <= TLAD_TOL, ("vmap(jvp)", j, n, e)
            assert tail_zero(got[k][j], lay), n
    # a tangent of t alone: pap's is a shared zero plane
    Vt = V[KEYS.index("t")]
    sub = lambda t: f(*[t if n == "t" else x[n] for n in KEYS])  # noqa: E731
    got = torch.func.vmap(lambda vt: torch.func.jvp(sub, (x["t"],), (vt,))[1])(Vt)
    for j in range(K):
        want = torch.func.jvp(sub, (x["t"],), (dxs[j]["t"],))[1]
        for k, n in enumerate(B.OUT_NAMES):
            assert rel_err(got[k][j], want[k]) <= TLAD_TOL, ("vmap(jvp), t alone", j, n)

    us = [seeded(B.OUT_NAMES, lay, 400 + j) for j in range(K)]
    U = tuple(torch.stack([u[n] for u in us]) for n in B.OUT_NAMES)
    _, pullback = torch.func.vjp(f, *xs)
    got = torch.func.vmap(pullback)(U)
    for j in range(K):
        want = pullback(tuple(us[j][n] for n in B.OUT_NAMES))
        for k, n in enumerate(KEYS):
            e = rel_err(got[k][j], want[k])
            assert e <= TLAD_TOL, ("vmap(vjp)", j, n, e)
            assert tail_zero(got[k][j], lay), n
    torch.cuda.synchronize()


@fp64_only
def test_jacfwd_and_jacrev_against_a_python_loop():
    tab = c2.random_table(137, 100, seed=26)
    prm = params(tab, levapls2=True, lregcl=True)
    x, ptsphy, lay = inputs15(tab, 32, 64, prm)
    f = fused(prm, ptsphy, lay)
    w = [0.5 + torch.rand(lay.shape(n), generator=torch.Generator(device=DEV).manual_seed(500 + k), dtype=B.torch_real(), device=DEV)
         for k, n in enumerate(B.OUT_NAMES)]
    fields = ("t", "pap", "q")
    spots = [(0, 90, 3), (1, 110, 17), (1, 125, 30), (0, 100, 9), (1, 70, 1)]  # five directions per field
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
    # the loop: one unbatched jvp of the fused op per entry of z
    loop = torch.zeros_like(jf)
    for i in range(len(fields)):
        for j in range(len(spots)):
            e = torch.zeros_like(z0)
            e[i, j] = 1.0
            loop[:, i, j] = torch.func.jvp(g, (z0,), (e,))[1]
    torch.cuda.synchronize()
    assert bool(torch.any(loop[:, fields.index("t")] != 0)) and bool(torch.any(loop[:, fields.index("pap")] != 0))
    for k, on in enumerate(B.OUT_NAMES):
        for i, n in enumerate(fields):
            for name, jac in (("jacfwd", jf), ("jacrev", jr)):
                e = rel_err(jac[k, i], loop[k, i])
                print(f"{name} block d {on} / d {n}: relative {e:.3e}")
                assert e <= TLAD_TOL, (name, on, n, e)


@pytest.mark.parametrize("nproma,ngptot", [(32, 128), (32, 100)])
def test_vmap_over_states_equals_separate_calls(nproma, ngptot):
    prm, states = None, []
    for seed in (27, 28, 29):
        tab = c2.random_table(137, 100, seed=seed)
        prm = prm or params(tab, levapls2=True)  # (one vertical grid: CETA comes from the first table)
        x, ptsphy, lay = inputs15(tab, nproma, ngptot, prm)
        states.append(x)
    f = fused(prm, ptsphy, lay)
    X = tuple(torch.stack([s[n] for s in states]) for n in KEYS)
    got = torch.func.vmap(f)(*X)
    loss = lambda *xs: sum(torch.sum(o) for o in f(*xs))  # noqa: E731
    args = (KEYS.index("t"), KEYS.index("pap"), KEYS.index("q"))
    ggot = torch.func.vmap(torch.func.grad(loss, argnums=args))(*X)
    for j, s in enumerate(states):
        want = f(*(s[n] for n in KEYS))
        for k, n in enumerate(B.OUT_NAMES):
            assert same_bits(got[k][j], want[k]), ("vmap(f)", j, n)
            assert tail_zero(got[k][j], lay), ("padded tail", j, n)
        gwant = torch.func.grad(loss, argnums=args)(*(s[n] for n in KEYS))
        for a, b in zip(ggot, gwant):
            assert same_bits(a[j], b), ("vmap(grad)", j)
            assert tail_zero(a[j], lay)
    torch.cuda.synchronize()


def test_what_stays_refused():
    tab = c2.random_table(137, 100, seed=30)
    prm = params(tab)
    x, ptsphy, lay = inputs15(tab, 32, 64, prm)
    f = fused(prm, ptsphy, lay)
    T = torch.stack([x["t"], x["t"]]).unsqueeze(0)
    with pytest.raises(NotImplementedError):
        torch.func.vmap(torch.func.vmap(lambda t: f(*[t if n == "t" else x[n] for n in KEYS])))(T)
    xt = x["t"].clone().requires_grad_()
    out = f(*[xt if n == "t" else x[n] for n in KEYS])
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(out[0], xt, torch.ones((2,) + tuple(out[0].shape), dtype=B.torch_real(), device=DEV), is_grads_batched=True)
    with pytest.raises(NotImplementedError):
        torch.func.vmap(lambda t: ag.satur(x["pap"], t, prm, lay.ngptot, differentiable=True))(T[0])
    with pytest.raises(ValueError, match="qsat"):
        ag.cloudsc2(dict(x, qsat=x["q"]), prm, ptsphy, lay.ngptot, satur=True)
    # the launchers refuse a qsat plane on either side
    dy = new(B.OUT_NAMES, lay)
    withq = dict(x, qsat=x["q"])
    rc = B.lib.cloudsc2_tl_launch_satur(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", withq, lay)),
                                        C.byref(ag._block("in", x, lay)), C.byref(ag._block("out", dy, lay)), stream())
    assert rc == B.CLOUDSC2_EINVAL and b"qsat" in B.lib.cloudsc2_last_error()
    rc = B.lib.cloudsc2_tl_launch_satur(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                        C.byref(ag._block("in", withq, lay)), C.byref(ag._block("out", dy, lay)), stream())
    assert rc == B.CLOUDSC2_EINVAL
    torch.cuda.synchronize()


def test_the_differentiable_satur_defaults_to_the_detached_result():
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab)
    x, _, lay = inputs15(tab, 32, 100, prm)
    pap, t = x["pap"].clone().requires_grad_(), x["t"].clone().requires_grad_()
    q0 = ag.satur(pap, t, prm, lay.ngptot)
    q1 = ag.satur(pap, t, prm, lay.ngptot, differentiable=True)
    assert not q0.requires_grad and q1.requires_grad
    assert same_bits(q0, q1) and tail_zero(q1, lay)
    gp, gt = torch.autograd.grad(torch.sum(q1), [pap, t])
    torch.cuda.synchronize()
    assert tail_zero(gp, lay) and tail_zero(gt, lay) and bool(torch.all(gt >= 0)) and bool(torch.all(gp <= 0))
    assert bool(torch.any(gt > 0))


def test_kernels_of_the_fused_sweeps_have_an_occupancy_and_a_pacing_verdict():
    B.check(B.lib.cloudsc2_device_prepare())
    for kernel, base in ((1, 128), (3, 128 + 8 + 64)):  # C2F_SATLIN; the reverse sweep with C2F_ASSIGN | C2F_VJP
        for flags in (0, 2, 4, 6, 32, 34, 36, 38):
            per_cu = C.c_int(0)
            B.check(B.lib.cloudsc2_kernel_occupancy(kernel, base + flags, C.byref(per_cu)))
            assert per_cu.value >= 1
            nap, pacing = C.c_int(-2), C.c_int(-2)
            B.check(B.lib.cloudsc2_device_rules(per_cu.value, C.byref(nap), C.byref(pacing)))
            assert pacing.value in (0, 1), (kernel, flags, per_cu.value)
        assert B.lib.cloudsc2_kernel_occupancy(kernel, base + 1, C.byref(per_cu)) == B.CLOUDSC2_EINVAL  # never with C2F_QSAT
    assert B.lib.cloudsc2_kernel_occupancy(3, 128, C.byref(per_cu)) == B.CLOUDSC2_EINVAL  # the reverse sweep: the VJP form only


def test_graph_capture_of_the_composed_op_replays_the_eager_bits():
    tab = c2.random_table(137, 100, seed=12)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = inputs15(tab, 64, 1000, prm)
    xs = {n: t.clone().requires_grad_() for n, t in x.items()}
    u = seeded(B.OUT_NAMES, lay, seed=5)

    def step():
        xin = dict(xs, t=(xs["t"] - 1.0) + 1.0, pap=xs["pap"] * 1.0)  # upstream torch ops
        out = ag.cloudsc2(xin, prm, ptsphy, lay.ngptot, satur=True)
        loss = sum(torch.sum(u[n] * torch.tanh(getattr(out, n))) for n in B.OUT_NAMES)  # a downstream one
        grads = torch.autograd.grad(loss, [xs[n] for n in KEYS])
        return [t.detach() for t in out], list(grads)

    eager_out, eager_g = step()  # the eager call: device probe and CETA table before the capture
    eager_out = [t.clone() for t in eager_out]
    eager_g = [t.clone() for t in eager_g]
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_out, cap_g = step()
    for _ in range(2):
        for t in cap_out + cap_g:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager_out + eager_g, cap_out + cap_g):
            assert same_bits(a, b)


def test_views_of_a_packed_buffer_are_not_copied():
    tab = c2.random_table(137, 100, seed=9)
    prm = params(tab)
    x, ptsphy, lay = inputs15(tab, 32, 1000, prm)
    cml = torch.stack([x["gtent"], x["gtenq"], x["gtenl"], x["gteni"]], dim=1)
    clv = torch.stack([x["l"], x["i"]], dim=1)
    xs = dict(x, gtent=cml[:, 0], gtenq=cml[:, 1], gtenl=cml[:, 2], gteni=cml[:, 3], l=clv[:, 0], i=clv[:, 1])
    got = ag.normalize(xs, lay, ag.SAT_GROUPS)
    for n in KEYS:
        assert got[n].data_ptr() == xs[n].data_ptr(), ("copied", n)
    out = ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=True)
    want = ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=True)
    torch.cuda.synchronize()
    for a, b in zip(out, want):
        assert same_bits(a, b)
