"""``cloudsc2_ensemble`` on the MI355X: K parameter sets in one launch, the parameters read on the device.

The promise: member k of every output, every per-member field gradient, every output tangent and every parameter gradient is BIT FOR
BIT what ``cloudsc2(inputs_k, ..., params={the four 0-d values of row k})`` gives.  The gradient of an input all members share is the
members' sum, which holds to the order of summation: the bound is K x 2^-52 times the elementwise sum of the absolute values of the K
single-call gradients, the reordering bound of a K-term sum (nothing measured enters it).

Shapes, the smallest at which the member mapping can go wrong: (a) nproma 24, 3 blocks, ngptot 70 -- 72 padded columns, less than one
workgroup of 128, with a padded tail; (b) nproma 64, ngptot 200 -- 256 padded columns, two workgroups per member, the second with the
padded tail.  K = 1 and K = 3 with three distinct rows, one of them prm's own values."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

from tests.gpu_util import DEV, hip_runtime, make_inputs, names_of, params, same_bits, tail_zero
from tests.util import B, c2, fp64_only
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = [pytest.mark.gpu, fp64_only]

P = c2.PARAM_NAMES
SHAPES = {"a": (24, 70), "b": (64, 200)}
# factors / offsets on prm's values (rlptrc: an offset in K): row 0 is prm's own
ROWS = [dict(rkconv=1.0, rclcrit=1.0, rlptrc=0.0, rpecons=1.0), dict(rkconv=1.3, rclcrit=0.8, rlptrc=-2.0, rpecons=1.1),
        dict(rkconv=0.7, rclcrit=1.25, rlptrc=1.5, rpecons=0.9)]
# (shape, table, flags, satur, K, the names given in params)
CASES = [("a", "synthetic", dict(), False, 3, P),
         ("b", "synthetic", dict(levapls2=True, lregcl=True), True, 3, P),
         ("a", "short", dict(levapls2=True), False, 1, ("rkconv", "rpecons")),
         ("b", "short", dict(lregcl=True), True, 1, P),
         ("b", "synthetic", dict(levapls2=True), False, 3, ("rclcrit", "rlptrc", "rpecons"))]
IDS = [f"{s}-{t}-{'+'.join(k for k in f) or 'plain'}-satur{int(sat)}-K{k}-{len(g)}given" for s, t, f, sat, k, g in CASES]
LOSS = ("tent", "fplsl", "covptot")  # the outputs the losses run over; the others take no part (their gradients are None)

_tables: dict = {}


def table(kind):
    if kind not in _tables:
        _tables[kind] = c2.synthetic_table() if kind == "synthetic" else c2.random_table(24, 100, seed=23)
    return _tables[kind]


def values(prm, K, given):
    """{name: [K values]} of the given names"""
    rows = ROWS[:K] if K > 1 else ROWS[1:2]
    return {n: [getattr(prm, n) + r[n] if n == "rlptrc" else getattr(prm, n) * r[n] for r in rows] for n in given}


def setup(case):
    shape, kind, flags, satur, K, given = case
    nproma, ngptot = SHAPES[shape]
    tab = table(kind)
    prm = params(tab, **flags)
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    x = {n: x[n] for n in names_of(satur)}
    return prm, x, ptsphy, lay, satur, K, values(prm, K, given)


def per_member_t(t, K):
    """a 4-D t, one state per member, as a view with a member stride of two states"""
    buf = torch.full((K, 2) + tuple(t.shape), float("nan"), dtype=t.dtype, device=DEV)
    for k in range(K):
        buf[k, 1] = t * (1.0 + 5e-4 * k)
    return buf[:, 1]


def device_params(vals, requires_grad=False):
    return {n: torch.tensor(v, dtype=torch.float64, device=DEV, requires_grad=requires_grad) for n, v in vals.items()}


def single_params(vals, k, requires_grad=False):
    return {n: torch.tensor(v[k], dtype=torch.float64, device=DEV, requires_grad=requires_grad) for n, v in vals.items()}


def weights(lay, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return {n: torch.randn((K,) + lay.shape(n), generator=g, dtype=B.torch_real(), device=DEV) for n in LOSS}


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_members_outputs_are_the_bits_of_the_single_op(case):
    prm, x, ptsphy, lay, satur, K, vals = setup(case)
    t4 = per_member_t(x["t"], K)
    B.launch_log_reset()
    shared = c2.cloudsc2_ensemble(x, prm, ptsphy, lay.ngptot, satur=satur, params=device_params(vals))
    own = c2.cloudsc2_ensemble(dict(x, t=t4), prm, ptsphy, lay.ngptot, satur=satur, params=device_params(vals))
    assert B.launch_log() == [], "the ensemble kernels are no logged sweep family"
    torch.cuda.synchronize()
    assert isinstance(shared, ag.Cloudsc2Outputs)
    differ = False
    for k in range(K):
        p = single_params(vals, k)
        want_shared = ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params=p)
        want_own = ag.cloudsc2(dict(x, t=t4[k].contiguous()), prm, ptsphy, lay.ngptot, satur=satur, params=p)
        torch.cuda.synchronize()
        for n in B.OUT_NAMES:
            got = getattr(shared, n)
            assert tuple(got.shape) == (K,) + lay.shape(n), n
            assert same_bits(got[k], getattr(want_shared, n)), ("all inputs shared", k, n)
            assert same_bits(getattr(own, n)[k], getattr(want_own, n)), ("4-D t", k, n)
            assert tail_zero(got[k], lay) and tail_zero(getattr(own, n)[k], lay), ("padded tail", k, n)
        differ |= k > 0 and not same_bits(shared.fplsl[k], shared.fplsl[0])
    assert differ or K == 1, "the members' parameters did not reach the kernels"


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_member_by_member_and_the_shared_inputs_sum(case):
    prm, x, ptsphy, lay, satur, K, vals = setup(case)
    t4 = per_member_t(x["t"], K).clone()  # (per member, contiguous)
    w = weights(lay, K, seed=41)
    p = device_params(vals, requires_grad=True)
    xe = dict(x, t=t4.requires_grad_(), q=x["q"].clone().requires_grad_())
    out = c2.cloudsc2_ensemble(xe, prm, ptsphy, lay.ngptot, satur=satur, params=p)
    leaves = [p[n] for n in vals] + [xe["t"], xe["q"]]
    g = torch.autograd.grad([getattr(out, n) for n in LOSS], leaves, [w[n] for n in LOSS], retain_graph=True)
    gp, gt, gq = dict(zip(vals, g[:len(vals)])), g[-2], g[-1]
    # clc and covptot depend on none of the four
    gz = torch.autograd.grad([out.clc, out.covptot], [p[n] for n in vals], [w["covptot"], w["covptot"]])
    torch.cuda.synchronize()
    assert tuple(gt.shape) == tuple(t4.shape) and tuple(gq.shape) == tuple(x["q"].shape)
    for n, a in gp.items():
        assert tuple(a.shape) == (K,) and a.dtype == torch.float64 and a.device == DEV, n
    for a in gz:
        assert bool(torch.all(a == 0)), "clc / covptot-only losses: exact zero parameter gradients"
    sum_q, abs_q = torch.zeros_like(gq), torch.zeros_like(gq)
    for k in range(K):
        pk = single_params(vals, k, requires_grad=True)
        xk = dict(x, t=t4[k].detach().clone().requires_grad_(), q=x["q"].clone().requires_grad_())
        o = ag.cloudsc2(xk, prm, ptsphy, lay.ngptot, satur=satur, params=pk)
        s = torch.autograd.grad([getattr(o, n) for n in LOSS], [pk[n] for n in vals] + [xk["t"], xk["q"]], [w[n][k] for n in LOSS])
        torch.cuda.synchronize()
        for n, a in zip(vals, s):
            assert same_bits(gp[n][k], a), ("parameter gradient", n, k, gp[n][k].item(), a.item())
        assert same_bits(gt[k], s[-2]), ("per-member t gradient", k)
        assert tail_zero(gt[k], lay), k
        sum_q += s[-1]
        abs_q += s[-1].abs()
    err = (gq - sum_q).abs()
    bound = K * 2.0 ** -52 * abs_q
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"shared q gradient: worst error / bound = {worst:.3f} (K = {K})")
    assert bool(torch.all(err <= bound)), ("shared input: the members' sum", worst)
    assert tail_zero(gq, lay) and bool(torch.any(gq != 0))
    if "rpecons" in vals and not (prm.levapls2 or prm.ldrain1d):
        assert bool(torch.all(gp["rpecons"] == 0)), "without the evaporation branch nothing depends on rpecons"


def test_torch_func_grad_and_vjp_give_the_bits_of_backward():
    prm, x, ptsphy, lay, satur, K, vals = setup(CASES[4])
    w = weights(lay, K, seed=45)
    t4 = per_member_t(x["t"], K).clone()
    fixed = {n: v for n, v in device_params(vals).items() if n != "rclcrit"}

    def loss(p, t):
        out = c2.cloudsc2_ensemble(dict(x, t=t), prm, ptsphy, lay.ngptot, satur=satur, params=dict(fixed, rclcrit=p))
        return sum((getattr(out, n) * w[n]).sum() for n in LOSS)

    p = device_params(vals)["rclcrit"]
    pa, ta = p.clone().requires_grad_(), t4.clone().requires_grad_()
    want = torch.autograd.grad(loss(pa, ta), [pa, ta])
    got = torch.func.grad(loss, argnums=(0, 1))(p, t4)
    _, pull = torch.func.vjp(loss, p, t4)
    back = pull(torch.ones((), dtype=B.torch_real(), device=DEV))
    torch.cuda.synchronize()
    for a, b, c in zip(want, got, back):
        assert same_bits(a, b) and same_bits(a, c)
    assert bool(torch.all(want[0] != 0))


# ---- 3. jvp ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jvp_with_parameter_and_field_tangents_is_the_single_ops(case):
    prm, x, ptsphy, lay, satur, K, vals = setup(case)
    names = list(vals)
    t4 = per_member_t(x["t"], K).clone()
    g = torch.Generator(device=DEV).manual_seed(43)
    dt4 = 0.01 * torch.randn(t4.shape, generator=g, dtype=t4.dtype, device=DEV)
    dq = 1e-6 * torch.randn(x["q"].shape, generator=g, dtype=t4.dtype, device=DEV)
    p = device_params(vals)
    dp = {n: 0.01 * p[n] * (1.0 + 0.5 * torch.arange(K, dtype=torch.float64, device=DEV)) for n in names}

    def ens(t, q, *ps):
        return tuple(c2.cloudsc2_ensemble(dict(x, t=t, q=q), prm, ptsphy, lay.ngptot, satur=satur, params=dict(zip(names, ps))))

    out, tan = torch.func.jvp(ens, (t4, x["q"]) + tuple(p[n] for n in names), (dt4, dq) + tuple(dp[n] for n in names))
    torch.cuda.synchronize()
    for k in range(K):
        def one(t, q, *ps):
            return tuple(ag.cloudsc2(dict(x, t=t, q=q), prm, ptsphy, lay.ngptot, satur=satur, params=dict(zip(names, ps))))

        o, d = torch.func.jvp(one, (t4[k].contiguous(), x["q"]) + tuple(p[n][k] for n in names),
                              (dt4[k].contiguous(), dq) + tuple(dp[n][k] for n in names))
        torch.cuda.synchronize()
        for i, n in enumerate(B.OUT_NAMES):
            assert same_bits(out[i][k], o[i]), ("primal", k, n)
            assert same_bits(tan[i][k], d[i]), ("tangent", k, n)
            assert tail_zero(tan[i][k], lay), (k, n)
    assert bool(torch.any(tan[0] != 0))


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------

def graph_is_a_chain(graph) -> int:
    """the captured graph's nodes form ONE chain (so its kernel nodes do), with no memory copy among them; returns the kernel nodes"""
    hip, g = hip_runtime(), C.c_void_p(graph.raw_cuda_graph())
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(count)) == 0 and count.value > 0
    n = count.value
    nodes = (C.c_void_p * n)()
    assert hip.hipGraphGetNodes(g, nodes, C.byref(count)) == 0
    kernels = 0
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0
        assert kind.value in (0, 2), ("neither a kernel nor a memset node (1 would be a copy)", kind.value)  # hipGraphNodeType
        kernels += kind.value == 0
    assert kernels >= 5  # at least: two launches forward, three backward
    assert hip.hipGraphGetEdges(g, None, None, C.byref(count)) == 0
    ne = count.value
    src, dst = (C.c_void_p * max(ne, 1))(), (C.c_void_p * max(ne, 1))()
    assert hip.hipGraphGetEdges(g, src, dst, C.byref(count)) == 0
    assert ne == n - 1, ("not a chain", n, ne)
    assert len(set(src[:ne])) == ne and len(set(dst[:ne])) == ne, "a node with two successors or two predecessors"
    return kernels


def test_forward_and_grad_capture_and_a_replay_reads_the_new_parameters_on_the_device():
    prm, x, ptsphy, lay, satur, K, _ = setup(("b", "synthetic", dict(levapls2=True), False, 3, P))
    first = values(prm, K, ("rkconv", "rclcrit"))
    other = {n: [v * f for v, f in zip(vs, (0.9, 1.2, 1.05))] for n, vs in first.items()}
    w = weights(lay, K, seed=47)
    pk = device_params({"rkconv": first["rkconv"]}, requires_grad=True)["rkconv"]
    ck = device_params({"rclcrit": first["rclcrit"]}, requires_grad=True)["rclcrit"]
    xs = dict(x, t=per_member_t(x["t"], K).clone().requires_grad_())

    def step():
        out = c2.cloudsc2_ensemble(xs, prm, ptsphy, lay.ngptot, satur=satur, params={"rkconv": pk, "rclcrit": ck})
        g = torch.autograd.grad([getattr(out, n) for n in LOSS], [pk, ck, xs["t"]], [w[n] for n in LOSS])
        return [t.detach() for t in out], list(g)

    def eager():
        o, g = step()
        torch.cuda.synchronize()
        return [t.clone() for t in o + g]

    eager_first = eager()  # the eager call a capture needs first: the device probe and the CETA table
    with torch.no_grad():
        pk.copy_(torch.tensor(other["rkconv"], dtype=torch.float64))
        ck.copy_(torch.tensor(other["rclcrit"], dtype=torch.float64))
    eager_other = eager()
    with torch.no_grad():
        pk.copy_(torch.tensor(first["rkconv"], dtype=torch.float64))
        ck.copy_(torch.tensor(first["rclcrit"], dtype=torch.float64))
    assert not same_bits(eager_first[5], eager_other[5]) and not same_bits(eager_first[-3], eager_other[-3])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        cap_out, cap_g = step()
    nodes = graph_is_a_chain(graph)
    print(f"captured forward + grad: {nodes} kernel nodes in one chain")
    graph.instantiate()
    cap = cap_out + cap_g
    for vals, want in ((first, eager_first), (other, eager_other), (first, eager_first)):
        with torch.no_grad():
            pk.copy_(torch.tensor(vals["rkconv"], dtype=torch.float64))
            ck.copy_(torch.tensor(vals["rclcrit"], dtype=torch.float64))
        for t in cap:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(want, cap)):
            assert same_bits(a, b), ("replay differs from the eager call at these values", i, vals)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------

def test_vmap_double_backward_and_misplaced_parameters_are_refused():
    prm, x, ptsphy, lay, satur, K, vals = setup(CASES[0])
    two = torch.stack([torch.tensor(vals["rkconv"], dtype=torch.float64, device=DEV)] * 2)
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.func.vmap(lambda p: c2.cloudsc2_ensemble(x, prm, ptsphy, lay.ngptot, params={"rkconv": p}).tent)(two)
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.func.vmap(lambda t: c2.cloudsc2_ensemble(dict(x, t=t), prm, ptsphy, lay.ngptot, params=device_params(vals)).tent)(
            torch.stack([x["t"], x["t"]]))
    pk = device_params(vals, requires_grad=True)
    out = c2.cloudsc2_ensemble(dict(x, t=x["t"].clone().requires_grad_()), prm, ptsphy, lay.ngptot, params=pk)
    g, = torch.autograd.grad(out.tent.sum() + out.fplsl.sum(), pk["rkconv"], create_graph=True)
    assert g.requires_grad and tuple(g.shape) == (K,)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(g.sum(), pk["rclcrit"])
    with pytest.raises(ValueError, match="inputs' device"):
        c2.cloudsc2_ensemble(x, prm, ptsphy, lay.ngptot, params={"rkconv": torch.tensor(vals["rkconv"], dtype=torch.float64)})
    off = params(table("synthetic"), levapls2=True)
    off.rpecons = 0.0
    with pytest.raises(ValueError, match="rpecons"):
        c2.cloudsc2_ensemble(x, off, ptsphy, lay.ngptot, params={"rkconv": device_params(vals)["rkconv"]})
