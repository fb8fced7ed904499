"""``cloudsc2_param_maps`` on the MI355X: rkconv, rclcrit, rlptrc, rpecons as (nblocks, nproma) fields read on the device.

The promise: column c of every output, every output tangent and every field gradient is BIT FOR BIT what
``cloudsc2(x, prm, ..., params={the four 0-d values of column c})`` gives at that column.  The gradient of a map is per column; the
scalar op only gives its fold, so for every group m of columns that share their values ``g[idx == m].sum()`` is held to the 0-d
parameter gradient of call m under the cotangent masked to the group, within ``n_m x 2^-52 x sum |g|`` over the group: the reordering
bound of an n_m-term sum (nothing measured enters it).

Shapes, the smallest at which a column mapping can go wrong: (a) nproma 24, ngptot 70 -- 72 padded columns, one partly idle workgroup
whose second wave holds 8 lanes, a padded tail of 2; (b) nproma 64, ngptot 200 -- 256 padded columns, two workgroups, a padded tail of 56
in the second.  Three values assigned by ``idx[c] = (c + c // nproma) % 3`` over the padded column number: they differ from lane to lane
inside a wave and shift phase at every block.  The values are ROWS and the cases those of tests/test_gpu_autograd_ens.py without its
K = 1 rows.

Condition, not a measurement: in every case each given parameter's map gradient is non-zero in at least half of each group's active
columns (rpecons only with the evaporation branch); otherwise a dead parameter would pass everything."""
from __future__ import annotations

import pytest
import torch

from tests.gpu_util import DEV, make_inputs, names_of, params, same_bits, tail_zero
from tests.test_gpu_autograd_ens import CASES as ENS_CASES, LOSS, ROWS, SHAPES, table
from tests.util import B, c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = [pytest.mark.gpu]

P = c2.PARAM_NAMES
# Where the gfx950 build misses the bits: the output tangents under a tangent map.  The device compiler contracts the level's parameter
# source terms differently when the ParLin members are a lane's registers and not the launch's scalars (laundering them at every level
# did not change it).  fp64: these planes alone are held to 1e-11 of the field's maximum, the project's bound for two routes to one
# derivative (TLAD_TOL); every other comparison of this module stays bit for bit.  Measured on the MI355X, fp64, worst over the three
# cases: 1 038 of 35 328 elements of a plane differ; largest difference 1.71 units in the last place of the field's maximum in tent, 1.62
# in tenq, 0.69 teni, 0.01 tenl, 0.52 fplsl, 0.54 fplsn, 0.88 fhpsl, 0.80 fhpsn; clc and covptot 0.  The bound is 1e-11 / 2^-52 = 45 036
# units.  With one parameter's tangent map alone (rkconv, rclcrit, rlptrc; no field tangent) every plane is the bits, in both precisions.
# fp32 (started by tests/test_single_parmap.py, which hands over the fp64 library's scalar-route tangents): the same planes are held to
# 4 x the error the fp32 scalar-parameter op itself has against the fp64 one on the same inputs.  Measured, worst over the three cases, in
# units in the last place of the field's maximum, difference / smallest bound: tent 0.41 / 203.6, tenq 0.10 / 201.4, tenl 0.27 / 1236.3,
# teni 2.90 / 586.3, fplsl 0.67 / 68.6, fplsn 0.32 / 119.2, fhpsl 1.13 / 68.7, fhpsn 0.47 / 119.2 (at most 521 of 35 072 elements of a
# plane differ); clc and covptot 0.  Without that reference an fp32 run of this module asks for the bits.
TLAD_TOL = 1e-11
TANGENT_PLANES_OFF_BITS = ("tent", "tenq", "tenl", "teni", "fplsl", "fplsn", "fhpsl", "fhpsn")
CASES = [(s, t, f, sat, g) for s, t, f, sat, k, g in ENS_CASES if k > 1]
IDS = [f"{s}-{t}-{'+'.join(k for k in f) or 'plain'}-satur{int(sat)}-{len(g)}given" for s, t, f, sat, g in CASES]
M = len(ROWS)


def setup(case):
    shape, kind, flags, satur, given = case
    nproma, ngptot = SHAPES[shape]
    tab = table(kind)
    prm = params(tab, **flags)
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    x = {n: x[n] for n in names_of(satur)}
    c = torch.arange(lay.nblocks * nproma, device=DEV)
    idx = ((c + c // nproma) % M).reshape(lay.nblocks, nproma)
    vals = {n: [getattr(prm, n) + r[n] if n == "rlptrc" else getattr(prm, n) * r[n] for r in ROWS] for n in given}
    return prm, x, ptsphy, lay, satur, idx, vals


def maps_of(vals, idx, requires_grad=False, scale=1.0):
    return {n: (scale * torch.tensor(v, dtype=torch.float64, device=DEV))[idx].contiguous().requires_grad_(requires_grad) for n, v in vals.items()}


def scalars_of(vals, m, requires_grad=False, scale=1.0):
    return {n: torch.tensor(scale * v[m], dtype=torch.float64, device=DEV, requires_grad=requires_grad) for n, v in vals.items()}


def plane_mask(idx, m):
    return (idx == m)[:, None, :]  # over (nblocks, nlevx, nproma)


def active_of(lay):
    c = torch.arange(lay.nblocks * lay.nproma, device=DEV).reshape(lay.nblocks, lay.nproma)
    return c < lay.ngptot


def weights(lay, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return {n: torch.randn(lay.shape(n), generator=g, dtype=B.torch_real(), device=DEV) for n in LOSS}


def selected(per_group, idx):
    """the planes of the M scalar calls joined by column: group m's columns from call m"""
    out = per_group[0]
    for m in range(1, M):
        out = torch.where(plane_mask(idx, m), per_group[m], out)
    return out


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_columns_outputs_are_the_bits_of_the_scalar_op(case):
    prm, x, ptsphy, lay, satur, idx, vals = setup(case)
    B.launch_log_reset()
    out = c2.cloudsc2_param_maps(x, prm, ptsphy, lay.ngptot, satur=satur, params=maps_of(vals, idx))
    assert B.launch_log() == [], "the parameter-map kernels are no logged sweep family"
    torch.cuda.synchronize()
    assert isinstance(out, ag.Cloudsc2Outputs)
    want = [ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params=scalars_of(vals, m)) for m in range(M)]
    torch.cuda.synchronize()
    for n in B.OUT_NAMES:
        got = getattr(out, n)
        assert tuple(got.shape) == lay.shape(n), n
        assert same_bits(got, selected([getattr(w, n) for w in want], idx)), ("output", n)
        assert tail_zero(got, lay), ("padded tail", n)
    assert not same_bits(out.fplsl, want[0].fplsl), "the maps did not reach the kernels"


# ---- 2. backward -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_column_by_column_and_the_map_gradients_group_by_group(case):
    prm, x, ptsphy, lay, satur, idx, vals = setup(case)
    evap = bool(prm.levapls2 or prm.ldrain1d)
    w = weights(lay, seed=41)
    p = maps_of(vals, idx, requires_grad=True)
    xe = dict(x, t=x["t"].clone().requires_grad_(), q=x["q"].clone().requires_grad_())
    out = c2.cloudsc2_param_maps(xe, prm, ptsphy, lay.ngptot, satur=satur, params=p)
    leaves = [p[n] for n in vals] + [xe["t"], xe["q"]]
    g = torch.autograd.grad([getattr(out, n) for n in LOSS], leaves, [w[n] for n in LOSS], retain_graph=True)
    gp, gt, gq = dict(zip(vals, g[:len(vals)])), g[-2], g[-1]
    gz = torch.autograd.grad([out.clc, out.covptot], [p[n] for n in vals], [w["covptot"], w["covptot"]])  # depend on none of the four
    torch.cuda.synchronize()
    for a in gz:
        assert bool(torch.all(a == 0)), "clc / covptot-only losses: exact zero maps"
    active = active_of(lay)
    for n, a in gp.items():
        assert tuple(a.shape) == (lay.nblocks, lay.nproma) and a.dtype == torch.float64 and a.device == DEV, n
        assert bool(torch.all(a[~active] == 0)), ("padded tail of a map gradient", n)
        assert bool(torch.all(torch.isfinite(a))), n
    st, sq = [], []
    for m in range(M):
        pm = scalars_of(vals, m, requires_grad=True)
        xm = dict(x, t=x["t"].clone().requires_grad_(), q=x["q"].clone().requires_grad_())
        o = ag.cloudsc2(xm, prm, ptsphy, lay.ngptot, satur=satur, params=pm)
        s = torch.autograd.grad([getattr(o, n) for n in LOSS], [pm[n] for n in vals] + [xm["t"], xm["q"]],
                                [w[n] * plane_mask(idx, m) for n in LOSS])
        torch.cuda.synchronize()
        st.append(s[-2])
        sq.append(s[-1])
        group = active & (idx == m)
        n_m = int(group.sum())
        for n, a in zip(vals, s):
            col = gp[n][group]
            err, bound = abs(float(col.sum()) - float(a)), n_m * 2.0 ** -52 * float(col.abs().sum())
            live = int((col != 0).sum())
            print(f"{n} group {m}: {live} of {n_m} columns non-zero; |sum - 0-d gradient| = {err:.3e}, bound {bound:.3e}")
            assert err <= bound, ("map gradient against the 0-d parameter gradient", n, m, err, bound)
            if n == "rpecons" and not evap:
                assert live == 0 and float(a) == 0.0, "without the evaporation branch nothing depends on rpecons"
            else:
                assert 2 * live >= n_m, ("a parameter that is dead in more than half of a group's columns", n, m, live, n_m)
    assert same_bits(gt, selected(st, idx)) and same_bits(gq, selected(sq, idx)), "field gradients, column by column"
    assert tail_zero(gt, lay) and tail_zero(gq, lay) and bool(torch.any(gq != 0))


def test_torch_func_grad_and_vjp_give_the_bits_of_backward():
    prm, x, ptsphy, lay, satur, idx, vals = setup(CASES[2])
    w = weights(lay, seed=45)
    fixed = {n: v for n, v in maps_of(vals, idx).items() if n != "rclcrit"}

    def loss(p, t):
        out = c2.cloudsc2_param_maps(dict(x, t=t), prm, ptsphy, lay.ngptot, satur=satur, params=dict(fixed, rclcrit=p))
        return sum((getattr(out, n) * w[n]).sum() for n in LOSS)

    p = maps_of(vals, idx)["rclcrit"]
    pa, ta = p.clone().requires_grad_(), x["t"].clone().requires_grad_()
    want = torch.autograd.grad(loss(pa, ta), [pa, ta])
    got = torch.func.grad(loss, argnums=(0, 1))(p, x["t"])
    _, pull = torch.func.vjp(loss, p, x["t"])
    back = pull(torch.ones((), dtype=B.torch_real(), device=DEV))
    loss(pa, ta).backward()
    torch.cuda.synchronize()
    for a, b, c in zip(want, got, back):
        assert same_bits(a, b) and same_bits(a, c)
    assert same_bits(pa.grad, want[0]) and same_bits(ta.grad, want[1]), ".backward()"
    assert bool(torch.any(want[0] != 0))


# ---- 3. jvp ----------------------------------------------------------------------------------------------------------------------

REFERENCE_ENV = "CLOUDSC2_PARMAP_FP64_TANGENTS"  # a .npz of scalar_route_tangents() from the fp64 library (tests/test_single_parmap.py)
ONE_PARAMETER = ("rkconv", "rclcrit", "rlptrc")  # the tangent maps given alone, without field tangents: bit for bit in fp64


def jvp_operands(case, only=None):
    """the operands of a jvp case: all field and parameter tangents, or (``only``) one parameter's tangent map and nothing else.  The
    random field tangents are drawn in float64 in both libraries, so the fp32 run has the fp64 run's tangents, rounded."""
    prm, x, ptsphy, lay, satur, idx, vals = setup(case)
    names = list(vals)
    g = torch.Generator(device=DEV).manual_seed(43)
    dt = (0.01 * torch.randn(x["t"].shape, generator=g, dtype=torch.float64, device=DEV)).to(x["t"].dtype)
    dq = (1e-6 * torch.randn(x["q"].shape, generator=g, dtype=torch.float64, device=DEV)).to(x["t"].dtype)
    rel = [0.01 * (1.0 + 0.5 * m) for m in range(M)]  # a tangent per group: dp = rel_m p
    if only is not None:
        dt, dq = torch.zeros_like(dt), torch.zeros_like(dq)
    on = lambda n: 1.0 if only in (None, n) else 0.0  # noqa: E731
    return prm, x, ptsphy, lay, satur, idx, vals, names, dt, dq, rel, on


def scalar_route_tangents(case, only=None):
    """primals and tangents of the M calls of cloudsc2(params=0-d), joined by column"""
    prm, x, ptsphy, lay, satur, idx, vals, names, dt, dq, rel, on = jvp_operands(case, only)
    prim, tang = [], []
    for m in range(M):
        pm = scalars_of(vals, m)

        def one(t, q, *ps):
            return tuple(ag.cloudsc2(dict(x, t=t, q=q), prm, ptsphy, lay.ngptot, satur=satur, params=dict(zip(names, ps))))

        o, d = torch.func.jvp(one, (x["t"], x["q"]) + tuple(pm[n] for n in names), (dt, dq) + tuple(pm[n] * (rel[m] * on(n)) for n in names))
        torch.cuda.synchronize()
        prim.append(o)
        tang.append(d)
    return ([selected([o[i] for o in prim], idx) for i in range(len(B.OUT_NAMES))],
            [selected([d[i] for d in tang], idx) for i in range(len(B.OUT_NAMES))])


def reference_key(case, only, n):
    return f"{IDS[CASES.index(case)]}__{only or 'all'}__{n}"


def hold_tangents(case, only):
    """fp64: bit for bit, but for the planes of TANGENT_PLANES_OFF_BITS when every tangent is given (TLAD_TOL).  fp32: bit for bit; where
    the fp64 library's scalar-route tangents are at hand (REFERENCE_ENV), the planes of TANGENT_PLANES_OFF_BITS are held to 4 x the error
    the fp32 scalar route itself has against them.  Every plane is measured before anything is asserted."""
    import os

    import numpy as np

    prm, x, ptsphy, lay, satur, idx, vals, names, dt, dq, rel, on = jvp_operands(case, only)
    p = maps_of(vals, idx)
    dp = {n: p[n] * (torch.tensor(rel, dtype=torch.float64, device=DEV) * on(n))[idx] for n in names}

    def maps(t, q, *ps):
        return tuple(c2.cloudsc2_param_maps(dict(x, t=t, q=q), prm, ptsphy, lay.ngptot, satur=satur, params=dict(zip(names, ps))))

    out, tan = torch.func.jvp(maps, (x["t"], x["q"]) + tuple(p[n] for n in names), (dt, dq) + tuple(dp[n] for n in names))
    with torch.autograd.forward_ad.dual_level():
        duals = {n: torch.autograd.forward_ad.make_dual(p[n], dp[n]) for n in names}
        o = c2.cloudsc2_param_maps(dict(x, t=torch.autograd.forward_ad.make_dual(x["t"], dt), q=torch.autograd.forward_ad.make_dual(x["q"], dq)),
                                   prm, ptsphy, lay.ngptot, satur=satur, params=duals)
        fwd_ad = [torch.autograd.forward_ad.unpack_dual(t).tangent for t in o]
    torch.cuda.synchronize()
    prim, wants = scalar_route_tangents(case, only)
    fp64 = tan[0].dtype == torch.float64
    ref = np.load(os.environ[REFERENCE_ENV]) if (not fp64 and os.environ.get(REFERENCE_ENV)) else None
    eps = 2.0 ** -52 if fp64 else 2.0 ** -23
    missed = []
    for i, n in enumerate(B.OUT_NAMES):
        assert same_bits(out[i], prim[i]), ("primal", n)
        assert same_bits(fwd_ad[i], tan[i]), ("forward_ad", n)
        assert tail_zero(tan[i], lay), n
        want = wants[i]
        diff, top = float((tan[i] - want).abs().max()), float(want.abs().max())
        bound, how = 0.0, "bits"
        if n in TANGENT_PLANES_OFF_BITS and fp64 and only is None:
            bound, how = TLAD_TOL * top, "1e-11 of the field's maximum"
        elif n in TANGENT_PLANES_OFF_BITS and ref is not None:
            w64 = torch.from_numpy(ref[reference_key(case, only, n)]).to(DEV)
            bound, how = 4.0 * float((want.double() - w64).abs().max()), "4 x the fp32 scalar route's error against the fp64 one"
        ulp = eps * top if top else 1.0
        print(f"tangent {n} ({only or 'all tangents'}): {int((tan[i] != want).sum())} of {want.numel()} elements differ, largest difference "
              f"{diff:.3e} = {diff / ulp:.2f} units in the last place of the field's maximum {top:.3e}; bound ({how}) {bound:.3e} = {bound / ulp:.1f} units")
        if not (same_bits(tan[i], want) if bound == 0.0 else diff <= bound):
            missed.append((n, diff, bound))
    assert not missed, ("tangents", only, missed)
    assert bool(torch.any(tan[0] != 0))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_jvp_with_tangent_maps_and_field_tangents_is_the_scalar_ops(case):
    hold_tangents(case, None)


@pytest.mark.parametrize("only", ONE_PARAMETER)
@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_jvp_with_one_parameters_tangent_map_alone_is_the_scalar_ops(case, only):
    """how far the miss of the bits reaches: with one parameter's tangent map alone (rkconv, rclcrit or rlptrc) it does not"""
    hold_tangents(case, only)


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------

def test_forward_and_grad_capture_and_a_replay_reads_the_new_maps_on_the_device():
    prm, x, ptsphy, lay, satur, idx, vals = setup(("b", "synthetic", dict(levapls2=True), False, ("rkconv", "rclcrit")))
    first = maps_of(vals, idx)
    other = {n: (v * torch.tensor([0.9, 1.2, 1.05], dtype=torch.float64, device=DEV)[(idx + 1) % M]).contiguous() for n, v in first.items()}
    w = weights(lay, seed=47)
    rk, rc = first["rkconv"].clone().requires_grad_(), first["rclcrit"].clone().requires_grad_()
    xs = dict(x, t=x["t"].clone().requires_grad_())

    def step():
        out = c2.cloudsc2_param_maps(xs, prm, ptsphy, lay.ngptot, satur=satur, params={"rkconv": rk, "rclcrit": rc})
        g = torch.autograd.grad([getattr(out, n) for n in LOSS], [rk, rc, xs["t"]], [w[n] for n in LOSS])
        return [t.detach() for t in out], list(g)

    def eager():
        o, g = step()
        torch.cuda.synchronize()
        return [t.clone() for t in o + g]

    def give(vals):
        with torch.no_grad():
            rk.copy_(vals["rkconv"])
            rc.copy_(vals["rclcrit"])

    eager_first = eager()  # the eager call a capture needs first: the device probe and the CETA table
    give(other)
    eager_other = eager()
    give(first)
    assert not same_bits(eager_first[5], eager_other[5]) and not same_bits(eager_first[-3], eager_other[-3])
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()

    B.launch_log_reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_out, cap_g = step()
    assert B.launch_log() == []
    cap = cap_out + cap_g
    for vals_, want in ((first, eager_first), (other, eager_other), (first, eager_first)):
        give(vals_)
        for t in cap:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(want, cap)):
            assert same_bits(a, b), ("replay differs from the eager call with these maps", i)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------

def test_vmap_double_backward_and_misplaced_maps_are_refused():
    prm, x, ptsphy, lay, satur, idx, vals = setup(CASES[0])
    p = maps_of(vals, idx)
    two = torch.stack([p["rkconv"]] * 2)
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.func.vmap(lambda q: c2.cloudsc2_param_maps(x, prm, ptsphy, lay.ngptot, params={"rkconv": q}).tent)(two)
    with pytest.raises(NotImplementedError, match="vmap"):
        torch.func.vmap(lambda t: c2.cloudsc2_param_maps(dict(x, t=t), prm, ptsphy, lay.ngptot, params=p).tent)(torch.stack([x["t"], x["t"]]))
    pg = maps_of(vals, idx, requires_grad=True)
    out = c2.cloudsc2_param_maps(dict(x, t=x["t"].clone().requires_grad_()), prm, ptsphy, lay.ngptot, params=pg)
    g, = torch.autograd.grad(out.tent.sum() + out.fplsl.sum(), pg["rkconv"], create_graph=True)
    assert g.requires_grad and tuple(g.shape) == (lay.nblocks, lay.nproma)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(g.sum(), pg["rclcrit"])
    with pytest.raises(ValueError, match="inputs' device"):
        c2.cloudsc2_param_maps(x, prm, ptsphy, lay.ngptot, params={"rkconv": p["rkconv"].cpu()})
    with pytest.raises(ValueError, match="cloudsc2_ensemble"):
        c2.cloudsc2_param_maps(x, prm, ptsphy, lay.ngptot, params={"rkconv": p["rkconv"][0, :3]})
    off = params(table("synthetic"), levapls2=True)
    off.rpecons = 0.0
    with pytest.raises(ValueError, match="rpecons"):
        c2.cloudsc2_param_maps(x, off, ptsphy, lay.ngptot, params={"rkconv": p["rkconv"]})
