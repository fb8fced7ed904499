"""Gradients with respect to the tunable parameters on the MI355X: cloudsc2_tl_launch_par / cloudsc2_vjp_launch_par through the C ABI
and ``cloudsc2(..., params=...)`` through torch.

Bounds.  The field adjoints and the forward: bits of the launchers without parameters.  par_adj on the device against the host
build's value for the same inputs: 1e-11 relative (the sums are formed in other orders).  Against central differences of the
reference's NL kernel: the cap and the bound of tests/test_hostcheck_par.py (2 of 100 columns, 1e-5 of a field's maximum).  The
dot-product identity: 1e-12.  d loss / d p from backward against a central difference (relative step 1e-6) of a quadratic loss through
the op's own forward: 2e-7 relative, ten times what the host build of the same sweeps reaches on the same cases (1.9e-8 at worst:
precise arithmetic, levapls2, rclcrit; the round-off of the difference)."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, names_of, new, params, same_bits, seeded, state, stream, tail_zero
from tests.host_sweeps import check_against_reference_differences, run_vjp_par
from tests.hostbuild import set_precise
from tests.util import B, FLAGS, c2, fp64_only, make_params, refcall, set_lib_params, the_tables
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

P = c2.PARAM_NAMES
GUARD = 64  # doubles after the workspace that must stay as they were


def forward_launch(x, prm, ptsphy, lay):
    """cloudsc2_ad_launch_forward: the trajectory outputs and the cover checkpoints"""
    traj = new(B.OUT_NAMES, lay)
    scratch = torch.zeros((lay.nblocks, lay.nlev, lay.nproma), dtype=B.torch_real(), device=DEV)
    B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                             C.byref(ag._block("out", traj, lay)), C.c_void_p(scratch.data_ptr()), stream()))
    return traj, scratch


def plain_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur):
    xa = new(names_of(satur), lay, fill=float("nan"))
    fn = B.lib.cloudsc2_vjp_launch_satur if satur else B.lib.cloudsc2_vjp_launch
    B.check(fn(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)), C.byref(ag._block("out", traj, lay)),
               C.byref(ag._block("in", xa, lay)), C.byref(ag._block("out", u, lay)), C.c_void_p(scratch.data_ptr()), stream()))
    return xa


def par_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur):
    """-> input adjoints, par_adj (4 device doubles), the workspace with its guard words"""
    xa = new(names_of(satur), lay, fill=float("nan"))
    n = C.c_longlong()
    B.check(B.lib.cloudsc2_par_work_doubles(lay.nproma, lay.ngptot, C.byref(n)))
    assert n.value == 4 * lay.nblocks * lay.nproma
    work = torch.full((n.value + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    par_adj = torch.full((4,), float("nan"), dtype=torch.float64, device=DEV)
    B.check(B.lib.cloudsc2_vjp_launch_par(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, int(satur), C.byref(ag._block("in", x, lay)),
                                          C.byref(ag._block("out", traj, lay)), C.byref(ag._block("in", xa, lay)),
                                          C.byref(ag._block("out", u, lay)), C.c_void_p(scratch.data_ptr()), C.c_void_p(work.data_ptr()),
                                          C.c_void_p(par_adj.data_ptr()), stream()))
    return xa, par_adj, work


def par_tl(x, dx, dpar, prm, ptsphy, lay, satur):
    dy = new(B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_tl_launch_par(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, int(satur), C.byref(ag._block("in", x, lay)),
                                         C.byref(ag._block("in", dx, lay)), (C.c_double * 4)(*dpar), C.byref(ag._block("out", dy, lay)),
                                         stream()))
    return dy


def dp_of(prm):
    return [0.01 * getattr(prm, n) for n in P]


# ---- 6. superset of the launchers without parameters ----------------------------------------------------------------------------

@pytest.mark.parametrize("satur", [0, 1])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nproma,ngptot,math_mode", [(32, 100, 1), (32, 100, 2), (128, 16384, 0)])
def test_field_adjoints_are_the_bits_of_the_plain_launchers(nproma, ngptot, math_mode, flags, satur):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, satur)
    traj, scratch = forward_launch(x, prm, ptsphy, lay)
    u = seeded(B.OUT_NAMES, lay, seed=3)
    if lay.tail < lay.nproma:
        for t in u.values():
            t[-1, :, lay.tail:] = float("nan")  # the padded tail of the cotangent must not be read into anything
    u0 = {n: t.clone() for n, t in u.items()}
    want = plain_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur)
    got, par_adj, work = par_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur)
    got2, par_adj2, _ = par_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur)
    torch.cuda.synchronize()
    for n in names_of(satur):
        assert same_bits(got[n], want[n]), ("not the bits of the plain launcher (NaN tail included: not written)", n)
        assert same_bits(got2[n], got[n]), n
    for n in B.OUT_NAMES:
        assert same_bits(u[n], u0[n]), ("output adjoint changed", n)
    # 7. the same bits from run to run, finite with a NaN tail, the workspace size honoured
    assert same_bits(par_adj, par_adj2), (par_adj, par_adj2)
    assert bool(torch.all(torch.isfinite(par_adj))), par_adj
    w = work[:-GUARD].view(4, -1)
    assert bool(torch.all(torch.isnan(work[-GUARD:]))), "the guard words after the workspace were written"
    assert bool(torch.all(torch.isfinite(w[:, :lay.ngptot]))) and bool(torch.all(torch.isnan(w[:, lay.ngptot:]))), "active columns only"
    evap = bool(prm.levapls2 or prm.ldrain1d)
    assert bool(par_adj[3] != 0) == evap and bool(torch.all(par_adj[:3] != 0)), par_adj


@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("where", ["cpu", "device"])
def test_forward_with_params_is_the_forward_with_the_values_in_prm(where, satur):
    tab = c2.synthetic_table()
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)
    vals = {"rkconv": 1.3 * prm.rkconv, "rclcrit": 0.8 * prm.rclcrit, "rlptrc": prm.rlptrc - 2.0, "rpecons": 1.1 * prm.rpecons}
    p = {n: torch.tensor(v, dtype=torch.float64, device=DEV if where == "device" else "cpu", requires_grad=True) for n, v in vals.items()}
    rkconv_before = prm.rkconv
    out = ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params=p)
    assert prm.rkconv == rkconv_before, "the caller's prm was changed"
    prm2 = copy.copy(prm)
    for n, v in vals.items():
        setattr(prm2, n, v)
    want = ag.cloudsc2(x, prm2, ptsphy, lay.ngptot, satur=satur)
    base = ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur)
    torch.cuda.synchronize()
    for n in B.OUT_NAMES:
        assert same_bits(getattr(out, n), getattr(want, n)), n
        assert tail_zero(getattr(out, n), lay), n
    assert not same_bits(out.fplsl, base.fplsl), "the parameters' values did not reach the kernels"
    assert out.tent.requires_grad


# ---- 7. par_adj against the host build ------------------------------------------------------------------------------------------

@fp64_only
@pytest.mark.parametrize("satur", [0, 1])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True)])
def test_par_adj_against_the_host_build(flags, satur):
    """Measured on the MI355X: see the printed figures (bound 1e-11 relative)."""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, 1, **flags)
    nproma, ngptot = 32, 100
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, satur)
    traj, scratch = forward_launch(x, prm, ptsphy, lay)
    u = seeded(B.OUT_NAMES, lay, seed=3)
    _, par_adj, _ = par_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur)
    torch.cuda.synchronize()
    # the host build of the same sweep on the same inputs: the state, the device's qsat, PFPLSL5 / PFPLSN5 and cover checkpoints
    st = c2.state_from_table(tab, nproma, ngptot)
    fwd = st.copy()
    fwd.PFPLSL[...] = traj["fplsl"].cpu().numpy()
    fwd.PFPLSN[...] = traj["fplsn"].cpu().numpy()
    qsat = None if satur else np.ascontiguousarray(x["qsat"].cpu().numpy())
    set_precise(0)
    _, _, want, _ = run_vjp_par(prm, st, fwd, np.ascontiguousarray(scratch.cpu().numpy()), {n: t.cpu().numpy() for n, t in u.items()}, qsat)
    got = par_adj.cpu().numpy()
    for k, n in enumerate(P):
        if want[k] == 0.0:
            assert got[k] == 0.0, n
            continue
        e = abs(got[k] - want[k]) / abs(want[k])
        print(f"{flags} satur={satur} {n}: device {got[k]!r} host {want[k]!r} rel {e:.3e}")
        assert e <= 1e-11, (n, e)


# ---- 8. against central differences of the reference's NL kernel, through the C ABI ---------------------------------------------

@fp64_only
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
@pytest.mark.parametrize("which", [0, 1])
def test_parameter_tangent_on_the_device_against_the_reference_differences(which, flags):
    if not refcall.have_ref():
        pytest.fail("the reference build (oracle/_ref) is missing: build() makes it")
    ref = refcall.RefLib()
    name, tab = the_tables()[which]
    prm = make_params(tab, lregcl=False, **flags)
    set_lib_params(ref, prm)
    st = c2.state_from_table(tab, 100, 100)
    qs = ref.satur(np.ascontiguousarray(st.PAP[0]), np.ascontiguousarray(st.PT[0]))
    x, ptsphy, lay = state(tab, 100, 100, prm, 0)
    x["qsat"] = torch.from_numpy(np.ascontiguousarray(qs[None])).to(DEV)
    zero = {n: torch.zeros_like(t) for n, t in x.items()}

    def tl_of(k):
        e = [0.0] * 4
        e[k] = 1.0
        dy = par_tl(x, zero, e, prm, ptsphy, lay, 0)
        torch.cuda.synchronize()
        return {n: dy[n][0].cpu().numpy() for n in B.OUT_NAMES}

    worst = check_against_reference_differences(ref, prm, st, qs, tl_of, f"device {name} {flags}")
    print(f"device {name} {flags}: worst {worst:.3e}")


# ---- 9. the dot-product identity ------------------------------------------------------------------------------------------------

def identity(tab, prm, nproma, ngptot, satur):
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, satur)
    v = {n: 0.01 * t for n, t in x.items()}
    dp = dp_of(prm)
    u = par_tl(x, v, dp, prm, ptsphy, lay, satur)
    traj, scratch = forward_launch(x, prm, ptsphy, lay)
    xa, par_adj, _ = par_vjp(x, traj, scratch, u, prm, ptsphy, lay, satur)
    torch.cuda.synchronize()
    act = torch.zeros((lay.nblocks, 1, lay.nproma), dtype=torch.bool, device=DEV)
    act[:-1] = True
    act[-1, :, :lay.tail] = True
    lhs = sum(float(torch.sum(torch.where(act, t, 0).double() ** 2)) for t in u.values())
    par = float(np.dot(dp, par_adj.cpu().numpy()))
    rhs = sum(float(torch.sum(torch.where(act, v[n] * xa[n], 0).double())) for n in v) + par
    return lhs, rhs, par


@fp64_only
@pytest.mark.parametrize("satur", [0, 1])
@pytest.mark.parametrize("flags", [dict(lregcl=True), dict(levapls2=True, lregcl=True)])
def test_dot_product_identity_at_16384_columns(flags, satur):
    tab = c2.random_table(137, 100, seed=8)
    lhs, rhs, par = identity(tab, params(tab, **flags), 128, 16384, satur)
    print(f"{flags} satur={satur}: <TL(dx, dp), u> = {lhs!r}, <dx, xa> + dp.par_adj = {rhs!r} (dp.par_adj = {par!r}), rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) / abs(lhs) <= 1e-12, (lhs, rhs)
    assert abs(par) / abs(lhs) > 1e-9, "the parameter term must matter to the identity"


@fp64_only
def test_dot_product_identity_at_160000_columns():
    """NPROMA 128: the paced launch with 32-bit offsets, 1250 blocks"""
    tab = c2.synthetic_table()
    lhs, rhs, par = identity(tab, params(tab, lregcl=True), 128, 160000, 0)
    print(f"160000 columns: <TL(dx, dp), u> = {lhs!r}, <dx, xa> + dp.par_adj = {rhs!r} (dp.par_adj = {par!r}), rel {abs(lhs - rhs) / abs(lhs):.3e}")
    assert abs(lhs - rhs) / abs(lhs) <= 1e-12, (lhs, rhs)


# ---- 10. through torch ----------------------------------------------------------------------------------------------------------

def ptensors(prm, where, grad=P):
    dev = DEV if where == "device" else "cpu"
    return {n: torch.tensor(getattr(prm, n), dtype=torch.float64, device=dev, requires_grad=n in grad) for n in P}


@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("where", ["cpu", "device"])
@pytest.mark.parametrize("flags", [dict(lregcl=True), dict(levapls2=True)])
def test_backward_and_grad_are_the_launchers_bits(flags, where, satur):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)
    names = names_of(satur)
    u = seeded(B.OUT_NAMES, lay, seed=1)
    traj, scratch = forward_launch(x, prm, ptsphy, lay)
    want_x, want_p, _ = par_vjp(x, traj, scratch, u, prm, ptsphy, lay, int(satur))
    torch.cuda.synchronize()

    def loss_of(out):
        return sum(torch.sum(getattr(out, n) * u[n]) for n in B.OUT_NAMES)

    # .backward(): every field and every parameter
    xs = {n: x[n].clone().requires_grad_() for n in names}
    p = ptensors(prm, where)
    loss_of(ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, params=p)).backward()
    for k, n in enumerate(P):
        g = p[n].grad
        assert g is not None and g.dim() == 0 and g.dtype == torch.float64 and g.device == p[n].device, n
        assert same_bits(g.to(DEV).reshape(1), want_p[k].reshape(1)), (n, g, want_p[k])
    for n in names:  # (the launcher leaves the padded tail as it was, the op returns it zero)
        assert same_bits(xs[n].grad[:-1], want_x[n][:-1]) and same_bits(xs[n].grad[-1, :, :lay.tail], want_x[n][-1, :, :lay.tail]), n
        assert tail_zero(xs[n].grad, lay), n

    # only some parameters require a gradient, and no field does
    p = ptensors(prm, where, grad=("rclcrit", "rlptrc"))
    loss_of(ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params=p)).backward()
    assert p["rkconv"].grad is None and p["rpecons"].grad is None
    for n in ("rclcrit", "rlptrc"):
        assert same_bits(p[n].grad.to(DEV).reshape(1), want_p[P.index(n)].reshape(1)), n

    # a subset of the names; no parameter requires a gradient: the field gradients are those of the op without params
    xs = {n: x[n].clone().requires_grad_() for n in names}
    p = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64)}
    loss_of(ag.cloudsc2(xs, prm, ptsphy, lay.ngptot, satur=satur, params=p)).backward()
    xs0 = {n: x[n].clone().requires_grad_() for n in names}
    loss_of(ag.cloudsc2(xs0, prm, ptsphy, lay.ngptot, satur=satur)).backward()
    for n in names:
        assert same_bits(xs[n].grad, xs0[n].grad), n

    # torch.func.grad with respect to the parameters (and torch.func.vjp underneath)
    pd = ptensors(prm, where, grad=())

    def f(rk, rc, rl, rp):
        return loss_of(ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params=dict(zip(P, (rk, rc, rl, rp)))))

    gs = torch.func.grad(f, argnums=(0, 1, 2, 3))(*(pd[n] for n in P))
    for k, n in enumerate(P):
        assert gs[k].dim() == 0 and same_bits(gs[k].to(DEV).reshape(1), want_p[k].reshape(1)), n


@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("where", ["cpu", "device"])
def test_forward_ad_and_jvp_are_the_launchers_bits(where, satur):
    import torch.autograd.forward_ad as fwAD

    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)
    names = names_of(satur)
    v = {n: 0.01 * t for n, t in x.items()}
    dp = dp_of(prm)
    want = par_tl(x, v, dp, prm, ptsphy, lay, int(satur))
    want_p_only = par_tl(x, {n: torch.zeros_like(t) for n, t in x.items()}, [dp[0], 0.0, 0.0, 0.0], prm, ptsphy, lay, int(satur))
    pd = ptensors(prm, where, grad=())
    tp = {n: torch.tensor(d, dtype=torch.float64, device=pd[n].device) for n, d in zip(P, dp)}
    with fwAD.dual_level():
        out = ag.cloudsc2({n: fwAD.make_dual(x[n], v[n]) for n in names}, prm, ptsphy, lay.ngptot, satur=satur,
                          params={n: fwAD.make_dual(pd[n], tp[n]) for n in P})
        tan = [fwAD.unpack_dual(o).tangent for o in out]

    def f(rk, *xs):  # a tangent of one parameter alone, the fields constant
        return tuple(ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params={"rkconv": rk}))

    _, tan1 = torch.func.jvp(f, (pd["rkconv"],), (tp["rkconv"],))
    torch.cuda.synchronize()
    for k, n in enumerate(B.OUT_NAMES):
        assert same_bits(tan[k], want[n]), ("forward_ad", n)
        assert same_bits(tan1[k], want_p_only[n]), ("torch.func.jvp", n)
        assert tail_zero(tan[k], lay), n
    assert bool(torch.any(tan1[B.OUT_NAMES.index("fplsl")] != 0))


@fp64_only
@pytest.mark.parametrize("math_mode", [1, 2])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
def test_backward_against_a_central_difference_of_a_quadratic_loss(flags, math_mode):
    """loss = sum over the fields of 0.5 sum (out / max|out|)^2 through the op's own forward, relative step 1e-6.  The host build of
    the same sweeps agrees with its own difference to 1.9e-8 at worst on these cases (precise, levapls2, rclcrit; the round-off of the
    difference); the bound is ten times that, 2e-7."""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode, lregcl=False, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, False)
    with torch.no_grad():
        out0 = ag.cloudsc2(x, prm, ptsphy, lay.ngptot)
        w = {n: (1.0 / float(torch.max(torch.abs(getattr(out0, n)))) ** 2 if bool(torch.any(getattr(out0, n) != 0)) else 0.0)
             for n in B.OUT_NAMES}

    def loss_of(out):
        return sum(0.5 * w[n] * torch.sum(getattr(out, n).double() ** 2) for n in B.OUT_NAMES)

    p = ptensors(prm, "cpu")
    loss_of(ag.cloudsc2(x, prm, ptsphy, lay.ngptot, params=p)).backward()
    h = 1e-6
    for n in P:
        p0 = getattr(prm, n)
        with torch.no_grad():
            lp = [float(loss_of(ag.cloudsc2(x, prm, ptsphy, lay.ngptot, params={n: torch.tensor(p0 * (1 + s * h), dtype=torch.float64)})))
                  for s in (1, -1)]
        fd = (lp[0] - lp[1]) / (2 * h * p0)
        g = float(p[n].grad)
        if fd == 0.0:
            assert g == 0.0 and n == "rpecons" and not flags, (n, g)
            continue
        e = abs(g - fd) / abs(fd)
        print(f"math_mode {math_mode} {flags} {n}: backward {g!r}, difference {fd!r}, rel {e:.3e}")
        assert e <= 2e-7, (n, g, fd, e)


@pytest.mark.parametrize("satur", [False, True])
def test_vmap_with_params_is_refused_and_without_them_works_as_before(satur):
    tab = c2.synthetic_table()
    prm = params(tab)
    x, ptsphy, lay = state(tab, 32, 64, prm, satur)
    names = names_of(satur)
    p = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64)}

    def f(t, params=p):
        return ag.cloudsc2({**x, "t": t}, prm, ptsphy, lay.ngptot, satur=satur, params=params).fplsl

    def g(rk):
        return ag.cloudsc2(x, prm, ptsphy, lay.ngptot, satur=satur, params={"rkconv": rk}).fplsl

    T = torch.stack([x["t"], x["t"] + 0.5])
    V = torch.stack([0.01 * x["t"], 0.02 * x["t"]])
    with pytest.raises(NotImplementedError, match="params"):
        torch.func.vmap(f)(T)
    with pytest.raises(NotImplementedError, match="params"):
        torch.func.vmap(lambda v: torch.func.jvp(f, (x["t"],), (v,))[1])(V)
    _, pullback = torch.func.vjp(g, p["rkconv"])
    U = torch.stack([seeded(("fplsl",), lay, 5)["fplsl"], seeded(("fplsl",), lay, 6)["fplsl"]])
    with pytest.raises(NotImplementedError, match="params"):
        torch.func.vmap(pullback)(U)
    with pytest.raises(NotImplementedError, match="params"):
        torch.func.jacfwd(g)(p["rkconv"])
    with pytest.raises(NotImplementedError, match="params"):
        torch.func.jacrev(g)(p["rkconv"])
    # without params: as before
    got = torch.func.vmap(lambda v: torch.func.jvp(lambda t: f(t, None), (x["t"],), (v,))[1])(V)
    for j in range(2):
        want = torch.func.jvp(lambda t: f(t, None), (x["t"],), (V[j],))[1]
        assert same_bits(got[j], want), j
    assert names  # (both input sets)


def test_params_are_refused_while_the_stream_is_capturing():
    tab = c2.synthetic_table()
    prm = params(tab)
    x, ptsphy, lay = state(tab, 32, 64, prm, False)
    p = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64)}
    ag.cloudsc2(x, prm, ptsphy, lay.ngptot, params=p)  # (the eager call a capture needs first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ag.cloudsc2(x, prm, ptsphy, lay.ngptot)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with pytest.raises(RuntimeError, match="capturing"):
            ag.cloudsc2(x, prm, ptsphy, lay.ngptot, params=p)
        out = ag.cloudsc2(x, prm, ptsphy, lay.ngptot)  # without params the op captures as before
    graph.replay()
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(out.fplsl)))
