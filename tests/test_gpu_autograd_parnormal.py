"""The Gauss-Newton normal equations of the parameters on the MI355X: cloudsc2_parnormal_launch through the C ABI and
``c2.param_normal_equations`` through torch.

The yardstick is the parent's parameter Jacobian, cloudsc2_tl_launch_parjac, contracted by torch in float64 on the device
(tests/parnormal_yardstick.py, which derives the bound): ``|got - want| <= 1e-12 * S`` entry by entry, ``S`` the sum of the absolute
products.  The numeric comparisons are fp64 statements: in the fp32 build the two kernels need not produce the same J bits, and that
gap is not measured.  Every residual and weight plane is NaN in the padded tail and, for the four fluxes, at half level 0 (the zero
flux at the model top): none of those values may be read.
Measured on the MI355X (worst |got - want| / S over the 14 entries and the eight cases): all ten outputs 3.2e-16, the subset 3.9e-16
((32, 100), precise arithmetic, no evaporation branch), qsat NULL 3.2e-16; the test prints every entry."""
from __future__ import annotations

import copy
import ctypes as C

import pytest
import torch

from tests.gpu_util import DEV, active, hip_runtime, new, params, parjac, same_bits, state, stream
from tests.parnormal_yardstick import BOUND, NPAR, RPECONS_ROWS, contract, row_g, row_h
from tests.util import B, c2, fp64_only, refcall
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

pytestmark = pytest.mark.gpu

P = c2.PARAM_NAMES
NAN = float("nan")
GUARD = 64  # doubles after the workspace that must stay as they were
# lanes and a ragged tail, fold threads with nothing to add | a tail, fold threads that add one or two columns | full blocks, sixteen
# columns per fold thread
SHAPES = [(32, 100, 1), (32, 100, 2), (128, 1300, 0), (128, 16384, 0)]
FLAGS = [dict(), dict(levapls2=True)]


def observations(lay, seed, names=B.OUT_NAMES):
    """seeded residuals and positive weights; NaN wherever the sweep must not read: the padded tail, half level 0 of the fluxes"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r, w = {}, {}
    for n in names:
        r[n] = torch.randn(lay.shape(n), generator=g, dtype=B.torch_real(), device=DEV)
        w[n] = torch.rand(lay.shape(n), generator=g, dtype=B.torch_real(), device=DEV) * 1.5 + 0.5
        for t in (r[n], w[n]):
            if lay.tail < lay.nproma:
                t[-1, :, lay.tail:] = NAN
            if n in refcall.HALF:
                t[:, 0, :] = NAN
    return r, w


def launch(x, prm, ptsphy, lay, r, w, work=None, normal=None):
    """cloudsc2_parnormal_launch -> (normal, work): 14 device doubles, and the NaN-prefilled workspace with its guard words.
    w None: the weight block itself is NULL; x without qsat: SATUR in the sweep"""
    n = C.c_longlong()
    B.check(B.lib.cloudsc2_parnormal_work_doubles(lay.nproma, lay.ngptot, C.byref(n)))
    assert n.value == B.NNORMAL * lay.nblocks * lay.nproma
    work = work if work is not None else torch.full((n.value + GUARD,), NAN, dtype=torch.float64, device=DEV)
    normal = normal if normal is not None else torch.full((B.NNORMAL,), NAN, dtype=torch.float64, device=DEV)
    B.check(B.lib.cloudsc2_parnormal_launch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                            C.byref(ag._block("out", r, lay)), C.byref(ag._block("out", w, lay)) if w is not None else None,
                                            C.c_void_p(work.data_ptr()), C.c_void_p(normal.data_ptr()), stream()))
    return normal, work


def yardstick(sens, np_dirs, r, w, lay):
    """{row: (want, S)} as Python floats from the parent's sensitivities, contracted in float64 over the active columns"""
    def f64(d):
        return {n: active(t, lay).to(torch.float64) for n, t in d.items()}

    per_column = contract([f64(sens[k]) for k in range(np_dirs)], f64(r), f64(w))
    return {row: (float(want.sum()), float(S.sum())) for row, (want, S) in per_column.items()}


def check(normal, want, evap, label) -> float:
    got = normal.cpu().tolist()
    worst = 0.0
    for row in range(B.NNORMAL):
        if row in RPECONS_ROWS and not evap:
            assert row not in want and got[row] == 0.0, (label, row, "an rpecons entry without the evaporation branch is not 0.0")
            continue
        w, S = want[row]
        assert got[row] == got[row] and abs(got[row]) != float("inf"), (label, row, "not finite: a value that must not be read was read?")
        assert S > 0.0, (label, row, "the yardstick is zero here: nothing is tested")
        ratio = abs(got[row] - w) / S
        print(f"{label} row {row}: got {got[row]:.17e} want {w:.17e} |got - want| / S {ratio:.3e}")
        assert ratio <= BOUND, (label, row, got[row], w, S)
        worst = max(worst, ratio)
    for a in range(NPAR):
        assert got[row_h(a, a)] >= 0.0, (label, "the diagonal of H", a)
    return worst


@fp64_only
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nproma,ngptot,math_mode", SHAPES)
def test_the_launcher_against_the_contraction_of_the_parameter_jacobian(nproma, ngptot, math_mode, flags):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, 0)
    x15 = {n: t for n, t in x.items() if n != "qsat"}
    evap = bool(prm.levapls2)
    np_dirs = 4 if evap else 3
    r, w = observations(lay, seed=21)
    kept = {k: {n: t.clone() for n, t in d.items()} for k, d in (("x", x), ("r", r), ("w", w))}
    label = f"{(nproma, ngptot, math_mode)} {flags}"

    # 1. all ten outputs observed and weighted, qsat given and qsat NULL, each against its own form of the parameter Jacobian
    normal, work = launch(x, prm, ptsphy, lay, r, w)
    again, _ = launch(x, prm, ptsphy, lay, r, w)
    fused, _ = launch(x15, prm, ptsphy, lay, r, w)
    torch.cuda.synchronize()
    for k, d in (("x", x), ("r", r), ("w", w)):
        for n in d:
            assert same_bits(d[n], kept[k][n]), ("a trajectory, residual or weight plane changed", k, n)
    sens = parjac(x, prm, ptsphy, lay)
    want = yardstick(sens, np_dirs, r, w, lay)
    worst = check(normal, want, evap, label + " all ten")
    # 4. an observed subset, weights None: the contraction over those two outputs
    sub = {n: r[n] for n in ("tent", "fplsl")}
    normal_sub, _ = launch(x, prm, ptsphy, lay, sub, None)
    worst_sub = check(normal_sub, yardstick(sens, np_dirs, sub, {}, lay), evap, label + " tent, fplsl")
    del sens
    sens = parjac(x15, prm, ptsphy, lay)
    worst_fused = check(fused, yardstick(sens, np_dirs, r, w, lay), evap, label + " qsat NULL")
    del sens

    # 2. the tails: every result finite although the planes' padded tails are NaN (check); the workspace's padded tail and guard untouched
    rows = work[:B.NNORMAL * lay.nblocks * lay.nproma].view(B.NNORMAL, -1)
    assert bool(torch.all(torch.isnan(rows[:, lay.ngptot:]))), "a padded tail column wrote its sums"
    assert bool(torch.all(torch.isnan(work[B.NNORMAL * lay.nblocks * lay.nproma:]))), "written past the workspace"
    for row in range(B.NNORMAL):
        written = row not in RPECONS_ROWS or evap
        assert bool(torch.all(torch.isfinite(rows[row, :lay.ngptot]))) if written else bool(torch.all(torch.isnan(rows[row]))), row

    # 3. run to run, and the special cases
    assert same_bits(again, normal), "two launches differ"
    zeros, _ = launch(x, prm, ptsphy, lay, {n: r[n] for n in ("clc", "covptot")}, {n: w[n] for n in ("clc", "covptot")})
    assert bool(torch.all(zeros == 0.0)), "clc and covptot depend on no parameter"
    print(f"{label}: worst |got - want| / S: all ten {worst:.3e}, subset {worst_sub:.3e}, qsat NULL {worst_fused:.3e}")


@pytest.mark.parametrize("flags", FLAGS)
def test_the_launcher_runs_in_this_build_and_repeats_its_bits(flags):
    """Every precision: finite sums, exact zeros where nothing depends on a parameter, the same bits twice."""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, 0)
    r, w = observations(lay, seed=22)
    normal, _ = launch(x, prm, ptsphy, lay, r, w)
    again, _ = launch(x, prm, ptsphy, lay, r, w)
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(normal))) and same_bits(normal, again)
    got = normal.cpu().tolist()
    for row in range(B.NNORMAL):
        assert (got[row] == 0.0) == (row in RPECONS_ROWS and not prm.levapls2), row
    assert all(got[row_h(a, a)] >= 0.0 for a in range(NPAR))


@fp64_only
@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("flags", FLAGS)
def test_param_normal_equations_is_the_launcher(flags, satur):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)  # (satur: the 15 inputs, SATUR in the sweep -- the qsat-NULL launch)
    r, w = observations(lay, seed=23, names=("tent", "tenq", "fplsl", "fhpsn", "clc"))
    w = {n: w[n] for n in ("tent", "fplsl")}
    normal, _ = launch(x, prm, ptsphy, lay, r, w)
    xg = {n: t.clone().requires_grad_() for n, t in x.items()}  # (inputs that require a gradient: the result carries no graph)
    ne = c2.param_normal_equations(xg, prm, ptsphy, lay.ngptot, residual=r, weights=w, satur=satur)
    torch.cuda.synchronize()
    assert isinstance(ne, c2.NormalEquations) and ne.names == P
    assert ne.jtj.shape == (NPAR, NPAR) and ne.jtr.shape == (NPAR,) and ne.jtj.dtype == ne.jtr.dtype == torch.float64
    assert ne.jtj.device == ne.jtr.device == x["pap"].device
    assert not ne.jtj.requires_grad and ne.jtj.grad_fn is None and not ne.jtr.requires_grad and ne.jtr.grad_fn is None
    assert same_bits(ne.jtj, ne.jtj.T.contiguous()), "jtj is not exactly symmetric"
    for a in range(NPAR):
        assert same_bits(ne.jtr[a], normal[row_g(a)]), ("jtr", a)
        for b in range(a, NPAR):
            assert same_bits(ne.jtj[a, b], normal[row_h(a, b)]), ("jtj", a, b)
    assert bool(torch.any(ne.jtj != 0)) and bool(torch.any(ne.jtr != 0))

    # a subset of the parameters: that block only, at the overridden value
    value = 0.8 * prm.rclcrit
    at = copy.copy(prm)
    at.rclcrit = value
    normal_at, _ = launch(x, at, ptsphy, lay, r, w)
    k = P.index("rclcrit")
    for where in ("cpu", DEV):
        sub = c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual=r, weights=w, satur=satur,
                                        params={"rclcrit": torch.tensor(value, dtype=torch.float64, device=where)})
        torch.cuda.synchronize()
        assert sub.names == ("rclcrit",) and sub.jtj.shape == (1, 1) and sub.jtr.shape == (1,) and prm.rclcrit != value
        assert same_bits(sub.jtj[0, 0], normal_at[row_h(k, k)]) and same_bits(sub.jtr[0], normal_at[row_g(k)])
        assert not same_bits(sub.jtj[0, 0], normal[row_h(k, k)]), "the overridden value did not reach the kernel"
    two = c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual=r, weights=w, satur=satur,
                                    params={n: torch.tensor(getattr(prm, n), dtype=torch.float64) for n in ("rlptrc", "rkconv")})
    assert two.names == ("rkconv", "rlptrc")
    assert same_bits(two.jtj, ne.jtj[[0, 2]][:, [0, 2]]) and same_bits(two.jtr, ne.jtr[[0, 2]])
    none = c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual=r, weights=w, satur=satur, params={})
    assert none.names == () and none.jtj.shape == (0, 0) and none.jtr.shape == (0,)


def test_batched_operands_and_a_zero_rpecons_are_refused():
    tab = c2.synthetic_table()
    prm = params(tab)
    x, ptsphy, lay = state(tab, 32, 64, prm, False)
    r, _ = observations(lay, seed=24, names=("tent",))
    T = torch.stack([x["t"], x["t"] + 0.5])
    with pytest.raises(NotImplementedError, match="param_normal_equations"):
        torch.func.vmap(lambda t: c2.param_normal_equations({**x, "t": t}, prm, ptsphy, lay.ngptot, residual=r).jtr)(T)
    R = torch.stack([r["tent"], r["tent"]])
    with pytest.raises(NotImplementedError, match="param_normal_equations"):
        torch.func.vmap(lambda t: c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual={"tent": t}).jtr)(R)
    evap = params(tab, levapls2=True)
    with pytest.raises(ValueError, match="rpecons"):
        c2.param_normal_equations(x, evap, ptsphy, lay.ngptot, residual=r, params={"rpecons": torch.tensor(0.0, dtype=torch.float64)})


def test_a_captured_launch_is_a_chain_of_two_kernels_and_replays_the_eager_bits():
    tab = c2.random_table(137, 100, seed=31)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = state(tab, 64, 1000, prm, 0)
    r, w = observations(lay, seed=25)
    eager, _ = launch(x, prm, ptsphy, lay, r, w)  # the eager call a capture needs first: the CETA table
    on_host = {n: torch.tensor(getattr(prm, n), dtype=torch.float64) for n in P}
    on_device = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64, device=DEV)}
    eager_ne = c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual=r, weights=w, params=on_host)  # (and the device probe)
    torch.cuda.synchronize()

    # the C ABI: two kernel nodes, the second after the first
    _, work = launch(x, prm, ptsphy, lay, r, w)
    cap = torch.full((B.NNORMAL,), NAN, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        launch(x, prm, ptsphy, lay, r, w, work=work, normal=cap)
    hip, g = hip_runtime(), C.c_void_p(graph.raw_cuda_graph())
    count = C.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, C.byref(count)) == 0 and count.value == 2, count.value
    nodes = (C.c_void_p * 2)()
    assert hip.hipGraphGetNodes(g, nodes, C.byref(count)) == 0
    for node in nodes:
        kind = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(kind)) == 0 and kind.value == 0, ("not a kernel node", kind.value)
    assert hip.hipGraphGetEdges(g, None, None, C.byref(count)) == 0 and count.value == 1, ("not a chain", count.value)
    graph.instantiate()
    for _ in range(2):
        cap.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(cap, eager)

    # the torch entry point, without params and with CPU params; device parameters would have to be read on the host
    for p in (None, on_host):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ne = c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual=r, weights=w, params=p)
            with pytest.raises(RuntimeError, match="capturing"):
                c2.param_normal_equations(x, prm, ptsphy, lay.ngptot, residual=r, weights=w, params=on_device)
        for _ in range(2):
            ne.jtj.fill_(NAN)
            ne.jtr.fill_(NAN)
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(ne.jtj, eager_ne.jtj) and same_bits(ne.jtr, eager_ne.jtr)
    for a in range(NPAR):
        assert same_bits(eager_ne.jtr[a], eager[row_g(a)])
