"""The parameter Jacobian and the normal equations of the column sums on the MI355X: cloudsc2_parjac_launch_colsum and
cloudsc2_parnormal_launch_colsum through the C ABI, ``c2.param_jacobian_column_sums`` and ``c2.param_normal_equations_column_sums``
through torch.

The yardstick is the parent's route: the planes of cloudsc2_tl_launch_parjac folded sequentially over the levels with separate torch
``mul`` and ``add`` (the fold of tests/colsum_variant_checks.py) in the library's real type, and for the normal equations contracted in
float64 by tests/parcolsum_yardstick.py, ``|got - want| <= 1e-12 * S`` entry by entry.  A sensitivity sum must be the bits of that fold.
Residual and weight arrays are NaN in the padded tail; every array a launch must not write is prefilled with NaN and looked at afterwards.
The module runs in the process's precision: tests/test_single_parcolsum.py starts it once more under CLOUDSC2_PRECISION=single (the
normal-equations comparisons are fp64 statements, as in tests/test_gpu_autograd_parnormal.py).
Measured on the MI355X: no element of any sum differs from the fold, in fp64 and in fp32 (every case prints its count); the normal
equations' worst |got - want| / S over the eight cases is 3.4e-16 ((32, 100), the evaporation branch, the subsets); the peak of allocated
memory rises by 1.85 MB (normal equations) and 1.06 MB (two sums) where a full-level plane is 17.96 MB."""
from __future__ import annotations

import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, params, same_bits, state
from tests.parcolsum_variant_checks import (NPAR, act, check_sums, folded, launch_normal, launch_sums, level_weights, observations,
                                             parjac_planes)
from tests.parcolsum_yardstick import BOUND, RPECONS_ROWS, contract_sums, row_g, row_h
from tests.util import B, ROOT, c2, fp64_only

pytestmark = pytest.mark.gpu

P = c2.PARAM_NAMES
NAN = float("nan")
# test_gpu_autograd_parnormal.py's: lanes and a ragged tail, fold threads with nothing to add | a tail, fold threads that add one or two
# columns | full blocks, sixteen columns per fold thread
SHAPES = [(32, 100, 1), (32, 100, 2), (128, 1300, 0), (128, 16384, 0)]
FLAGS = [dict(), dict(levapls2=True)]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("nproma,ngptot,math_mode", SHAPES)
def test_the_sums_launcher_gives_the_bits_of_the_fold_of_the_parameter_jacobian(nproma, ngptot, math_mode, flags):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, 0)
    x15 = {n: t for n, t in x.items() if n != "qsat"}
    np_dirs = 4 if prm.levapls2 else 3
    kept = {n: t.clone() for n, t in x.items()}
    for qname, xin in (("qsat", x), ("qsat NULL", x15)):
        sens = parjac_planes(xin, prm, ptsphy, lay)
        for wname, weights in level_weights():
            label = f"{(nproma, ngptot, math_mode)} {flags} {qname} {wname}"
            want = folded(sens, np_dirs, weights)
            differ = check_sums(launch_sums(xin, prm, ptsphy, lay, weights), want, np_dirs, lay, label)
            print(f"{label}: {differ} elements differ from the fold")
            assert differ == 0, (label, differ)
        del sens
    for n in x:
        assert same_bits(x[n], kept[n]), ("a trajectory plane changed", n)


@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("flags", FLAGS)
def test_param_jacobian_column_sums_is_the_launcher(flags, satur):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)
    evap = bool(prm.levapls2)
    weights = dict(level_weights())["all ten"]
    weights = {n: weights[n] for n in ("tenq", "clc", "fplsl", "fplsn")}
    raw = launch_sums(x, prm, ptsphy, lay, {n: w for n, w in weights.items() if n != "clc"})
    xg = {n: t.clone().requires_grad_() for n, t in x.items()}  # (inputs that require a gradient: the result carries no graph)
    sens = c2.param_jacobian_column_sums(xg, prm, ptsphy, lay.ngptot, level_weights=weights, satur=satur)
    torch.cuda.synchronize()
    assert tuple(sens) == P
    for k, pname in enumerate(P):
        out = sens[pname]
        assert isinstance(out, c2.Cloudsc2Outputs)
        for n in B.OUT_NAMES:
            t = getattr(out, n)
            if n not in weights:
                assert t is None, (pname, n)
                continue
            assert t.shape == (lay.nblocks, lay.nproma) and t.dtype == B.torch_real() and not t.requires_grad and t.grad_fn is None
            assert bool(torch.all(t.reshape(-1)[lay.ngptot:] == 0)), (pname, n, "the padded tail is not zero")
            if n == "clc" or (pname == "rpecons" and not evap):
                assert bool(torch.all(t == 0)), (pname, n, "must be zero tensors")
            else:
                assert same_bits(act(t, lay), act(raw[k][n], lay)), (pname, n, "not the launcher's bits")
                assert bool(torch.any(t != 0)), (pname, n)

    # a subset of the parameters: that entry only, at the overridden value
    value = 0.8 * prm.rclcrit
    at = copy.copy(prm)
    at.rclcrit = value
    raw_at = launch_sums(x, at, ptsphy, lay, {n: w for n, w in weights.items() if n != "clc"})
    k = P.index("rclcrit")
    for where in ("cpu", DEV):
        sub = c2.param_jacobian_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights, satur=satur,
                                            params={"rclcrit": torch.tensor(value, dtype=torch.float64, device=where)})
        torch.cuda.synchronize()
        assert tuple(sub) == ("rclcrit",) and prm.rclcrit != value
        assert same_bits(act(sub["rclcrit"].fplsl, lay), act(raw_at[k]["fplsl"], lay))
        assert not same_bits(act(sub["rclcrit"].tenq, lay), act(raw[k]["tenq"], lay)), "the overridden value did not reach the kernel"
    zeros = c2.param_jacobian_column_sums(x, prm, ptsphy, lay.ngptot, level_weights={"covptot": dict(level_weights())["all ten"]["covptot"]},
                                          satur=satur)
    assert all(bool(torch.all(zeros[p].covptot == 0)) and zeros[p].tent is None for p in P)
    T = torch.stack([x["t"], x["t"] + 0.5])
    with pytest.raises(NotImplementedError, match="param_jacobian_column_sums"):
        torch.func.vmap(lambda t: c2.param_jacobian_column_sums({**x, "t": t}, prm, ptsphy, lay.ngptot, level_weights=weights, satur=satur)["rkconv"].tenq)(T)


# ---- the normal form ----------------------------------------------------------------------------------------------------------------------

def yardstick(want_sums, np_dirs, r, w, lay):
    """{row: (want, S)} as Python floats: the folded sums of the parent's planes contracted in float64 over the active columns"""
    f64 = lambda d: {n: act(t, lay).to(torch.float64) for n, t in d.items()}  # noqa: E731
    per_column = contract_sums([f64(want_sums[k]) for k in range(np_dirs)], f64(r), f64(w))
    return {row: (float(want.sum()), float(S.sum())) for row, (want, S) in per_column.items()}


def check_normal(normal, want, evap, label) -> float:
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
def test_the_normal_launcher_against_the_contraction_of_the_folded_parameter_jacobian(nproma, ngptot, math_mode, flags):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, math_mode, **flags)
    x, ptsphy, lay = state(tab, nproma, ngptot, prm, 0)
    x15 = {n: t for n, t in x.items() if n != "qsat"}
    evap = bool(prm.levapls2)
    np_dirs = 4 if evap else 3
    weights = dict(level_weights())["all ten"]
    r, w = observations(lay, tuple(weights), seed=41)
    kept = {k: {n: t.clone() for n, t in d.items()} for k, d in (("x", x), ("r", r), ("w", w))}
    label = f"{(nproma, ngptot, math_mode)} {flags}"

    normal, work = launch_normal(x, prm, ptsphy, lay, weights, r, w)
    again, _ = launch_normal(x, prm, ptsphy, lay, weights, r, w)
    fused, _ = launch_normal(x15, prm, ptsphy, lay, weights, r, w)
    torch.cuda.synchronize()
    for k, d in (("x", x), ("r", r), ("w", w)):
        for n in d:
            assert same_bits(d[n], kept[k][n]), ("a trajectory plane, residual or weight changed", k, n)
    want_sums = folded(parjac_planes(x, prm, ptsphy, lay), np_dirs, weights)
    worst = check_normal(normal, yardstick(want_sums, np_dirs, r, w, lay), evap, label + " all ten")
    # a subset of the sums given weights, observed with weights=None; then the surface fluxes alone with one weight
    sub = {n: r[n] for n in ("tent", "fplsl")}
    normal_sub, _ = launch_normal(x, prm, ptsphy, lay, weights, sub, None)
    worst_sub = check_normal(normal_sub, yardstick(want_sums, np_dirs, sub, {}, lay), evap, label + " tent, fplsl")
    surf = dict(level_weights())["surface"]
    rs, ws = {n: r[n] for n in surf}, {"fplsn": w["fplsn"]}
    normal_surf, _ = launch_normal(x, prm, ptsphy, lay, surf, rs, ws)
    worst_sub = max(worst_sub, check_normal(normal_surf, yardstick(folded(parjac_planes(x, prm, ptsphy, lay), np_dirs, surf), np_dirs, rs, ws, lay),
                                            evap, label + " surface"))
    worst_fused = check_normal(fused, yardstick(folded(parjac_planes(x15, prm, ptsphy, lay), np_dirs, weights), np_dirs, r, w, lay), evap,
                               label + " qsat NULL")

    # the workspace's padded tail and guard untouched; every written row finite
    rows = work[:B.NNORMAL * lay.nblocks * lay.nproma].view(B.NNORMAL, -1)
    assert bool(torch.all(torch.isnan(rows[:, lay.ngptot:]))), "a padded tail column wrote its sums"
    assert bool(torch.all(torch.isnan(work[B.NNORMAL * lay.nblocks * lay.nproma:]))), "written past the workspace"
    for row in range(B.NNORMAL):
        written = row not in RPECONS_ROWS or evap
        assert bool(torch.all(torch.isfinite(rows[row, :lay.ngptot]))) if written else bool(torch.all(torch.isnan(rows[row]))), row
    assert same_bits(again, normal), "two launches differ"
    zeros, _ = launch_normal(x, prm, ptsphy, lay, weights, {n: r[n] for n in ("clc", "covptot")}, {n: w[n] for n in ("clc", "covptot")})
    assert bool(torch.all(zeros == 0.0)), "clc and covptot depend on no parameter"
    print(f"{label}: worst |got - want| / S: all ten {worst:.3e}, subsets {worst_sub:.3e}, qsat NULL {worst_fused:.3e}")


@pytest.mark.parametrize("flags", FLAGS)
def test_the_normal_launcher_runs_in_this_build_and_repeats_its_bits(flags):
    """Every precision: finite sums, exact zeros where nothing depends on a parameter, the same bits twice."""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, 0)
    weights = dict(level_weights())["surface"]
    r, w = observations(lay, tuple(weights), seed=42)
    normal, _ = launch_normal(x, prm, ptsphy, lay, weights, r, w)
    again, _ = launch_normal(x, prm, ptsphy, lay, weights, r, w)
    torch.cuda.synchronize()
    assert bool(torch.all(torch.isfinite(normal))) and same_bits(normal, again)
    got = normal.cpu().tolist()
    for row in RPECONS_ROWS:
        assert (got[row] == 0.0) == (not prm.levapls2), row
    assert all(got[row_h(a, a)] >= 0.0 for a in range(NPAR)) and got[row_h(0, 0)] > 0.0


@fp64_only
@pytest.mark.parametrize("satur", [False, True])
@pytest.mark.parametrize("flags", FLAGS)
def test_param_normal_equations_column_sums_is_the_launcher(flags, satur):
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, **flags)
    x, ptsphy, lay = state(tab, 32, 100, prm, satur)
    every = dict(level_weights())["all ten"]
    weights = {n: every[n] for n in ("tent", "tenq", "fplsl", "fhpsn", "clc")}
    r, w = observations(lay, ("tent", "fplsl", "fhpsn", "clc"), seed=43)
    w = {n: w[n] for n in ("tent", "fplsl")}
    normal, _ = launch_normal(x, prm, ptsphy, lay, weights, r, w)
    xg = {n: t.clone().requires_grad_() for n, t in x.items()}
    call = lambda xx=x, **kw: c2.param_normal_equations_column_sums(xx, prm, ptsphy, lay.ngptot, level_weights=weights, residual=r,  # noqa: E731
                                                                    weights=w, satur=satur, **kw)
    ne = call(xg)
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
    none_w = c2.param_normal_equations_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights, residual={"fplsl": r["fplsl"]},
                                                   weights=None, satur=satur)
    unweighted, _ = launch_normal(x, prm, ptsphy, lay, weights, {"fplsl": r["fplsl"]}, None)
    assert same_bits(none_w.jtr[0], unweighted[row_g(0)]) and same_bits(none_w.jtj[0, 1], unweighted[row_h(0, 1)])

    value = 0.8 * prm.rclcrit
    at = copy.copy(prm)
    at.rclcrit = value
    normal_at, _ = launch_normal(x, at, ptsphy, lay, weights, r, w)
    k = P.index("rclcrit")
    for where in ("cpu", DEV):
        sub = call(params={"rclcrit": torch.tensor(value, dtype=torch.float64, device=where)})
        torch.cuda.synchronize()
        assert sub.names == ("rclcrit",) and sub.jtj.shape == (1, 1) and sub.jtr.shape == (1,) and prm.rclcrit != value
        assert same_bits(sub.jtj[0, 0], normal_at[row_h(k, k)]) and same_bits(sub.jtr[0], normal_at[row_g(k)])
        assert not same_bits(sub.jtj[0, 0], normal[row_h(k, k)]), "the overridden value did not reach the kernel"
    none = call(params={})
    assert none.names == () and none.jtj.shape == (0, 0) and none.jtr.shape == (0,)
    R = torch.stack([r["tent"], r["tent"]])
    with pytest.raises(NotImplementedError, match="param_normal_equations_column_sums"):
        torch.func.vmap(lambda t: c2.param_normal_equations_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights,
                                                                        residual={"tent": t}, satur=satur).jtr)(R)


def test_neither_call_allocates_a_full_level_plane():
    """(128, 16384), NLEV 137: the peak of torch.cuda.max_memory_allocated across either call rises by less than one full-level plane (the
    normal form's workspace is 14 rows per column against a plane's 137)"""
    tab = c2.random_table(137, 100, seed=5)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = state(tab, 128, 16384, prm, 0)
    weights = dict(level_weights())["surface"]
    r, w = observations(lay, tuple(weights), seed=44)
    plane = lay.nblocks * lay.nlev * lay.nproma * x["pap"].element_size()
    for name, call in (("normal equations", lambda: c2.param_normal_equations_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights,
                                                                                          residual=r, weights=w)),
                       ("two sums", lambda: c2.param_jacobian_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights))):
        call()  # (the CETA table, the device probe)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        out = call()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(DEV) - base
        print(f"{name}: peak rises by {rise} bytes, a full-level plane is {plane}")
        assert 0 < rise < plane, (name, rise, plane)
        del out


def test_both_calls_capture_and_replay_the_eager_bits_for_a_new_residual():
    tab = c2.random_table(137, 100, seed=31)
    prm = params(tab, levapls2=True)
    x, ptsphy, lay = state(tab, 64, 1000, prm, 0)
    weights = dict(level_weights())["surface"]
    r, w = observations(lay, tuple(weights), seed=45)
    r2, _ = observations(lay, tuple(weights), seed=46)
    on_host = {n: torch.tensor(getattr(prm, n), dtype=torch.float64) for n in P}
    on_device = {"rkconv": torch.tensor(prm.rkconv, dtype=torch.float64, device=DEV)}
    ne_call = lambda rr, p=None: c2.param_normal_equations_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights, residual=rr,  # noqa: E731
                                                                       weights=w, params=p)
    js_call = lambda p=None: c2.param_jacobian_column_sums(x, prm, ptsphy, lay.ngptot, level_weights=weights, params=p)  # noqa: E731
    eager, eager2, eager_js = ne_call(r), ne_call(r2), js_call()  # one eager call first: the CETA table, the device probe
    torch.cuda.synchronize()
    assert not same_bits(eager.jtr, eager2.jtr)
    for p in (None, on_host):
        live = {n: t.clone() for n, t in r.items()}
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ne = ne_call(live, p)
            js = js_call(p)
            with pytest.raises(RuntimeError, match="capturing"):
                ne_call(live, on_device)
            with pytest.raises(RuntimeError, match="capturing"):
                js_call(on_device)
        for rr, want in ((r, eager), (r2, eager2)):
            for n in live:
                live[n].copy_(rr[n])  # the residual changed in place
            ne.jtj.fill_(NAN)
            ne.jtr.fill_(NAN)
            js["rkconv"].fplsl.fill_(NAN)
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(ne.jtj, want.jtj) and same_bits(ne.jtr, want.jtr)
            for pn in P:
                assert same_bits(js[pn].fplsl, eager_js[pn].fplsl) and same_bits(js[pn].fplsn, eager_js[pn].fplsn)


# ---- both addressing forms -----------------------------------------------------------------------------------------------------------------

_device_trouble = []


def test_both_addressing_forms_give_the_same_bits(tmp_path):
    """tests/parcolsum_variant_checks.py for CLOUDSC2_OFF32 = 0, 1, one child after the other, each under its own time limit, no retry; the
    second is not started if the first did not end well.  Each child compares with the fold of its own process's parameter Jacobian; the
    parent compares the two forms' arrays bit for bit."""
    if _device_trouble:
        pytest.fail(f"not started: {_device_trouble[0]}")
    runs = []
    for mode in ("0", "1"):
        f = str(tmp_path / f"parcolsum_off32_{mode}.npz")
        try:
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "parcolsum_variant_checks.py"), f], cwd=ROOT,
                               env={**os.environ, "CLOUDSC2_OFF32": mode}, capture_output=True, text=True, timeout=240)
            rc, text = p.returncode, p.stdout + p.stderr
        except subprocess.TimeoutExpired as e:
            rc, text = 124, f"time limit: {e}"
        print(f"CLOUDSC2_OFF32={mode}: return code {rc}\n{text[-3000:]}")
        if rc in (124, 134, 137, 139) or rc < 0:
            _device_trouble.append(f"tests/parcolsum_variant_checks.py with CLOUDSC2_OFF32={mode} ended with {rc}")
        assert rc == 0, (mode, text[-4000:])
        with np.load(f) as z:
            runs.append({k: z[k] for k in z.files})
    assert list(runs[0]) == list(runs[1]) and len(runs[0]) >= 2 * 2 * 2 * 2
    for k in runs[0]:
        assert runs[0][k].tobytes() == runs[1][k].tobytes(), (k, "the two addressing forms differ")
