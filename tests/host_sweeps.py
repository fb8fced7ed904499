"""Runners and yardsticks several host-build tests share (tests/test_hostcheck_*.py, and the GPU tests that hold a kernel to a host
sweep): the SATUR-fused and the parameter sweeps of the host build run on a state, the parameter tangent against central differences of
the reference, the parameter Jacobian's sweep, and the column sums' weights, table and fold.  The tests that own a bound state it."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from tests.hostbuild import host_lib
from tests.util import B, PARAM_NAMES, flat_block, flat_fields, host_traj_blocks, increments_of, refcall, set_lib_params

NPROMA, NGPTOT = 32, 100  # the parameter Jacobian's shape: four blocks, a ragged tail
HALF = ("fplsl", "fplsn", "fhpsl", "fhpsn")


# ---- SATUR in the sweep (tests/test_hostcheck_satur_lin.py) ----
def increments15(st) -> dict:
    inc = increments_of(st, np.zeros_like(st.PAP))
    del inc["qsat"]
    return inc


def run_tl_satur(prm, st, inc15) -> dict:
    nb, nlev, nproma = st.nblocks, st.nlev, st.nproma
    i, _ = host_traj_blocks(st, None)
    tl = flat_fields("out", nb, nlev, nproma, fill=np.nan)
    assert host_lib("satur_lin").hostcheck_tl_satur(C.byref(prm), st.ptsphy, nproma, nlev, st.ngptot, C.byref(i), C.byref(flat_block("in", inc15)),
                                                    C.byref(flat_block("out", tl))) == 0
    return tl


def field_err(ref_blocks: list, got_blocks: list) -> float:
    """max |got - ref| over the active columns relative to the field's maximum there"""
    d = max(float(np.max(np.abs(g - r))) for r, g in zip(ref_blocks, got_blocks))
    m = max(float(np.max(np.abs(r))) for r in ref_blocks)
    return 0.0 if d == 0.0 else d / m


def trajectory_for_reverse(prm, st, qsat):
    """PFPLSL5 / PFPLSN5 and the cover checkpoints, as cloudsc2_ad_launch_forward leaves them"""
    scratch = np.zeros((st.nblocks, st.nlev, st.nproma), dtype=B.REAL)
    fwd = st.copy()
    fi, fo = host_traj_blocks(fwd, qsat)
    assert host_lib("vjp").hostcheck_vjp_sweep(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(fi), C.byref(fo), None, None,
                                               scratch.ctypes.data, 1, 0) == 0
    return fwd, scratch


def run_vjp_satur(prm, st, fwd, scratch, u: dict):
    nb, nlev, nproma = st.nblocks, st.nlev, st.nproma
    i, _ = host_traj_blocks(st, None)
    _, o = host_traj_blocks(fwd, None)
    xa = flat_fields("in", nb, nlev, nproma, fill=np.nan)
    del xa["qsat"]  # no plane for it: a write through its (NULL) pointer would fault
    y = {n: a.copy() for n, a in u.items()}
    assert host_lib("satur_lin").hostcheck_vjp_satur(C.byref(prm), st.ptsphy, nproma, nlev, st.ngptot, C.byref(i), C.byref(o),
                                                     C.byref(flat_block("in", xa)), C.byref(flat_block("out", y)), scratch.ctypes.data) == 0
    return xa, y


# ---- the parameter sweeps (tests/test_hostcheck_par.py states the cap and the bound of the differences) ----
def dvec(values) -> C.Array:
    return (C.c_double * 4)(*[float(v) for v in values])


def run_tl_par(prm, st, inc: dict, dpar, qsat=None) -> dict:
    """TL(dx, dp) of the host build; qsat given: the satur = 0 form (inc holds 16 fields), None: satur = 1 (15 fields)"""
    nb, nlev, nproma = st.nblocks, st.nlev, st.nproma
    i, _ = host_traj_blocks(st, qsat)
    tl = flat_fields("out", nb, nlev, nproma, fill=np.nan)
    assert host_lib("par").hostcheck_tl_par(C.byref(prm), st.ptsphy, nproma, nlev, st.ngptot, int(qsat is None), C.byref(i),
                                            C.byref(flat_block("in", inc)), dvec(dpar), C.byref(flat_block("out", tl))) == 0
    return tl


def run_vjp_par(prm, st, fwd, scratch, u: dict, qsat=None):
    """the input adjoints, the (read-only) output adjoints, par_adj[4] and the workspace of the host build's parameter VJP"""
    nb, nlev, nproma = st.nblocks, st.nlev, st.nproma
    i, _ = host_traj_blocks(st, qsat)
    _, o = host_traj_blocks(fwd, qsat)
    xa = flat_fields("in", nb, nlev, nproma, fill=np.nan)
    if qsat is None:
        del xa["qsat"]
    y = {n: a.copy() for n, a in u.items()}
    work = np.full((4, nb * nproma), np.nan)
    par_adj = dvec([np.nan] * 4)
    assert host_lib("par").hostcheck_vjp_par(C.byref(prm), st.ptsphy, nproma, nlev, st.ngptot, int(qsat is None), C.byref(i), C.byref(o),
                                             C.byref(flat_block("in", xa)), C.byref(flat_block("out", y)), scratch.ctypes.data,
                                             work.ctypes.data, par_adj) == 0
    return xa, y, np.array(par_adj[:]), work


def with_param(prm, name: str, value: float):
    p = copy.copy(prm)
    setattr(p, name, value)
    return p


def reference_difference(ref, prm, st, qs, name: str, h: float) -> dict:
    """(F(p (1 + h)) - F(p (1 - h))) / (2 h p) of the reference's NL kernel, one block"""
    p0 = getattr(prm, name)
    outs = []
    for s in (+1.0, -1.0):
        set_lib_params(ref, with_param(prm, name, p0 * (1.0 + s * h)))
        outs.append(ref.cloudsc2(st.ptsphy, refcall.block_inputs(st, 0, qs), ldrain1d=bool(prm.ldrain1d)))
    set_lib_params(ref, prm)
    return {n: (outs[0][n] - outs[1][n]) / (2.0 * h * p0) for n in B.OUT_NAMES}


def exact_zero_fields(name: str, evap: bool) -> tuple:
    if name == "rpecons" and not evap:
        return tuple(B.OUT_NAMES)
    z = ["clc", "covptot"]
    if name == "rclcrit" and evap:
        z.append("teni")
    return tuple(z)


def check_against_reference_differences(ref, prm, st, qs, tl_of, label: str) -> float:
    """tl_of(k) -> the parameter tangent for dpar = e_k as {field: (nlev[+1], 100)}; returns the worst error of the case"""
    evap = bool(prm.levapls2 or prm.ldrain1d)
    worst = 0.0
    for k, name in enumerate(PARAM_NAMES):
        fd5 = reference_difference(ref, prm, st, qs, name, 1e-5)
        fd6 = reference_difference(ref, prm, st, qs, name, 1e-6)
        tl = tl_of(k)
        out = np.zeros(st.ngptot, dtype=bool)
        for n in B.OUT_NAMES:
            m = float(np.max(np.abs(fd6[n])))
            if m > 0.0:
                out |= np.max(np.abs(fd5[n] - fd6[n]), axis=0) > 1e-5 * m
        assert out.sum() <= 2, (label, name, "columns left out", int(out.sum()))
        keep = ~out
        zeros = exact_zero_fields(name, evap)
        errs = {}
        for n in B.OUT_NAMES:
            got, want = tl[n][:, keep], fd6[n][:, keep]
            assert not np.any(np.isnan(got)), (label, name, n)
            if n in zeros:
                assert np.all(got == 0.0) and np.all(want == 0.0), (label, name, n, "must be exactly zero")
                continue
            m = float(np.max(np.abs(want)))
            if m == 0.0:  # a field the reference does not move at all (tenl under rpecons): nor may the tangent
                assert np.all(got == 0.0), (label, name, n, "the reference's difference vanishes, the tangent does not")
                continue
            errs[n] = float(np.max(np.abs(got - want))) / m
        e = max(errs.values()) if errs else 0.0
        print(f"{label} {name}: left out {int(out.sum())}, worst {e:.3e} " + " ".join(f"{n} {v:.1e}" for n, v in errs.items()))
        for n, v in errs.items():
            assert v <= 1e-5, (label, name, n, v)
        worst = max(worst, e)
    return worst


def run_parjac(prm, st, qsat=None) -> list:
    """the four blocks of the host build's sweep, NaN-prefilled; qsat None: SATUR evaluated in the sweep"""
    i, _ = host_traj_blocks(st, qsat)
    sens = [flat_fields("out", st.nblocks, st.nlev, st.nproma, fill=np.nan) for _ in PARAM_NAMES]
    blocks = (B.Outputs * len(PARAM_NAMES))(*(flat_block("out", s) for s in sens))
    assert host_lib("parjac").hostcheck_tl_parjac(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(i), blocks) == 0
    return sens


# ---- column sums (tests/test_hostcheck_colsum.py): numpy, in the library's real type ----
def weight_patterns(nlev: int) -> list:
    """(name, {output: weights of length nlevx}); (a) has negative entries, exact zeros and non-zero entries at both ends"""
    rng = np.random.default_rng(20261020)
    nlevx = lambda n: nlev + (1 if n in HALF else 0)  # noqa: E731
    a = {}
    for n in B.OUT_NAMES:
        w = rng.uniform(-1.0, 1.0, nlevx(n))
        w[rng.random(nlevx(n)) < 0.2] = 0.0
        w[0], w[-1] = -0.75, 0.625
        a[n] = w.astype(B.REAL)
    assert all((w < 0).any() and (w == 0).any() for w in a.values())
    surface = np.zeros(nlev + 1, dtype=B.REAL)
    surface[-1] = 1.0
    pick = lambda *names: {n: a[n] for n in names}  # noqa: E731
    return [("all", a), ("surface", {"fplsl": surface, "fplsn": surface.copy()}), ("tent,tenq", pick("tent", "tenq")), ("covptot", pick("covptot"))]


def table_of(weights: dict, nlev: int) -> np.ndarray:
    """the launchers' table: ten rows of nlev + 1, NaN where a row is not given or an entry is unused"""
    t = np.full((len(B.OUT_NAMES), nlev + 1), np.nan, dtype=B.REAL)
    for n, w in weights.items():
        t[B.OUT_NAMES.index(n), :len(w)] = w
    return t


def fold(w: np.ndarray, plane: np.ndarray) -> np.ndarray:
    """the contract: acc = +0; acc = fl(acc + fl(w[k] * plane[:, k, :])) in the library's real type"""
    assert w.dtype == B.REAL and plane.dtype == B.REAL and len(w) == plane.shape[1]
    acc = np.zeros((plane.shape[0], plane.shape[2]), dtype=B.REAL)
    for k in range(len(w)):
        p = w[k] * plane[:, k, :]
        acc = acc + p
    return acc
