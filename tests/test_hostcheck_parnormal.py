"""The normal-equations sweep of the parameters (parnormal_column: the first kernel of cloudsc2_parnormal_launch), compiled for the HOST:
NPROMA 32 x 100 columns (four blocks, a ragged tail), both arithmetics, the synthetic table and random_table(137, 100, seed=5).

The yardstick is the parent's parameter Jacobian, hostcheck_tl_parjac, contracted in float64 by tests/parnormal_yardstick.py, which
also derives the bound 1e-12 * S.  The host builds have no contraction, so the sweep's J is hostcheck_tl_parjac's bits in both
precisions and each column's sums differ from the yardstick's only in the order of the additions.  Every residual and weight plane is
NaN in the padded tail and, for the four fluxes, at half level 0: none of those values may be read.
Measured (worst |got - want| / S over rows and columns; fast and precise, both tables, the four flag sets): 2.1e-15 in fp64 (seed5, no
evaporation branch, the subset), 2.4e-15 in fp32; the test prints every case."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.host_sweeps import NGPTOT, NPROMA, run_parjac
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.parnormal_yardstick import BOUND, RPECONS_ROWS, contract
from tests.util import FLAG_SETS, B, blocks_of, c2, columns, flat_block, host_qsat, host_traj_blocks, make_params, refcall, the_tables


def observations(st, seed: int):
    """seeded residuals and positive weights on all ten outputs, (nblocks, nlevx, nproma); NaN wherever the sweep must not read: the
    padded tail of every plane and half level 0 of the fluxes"""
    rng = np.random.default_rng(seed)
    r, w = {}, {}
    for n in B.OUT_NAMES:
        shape = (st.nblocks, st.nlev + (1 if n in refcall.HALF else 0), st.nproma)
        r[n] = rng.standard_normal(shape).astype(B.REAL)
        w[n] = rng.uniform(0.5, 2.0, shape).astype(B.REAL)
        for a in (r[n], w[n]):
            for ibl, icend in blocks_of(st):
                a[ibl][:, icend:] = np.nan
            if n in refcall.HALF:
                a[:, 0, :] = np.nan
    return r, w


def run_parnormal(prm, st, qsat, r: dict, w) -> np.ndarray:
    """the host sweep's workspace (CLOUDSC2_NNORMAL, padded columns), NaN-prefilled; w None: the weight block itself is NULL"""
    i, _ = host_traj_blocks(st, qsat)
    work = np.full((B.NNORMAL, st.nblocks * st.nproma), np.nan)
    assert host_lib("parnormal").hostcheck_parnormal(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(i),
                                                     C.byref(flat_block("out", r)), C.byref(flat_block("out", w)) if w is not None else None,
                                                     work.ctypes.data) == 0
    return work


def yardstick(sens: list, np_dirs: int, r: dict, w: dict) -> dict:
    def f64(d):
        return {n: columns(a, NGPTOT).astype(np.float64) for n, a in d.items()}

    return contract([f64(sens[k]) for k in range(np_dirs)], f64(r), f64(w))


def check(work: np.ndarray, want: dict, evap: bool, label) -> float:
    worst = 0.0
    for row in range(B.NNORMAL):
        assert np.all(np.isnan(work[row, NGPTOT:])), (label, row, "a padded tail column wrote its sums")
        if row in RPECONS_ROWS and not evap:
            assert row not in want and np.all(np.isnan(work[row])), (label, row, "an rpecons row was written without the evaporation branch")
            continue
        got, (w, S) = work[row, :NGPTOT], want[row]
        assert np.all(np.isfinite(got)), (label, row, "an active column left no sum, or read a NaN it must not read")
        err = np.abs(got - w)
        assert np.all(err <= BOUND * S), (label, row, float(np.max(err / np.maximum(S, 1e-300))))
        worst = max(worst, float(np.max(np.where(S > 0, err / np.where(S > 0, S, 1.0), 0.0))))
    return worst


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("which", [0, 1])
def test_every_column_holds_the_contraction_of_the_parameter_jacobian(precise, which, flags):
    name, tab = the_tables()[which]
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, NPROMA, NGPTOT)
    evap = bool(prm.levapls2 or prm.ldrain1d)
    np_dirs = 4 if evap else 3
    qsat = host_qsat(st)
    r, w = observations(st, seed=11 + which)
    label = (name, flags, "precise" if precise else "fast")

    sens = run_parjac(prm, st, qsat)
    worst = check(run_parnormal(prm, st, qsat, r, w), yardstick(sens, np_dirs, r, w), evap, label + ("all ten, weighted",))
    moved = yardstick(sens, np_dirs, r, w)
    assert all(np.any(moved[row][1] > 0) for row in moved), (label, "a row the yardstick finds zero everywhere: nothing is tested there")

    # an observed subset, the weight block NULL: the contraction over those two outputs with weight 1
    sub = {n: r[n] for n in ("tent", "fplsl")}
    worst_sub = check(run_parnormal(prm, st, qsat, sub, None), yardstick(sens, np_dirs, sub, {}), evap, label + ("tent, fplsl",))
    # ... and with one weight of the two given
    one = {"fplsl": w["fplsl"]}
    worst_sub = max(worst_sub, check(run_parnormal(prm, st, qsat, sub, one), yardstick(sens, np_dirs, sub, one), evap, label + ("one weight",)))

    # SATUR evaluated in the sweep, against the contraction of hostcheck_tl_parjac's qsat-NULL form
    fused = run_parjac(prm, st, None)
    worst_fused = check(run_parnormal(prm, st, None, r, w), yardstick(fused, np_dirs, r, w), evap, label + ("qsat NULL",))
    print(f"{label}: worst |got - want| / S: all ten {worst:.3e}, subset {worst_sub:.3e}, qsat NULL {worst_fused:.3e}")


def test_clc_and_covptot_contribute_exact_zeros_and_their_planes_are_not_read(precise):
    tab = c2.random_table(137, 100, seed=5)
    prm = make_params(tab, levapls2=True)
    st = c2.state_from_table(tab, NPROMA, NGPTOT)
    nan = {n: np.full((st.nblocks, st.nlev, st.nproma), np.nan, dtype=B.REAL) for n in ("clc", "covptot")}
    work = run_parnormal(prm, st, host_qsat(st), nan, nan)
    assert np.all(work[:, :NGPTOT] == 0.0) and np.all(np.isnan(work[:, NGPTOT:]))
