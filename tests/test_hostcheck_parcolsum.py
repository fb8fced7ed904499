"""The parameter column-sum sweep (parcolsum_column: what cloudsc2_parjac_launch_colsum and cloudsc2_parnormal_launch_colsum run), compiled
for the HOST: NPROMA 32 x 100 columns (four blocks, a ragged tail), the four FLAG_SETS, both arithmetics, qsat given and SATUR in the
sweep, the synthetic table and random_table(137, 100, seed=5).

The yardstick is the parent's parameter Jacobian, hostcheck_tl_parjac, folded sequentially over the levels by the column-sum tests'
``fold`` in the library's real type.  The host builds have no contraction, so every sensitivity sum must be those bits, in both
precisions.  For the normal form the folded sums are contracted in float64 by tests/parcolsum_yardstick.py, bound 1e-12 * S.  Residual
and weight arrays are NaN in the padded tail, absent arrays are NULL, and every array the sweep must not write is prefilled and compared.
Measured (worst |got - want| / S over rows and columns, all cases): 0 -- a column's products are the yardstick's and are added in the same
order; the test prints every case."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.host_sweeps import NGPTOT, NPROMA, fold, run_parjac, table_of, weight_patterns
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.parcolsum_yardstick import BOUND, PAR_SUMS, RPECONS_ROWS, contract_sums
from tests.util import (FLAG_SETS, PARAM_NAMES, B, blocks_of, c2, flat_block, host_qsat, host_traj_blocks, make_params, same_bits,
                        the_tables)

NLEV = 137


def patterns() -> list:
    """(name, {sum: weights}): the surface fluxes alone, all ten names (negative entries, exact zeros), one full-level sum"""
    every = dict(weight_patterns(NLEV))["all"]
    surface = np.zeros(NLEV + 1, dtype=B.REAL)
    surface[-1] = 1.0
    return [("surface", {"fplsl": surface, "fplsn": surface.copy()}), ("all ten", every), ("tenq", {"tenq": every["tenq"]})]


def folded(sens: list, np_dirs: int, weights: dict) -> list:
    """the yardstick's sums: direction k, name n -> (nblocks, nproma); the planes' NaN tails stay NaN"""
    return [{n: fold(w, sens[k][n]) for n, w in weights.items()} for k in range(np_dirs)]


def run_sums(prm, st, qsat, weights: dict) -> list:
    """the host sweep's four blocks of sums, NaN-prefilled (the fourth is passed, and must stay untouched, without the evaporation branch)"""
    i, _ = host_traj_blocks(st, qsat)
    table = table_of(weights, st.nlev)
    sums = [{n: np.full((st.nblocks, st.nproma), np.nan, dtype=B.REAL) for n in weights} for _ in PARAM_NAMES]
    blocks = (B.Outputs * len(PARAM_NAMES))(*(flat_block("out", s) for s in sums))
    assert host_lib("parcolsum").hostcheck_parjac_colsum(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(i), table.ctypes.data,
                                                         blocks) == 0
    return sums


def check_sums(got: list, want: list, np_dirs: int, st, label) -> None:
    for k, pname in enumerate(PARAM_NAMES):
        for n, g in got[k].items():
            if k >= np_dirs:
                assert np.all(np.isnan(g)), (label, pname, n, "the rpecons block was written without the evaporation branch")
                continue
            for ibl, icend in blocks_of(st):
                assert not np.any(np.isnan(g[ibl, :icend])), (label, pname, n, "an active sum was not written")
                assert same_bits(g[ibl, :icend], want[k][n][ibl, :icend]), (label, pname, n, "differs from the fold over hostcheck_tl_parjac's planes")
                assert np.all(np.isnan(g[ibl, icend:])), (label, pname, n, "the padded tail was touched")
                if n not in PAR_SUMS:
                    assert np.all(g[ibl, :icend] == 0.0), (label, pname, n, "must be exactly zero")


def observations(st, names, seed: int):
    """seeded residuals and positive weights per column, (nblocks, nproma), NaN in the padded tail"""
    rng = np.random.default_rng(seed)
    r, w = {}, {}
    for n in names:
        r[n] = rng.standard_normal((st.nblocks, st.nproma)).astype(B.REAL)
        w[n] = rng.uniform(0.5, 2.0, (st.nblocks, st.nproma)).astype(B.REAL)
        for a in (r[n], w[n]):
            for ibl, icend in blocks_of(st):
                a[ibl, icend:] = np.nan
    return r, w


def run_normal(prm, st, qsat, weights: dict, r: dict, w) -> np.ndarray:
    """the host sweep's workspace (CLOUDSC2_NNORMAL, padded columns), NaN-prefilled; w None: the weight block itself is NULL"""
    i, _ = host_traj_blocks(st, qsat)
    table = table_of(weights, st.nlev)
    work = np.full((B.NNORMAL, st.nblocks * st.nproma), np.nan)
    before = {id(a): a.copy() for a in list(r.values()) + list((w or {}).values())}
    assert host_lib("parcolsum").hostcheck_parnormal_colsum(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(i), table.ctypes.data,
                                                            C.byref(flat_block("out", r)),
                                                            C.byref(flat_block("out", w)) if w is not None else None, work.ctypes.data) == 0
    for a in list(r.values()) + list((w or {}).values()):
        assert same_bits(a, before[id(a)]), "the sweep changed a residual or a weight"
    return work


def yardstick(want_sums: list, np_dirs: int, r: dict, w: dict) -> dict:
    def cols(a):
        return a.reshape(-1)[:NGPTOT].astype(np.float64)

    return contract_sums([{n: cols(a) for n, a in want_sums[k].items()} for k in range(np_dirs)], {n: cols(a) for n, a in r.items()},
                         {n: cols(a) for n, a in w.items()})


def check_normal(work: np.ndarray, want: dict, evap: bool, label) -> float:
    worst = 0.0
    for row in range(B.NNORMAL):
        assert np.all(np.isnan(work[row, NGPTOT:])), (label, row, "a padded tail column wrote its sums")
        if row in RPECONS_ROWS and not evap:
            assert row not in want and np.all(np.isnan(work[row])), (label, row, "an rpecons row was written without the evaporation branch")
            continue
        got, (w, S) = work[row, :NGPTOT], want[row]
        assert np.all(np.isfinite(got)), (label, row, "an active column left no sum, or read a NaN it must not read")
        assert np.any(S > 0), (label, row, "a row the yardstick finds zero everywhere: nothing is tested there")
        err = np.abs(got - w)
        assert np.all(err <= BOUND * S), (label, row, float(np.max(err / np.maximum(S, 1e-300))))
        # the entry of the normal equations itself: the columns added up (in float64, any order: the bound covers the fold's chain)
        assert abs(float(got.sum()) - float(w.sum())) <= BOUND * float(S.sum()) and float(S.sum()) > 0, (label, row, "summed over the columns")
        worst = max(worst, float(np.max(np.where(S > 0, err / np.where(S > 0, S, 1.0), 0.0))))
    return worst


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("which", [0, 1])
def test_sums_are_the_fold_of_the_parameter_jacobian_and_the_normal_form_its_contraction(precise, which, flags):
    name, tab = the_tables()[which]
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, NPROMA, NGPTOT)
    evap = bool(prm.levapls2 or prm.ldrain1d)
    np_dirs = 4 if evap else 3
    worst = 0.0
    for qname, qsat in (("qsat", host_qsat(st)), ("qsat NULL", None)):
        sens = run_parjac(prm, st, qsat)  # the parent's planes (qsat None: its own form with SATUR in the sweep)
        before = st.copy()
        for wname, weights in patterns():
            label = (name, flags, "precise" if precise else "fast", qname, wname)
            want = folded(sens, np_dirs, weights)
            check_sums(run_sums(prm, st, qsat, weights), want, np_dirs, st, label)

            # ---- the normal form: every name observed and weighted, then a subset with the weight block NULL, then one weight of two
            r, w = observations(st, tuple(weights), seed=31 + which)
            worst = max(worst, check_normal(run_normal(prm, st, qsat, weights, r, w), yardstick(want, np_dirs, r, w), evap, label + ("weighted",)))
            first = tuple(weights)[:2]
            sub = {n: r[n] for n in first if n in PAR_SUMS} or {n: r[n] for n in PAR_SUMS if n in r}
            worst = max(worst, check_normal(run_normal(prm, st, qsat, weights, sub, None), yardstick(want, np_dirs, sub, {}), evap, label + ("subset",)))
            one = {n: w[n] for n in list(sub)[:1]}
            worst = max(worst, check_normal(run_normal(prm, st, qsat, weights, sub, one), yardstick(want, np_dirs, sub, one), evap, label + ("one weight",)))
        for a, b in ((st.PAP, before.PAP), (st.PT, before.PT), (st.PQ, before.PQ), (st.PCLV, before.PCLV), (st.B_LOC, before.B_LOC)):
            assert same_bits(a, b), (name, flags, "the sweep changed the state")
    print(f"{(name, flags, 'precise' if precise else 'fast')}: worst |got - want| / S {worst:.3e}")


def test_clc_and_covptot_alone_give_exact_zeros_and_read_neither_row_nor_residual(precise):
    tab = c2.random_table(137, 100, seed=5)
    prm = make_params(tab, levapls2=True)
    st = c2.state_from_table(tab, NPROMA, NGPTOT)
    nan_rows = {n: np.full(NLEV, np.nan, dtype=B.REAL) for n in ("clc", "covptot")}
    sums = run_sums(prm, st, host_qsat(st), nan_rows)
    for k in range(len(PARAM_NAMES)):
        for n, g in sums[k].items():
            for ibl, icend in blocks_of(st):
                assert np.all(g[ibl, :icend] == 0.0) and np.all(np.isnan(g[ibl, icend:])), (k, n)
    nan = {n: np.full((st.nblocks, st.nproma), np.nan, dtype=B.REAL) for n in ("clc", "covptot")}
    work = run_normal(prm, st, host_qsat(st), nan_rows, nan, nan)
    assert np.all(work[:, :NGPTOT] == 0.0) and np.all(np.isnan(work[:, NGPTOT:]))
