"""The parameter Jacobian's sweep (tl_parjac_column: what cloudsc2_tl_launch_parjac runs), compiled for the HOST: NPROMA 32 x 100 columns
(four blocks, a ragged tail), both arithmetics, the synthetic table and random_table(137, 100, seed=5).

Every direction must be the bits of the single-direction parameter TL (hostcheck_tl_par, satur = 0) run on all-zero increments with
dpar = e_k: the host builds are compiled without contraction, so this holds exactly or the sweep is not the same arithmetic.  The form
with SATUR evaluated in the sweep (qsat NULL) must be the bits of the form fed the host SATUR's plane.  Against the reference: central
differences of its NL kernel, through check_against_reference_differences of tests/host_sweeps.py -- tests/test_hostcheck_par.py's bound 1e-5 of a field's
maximum at relative step 1e-6, a column left out when the steps 1e-5 and 1e-6 disagree by more than that, at most 2 of 100 columns;
numbers established there from the reference alone.  Measured here, worst over the 8 cases: 1.658e-06 (synthetic, no evaporation,
rkconv), no column left out but one (seed5, levapls2, rpecons) -- the figures of the single-direction sweep, whose bits these are."""
from __future__ import annotations

import numpy as np
import pytest

from tests.host_sweeps import NGPTOT, NPROMA, check_against_reference_differences, exact_zero_fields, run_parjac, run_tl_par
from tests.hostbuild import precise  # noqa: F401
from tests.util import (FLAG_SETS, PARAM_NAMES, B, bits, blocks_of, c2, columns, fp64_only, host_qsat, increments_of, make_params,
                        refcall, set_lib_params, the_tables)


@pytest.fixture(scope="module")
def ref():
    """the reference itself where it is built, else its C restatement"""
    return refcall.RefLib() if refcall.have_ref() else refcall.OracleLib()


def unit(k: int) -> list:
    e = [0.0] * len(PARAM_NAMES)
    e[k] = 1.0
    return e


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("which", [0, 1])
def test_every_direction_is_the_bits_of_the_single_direction_sweep_on_zero_increments(precise, which, flags):
    name, tab = the_tables()[which]
    prm = make_params(tab, **flags)
    st = c2.state_from_table(tab, NPROMA, NGPTOT)
    evap = bool(prm.levapls2 or prm.ldrain1d)
    qsat = host_qsat(st)
    zero = {n: np.zeros_like(a) for n, a in increments_of(st, qsat).items()}
    sens = run_parjac(prm, st, qsat)
    fused = run_parjac(prm, st, None)
    for k, pname in enumerate(PARAM_NAMES):
        if pname == "rpecons" and not evap:  # not run: the block is untouched
            for n in B.OUT_NAMES:
                assert np.all(np.isnan(sens[k][n])) and np.all(np.isnan(fused[k][n])), (name, flags, n, "the rpecons block was written")
            continue
        single = run_tl_par(prm, st, zero, unit(k), qsat)  # (NaN-prefilled as well)
        for n in B.OUT_NAMES:
            assert np.array_equal(bits(sens[k][n]), bits(single[n])), (name, flags, pname, n, "not the bits of hostcheck_tl_par")
            assert np.array_equal(bits(fused[k][n]), bits(sens[k][n])), (name, flags, pname, n, "SATUR in the sweep: other bits")
            for ibl, icend in blocks_of(st):
                assert not np.any(np.isnan(sens[k][n][ibl][:, :icend])), (pname, n, "active element not written")
                assert np.all(np.isnan(sens[k][n][ibl][:, icend:])), (pname, n, "the padded tail was touched")
                if n in exact_zero_fields(pname, evap):
                    assert np.all(sens[k][n][ibl][:, :icend] == 0.0), (name, flags, pname, n, "must be exactly zero")
        moved = [n for n in B.OUT_NAMES if np.any(np.nan_to_num(sens[k][n]) != 0.0)]
        assert moved, (name, flags, pname, "a sensitivity that is zero everywhere")


@fp64_only
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True)])
@pytest.mark.parametrize("which", [0, 1])
def test_against_central_differences_of_the_reference(precise, ref, which, flags):
    """Measured (worst over the 8 cases, fast and precise): 1.658e-06 of a field's maximum (synthetic, no evaporation, rkconv)."""
    name, tab = the_tables()[which]
    prm = make_params(tab, lregcl=False, **flags)
    set_lib_params(ref, prm)
    st = c2.state_from_table(tab, NPROMA, NGPTOT)
    one = c2.state_from_table(tab, NGPTOT, NGPTOT)  # the same columns as one block, for the reference
    qs = ref.satur(np.ascontiguousarray(one.PAP[0]), np.ascontiguousarray(one.PT[0]))
    qsat = np.zeros_like(st.PAP)
    for ibl, icend in blocks_of(st):
        qsat[ibl][:, :icend] = qs[:, ibl * NPROMA:ibl * NPROMA + icend]
    sens = run_parjac(prm, st, qsat)
    evap = bool(prm.levapls2)

    def tl_of(k):
        if PARAM_NAMES[k] == "rpecons" and not evap:  # not run and not written: the sensitivity is the exact zero
            return {n: np.zeros((st.nlev + (1 if n in refcall.HALF else 0), NGPTOT), dtype=B.REAL) for n in B.OUT_NAMES}
        return {n: columns(a, NGPTOT) for n, a in sens[k].items()}

    worst = check_against_reference_differences(ref, prm, one, qs, tl_of, f"{name} {flags}")
    print(f"{name} {flags}: worst {worst:.3e}")
