"""Branch atlas, CPU part: the census of level_forward's branch outcomes (tests/hostcheck/hostcheck_census.hip), the atmosphere that
reaches every outcome (tests/branch_atlas.atlas_table), the per-class error metric, and the host build of the NL, TL, AD and VJP
sweeps held to the per-class bounds against the reference.  tests/test_gpu_branch_atlas.py holds the kernels to the same bounds.

Why: the older atmospheres (synthetic_table, random_table) never take some branches of the level physics in a cell whose outputs
the branch changes, and tests/util.relerr divides by the maximum of a whole field, so a statement that is wrong on a rare branch
passes.  Here a class is the set of cells with one outcome of one predicate, and the error inside a class is measured against the
class's own magnitude and bounded by the reference's own conditioning inside that class (see branch_atlas.Case).

In an fp32 process (CLOUDSC2_PRECISION=single; tests/test_single.py starts one) the same tests hold the fp32 host build to
ERR_FACTOR x the error of the reference's own -DSINGLE build inside every class, the fp64 reference on the same fp32 values being
the truth (branch_atlas.Case._init_single).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import branch_atlas as A
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.util import B, c2, host_traj_blocks, hostcheck, make_params, relerr

BITS_VIEW = np.int32 if B.SINGLE else np.int64  # the integer of an element's size: bits are compared through it

# Outcomes the atlas cannot reach: name -> the reason, argued from level_forward.  None is left: `esdp_clip&cloud=1`, the one
# candidate, needs condensate where e_s(T)/p > 0.5, i.e. in thin hot air above the tropopause, where the critical relative
# humidity is 1 and the cover scheme gives ZQC1 = (1 - ZSCALM)(ZQSAT - ZQCRIT) = 0 in every regime -- but convective detrainment
# (llo1: ZQC2 = ZQC1 + ZLUDE) does not ask about humidity, and group A' of the atlas detrains there.
UNREACHED: dict = {}

SHAPES = [(137, 96), (60, 96)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the census walks the column the NL sweep computes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nproma, ngptot", [(32, 90), (1, 5)])
@pytest.mark.parametrize("levapls2", [False, True])
@pytest.mark.parametrize("satur", [False, True])
def test_census_walk_is_the_nl_sweep(precise, nproma, ngptot, levapls2, satur):
    tab = A.atlas_table(137, 96, A.SEED)
    prm = make_params(tab, levapls2=levapls2)
    st = c2.state_from_table(tab, nproma, ngptot, poison_outputs=-5.0)
    qsat = None if satur else A.to_blocks(A._host_qsat(tab)[:, :ngptot].astype(B.REAL), nproma)
    sig, walked, differ = A.census(prm, st, qsat, precise)
    got = st.copy()
    i, o = host_traj_blocks(got, qsat)
    assert hostcheck().hostcheck_nl(C.byref(prm), st.ptsphy, nproma, st.nlev, ngptot, C.byref(i), C.byref(o), B.Field(), 0.0) == 0
    for n in ("B_LOC", "PA", "PFPLSL", "PFPLSN", "PFHPSL", "PFHPSN"):
        a, b = getattr(walked, n), getattr(got, n)
        assert np.array_equal(a.view(BITS_VIEW), b.view(BITS_VIEW)), n
    # (PCOVPTOT: the sweep also zeroes the padded tail, the walk leaves it alone)
    assert np.array_equal(A.active_cols(walked.PCOVPTOT, ngptot).view(BITS_VIEW), A.active_cols(got.PCOVPTOT, ngptot).view(BITS_VIEW))
    act = A.active_cols(sig, ngptot)
    assert np.all(act & A.SIG_ACTIVE) and np.count_nonzero(sig & A.SIG_ACTIVE) == st.nlev * ngptot
    assert differ == 0, "dpr_clip and reset are one predicate (hostcheck_census.hip)"
    if not levapls2:
        assert not np.any(act & np.uint32((1 << A.BITS["llo2"]) | (1 << A.BITS["dpr_clip"])))


# ---------------------------------------------------------------------------------------------------------------------
# 2. the atlas reaches every outcome, often enough and in more than one place
# ---------------------------------------------------------------------------------------------------------------------
def _table_census(tab, flags, precise, nproma=32):
    ncol = tab["PT"].shape[1]
    st = c2.state_from_table(tab, nproma, ncol)
    sig, _, differ = A.census(make_params(tab, **flags), st, None, precise)
    assert differ == 0
    return sig


def _print_census(title, counts):
    print(f"\ncensus of {title}")
    names = sorted({n.split("=")[0] + ("|" + n.split("|")[1] if "|" in n else "") for n in counts})
    for base in names:
        b, _, dom = base.partition("|")
        tag = "|" + dom if dom else ""
        vals = [counts.get(f"{b}={v}{tag}") for v in (0, 1, 2)]
        print(f"  {base:24s}" + "".join(f" {v:8d}" for v in vals if v is not None))


@pytest.mark.parametrize("nlev, ncol", SHAPES)
@pytest.mark.parametrize("levapls2", [False, True])
def test_atlas_reaches_every_outcome(precise, nlev, ncol, levapls2):
    flags = dict(levapls2=levapls2)
    sig = _table_census(A.atlas_table(nlev, ncol, A.SEED), flags, precise)  # (blocks, levels, lanes)
    masks = A.outcome_masks(sig, levapls2)
    _print_census(f"atlas_table({nlev}, {ncol}) {flags} {'precise' if precise else 'fast'}", {n: int(m.sum()) for n, m in masks.items()})
    for name, m in masks.items():
        blocks, levels, lanes = np.nonzero(m)
        if name in UNREACHED:
            assert m.sum() == 0, (name, "is reached after all: take it out of UNREACHED")
            continue
        assert m.sum() >= A.MIN_CELLS, (name, int(m.sum()))
        assert name in A.ONE_LEVEL or len(set(levels)) >= 2, (name, "one level only")
        assert len(set(blocks)) >= 2 and len(set(lanes)) >= 2, (name, "one block or one lane only")
    assert set(UNREACHED) <= set(masks)


def test_census_of_the_older_atmospheres():
    """What the suite visited before the atlas (the table in DESIGN.md, "Tests per component"): printed, and the gaps the atlas
    closes asserted so that the table stays true."""
    for flags in (dict(), dict(levapls2=True)):
        evap = bool(flags)
        syn = A.census_counts(_table_census(c2.synthetic_table(), flags, 0), evap)
        _print_census(f"synthetic_table() {flags}", syn)
        rnd = {}
        for seed in (1, 2, 3):
            for n, v in A.census_counts(_table_census(c2.random_table(137, 100, seed=seed), flags, 0), evap).items():
                rnd[n] = rnd.get(n, 0) + v
        _print_census(f"random_table(137, 100, seed=1..3) {flags}", rnd)
        for n in ("esdp_clip=1", "a_clip0=1", "a_clip1=1"):
            assert syn[n] == 0, n
        for n in ("a_clip1=1", "a_clip0&dq_pos=1", "a_clip1&dq_pos=1", "esdp_clip&cloud=1"):
            assert rnd[n] == 0, n
        assert rnd["esdp_clip=1"] < A.MIN_CELLS


# ---------------------------------------------------------------------------------------------------------------------
# 3. the metric
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlev", [137, 60])
@pytest.mark.parametrize("flagset", list(A.FLAG_SETS))
def test_threshold_cells_are_few(nlev, flagset):
    """Cells whose signature depends on the arithmetic mode, on the source of QSAT or on one ulp of the inputs are taken out of the
    class comparison (they stay under the whole-field bound): at most 5 % of any class, and 32 cells are left in every class."""
    c = A.case(nlev, flagset)
    assert c.dpr_clip_ne_reset == 0
    share, smallest = (0.0, ""), (c.sig.size, "")
    for name, full in c.full_classes.items():
        kept = c.classes[name]
        share = max(share, ((full.sum() - kept.sum()) / full.sum(), name))
        smallest = min(smallest, (int(kept.sum()), name))
        assert kept.sum() >= A.MIN_CELLS, (name, int(kept.sum()))
        assert full.sum() - kept.sum() <= A.MAX_EXCLUDED * full.sum(), (name, int(full.sum()), int(kept.sum()))
    if B.SINGLE:  # (fp32: also the cells on whose branch the fp32 and the fp64 host census of the same values differ)
        print(f"\n{nlev} levels, {flagset}: {int(c.excluded.sum())} threshold cells of {c.sig.size}; largest excluded share "
              f"{100.0 * share[0]:.1f} % ({share[1]}); smallest kept class {smallest[0]} ({smallest[1]}); DRAWS = {A.DRAWS}")
        for kind in ("nl", "tl", "ad"):
            print("  E / max|ref|", kind, " ".join(f"{f}={c.sets[False]['E'][kind, f].max() / max(np.abs(r).max(), 1e-300):.1e}" for f, r in c.ref[kind].items()))
        return
    print(f"\n{nlev} levels, {flagset}: {int(c.excluded.sum())} threshold cells of {c.sig.size}; K_NL = {c.K_NL:.2f}, K_TLAD = {c.K_TLAD:.2f}")
    for kind in ("nl", "tl", "ad"):
        print("  floor", kind, " ".join(f"{f}={c.floor_field[kind, f]:.1e}" for f in c.ref[kind]))


@pytest.mark.parametrize("nlev", [137, 60])
def test_class_metric_sees_what_the_field_norm_does_not(nlev):
    """An error of 1e-9 relative, confined to the cells of a class whose values lie three orders below the field's maximum,
    passes relerr <= NL_TOL over the field and must fail the class bound."""
    if B.SINGLE:
        return _class_metric_single(nlev)
    c = A.case(nlev, "plain").columns(np.arange(A.NGPTOT)[np.arange(A.NGPTOT) % 8 == 7])  # group D: the unchanged random_table
    ref = c.ref["nl"]
    tried = 0
    for f in ("tent", "tenq", "tenl", "teni", "fplsl", "fplsn"):
        r = ref[f]
        rows = r[1:] if r.shape[0] == nlev + 1 else r
        for cn, mask in c.classes.items():
            if not mask.any() or not (0.0 < float(np.abs(rows[mask]).max()) < 1e-3 * c.scale["nl", f]):
                continue
            got = {n: a.copy() for n, a in ref.items()}
            g = got[f][1:] if r.shape[0] == nlev + 1 else got[f]
            g[mask] *= 1.0 + 1e-9
            assert relerr(r, got[f]) <= A.NL_TOL, (f, cn)
            bad, _, _ = c.compare("nl", got)
            assert any(b[1] == f and b[2] == cn for b in bad), (f, cn, "the class metric did not see it")
            assert A.class_err(rows, g, mask) > 1e-10
            tried += 1
    assert tried >= 3, "no rare class to try the metric on"
    bad, worst, _ = c.compare("nl", ref)
    assert not bad and worst == 0.0


def _class_metric_single(nlev):
    """fp32: a relative error inside a rare class that is 8 x the class bound at the class's largest value and still inside the
    whole-field bound (so the class's E is at most 1/8 of the field's): both sizes come from E, the yardstick measured on the two
    references."""
    c = A.case(nlev, "plain")
    ref = c.ref["nl"]
    tried = 0
    for f in ("tent", "tenq", "tenl", "teni", "fplsl", "fplsn"):
        r, e = ref[f], c.sets[False]["E"]["nl", f]
        half = r.shape[0] == nlev + 1
        rows = r[1:] if half else r
        field_bound = A.ERR_FACTOR * float(e.max())
        for cn, mask in c.classes.items():
            if not mask.any():
                continue
            class_bound = A.ERR_FACTOR * float(c.class_rows(f, e, mask).max())
            top = float(np.abs(rows[mask]).max())
            if not (0.0 < 8.0 * class_bound <= field_bound) or top == 0.0:
                continue
            rel = 8.0 * class_bound / top
            got = {n: a.copy() for n, a in ref.items()}
            g = got[f][1:] if half else got[f]
            g[mask] *= 1.0 + rel
            assert float(np.abs(got[f] - r).max()) <= field_bound, (f, cn)
            bad, _, _ = c.compare("nl", got)
            assert not any(b[1] == f and b[2] == "field" for b in bad), (f, cn, "the planted error does not pass the whole-field bound")
            assert any(b[1] == f and b[2] == cn for b in bad), (f, cn, "the class metric did not see it")
            tried += 1
    print(f"\n{nlev} levels: the class metric caught {tried} planted errors that pass the whole-field bound")
    assert tried >= 3, "no rare class to try the metric on"
    bad, worst, _ = c.compare("nl", ref)
    assert not bad and worst == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. the host build against the reference, per class
# ---------------------------------------------------------------------------------------------------------------------
def host_vjp(c, satur: bool) -> dict:
    """cloudsc2_vjp_launch's sweep on the host: the trajectory pass, then the reverse sweep in the vector-Jacobian form."""
    hv = host_lib("vjp")
    got = c.st.copy()
    i, o = host_traj_blocks(got, None if satur else c.qsat)
    scratch = np.zeros((c.st.nblocks, c.nlev, A.NPROMA), dtype=B.REAL)
    assert hv.hostcheck_vjp_sweep(C.byref(c.prm), c.ptsphy, A.NPROMA, c.nlev, A.NGPTOT, C.byref(i), C.byref(o), None, None,
                                  scratch.ctypes.data, 1, 0) == 0
    x = A.blocks_of({n: np.full(a.shape, np.nan, dtype=B.REAL) for n, a in c.ref["ad"].items()}, fill=np.nan)
    y = A.blocks_of(c.refset(satur)["y"])
    assert hv.hostcheck_vjp_sweep(C.byref(c.prm), c.ptsphy, A.NPROMA, c.nlev, A.NGPTOT, C.byref(i), C.byref(o),
                                  C.byref(A._flat("in", x)), C.byref(A._flat("out", y)), scratch.ctypes.data, 2, 1) == 0
    return A.cols_of(x)


def vjp_as_adjoint(c, x: dict) -> dict:
    """The VJP's PSUPSAT entry is the true derivative; CLOUDSC2AD's carries a factor PTSPHY (cloudsc2ad.F90:1733)."""
    out = dict(x)
    out["supsat"] = x["supsat"] * c.ptsphy
    return out


def background(c) -> dict:
    """A non-zero background for the accumulating adjoint, of the size of the result cell by cell."""
    rng = np.random.default_rng(5)
    return {n: (a * rng.uniform(-1.0, 1.0, size=a.shape)).astype(B.REAL) for n, a in c.ref["ad"].items()}


WORST = {}


@pytest.mark.parametrize("nlev", [137, 60])
@pytest.mark.parametrize("flagset", list(A.FLAG_SETS))
@pytest.mark.parametrize("satur", [False, True], ids=["qsat-fed", "satur-in-sweep"])
def test_host_build_within_the_class_bounds(precise, nlev, flagset, satur):
    c = A.case(nlev, flagset)
    results = {}
    # (satur: in fp32 the references that ran their own SATUR; fp64 has one set and ignores it)
    results["nl"] = c.compare("nl", A.host_nl(c, satur), satur=satur)
    traj, tl = A.host_tl(c, satur)
    results["traj"] = c.compare("traj", traj, satur=satur)
    results["tl"] = c.compare("tl", tl, satur=satur)
    x0 = background(c)
    results["ad accumulate"] = c.compare("ad", A.host_ad(c, satur, x0, assign=False), A.reference_ad(c, x0, satur), satur=satur)
    results["ad assign"] = c.compare("ad", A.host_ad(c, satur, {n: np.full_like(a, 7.25) for n, a in x0.items()}, assign=True), satur=satur)
    results["vjp"] = c.compare("ad", vjp_as_adjoint(c, host_vjp(c, satur)), satur=satur)
    failures = []
    for what, (bad, worst, where) in results.items():
        print(f"{what:14s} worst err/bound {worst:.3f} at {where}")
        WORST[nlev, flagset, satur, precise, what] = worst
        failures += [(what,) + b for b in bad]
    assert not failures, failures[:8]
