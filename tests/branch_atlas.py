"""Branch atlas (test helpers): the census of level_forward's branch outcomes, an atmosphere that reaches every one of them, and
the per-class error metric with bounds measured on the reference alone.

* ``census``       one signature word per cell from tests/hostcheck/hostcheck_census.hip (the predicates LevelTraj records);
* ``atlas_table``  random_table plus directed column groups;
* ``Classes``      class = the active cells that share one outcome of one signature bit; threshold cells taken out;
* ``Bounds``       floor(f, c): the reference's own response to a one-ulp perturbation of every input, per field and class;
                   K = the accepted whole-field tolerance over the largest whole-field floor; bound(f, c) = K floor(f, c), never
                   looser than the whole-field bound.  In an fp32 process (B.SINGLE): E(f, c) = the larger of the error of the
                   reference's -DSINGLE build against the fp64 reference on the same values and its response to one fp32 ulp of
                   every input; bound(f, c) = ERR_FACTOR E(f, c) on |ours - fp64 reference| (Case._init_single).

Nothing here is imported by the package.
"""
from __future__ import annotations

import copy
import ctypes as C
import dataclasses
import functools

import numpy as np

from tests.hostbuild import host_lib
from tests.util import B, c2, hfld, host_traj_blocks, hostcheck, increments_of, make_params, refcall, set_lib_params

NL_TOL = 1e-12    # the whole-field bounds the project accepts (tests/test_gpu_parity.py)
TLAD_TOL = 1e-11
MIN_CELLS = 32    # every class, before and after the exclusion of threshold cells
MAX_EXCLUDED = 0.05

if B.SINGLE:
    from tests.single_checks import ERR_FACTOR  # the project's "as accurate as the reference's -DSINGLE" factor (4)

# name -> bit of the signature word (hostcheck_census.hip); "regime" is the two-bit field at 4
BITS = {"cold": 0, "esdp_clip": 1, "qlim_is_qs": 2, "below_rtice": 3, "llo1": 6, "llo3": 7, "newmax": 8, "melt": 9, "warm2": 10,
        "melt_all": 11, "cloudy": 12, "frz1": 13, "llo2": 14, "dpr_clip": 15, "warm_adj": 16, "a_clip0": 17, "a_clip1": 18,
        "dq_pos": 19, "frz2": 20, "last": 21, "partial_melt": 22, "regcl_capped": 23, "a_clip0&dq_pos": 24, "a_clip1&dq_pos": 25,
        "esdp_clip&cloud": 26, "llo2&dpr_clip": 27}
SIG_ACTIVE = np.uint32(1 << 31)
# a bit that is only defined where another holds: its two outcomes are classes inside that domain (level_forward sets warm2 and
# melt_all under `melt`, dpr_clip under `llo2`; regcl_factor is evaluated in the partial-cover regime only)
DOMAIN = {"warm2": "melt", "melt_all": "melt", "partial_melt": "melt", "dpr_clip": "llo2", "regcl_capped": "regime=2"}
# bits that do not exist without the evaporation branch: with EVAP = false t.llo2 is a compile-time false (level_forward stage J)
EVAP_ONLY = ("llo2", "dpr_clip", "llo2&dpr_clip")
# `last` is true on the bottom level only: it cannot be spread over two levels
ONE_LEVEL = ("last=1",)


def census(prm, st, qsat: np.ndarray | None = None, precise: int = 0, single: bool = B.SINGLE):
    """Signature words (NBLOCKS, NLEV, NPROMA) of a state (0 in the padded tail), the state the walk left (its outputs are the
    walk's LevelOut) and the number of cells where dpr_clip and reset differ.  `single`: the precision of the census build; the
    state and qsat hold elements of that precision."""
    lib = host_lib("census", single)  # (its field blocks then hold elements of that precision)
    got = st.copy()
    i, o = host_traj_blocks(got, qsat, real=np.float32 if single else np.float64)
    sig = np.zeros((st.nblocks, st.nlev, st.nproma), dtype=np.uint32)
    lib.hostcheck_set_precise(int(precise))
    try:
        differ = lib.hostcheck_census(C.byref(prm), st.ptsphy, st.nproma, st.nlev, st.ngptot, C.byref(i), C.byref(o), sig.ctypes.data)
    finally:
        lib.hostcheck_set_precise(0)
    assert differ >= 0
    return sig, got, int(differ)


# ---------------------------------------------------------------------------------------------------------------------
# the atmosphere
# ---------------------------------------------------------------------------------------------------------------------
def atlas_table(nlev: int, ncol: int, seed: int) -> dict:
    """random_table plus directed groups of columns, interleaved (column j belongs to group j mod 8) so that every group has
    columns in every NPROMA block:

    0 A   hot, thin air aloft (PAP < 2000 Pa, +20..120 K), half of those cells moist with a little cloud water: the saturation
          pressure over p passes the 0.5 cap in stage A (esdp_clip) and in the saturation adjustment (a_clip), with condensation;
    1 A'  as A, warmer still and always moist;
    2 B   +5..20 K at all levels: a deep melting layer (warm2, melt_all), and F on top of it;
    3 B'  first-guess temperature a fraction of a kelvin above RTT + 2 through the layer where it lies between RTT and 292 K: the
          snow from above melts a little on each of those levels (partial melt);
    4 C   PQ x 1.0..1.6: overcast and supersaturated cells;
    5 E   total water set just below saturation in the troposphere: partial cover with regcl_factor under its cap;
    6 F   below the 262 K level the first-guess temperature alternates between 271..272.5 K and 279..289 K from level to level: the
          cold levels make snow, the warm ones melt all of it (melt_all, far more often than the residues that a complete
          evaporation leaves in the snow flux, which are threshold cells);
    7 D   the unchanged random_table.
    """
    tab = c2.random_table(nlev, ncol, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    grp = np.arange(ncol) % 8
    u = lambda a, b, shape=(nlev, ncol): rng.uniform(a, b, size=shape)  # noqa: E731
    pap = tab["PAP"]
    col = lambda g: np.broadcast_to(grp == g, (nlev, ncol))  # noqa: E731

    top = pap < 2000.0
    hot = top & (col(0) | col(1))
    tab["PT"] = np.where(hot, tab["PT"] + np.where(col(1), u(60.0, 140.0), u(20.0, 120.0)), tab["PT"])
    wet = hot & (col(1) | (u(0.0, 1.0) < 0.5))
    tab["PQ"] = np.where(wet, u(0.3, 0.95), tab["PQ"])
    tab["PCLV_QL"] = np.where(wet, u(0.0, 1e-4), tab["PCLV_QL"])
    # A': convective detrainment into those cells, the one source of condensate where the critical relative humidity is 1
    tab["PLUDE"] = np.where(wet & col(1), u(0.0, 2.0e-6), tab["PLUDE"])
    tab["PLU"] = np.where(col(1) & (pap < 2500.0), u(1.0e-5, 1.0e-3), tab["PLU"])

    tab["PT"] = tab["PT"] + np.where(col(2), u(5.0, 20.0, (1, ncol)), 0.0)
    ptsphy = float(tab["PTSPHY"])
    ztp2 = tab["PT"] + ptsphy * tab["TENDENCY_CML_T"]  # the first guess of level_forward
    thaw = col(3) & (ztp2 > 273.16) & (ztp2 < 292.0)
    # (fp32: one ulp at 275 K is 3e-5 K, and an excess below 1e-3 K makes partial melt a threshold outcome in a tenth of its cells;
    # the same number of draws, so the random stream of everything after it is the fp64 recipe's)
    lo = -3.0 if B.SINGLE else -4.5
    tab["PT"] = np.where(thaw, 275.16 + 10.0 ** u(lo, -1.5) - ptsphy * tab["TENDENCY_CML_T"], tab["PT"])

    # B and F: freezing and warm levels in turn below the 262 K level: the cold ones make snow, the warm ones melt all of it
    ztp2 = tab["PT"] + ptsphy * tab["TENDENCY_CML_T"]
    low = (col(2) | col(6)) & (ztp2 > 262.0)
    odd = np.broadcast_to((np.arange(nlev) % 2 == 1)[:, None], (nlev, ncol))
    tab["PT"] = np.where(low, np.where(odd, 279.0 + u(0.0, 10.0), 271.0 + u(0.0, 1.5)) - ptsphy * tab["TENDENCY_CML_T"], tab["PT"])

    tab["PQ"] = np.where(col(4), tab["PQ"] * u(1.0, 1.6), tab["PQ"])

    # E: first-guess total water (ZQP2 + ZL + ZI of level_forward) a little below ZQSAT = qsat(PAP, PT) * ZSUPSAT
    ztp2 = tab["PT"] + ptsphy * tab["TENDENCY_CML_T"]
    zqsat = _host_qsat(tab) * np.where(ztp2 < 250.16, 1.8 - 3.0e-3 * ztp2, 1.0)  # RTICE = RTT - 23
    rest = (ptsphy * tab["TENDENCY_CML_Q"] + tab["PSUPSAT"] + tab["PCLV_QL"] + ptsphy * tab["TENDENCY_CML_QL"] + tab["PCLV_QI"] +
            ptsphy * tab["TENDENCY_CML_QI"])
    pq = zqsat * u(0.95, 0.99995) - rest
    tab["PQ"] = np.where(col(5) & (pap > 1.0e4) & (pq > 0.0), pq, tab["PQ"])
    return tab


def _host_qsat(tab: dict) -> np.ndarray:
    """SATUR of the host build on a table's (PAP, PT): an input recipe needs it, not a reference."""
    pap, t = np.ascontiguousarray(tab["PAP"], dtype=B.REAL), np.ascontiguousarray(tab["PT"], dtype=B.REAL)
    nlev, ncol = pap.shape
    qsat = np.zeros_like(pap)
    prm = c2.default_params(np.full(nlev, 0.5))
    f = lambda a: B.Field(a.ctypes.data, a.size)  # noqa: E731
    hc = host_lib("census")  # (precise for the length of this call, whatever mode the tests have set: an input recipe has one arithmetic)
    hc.hostcheck_set_precise(1)
    try:
        assert hc.hostcheck_satur(C.byref(prm), ncol, nlev, ncol, f(pap), f(t), f(qsat)) == 0
    finally:
        hc.hostcheck_set_precise(0)
    return qsat.astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# layout: the reference works on (NLEVx, columns) matrices, the sweeps on (NBLOCKS, NLEVx, NPROMA) blocks
# ---------------------------------------------------------------------------------------------------------------------
def active_cols(a: np.ndarray, ngptot: int) -> np.ndarray:
    """(NBLOCKS, NLEVx, NPROMA) -> (NLEVx, ngptot): the active columns in global order (blocks are contiguous)."""
    nb, nlevx, nproma = a.shape
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(nlevx, nb * nproma)[:, :ngptot]


def to_blocks(m: np.ndarray, nproma: int, fill: float = 0.0) -> np.ndarray:
    """(NLEVx, ngptot) -> (NBLOCKS, NLEVx, NPROMA), the padded tail filled with `fill`."""
    nlevx, ngptot = m.shape
    nb = (ngptot + nproma - 1) // nproma
    out = np.full((nlevx, nb * nproma), fill, dtype=m.dtype)
    out[:, :ngptot] = m
    return np.ascontiguousarray(out.reshape(nlevx, nb, nproma).transpose(1, 0, 2))


TABLE_FIELDS = ("PT", "PQ", "PAP", "PAPH", "PLU", "PLUDE", "PMFU", "PMFD", "PCLV_QL", "PCLV_QI", "TENDENCY_CML_T", "TENDENCY_CML_Q",
                "TENDENCY_CML_QL", "TENDENCY_CML_QI", "PSUPSAT")


ULP = 2.0 ** -23 if B.SINGLE else 2.0 ** -52


def one_ulp(a: np.ndarray, rng) -> np.ndarray:
    """Every element times 1 + ULP or 1 - ULP (2^-52; 2^-23 in an fp32 process, rounded to fp32), the sign drawn from rng."""
    return (a * (1.0 + np.where(rng.integers(0, 2, size=a.shape) == 1, 1.0, -1.0) * ULP)).astype(a.dtype, copy=False)


def perturbed_table(tab: dict, seed: int = 77) -> dict:
    rng = np.random.default_rng(seed)
    out = dict(tab)
    for n in TABLE_FIELDS:
        out[n] = one_ulp(np.asarray(tab[n], dtype=B.REAL), rng).astype(np.float64)  # (fp32: one ulp of the value the state holds)
    return out


def checker():
    """The reference itself where it was built, else its plain-C restatement."""
    return refcall.RefLib() if refcall.have_ref() else refcall.OracleLib()


# ---------------------------------------------------------------------------------------------------------------------
# classes
# ---------------------------------------------------------------------------------------------------------------------
def outcome_masks(sig: np.ndarray, evap: bool) -> dict:
    """name -> boolean mask over the cells of `sig` (any shape): one entry per outcome of every signature bit.  A bit with a
    domain (DOMAIN) has its outcomes inside the domain only."""
    act = (sig & SIG_ACTIVE) != 0
    bit = lambda n: ((sig >> np.uint32(BITS[n])) & np.uint32(1)) != 0  # noqa: E731
    reg = (sig >> np.uint32(4)) & np.uint32(3)
    out = {f"regime={r}": act & (reg == r) for r in range(3)}
    for n in BITS:
        if n in EVAP_ONLY and not evap:
            continue
        dom, tag = act, ""
        if n in DOMAIN:
            d = DOMAIN[n]
            dom, tag = act & (out[d] if d.startswith("regime") else bit(d)), "|" + d
        out[f"{n}=0{tag}"] = dom & ~bit(n)
        out[f"{n}=1{tag}"] = dom & bit(n)
    return out


def census_counts(sig: np.ndarray, evap: bool) -> dict:
    return {n: int(m.sum()) for n, m in outcome_masks(sig, evap).items()}


# ---------------------------------------------------------------------------------------------------------------------
# one case: an atmosphere, a flag set, the reference's results on it, its classes and the bounds
# ---------------------------------------------------------------------------------------------------------------------
FLAG_SETS = {"plain": dict(), "lregcl": dict(lregcl=True), "levapls2": dict(levapls2=True),
             "levapls2+lregcl": dict(levapls2=True, lregcl=True)}
NPROMA, NGPTOT, NCOL, SEED = 32, 90, 96, 3
DRAWS = 6  # sign patterns of the one-ulp perturbation
F64 = np.float64
FLUX = ("fplsl", "fplsn", "fhpsl", "fhpsn")


def _inputs_of(tab: dict, ngptot: int) -> dict:
    st = c2.state_from_table(tab, ngptot, ngptot, real=B.REAL)
    return refcall.block_inputs(st, 0, None)


class Case:
    """Everything the per-class comparison of one (levels, flag set) needs; built once (see `case`)."""

    def __init__(self, nlev: int, flagset: str):
        self.nlev, self.flagset = nlev, flagset
        self.flags = FLAG_SETS[flagset]
        self.evap = bool(self.flags.get("levapls2"))
        self.tab = atlas_table(nlev, NCOL, SEED)
        self.prm = make_params(self.tab, **self.flags)
        self.st = c2.state_from_table(self.tab, NPROMA, NGPTOT)
        self.ptsphy = self.st.ptsphy
        if B.SINGLE:
            self._init_single()
            return
        self.chk = checker()
        set_lib_params(self.chk, self.prm)
        # the reference on the state ...
        self.inp = _inputs_of(self.tab, NGPTOT)
        self.inp["qsat"] = self.chk.satur(self.inp["pap"], self.inp["t"])
        self.qsat = to_blocks(self.inp["qsat"], NPROMA)  # what a sweep with QSAT fed reads
        self.dinp = {n: np.ascontiguousarray(a * 0.01) for n, a in self.inp.items()}  # the test drivers' increments
        self.ref = self._reference(self.inp, self.dinp, None)
        # ... and on the state with every input one ulp off, DRAWS sign patterns: the floor is the largest response of the
        # reference over them (one pattern alone can cancel inside a small class)
        self.tab_p, refs_p = [], []
        for k in range(DRAWS):
            rng = np.random.default_rng(78 + k)
            tab_p = perturbed_table(self.tab, seed=177 + k)
            inp_p = _inputs_of(tab_p, NGPTOT)
            inp_p["qsat"] = one_ulp(self.inp["qsat"], rng)  # QSAT is an input of CLOUDSC2 like the others
            dinp_p = {n: one_ulp(a, rng) for n, a in self.dinp.items()}
            refs_p.append(self._reference(inp_p, dinp_p, rng))
            self.tab_p.append(tab_p)
        self._refs_p = refs_p
        self._classes()
        self._bounds()

    # -- reference ----------------------------------------------------------------------------------------------------
    def _reference(self, inp, dinp, rng):
        """NL, TL (about inp, increments dinp) and AD (output adjoints = the TL outputs, one ulp off if rng) of the checker."""
        chk, nlev, ncol = self.chk, self.nlev, NGPTOT
        cp = lambda d: {n: a.copy() for n, a in d.items()}  # noqa: E731
        nl = chk.cloudsc2(self.ptsphy, cp(inp))
        traj, tl = chk.cloudsc2tl(self.ptsphy, cp(inp), cp(dinp))
        y = {n: (one_ulp(a, rng) if rng is not None else a.copy()) for n, a in tl.items()}
        x = refcall.new_inputs(nlev, ncol)
        chk.cloudsc2ad(self.ptsphy, cp(inp), x, cp(y))
        return dict(nl=nl, traj=traj, tl=tl, ad=x, y=y)

    def reference_ad(self, x0: dict, satur: bool = False) -> dict:
        """The checker's adjoint accumulated on the background x0 (PSUPSAT's is assigned, cloudsc2ad.F90:1733).  fp32: the fp64
        reference's, with the yardstick E of the adjoint taken from both references' runs on the same x0 (RefWithError)."""
        if B.SINGLE:
            return self._reference_ad_single(x0, satur)
        set_lib_params(self.chk, self.prm)
        x = {n: a.copy() for n, a in x0.items()}
        self.chk.cloudsc2ad(self.ptsphy, {n: a.copy() for n, a in self.inp.items()}, x, {n: a.copy() for n, a in self.ref["y"].items()})
        return x

    # -- fp32: two references, the fp64 one is the truth ------------------------------------------------------------------------
    def _init_single(self):
        """No golden fp32 data exists: the fp64 reference on the same fp32 values is the truth, and the yardstick is the error the
        reference's own -DSINGLE build makes against it (P) or its response to one fp32 ulp of every input (U), whichever is
        larger, over the state and DRAWS perturbed states.  Two sets: QSAT fed (the fp32 reference's SATUR, upcast for the fp64
        run) and SATUR in the sweep (each reference its own SATUR)."""
        self.chk32, self.chk64 = refcall.RefLib(single=True), refcall.RefLib()
        self.chk = self.chk64
        self._set_params()
        self.inp = _inputs_of(self.tab, NGPTOT)
        assert self.inp["pap"].dtype == np.float32
        self.inp["qsat"] = self.chk32.satur(self.inp["pap"], self.inp["t"])
        self.qsat = to_blocks(self.inp["qsat"], NPROMA)
        self.dinp = {n: np.ascontiguousarray(a * B.REAL(0.01)) for n, a in self.inp.items()}
        samples = [(self.inp, self.dinp, None)]
        self.tab_p = []
        for k in range(DRAWS):
            rng = np.random.default_rng(78 + k)
            tab_p = perturbed_table(self.tab, seed=177 + k)
            inp_p = _inputs_of(tab_p, NGPTOT)
            inp_p["qsat"] = one_ulp(self.inp["qsat"], rng)
            dinp_p = {n: one_ulp(a, rng) for n, a in self.dinp.items()}
            samples.append((inp_p, dinp_p, rng))
            self.tab_p.append(tab_p)
        self._runs, self.sets = {}, {}
        for satur in (False, True):
            runs = []
            for inp, dinp, rng in samples:
                # (the same sign patterns of the output adjoints in both sets)
                runs.append(self._pair(inp, dinp, copy.deepcopy(rng), satur))
            self._runs[satur] = runs
            ref = dict(runs[0]["r64"], y=runs[0]["y"])
            E = {(kind, f): self._error_of([r["r32"][kind][f] for r in runs], [r["r64"][kind][f] for r in runs])
                 for kind in ("nl", "traj", "tl", "ad") for f in ref[kind]}
            self.sets[satur] = dict(ref=ref, E=E)
        self.ref = self.sets[False]["ref"]
        self._classes()

    def _set_params(self):
        for chk in (self.chk32, self.chk64):
            set_lib_params(chk, self.prm)

    def _pair(self, inp, dinp, rng, satur: bool, x0: dict | None = None, y: dict | None = None) -> dict:
        """Both references on identical values (satur: except QSAT, each its own SATUR's).  The output adjoints are the fp32
        reference's TL outputs (one ulp off if rng), the same for both.  With x0 and y: the adjoint alone, accumulated on x0."""
        up = lambda d: {n: np.ascontiguousarray(a, dtype=F64) for n, a in d.items()}  # noqa: E731
        cp = lambda d: {n: a.copy() for n, a in d.items()}  # noqa: E731
        c32, c64, pt = self.chk32, self.chk64, self.ptsphy
        i32, i64 = cp(inp), up(inp)
        if satur:
            i32["qsat"], i64["qsat"] = c32.satur(i32["pap"], i32["t"]), c64.satur(i64["pap"], i64["t"])
        r32, r64 = {}, {}
        if y is None:
            r32["nl"], r64["nl"] = c32.cloudsc2(pt, cp(i32)), c64.cloudsc2(pt, cp(i64))
            (r32["traj"], r32["tl"]), (r64["traj"], r64["tl"]) = c32.cloudsc2tl(pt, cp(i32), cp(dinp)), c64.cloudsc2tl(pt, cp(i64), up(dinp))
            y = {n: (one_ulp(a, rng) if rng is not None else a.copy()) for n, a in r32["tl"].items()}
        x32 = ({n: np.ascontiguousarray(a, dtype=np.float32) for n, a in x0.items()} if x0 is not None
               else refcall.new_inputs(self.nlev, NGPTOT, dtype=np.float32))
        x64 = up(x32)
        c32.cloudsc2ad(pt, cp(i32), x32, cp(y))
        c64.cloudsc2ad(pt, cp(i64), x64, up(y))
        r32["ad"], r64["ad"] = x32, x64
        return dict(r32={k: up(d) for k, d in r32.items()}, r64=r64, y=y, inp=inp)

    @staticmethod
    def _error_of(s32: list, s64: list) -> np.ndarray:
        """E per element: the larger of P = max over the samples |ref32 - ref64| and U = max over the draws |ref32(draw) -
        ref32(state)|."""
        p = np.max([np.abs(a - b) for a, b in zip(s32, s64)], axis=0)
        u = np.max([np.abs(a - s32[0]) for a in s32[1:]], axis=0)
        return np.maximum(p, u)

    def _reference_ad_single(self, x0: dict, satur: bool) -> dict:
        self._set_params()
        runs = [self._pair(r["inp"], None, None, satur, x0=x0, y=r["y"]) for r in self._runs[bool(satur)]]
        ref = RefWithError(runs[0]["r64"]["ad"])
        ref.E = {f: self._error_of([r["r32"]["ad"][f] for r in runs], [r["r64"]["ad"][f] for r in runs]) for f in ref}
        return ref

    def refset(self, satur: bool = False) -> dict:
        """The references a sweep is compared with and takes its output adjoints (`y`) from: one set in fp64; in fp32 the set
        that matches where the sweep's QSAT comes from."""
        return self.sets[bool(satur)]["ref"] if B.SINGLE else self.ref

    def _compare_single(self, kind: str, got: dict, ref: dict | None, satur: bool):
        """|got - ref64(state)| under ERR_FACTOR x E: over all cells of a field, and over the cells of every class."""
        s = self.sets[bool(satur)]
        ref = ref if ref is not None else s["ref"][kind]
        E = ref.E if isinstance(ref, RefWithError) else {f: s["E"][kind, f] for f in ref}
        bad, worst, where = [], 0.0, None
        for f, r in ref.items():
            g = np.asarray(got[f], dtype=F64)
            assert g.shape == r.shape, (f, g.shape, r.shape)
            if not np.all(np.isfinite(g)):
                bad.append((kind, f, "not finite"))
                continue
            d = np.abs(g - r)
            cells = [("field", float(d.max()), ERR_FACTOR * float(E[f].max()))]
            for cn, mask in self.classes.items():
                v = self.class_rows(f, d, mask)
                if v.size:
                    cells.append((cn, float(v.max()), ERR_FACTOR * float(self.class_rows(f, E[f], mask).max())))
            for cn, e, b in cells:
                if b == 0.0:
                    if e != 0.0:
                        bad.append((kind, f, cn, e, "both references agree and do not move: the numbers must be equal"))
                    continue
                if e / b > worst:
                    worst, where = e / b, (kind, f, cn)
                if e > b:
                    bad.append((kind, f, cn, e, b))
        return bad, worst, where

    # -- classes ------------------------------------------------------------------------------------------------------
    def _classes(self):
        sigs, differ = [], 0
        for st in [self.st] + [c2.state_from_table(t, NPROMA, NGPTOT) for t in self.tab_p]:
            for qs in (self.qsat, None):
                for precise in (0, 1):
                    s, _, d = census(self.prm, st, qs, precise)
                    sigs.append(active_cols(s, NGPTOT))
                    differ += d
                    if B.SINGLE:  # the fp64 host census of the same fp32 values: a cell on whose branch the precisions differ
                        s, _, d = census(self.prm, upcast_state(st), None if qs is None else qs.astype(F64), precise, single=False)
                        sigs.append(active_cols(s, NGPTOT))
                        differ += d
        self.dpr_clip_ne_reset = differ
        self.sig = sigs[0]
        # threshold cells: the signature depends on the arithmetic mode, on where QSAT comes from or on one ulp of the inputs
        self.excluded = np.zeros(self.sig.shape, dtype=bool)
        for s in sigs[1:]:
            self.excluded |= s != self.sig
        self.full_classes = outcome_masks(self.sig, self.evap)
        self.classes = {n: m & ~self.excluded for n, m in self.full_classes.items()}

    # -- bounds -------------------------------------------------------------------------------------------------------
    def class_rows(self, f: str, a: np.ndarray, mask: np.ndarray):
        """The values of field f that belong to the cells of a class.  Full-level fields: the cell's own.  Half-level fields (the
        fluxes; the adjoint of PAPH): the half level below the cell, where its rain and snow arrive and whose pressure closes its
        layer.  The adjoint of PLU: level jk reads PLU(JK+1) and nothing else does (cloudsc2.F90:435), so the value at jk+1 is
        the work of cell jk.  The top row of those fields belongs to no cell and stays under the whole-field bound."""
        if a.shape[0] == self.nlev + 1:
            return a[1:][mask]
        if f == "lu":
            return a[1:][mask[:-1]]
        return a[mask]

    def _bounds(self):
        refs_p = self._refs_p
        self.floor_abs, self.floor_field, self.scale = {}, {}, {}
        for kind in ("nl", "traj", "tl", "ad"):
            for f, r in self.ref[kind].items():
                d = np.max([np.abs(rp[kind][f] - r) for rp in refs_p], axis=0)
                m = float(np.abs(r).max())
                self.scale[kind, f] = m
                self.floor_field[kind, f] = float(d.max()) / m if m > 0.0 else 0.0
                for cn, mask in self.classes.items():
                    v = self.class_rows(f, d, mask)
                    self.floor_abs[kind, f, cn] = float(v.max()) if v.size else 0.0
        worst = lambda kinds: max(v for (k, f), v in self.floor_field.items() if k in kinds)  # noqa: E731
        self.K_NL = NL_TOL / worst(("nl",))
        self.K_TLAD = TLAD_TOL / worst(("tl", "ad"))

    def columns(self, cols: np.ndarray) -> "Case":
        """The same case with the field cut down to some columns: references, classes, floors, scales and K are those of the
        subset (compare() then takes results cut down alike)."""
        assert not B.SINGLE, "the fp32 yardstick is not cut down to columns"
        v = copy.copy(self)
        cut = lambda d: {n: np.ascontiguousarray(a[:, cols]) for n, a in d.items()}  # noqa: E731
        v.ref = {k: cut(d) for k, d in self.ref.items()}
        v._refs_p = [{k: cut(d) for k, d in rp.items()} for rp in self._refs_p]
        v.classes = cut(self.classes)
        v.full_classes = cut(self.full_classes)
        v._bounds()
        return v

    def tol(self, kind: str) -> float:
        return NL_TOL if kind in ("nl", "traj") else TLAD_TOL

    def K(self, kind: str) -> float:
        return self.K_NL if kind in ("nl", "traj") else self.K_TLAD

    def bound_abs(self, kind: str, f: str, cn: str) -> float:
        """K floor(f, c) as an absolute error, never looser than the whole-field bound; 0: the numbers must be equal."""
        return min(self.K(kind) * self.floor_abs[kind, f, cn], self.tol(kind) * self.scale[kind, f])

    def compare(self, kind: str, got: dict, ref: dict | None = None, satur: bool = False):
        """got: name -> (NLEVx, NGPTOT).  Returns (violations, worst err / bound, its place): every field under the whole-field
        bound, every (field, class) under its class bound.  satur (fp32 only): the sweep evaluated SATUR itself."""
        if B.SINGLE:
            return self._compare_single(kind, got, ref, satur)
        ref = ref if ref is not None else self.ref[kind]
        bad, worst, where = [], 0.0, None
        for f, r in ref.items():
            g = got[f]
            assert g.shape == r.shape, (f, g.shape, r.shape)
            if not np.all(np.isfinite(g)):
                bad.append((kind, f, "not finite"))
                continue
            d = np.abs(g - r)
            if float(d.max()) > self.tol(kind) * self.scale[kind, f]:
                bad.append((kind, f, "field", float(d.max()) / max(self.scale[kind, f], 1e-300), self.tol(kind)))
            for cn, mask in self.classes.items():
                v = self.class_rows(f, d, mask)
                if not v.size:
                    continue
                e, b = float(v.max()), self.bound_abs(kind, f, cn)
                if b == 0.0:
                    if e != 0.0:
                        bad.append((kind, f, cn, e, "reference does not move: the numbers must be equal"))
                    continue
                if e / b > worst:
                    worst, where = e / b, (kind, f, cn)
                if e > b:
                    bad.append((kind, f, cn, e, b))
        return bad, worst, where


class RefWithError(dict):
    """A reference result (field -> matrix) that carries its own yardstick E (field -> matrix)."""

    E: dict


def upcast_state(st):
    """The same values in fp64 arrays."""
    return dataclasses.replace(st, **{f.name: getattr(st, f.name).astype(F64) for f in dataclasses.fields(st)
                                      if isinstance(getattr(st, f.name), np.ndarray)})


@functools.lru_cache(maxsize=None)
def case(nlev: int, flagset: str) -> Case:
    return Case(nlev, flagset)


_ref_ad = {}


def reference_ad(c: Case, x0: dict, satur: bool = False) -> dict:
    """c.reference_ad(x0, satur), computed once per (case, set, background): the tests of both arithmetic modes share it."""
    import hashlib

    h = hashlib.sha1()
    for n in sorted(x0):
        h.update(np.ascontiguousarray(x0[n]).tobytes())
    key = (c.nlev, c.flagset, bool(satur) and B.SINGLE, h.hexdigest())
    if key not in _ref_ad:
        _ref_ad[key] = c.reference_ad(x0, satur)
    return _ref_ad[key]


def class_err(ref: np.ndarray, got: np.ndarray, mask: np.ndarray) -> float:
    """err(f, c) = max_c |got - ref| / max_c |ref| (0 if both vanish, infinite if only the reference does)."""
    d, m = float(np.abs(got - ref)[mask].max()), float(np.abs(ref)[mask].max())
    if m == 0.0:
        return 0.0 if d == 0.0 else np.inf
    return d / m


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the sweeps on a case (tests/hostcheck): results as (NLEVx, NGPTOT) matrices, like the reference's
# ---------------------------------------------------------------------------------------------------------------------
def state_outputs(st) -> dict:
    return {n: active_cols(np.ascontiguousarray(a), st.ngptot) for n, a in c2.op_outputs(st).items()}


def blocks_of(d: dict, fill: float = 0.0) -> dict:
    return {n: to_blocks(a, NPROMA, fill) for n, a in d.items()}


def cols_of(d: dict) -> dict:
    return {n: active_cols(a, NGPTOT) for n, a in d.items()}


def _flat(kind: str, arrays: dict):
    blk = B.Inputs() if kind == "in" else B.Outputs()
    for n, a in arrays.items():
        setattr(blk, n, hfld(a))
    return blk


def host_nl(c: Case, satur: bool) -> dict:
    """satur: SATUR in the sweep (no QSAT plane), else QSAT fed from the reference's SATUR."""
    got = c.st.copy()
    i, o = host_traj_blocks(got, None if satur else c.qsat)
    assert hostcheck().hostcheck_nl(C.byref(c.prm), c.ptsphy, NPROMA, c.nlev, NGPTOT, C.byref(i), C.byref(o), B.Field(), 0.0) == 0
    return state_outputs(got)


def host_tl(c: Case, satur: bool):
    """(trajectory outputs, tangent outputs) of hostcheck_tl with the reference's increments."""
    got = c.st.copy()
    i, o = host_traj_blocks(got, None if satur else c.qsat)
    inc = blocks_of(c.dinp)
    tl = {n: np.zeros((c.st.nblocks, c.nlev + (1 if n in refcall.HALF else 0), NPROMA), dtype=B.REAL) for n in B.OUT_NAMES}
    assert hostcheck().hostcheck_tl(C.byref(c.prm), c.ptsphy, NPROMA, c.nlev, NGPTOT, C.byref(i), C.byref(o),
                                    C.byref(_flat("in", inc)), C.byref(_flat("out", tl))) == 0
    return state_outputs(got), cols_of(tl)


def host_ad(c: Case, satur: bool, x0: dict, assign: bool) -> dict:
    """hostcheck_ad (both sweeps) with the output adjoints of the case; the input adjoints start from x0 (NGPTOT matrices)."""
    hc = hostcheck()
    got = c.st.copy()
    i, o = host_traj_blocks(got, None if satur else c.qsat)
    x, y = blocks_of(x0), blocks_of(c.refset(satur)["y"])
    scratch = np.zeros((c.st.nblocks, c.nlev, NPROMA), dtype=B.REAL)
    hc.hostcheck_set_assign(int(assign))
    try:
        assert hc.hostcheck_ad(C.byref(c.prm), c.ptsphy, NPROMA, c.nlev, NGPTOT, C.byref(i), C.byref(o), C.byref(_flat("in", x)),
                               C.byref(_flat("out", y)), scratch.ctypes.data) == 0
    finally:
        hc.hostcheck_set_assign(0)
    return cols_of(x)
