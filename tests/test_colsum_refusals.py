"""What cloudsc2_nl_launch_colsum, cloudsc2_tl_launch_colsum and cloudsc2_vjp_launch_colsum refuse: the return code and the text of
``cloudsc2_last_error()`` of every refusal, with the geometry and the pointers of test_launcher_refusals.py (World in
tests/gpu_util.py: NPROMA 8, NLEV 4, NGPTOT 12;
dummies without a device).  All of them are checked before the device is looked for, so every case is CLOUDSC2_EINVAL on the CPU too;
the message names the launcher, and after every refusal the calling thread's launch log is empty.  A well-formed call answers
CLOUDSC2_ENODEVICE where there is no device."""
from __future__ import annotations

import ctypes as C

import pytest

from tests.gpu_util import R_NGPTOT as NGPTOT, R_NLEV as NLEV, R_NPROMA as NPROMA, S, SH, SumWorld, refusal_params as params
from tests.util import B

EINVAL = B.CLOUDSC2_EINVAL
NL, TL, VJP = "cloudsc2_nl_launch_colsum", "cloudsc2_tl_launch_colsum", "cloudsc2_vjp_launch_colsum"
NULL_BLOCK = "NULL argument block"
GEOM = "nproma >= 1, 2 <= nlev = params.nlev <= CLOUDSC2_MAX_NLEV, ngptot >= 1, params.math_mode in 0..2 required"
TABLE = "the weight table is NULL"
SUM_STRIDES = "the sums given must share one block stride"
SUM_STRIDE = "the block stride of the sums is below nproma"
SATUR = "satur must be 0 (qsat given) or 1 (SATUR differentiated in the sweep)"
QSAT1 = "satur = 1: SATUR is differentiated in the sweep, every qsat field must be NULL"
QSAT0 = "satur = 0: traj_in->qsat is required"
TRAJ = "a required input field has a NULL pointer"
KEEP_BOTH = "keep needs both planes, fplsl and fplsn"
KEEP_SCRATCH = "keep with LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required"
KEEP_STRIDE = "the kept flux planes must have the block stride of in->paph"


def cases(W: SumWorld):
    """(id, the launcher, the expected message without the launcher's name, the call)"""
    L, r, out = B.lib, C.byref, []
    p, pe, pd, p0 = params(), params(levapls2=1), params(ldrain1d=1), params(lphylin=0)
    G = (NPROMA, NLEV, NGPTOT)
    ti, to, scr, tab = W.ins(), W.outs(), W.real("scratch"), W.real("table")
    ti_q0 = W.ins(qsat=None)
    ref = lambda b: r(b) if b is not None else None  # noqa: E731

    def nl(q=p, g=G, i=ti, w=tab, y="surface", keep=None, s=None):
        y = W.sums("sums") if y == "surface" else y
        return L.cloudsc2_nl_launch_colsum(ref(q), 3600.0, *g, ref(i), w, ref(y), ref(keep), s, None)

    def tl(q=p, g=G, satur=0, i=ti, x="narrow", w=tab, y="surface"):
        x = W.ins("pert", only=("q", "t")) if x == "narrow" else x
        y = W.sums("dsums") if y == "surface" else y
        return L.cloudsc2_tl_launch_colsum(ref(q), 3600.0, *g, satur, ref(i), ref(x), w, ref(y), None)

    def vjp(q=p, g=G, satur=0, i=ti, o=to, x="narrow", w=tab, y="surface", s=scr):
        x = W.ins("adj", only=("q", "t")) if x == "narrow" else x
        y = W.sums("ysums") if y == "surface" else y
        return L.cloudsc2_vjp_launch_colsum(ref(q), 3600.0, *g, satur, ref(i), ref(o), ref(x), w, ref(y), s, None)

    def case(name, who, msg, fn):
        out.append((name, who, msg, fn))

    bad_geoms = (("nproma=0", (0, NLEV, NGPTOT)), ("nlev=1", (NPROMA, 1, NGPTOT)), ("ngptot=0", (NPROMA, NLEV, 0)),
                 ("nlev_vs_params", (NPROMA, NLEV + 1, NGPTOT)))
    for who, fn in ((NL, nl), (TL, tl), (VJP, vjp)):
        tag = who.split("_")[1]
        case(f"{tag}/prm_null", who, NULL_BLOCK, lambda fn=fn: fn(q=None))
        case(f"{tag}/in_null", who, NULL_BLOCK, lambda fn=fn: fn(i=None))
        case(f"{tag}/sums_null", who, NULL_BLOCK, lambda fn=fn: fn(y=None))
        for gname, g in bad_geoms:
            case(f"{tag}/{gname}", who, GEOM, lambda fn=fn, g=g: fn(g=g))
        case(f"{tag}/math_mode", who, GEOM, lambda fn=fn: fn(q=params(math_mode=3)))
        case(f"{tag}/table_null", who, TABLE, lambda fn=fn: fn(w=None))
        case(f"{tag}/sum_strides_differ", who, SUM_STRIDES, lambda fn=fn, tag=tag: fn(y=W.sums(tag + "s", fplsn=2 * NPROMA)))
        case(f"{tag}/sum_stride_below_nproma", who, SUM_STRIDE, lambda fn=fn, tag=tag: fn(y=W.sums(tag + "s", fplsl=NPROMA - 1, fplsn=NPROMA - 1)))
        case(f"{tag}/traj_incomplete", who, TRAJ, lambda fn=fn: fn(i=W.ins(mfu=None)))
    # ---- NL ----
    case("nl/lphylin=0", NL, "the LPHYLIN form only (prm->lphylin = 0)", lambda: nl(q=p0))
    case("nl/no_sum", NL, "no sum is given (every sums field is NULL)", lambda: nl(y=B.Outputs()))
    case("nl/keep_only_fplsl", NL, KEEP_BOTH, lambda: nl(keep=W.outs("keep", only=("fplsl",))))
    case("nl/keep_only_fplsn", NL, KEEP_BOTH, lambda: nl(keep=W.outs("keep", only=("fplsn",))))
    case("nl/keep_neither", NL, KEEP_BOTH + " (neither is given)", lambda: nl(keep=B.Outputs()))
    case("nl/keep_stride", NL, KEEP_STRIDE, lambda: nl(keep=W.outs("keep", only=("fplsl", "fplsn"), fplsn=2 * SH)))
    case("nl/keep_evap_no_scratch", NL, KEEP_SCRATCH, lambda: nl(q=pe, keep=W.outs("keep", only=("fplsl", "fplsn"))))
    case("nl/keep_drain_no_scratch", NL, KEEP_SCRATCH, lambda: nl(q=pd, keep=W.outs("keep", only=("fplsl", "fplsn"))))
    # ---- TL ----
    case("tl/pert_in_null", TL, NULL_BLOCK, lambda: tl(x=None))
    case("tl/satur=2", TL, SATUR, lambda: tl(satur=2))
    case("tl/lphylin=0", TL, "sparse sweep: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)", lambda: tl(q=p0))
    case("tl/satur=1_traj_qsat", TL, QSAT1, lambda: tl(satur=1))
    case("tl/satur=1_pert_qsat", TL, QSAT1, lambda: tl(satur=1, i=ti_q0, x=W.ins("pert", only=("qsat", "t"))))
    case("tl/satur=0_without_qsat", TL, QSAT0, lambda: tl(i=ti_q0))
    case("tl/no_sum", TL, "no sum is wanted (every pert_sums field is NULL)", lambda: tl(y=B.Outputs()))
    case("tl/pert_in_stride", TL, "sparse sweep: the present fields of one layout group must share one block stride",
         lambda: tl(x=W.ins("pert", only=("q", "t"), q=2 * S)))
    # ---- reverse sweep ----
    case("vjp/traj_out_null", VJP, NULL_BLOCK, lambda: vjp(o=None))
    case("vjp/adj_in_null", VJP, NULL_BLOCK, lambda: vjp(x=None))
    case("vjp/satur=-1", VJP, SATUR, lambda: vjp(satur=-1))
    case("vjp/lphylin=0", VJP, "sparse sweep: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)", lambda: vjp(q=p0))
    case("vjp/satur=1_traj_qsat", VJP, QSAT1, lambda: vjp(satur=1))
    case("vjp/satur=1_adj_qsat", VJP, QSAT1, lambda: vjp(satur=1, i=ti_q0, x=W.ins("adj", only=("qsat",))))
    case("vjp/traj_flux_missing", VJP, "traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required", lambda: vjp(o=W.outs(fplsn=None)))
    case("vjp/scratch_missing", VJP, "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required", lambda: vjp(q=pe, s=None))
    case("vjp/no_cotangent", VJP, "no cotangent is given (every adj_sums field is NULL)", lambda: vjp(y=B.Outputs()))
    case("vjp/no_gradient", VJP, "no gradient is wanted (every adj_in field is NULL)", lambda: vjp(x=B.Inputs()))
    case("vjp/written_twice", VJP, "sparse sweep: a written plane is given twice",
         lambda: vjp(x=(lambda b: (setattr(b, "t", b.q), b)[1])(W.ins("adj", only=("q", "t")))))
    wellformed = (("nl/lean", lambda: nl()), ("nl/keep", lambda: nl(q=pe, keep=W.outs("keep", only=("fplsl", "fplsn")), s=scr)),
                  ("tl", lambda: tl()), ("tl/satur", lambda: tl(satur=1, i=ti_q0)), ("vjp", lambda: vjp()), ("vjp/evap", lambda: vjp(q=pe)))
    return out, wellformed


def test_colsum_refusals_before_the_device_is_looked_for():
    # (dummy pointers: with or without a device nothing may launch; every case is refused before the device is asked for)
    refusals, _ = cases(SumWorld(False))
    assert len({c[0] for c in refusals}) == len(refusals)
    for name, who, msg, fn in refusals:
        B.lib.cloudsc2_debug_launch_log_reset()
        rc = fn()
        text = B.lib.cloudsc2_last_error().decode()
        assert (rc, text) == (EINVAL, f"{who}: {msg}"), (name, rc, text)
        assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0, (name, "the launch log is not empty after a refusal")


def test_a_well_formed_call_needs_a_device():
    if B.device_available():
        pytest.skip("a device is present: the well-formed calls would launch on dummy pointers")
    _, wellformed = cases(SumWorld(False))
    for name, fn in wellformed:
        B.lib.cloudsc2_debug_launch_log_reset()
        assert fn() == B.CLOUDSC2_ENODEVICE, (name, B.lib.cloudsc2_last_error().decode())
        assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0, name


def test_header_binding_and_library_agree_on_the_new_symbols():
    for name in (NL, TL, VJP):
        assert name in B.EXPORTED and hasattr(B.lib, name)
    assert len(B.FAMILIES) == 10 and not any("colsum" in f for f in B.FAMILIES)  # not sweep families
    assert B.lib.cloudsc2_variant_built(10, 1) == EINVAL  # family 10 stays no family
