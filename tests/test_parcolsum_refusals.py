"""What cloudsc2_parjac_launch_colsum and cloudsc2_parnormal_launch_colsum refuse: the return code and the text of
``cloudsc2_last_error()`` of every refusal, with the geometry and the pointers of test_launcher_refusals.py (World in
tests/gpu_util.py: NPROMA 8, NLEV 4, NGPTOT 12;
dummies without a device, device memory of more than the implied extent with one).  All of them are checked before the device is looked
for, so every case is CLOUDSC2_EINVAL on the CPU too; the message names the launcher; the cases whose loss would still be a valid small
launch run again under ``-m gpu``.  After every refusal the calling thread's launch log is empty.  A well-formed call answers
CLOUDSC2_ENODEVICE where there is no device.  (Every variant of the flag words the launchers can form is built, so "kernel variant not
built" cannot be provoked from outside.)"""
from __future__ import annotations

import ctypes as C
import os

import pytest

from tests.gpu_util import R_NGPTOT as NGPTOT, R_NLEV as NLEV, R_NPROMA as NPROMA, S, SumWorld, refusal_params as params
from tests.util import B, ROOT

EINVAL = B.CLOUDSC2_EINVAL
JAC, NORMAL = "cloudsc2_parjac_launch_colsum", "cloudsc2_parnormal_launch_colsum"
NULL_BLOCK = "NULL argument block"
NULL_NORMAL = "NULL argument block, workspace or result"
GEOM = "nproma >= 1, 2 <= nlev = params.nlev <= CLOUDSC2_MAX_NLEV, ngptot >= 1, params.math_mode in 0..2 required"
LPHYLIN = "CLOUDSC2TL linearises the LPHYLIN form only (prm->lphylin = 0)"
RPECONS = "parameter derivative with the evaporation branch: rpecons must not be 0"
TABLE = "the weight table is NULL"
SUM_STRIDES = "the sums given must share one block stride"
SUM_STRIDE = "the block stride of the sums is below nproma"
NO_SUM = "no sum is wanted (every field of sens_sums[0] is NULL)"
ONE_EMPTY = "every parameter's block of sens_sums must hold the same sums (one holds none)"
MASKS = "every parameter's block of sens_sums must hold the same sums"
NO_OBS = "no sum is observed (every residual field is NULL)"
UNOBSERVED = "a weight is given for a sum that is not observed (its residual is NULL)"
RW_STRIDE = "residuals and weights must share one block stride"
TRAJ = "a required input field has a NULL pointer"


def cases(W: SumWorld):
    """(id, runs with a device too, the launcher, the expected message without the launcher's name or None for any, the call)"""
    L, r, out = B.lib, C.byref, []
    p, pe, pe0, pd0, p0 = params(), params(levapls2=1), params(levapls2=1, rpecons=0.0), params(ldrain1d=1, rpecons=0.0), params(lphylin=0)
    G = (NPROMA, NLEV, NGPTOT)
    ti, tab = W.ins(), W.real("table")
    work, normal = W.dbl("work"), W.dbl("normal", 14)
    ref = lambda b: r(b) if b is not None else None  # noqa: E731

    def four(n=4, **edits):
        """n blocks of the two surface sums; edits["b<k>"] = keyword arguments of SumWorld.sums for block k"""
        return (B.Outputs * 4)(*[W.sums(f"sens{k}", **edits.get(f"b{k}", {})) for k in range(n)])

    def jac(q=p, g=G, i=ti, w=tab, y="four"):
        y = four() if y == "four" else y
        return L.cloudsc2_parjac_launch_colsum(ref(q), 3600.0, *g, ref(i), w, y, None)

    def nrm(q=p, g=G, i=ti, w=tab, rs="surface", wt="surface", wk=work, nm=normal):
        rs = W.sums("resid") if rs == "surface" else rs
        wt = W.sums("weight") if wt == "surface" else wt
        return L.cloudsc2_parnormal_launch_colsum(ref(q), 3600.0, *g, ref(i), w, ref(rs), ref(wt), wk, nm, None)

    def case(name, gpu, who, msg, fn):
        out.append((name, gpu, who, msg, fn))

    bad_geoms = (("nproma=0", (0, NLEV, NGPTOT)), ("nlev=1", (NPROMA, 1, NGPTOT)), ("ngptot=0", (NPROMA, NLEV, 0)),
                 ("nlev_vs_params", (NPROMA, NLEV + 1, NGPTOT)))
    for tag, who, fn, null in (("jac", JAC, jac, NULL_BLOCK), ("normal", NORMAL, nrm, NULL_NORMAL)):
        case(f"{tag}/prm_null", False, who, null, lambda fn=fn: fn(q=None))
        case(f"{tag}/traj_in_null", False, who, null, lambda fn=fn: fn(i=None))
        for gname, g in bad_geoms:
            case(f"{tag}/{gname}", False, who, GEOM, lambda fn=fn, g=g: fn(g=g))
        case(f"{tag}/math_mode", False, who, GEOM, lambda fn=fn: fn(q=params(math_mode=3)))
        case(f"{tag}/lphylin=0", True, who, LPHYLIN, lambda fn=fn: fn(q=p0))
        case(f"{tag}/rpecons=0", True, who, RPECONS, lambda fn=fn: fn(q=pe0))
        case(f"{tag}/rpecons=0_ldrain1d", True, who, RPECONS, lambda fn=fn: fn(q=pd0))
        case(f"{tag}/lphylin=0+rpecons=0", True, who, LPHYLIN, lambda fn=fn: fn(q=params(lphylin=0, levapls2=1, rpecons=0.0)))
        case(f"{tag}/table_null", False, who, TABLE, lambda fn=fn: fn(w=None))
        case(f"{tag}/traj_incomplete", False, who, TRAJ, lambda fn=fn: fn(i=W.ins(mfu=None)))
        case(f"{tag}/traj_in_stride", True, who, None, lambda fn=fn: fn(i=W.ins(pap=2 * S)))
    # ---- the sums form ----
    case("jac/sens_sums_null", False, JAC, NULL_BLOCK, lambda: jac(y=None))
    case("jac/no_sum", True, JAC, NO_SUM, lambda: jac(y=(B.Outputs * 4)()))
    case("jac/strides_differ_inside_a_block", True, JAC, SUM_STRIDES, lambda: jac(y=four(b0=dict(fplsn=2 * NPROMA))))
    case("jac/strides_differ_inside_a_later_block", True, JAC, SUM_STRIDES, lambda: jac(y=four(b2=dict(fplsn=2 * NPROMA))))
    case("jac/strides_differ_between_blocks", True, JAC, SUM_STRIDES, lambda: jac(y=four(b1=dict(fplsl=2 * NPROMA, fplsn=2 * NPROMA))))
    case("jac/stride_below_nproma", False, JAC, SUM_STRIDE,
         lambda: jac(y=four(**{f"b{k}": dict(fplsl=NPROMA - 1, fplsn=NPROMA - 1) for k in range(4)})))
    case("jac/a_block_holds_no_sum", True, JAC, ONE_EMPTY, lambda: jac(y=four(b1=dict(only=()))))
    case("jac/masks_differ", True, JAC, MASKS, lambda: jac(y=four(b2=dict(only=("fplsl",)))))
    case("jac/masks_differ_more_in_a_later_block", True, JAC, MASKS, lambda: jac(y=four(b1=dict(only=("fplsl", "fplsn", "tent")))))
    case("jac/rpecons_block_looked_at_with_evaporation", True, JAC, ONE_EMPTY, lambda: jac(q=pe, y=four(3)))
    # ---- the normal form ----
    case("normal/resid_null", False, NORMAL, NULL_NORMAL, lambda: nrm(rs=None))
    case("normal/work_null", False, NORMAL, NULL_NORMAL, lambda: nrm(wk=None))
    case("normal/normal_null", False, NORMAL, NULL_NORMAL, lambda: nrm(nm=None))
    case("normal/nothing_observed", True, NORMAL, NO_OBS, lambda: nrm(rs=B.Outputs(), wt=None))
    case("normal/weight_without_residual", True, NORMAL, UNOBSERVED, lambda: nrm(rs=W.sums("resid", only=("fplsl",))))
    case("normal/weight_without_residual+stride", True, NORMAL, UNOBSERVED,
         lambda: nrm(rs=W.sums("resid", only=("fplsl",)), wt=W.sums("weight", fplsn=2 * NPROMA)))
    case("normal/resid_strides_differ", True, NORMAL, SUM_STRIDES, lambda: nrm(rs=W.sums("resid", fplsn=2 * NPROMA), wt=None))
    case("normal/weight_strides_differ", True, NORMAL, SUM_STRIDES, lambda: nrm(wt=W.sums("weight", fplsn=2 * NPROMA)))
    case("normal/resid_vs_weight_stride", True, NORMAL, RW_STRIDE, lambda: nrm(wt=W.sums("weight", fplsl=2 * NPROMA, fplsn=2 * NPROMA)))
    case("normal/stride_below_nproma", False, NORMAL, SUM_STRIDE,
         lambda: nrm(rs=W.sums("resid", fplsl=NPROMA - 1, fplsn=NPROMA - 1), wt=None))
    wellformed = (("jac", lambda: jac()), ("jac/evap", lambda: jac(q=pe)), ("jac/rpecons_block_null", lambda: jac(y=four(3))),
                  ("jac/satur", lambda: jac(i=W.ins(qsat=None))), ("normal", lambda: nrm()), ("normal/no_weights", lambda: nrm(wt=None)),
                  ("normal/one_weight", lambda: nrm(wt=W.sums("weight", only=("fplsn",)))), ("normal/evap", lambda: nrm(q=pe)))
    return out, wellformed


def run(device: bool, only_gpu: bool) -> None:
    refusals, _ = cases(SumWorld(device))
    assert len({c[0] for c in refusals}) == len(refusals)
    for name, gpu, who, msg, fn in refusals:
        if only_gpu and not gpu:
            continue
        B.lib.cloudsc2_debug_launch_log_reset()
        rc = fn()
        text = B.lib.cloudsc2_last_error().decode()
        assert rc == EINVAL and text.startswith(f"{who}: ") and (msg is None or text == f"{who}: {msg}"), (name, rc, text)
        assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0, (name, "the launch log is not empty after a refusal")


def test_parcolsum_refusals_before_the_device_is_looked_for():
    # (dummy pointers: with or without a device nothing may launch; every case is refused before the device is asked for)
    run(device=False, only_gpu=False)


@pytest.mark.gpu
def test_parcolsum_refusals_with_a_device():
    import torch

    run(device=True, only_gpu=True)
    torch.cuda.synchronize()


def test_a_well_formed_call_needs_a_device():
    if B.device_available():  # (the well-formed calls would launch on dummy pointers)
        return
    _, wellformed = cases(SumWorld(False))
    for name, fn in wellformed:
        B.lib.cloudsc2_debug_launch_log_reset()
        assert fn() == B.CLOUDSC2_ENODEVICE, (name, B.lib.cloudsc2_last_error().decode())
        assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0, name


def test_header_binding_and_library_agree_on_the_new_symbols():
    with open(os.path.join(ROOT, "include", "cloudsc2_hip.h")) as f:
        header = f.read()
    for name in (JAC, NORMAL):
        assert f"int {name}(" in header, name  # declared
        assert name in B.EXPORTED and hasattr(B.lib, name)  # exported (tests/test_abi.py then covers both libraries)
    assert len(B.FAMILIES) == 10 and not any("colsum" in f for f in B.FAMILIES)  # not a sweep family
    assert B.lib.cloudsc2_variant_built(10, 1) == EINVAL  # family 10 stays no family
