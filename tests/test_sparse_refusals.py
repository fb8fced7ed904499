"""What cloudsc2_tl_launch_sparse and cloudsc2_vjp_launch_sparse refuse: the return code and the text of ``cloudsc2_last_error()`` of
every refusal, with the geometry and the pointers of test_launcher_refusals.py (World in
tests/gpu_util.py: NPROMA 8, NLEV 4, NGPTOT 12; dummies without a device,
device memory of more than the implied extent with one).  All of them are checked before the device is looked for, so every case is
CLOUDSC2_EINVAL on the CPU too; the cases whose loss would still be a valid small launch run again under ``-m gpu``.  After every
refusal the calling thread's launch log is empty."""
from __future__ import annotations

import ctypes as C

import pytest

from tests.gpu_util import DistinctWorld, R_NGPTOT as NGPTOT, R_NLEV as NLEV, R_NPROMA as NPROMA, S, SH, World, refusal_params as params
from tests.util import B

EINVAL = B.CLOUDSC2_EINVAL
NULL_BLOCK = "NULL argument block"
SATUR = "satur must be 0 (qsat given) or 1 (SATUR differentiated in the sweep)"
LPHYLIN = "sparse sweep: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only (prm->lphylin = 0)"
QSAT1 = "satur = 1: SATUR is differentiated in the sweep, every qsat field must be NULL"
QSAT0 = "satur = 0: traj_in->qsat is required"
TRAJ = "a required input field has a NULL pointer"
FLUX = "reverse sweep: traj_out->fplsl and ->fplsn (PFPLSL5, PFPLSN5) are required"
SCRATCH = "LEVAPLS2/LDRAIN1D: the cover-checkpoint plane `scratch` is required"
NO_OUT = "sparse TL sweep: no output tangent is wanted (every pert_out field is NULL)"
NO_COT = "sparse reverse sweep: no cotangent is given (every adj_out field is NULL)"
NO_GRAD = "sparse reverse sweep: no gradient is wanted (every adj_in field is NULL)"
STRIDE = "sparse sweep: the present fields of one layout group must share one block stride"
TWICE = "sparse sweep: a written plane is given twice"


def cases(W: World):
    """(id, runs with a device too, expected message, the call)"""
    L, r, out = B.lib, C.byref, []
    p, pe, p0 = params(), params(levapls2=1), params(lphylin=0)
    G = (NPROMA, NLEV, NGPTOT)
    ti, to, scr = W.ins(), W.outs(), W.real("scratch")
    ti_q0 = W.ins(qsat=None)
    narrow_in = dict(only=("q", "t"))
    narrow_out = dict(only=("fplsl", "fplsn"))

    def tl(q=p, satur=0, i=ti, x="narrow", y="all"):
        x = W.ins("pert", **narrow_in) if x == "narrow" else x
        y = W.outs("pert") if y == "all" else y
        return L.cloudsc2_tl_launch_sparse(r(q) if q is not None else None, 3600.0, *G, satur, r(i) if i is not None else None,
                                           r(x) if x is not None else None, r(y) if y is not None else None, None)

    def vjp(q=p, satur=0, i=ti, o=to, x="narrow", y="narrow", s=scr):
        x = W.ins("adj", **narrow_in) if x == "narrow" else x
        y = W.outs("adj", **narrow_out) if y == "narrow" else y
        return L.cloudsc2_vjp_launch_sparse(r(q) if q is not None else None, 3600.0, *G, satur, r(i) if i is not None else None,
                                            r(o) if o is not None else None, r(x) if x is not None else None,
                                            r(y) if y is not None else None, s, None)

    def twice(blk, a, b):
        setattr(blk, b, getattr(blk, a))
        return blk

    def case(name, gpu, msg, fn):
        out.append((name, gpu, msg, fn))

    # ---- TL ----
    case("tl/prm_null", False, NULL_BLOCK, lambda: tl(q=None))
    case("tl/traj_in_null", False, NULL_BLOCK, lambda: tl(i=None))
    case("tl/pert_in_null", False, NULL_BLOCK, lambda: tl(x=None))
    case("tl/pert_out_null", False, NULL_BLOCK, lambda: tl(y=None))
    case("tl/satur=2", True, SATUR, lambda: tl(satur=2))
    case("tl/satur=-1", True, SATUR, lambda: tl(satur=-1))
    case("tl/lphylin=0", True, LPHYLIN, lambda: tl(q=p0))
    case("tl/satur=1_traj_qsat", True, QSAT1, lambda: tl(satur=1))
    case("tl/satur=1_pert_qsat", True, QSAT1, lambda: tl(satur=1, i=ti_q0, x=W.ins("pert", only=("qsat", "t"))))
    case("tl/satur=0_without_qsat", False, QSAT0, lambda: tl(i=ti_q0))
    case("tl/traj_incomplete", False, TRAJ, lambda: tl(i=W.ins(mfu=None)))
    case("tl/no_output", True, NO_OUT, lambda: tl(y=B.Outputs()))
    case("tl/pert_in_stride", True, STRIDE, lambda: tl(x=W.ins("pert", only=("q", "t"), q=2 * S)))
    case("tl/pert_out_stride", True, STRIDE, lambda: tl(y=W.outs("pert", only=("tent", "teni"), teni=2 * S)))
    case("tl/full_out_vs_in", True, STRIDE, lambda: tl(y=W.outs("pert", only=("clc",), clc=2 * S)))
    case("tl/half_out_vs_in", True, STRIDE, lambda: tl(x=W.ins("pert", only=("paph",)), y=W.outs("pert", only=("fplsl",), fplsl=2 * SH)))
    case("tl/written_twice", True, TWICE, lambda: tl(y=twice(W.outs("pert", only=("tent", "tenq")), "tent", "tenq")))
    case("tl/satur=2+lphylin=0", True, SATUR, lambda: tl(q=p0, satur=2))
    # ---- reverse sweep ----
    case("vjp/prm_null", False, NULL_BLOCK, lambda: vjp(q=None))
    case("vjp/traj_out_null", False, NULL_BLOCK, lambda: vjp(o=None))
    case("vjp/adj_in_null", False, NULL_BLOCK, lambda: vjp(x=None))
    case("vjp/adj_out_null", False, NULL_BLOCK, lambda: vjp(y=None))
    case("vjp/satur=2", True, SATUR, lambda: vjp(satur=2))
    case("vjp/lphylin=0", True, LPHYLIN, lambda: vjp(q=p0))
    case("vjp/satur=1_traj_qsat", True, QSAT1, lambda: vjp(satur=1))
    case("vjp/satur=1_adj_qsat", True, QSAT1, lambda: vjp(satur=1, i=ti_q0, x=W.ins("adj", only=("qsat",))))
    case("vjp/satur=0_without_qsat", False, QSAT0, lambda: vjp(i=ti_q0))
    case("vjp/traj_incomplete", False, TRAJ, lambda: vjp(i=W.ins(paph=None)))
    case("vjp/traj_flux_missing", False, FLUX, lambda: vjp(o=W.outs(fplsn=None)))
    case("vjp/scratch_missing", False, SCRATCH, lambda: vjp(q=pe, s=None))
    case("vjp/no_cotangent", True, NO_COT, lambda: vjp(y=B.Outputs()))
    case("vjp/no_gradient", True, NO_GRAD, lambda: vjp(x=B.Inputs()))
    case("vjp/adj_in_stride", True, STRIDE, lambda: vjp(x=W.ins("adj", only=("q", "t"), t=2 * S)))
    case("vjp/adj_out_stride", True, STRIDE, lambda: vjp(y=W.outs("adj", only=("fplsl", "fplsn"), fplsn=2 * SH)))
    case("vjp/full_out_vs_in", True, STRIDE, lambda: vjp(y=W.outs("adj", only=("covptot",), covptot=2 * S)))
    case("vjp/written_twice", True, TWICE, lambda: vjp(x=twice(W.ins("adj", only=("q", "t")), "q", "t")))
    case("vjp/no_cotangent+no_gradient", True, NO_COT, lambda: vjp(x=B.Inputs(), y=B.Outputs()))
    return out


def run(device: bool, only_gpu: bool) -> None:
    W = DistinctWorld(device)
    for name, gpu, msg, fn in cases(W):
        if only_gpu and not gpu:
            continue
        B.lib.cloudsc2_debug_launch_log_reset()
        rc = fn()
        text = B.lib.cloudsc2_last_error().decode()
        assert (rc, text) == (EINVAL, msg), (name, rc, text)
        assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0, (name, "the launch log is not empty after a refusal")


def test_sparse_refusals_before_the_device_is_looked_for():
    # (dummy pointers: with or without a device nothing may launch; every case is refused before the device is asked for)
    run(device=False, only_gpu=False)
    assert len({c[0] for c in cases(DistinctWorld(False))}) == len(cases(DistinctWorld(False)))


@pytest.mark.gpu
def test_sparse_refusals_with_a_device():
    run(device=True, only_gpu=True)
