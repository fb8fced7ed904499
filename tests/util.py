"""Shared helpers of the test-suite (host side)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.hostbuild import HIPCC, HOSTCHECK_DIR, ROOT, B, host_lib  # noqa: F401  (ROOT is on sys.path from here on)

import dwarf_p_cloudsc2_tl_ad_amd as c2  # noqa: E402
from oracle import refcall  # noqa: E402


def hostcheck():
    """The per-column device functions compiled for the host (tests/hostcheck) -- a unit-test vehicle, not a product path."""
    return host_lib("")


def hfld(a: np.ndarray, offset: int = 0, stride: int | None = None, real=None) -> B.Field:
    """real: the element type of a host build of the other precision (tests/branch_atlas.py), else the process's own"""
    real = np.dtype(real or B.REAL)
    assert a.dtype == real and a.flags["C_CONTIGUOUS"]
    f = B.Field()
    f.ptr = a.ctypes.data + real.itemsize * offset
    f.block_stride = stride if stride is not None else int(np.prod(a.shape[1:]))
    return f


def host_traj_blocks(st: c2.Cloudsc2State, qsat: np.ndarray | None = None, real=None):
    """Inputs/Outputs blocks with HOST pointers into a Cloudsc2State (same mapping as DeviceState)."""
    S = st.nproma * st.nlev
    fld = lambda a, offset=0, stride=None: hfld(a, offset, stride, real)  # noqa: E731
    i = B.Inputs()
    i.paph = fld(st.PAPH); i.pap = fld(st.PAP); i.q = fld(st.PQ)
    i.qsat = fld(qsat) if qsat is not None else B.Field()
    i.t = fld(st.PT)
    i.l = fld(st.PCLV, 0 * S, 5 * S); i.i = fld(st.PCLV, 1 * S, 5 * S)
    i.lude = fld(st.PLUDE); i.lu = fld(st.PLU); i.mfu = fld(st.PMFU); i.mfd = fld(st.PMFD)
    i.gtent = fld(st.B_CML, 0 * S, 8 * S); i.gtenq = fld(st.B_CML, 2 * S, 8 * S)
    i.gtenl = fld(st.B_CML, 3 * S, 8 * S); i.gteni = fld(st.B_CML, 4 * S, 8 * S)
    i.supsat = fld(st.PSUPSAT)
    o = B.Outputs()
    o.tent = fld(st.B_LOC, 0 * S, 8 * S); o.tenq = fld(st.B_LOC, 2 * S, 8 * S)
    o.tenl = fld(st.B_LOC, 3 * S, 8 * S); o.teni = fld(st.B_LOC, 4 * S, 8 * S)
    o.clc = fld(st.PA); o.covptot = fld(st.PCOVPTOT)
    o.fplsl = fld(st.PFPLSL); o.fplsn = fld(st.PFPLSN); o.fhpsl = fld(st.PFHPSL); o.fhpsn = fld(st.PFHPSN)
    return i, o


def flat_fields(kind: str, nb: int, nlev: int, nproma: int, fill: float = 0.0) -> dict:
    names = B.IN_NAMES if kind == "in" else B.OUT_NAMES
    return {n: np.full((nb, nlev + (1 if n in refcall.HALF else 0), nproma), fill, dtype=B.REAL) for n in names}


def flat_block(kind: str, arrays: dict):
    blk = B.Inputs() if kind == "in" else B.Outputs()
    for n, a in arrays.items():
        setattr(blk, n, hfld(a))
    return blk


def increments_of(st: c2.Cloudsc2State, qsat: np.ndarray, zero_supsat: bool = False) -> dict:
    """dx = 0.01*x for the 16 inputs, flat (NBLOCKS, NLEVx, NPROMA) (cloudsc_driver_tl_mod.F90:156-171)."""
    out = {n: np.ascontiguousarray(a * B.REAL(0.01)) for n, a in c2.op_inputs(st, qsat).items()}
    if zero_supsat:
        out["supsat"][...] = 0.0
    return out


def make_params(tab: dict, **flags) -> B.Params:
    return c2.default_params(c2.ceta_from_table(tab), **flags)


def set_lib_params(lib, prm: B.Params):
    lib.set_params(prm.doubles30(), prm.ceta_array(), lphylin=bool(prm.lphylin), levapls2=bool(prm.levapls2),
                   lregcl=bool(prm.lregcl))


def relerr(ref: np.ndarray, got: np.ndarray) -> float:
    """max |got-ref| / max|ref| (0 if both vanish)."""
    d = float(np.max(np.abs(got - ref))) if ref.size else 0.0
    m = float(np.max(np.abs(ref))) if ref.size else 0.0
    if m == 0.0:
        return 0.0 if d == 0.0 else np.inf
    return d / m


# ---------------------------------------------------------------------------------------------------------------------
# what the host-build tests share
# ---------------------------------------------------------------------------------------------------------------------
BITS = np.int32 if B.SINGLE else np.int64  # the integer of an element's size: bits are compared through it
PARAM_NAMES = c2.PARAM_NAMES  # rkconv, rclcrit, rlptrc, rpecons: the order of CLOUDSC2_NPAR
FLAG_SETS = FLAGS = [dict(), dict(levapls2=True, lregcl=True), dict(ldrain1d=True), dict(lregcl=True)]
fp64_only = pytest.mark.skipif(B.SINGLE, reason="the bounds are fp64 statements")


# C2F_* of csrc/cloudsc2_column.hpp (several bits mean different things to different families)
QSAT, PRECISE, EVAP, OFF32 = 1, 2, 4, 32
PERT = TRAJ = ASSIGN = 8
CKPT = SELFINC = ADNORM = 16
NOLIN = VJP = 64
SATLIN, PARLIN = 128, 256


def the_tables():
    return [("synthetic", c2.synthetic_table()), ("seed5", c2.random_table(137, 100, seed=5))]


def host_qsat(st) -> np.ndarray:
    qsat = np.zeros_like(st.PAP)
    pap, t = np.ascontiguousarray(st.PAP), np.ascontiguousarray(st.PT)
    f = lambda a: B.Field(a.ctypes.data, int(np.prod(a.shape[1:])))  # noqa: E731
    prm = c2.default_params(np.full(st.nlev, 0.5))
    assert hostcheck().hostcheck_satur(C.byref(prm), st.nproma, st.nlev, st.ngptot, f(pap), f(t), f(qsat)) == 0
    return qsat


def bits(a: np.ndarray) -> np.ndarray:
    return a.view(BITS)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    return np.array_equal(np.ascontiguousarray(a).view(BITS), np.ascontiguousarray(b).view(BITS))


def blocks_of(st):
    for ibl in range(st.nblocks):
        yield ibl, min(st.nproma, st.ngptot - ibl * st.nproma)


def columns(a: np.ndarray, ngptot: int) -> np.ndarray:
    """(nblocks, nlevx, nproma) -> (nlevx, ngptot): the active columns in grid order"""
    return a.transpose(1, 0, 2).reshape(a.shape[1], -1)[:, :ngptot]


def tail_checks(arrays: dict, nproma: int, ngptot: int, what: str) -> None:
    """arrays were NaN-filled before the sweep: every active element written, the padded tail still NaN"""
    for n, a in arrays.items():
        for ibl in range(a.shape[0]):
            icend = min(nproma, ngptot - ibl * nproma)
            assert not np.any(np.isnan(a[ibl][:, :icend])), (what, "active element not written", n, ibl)
            assert np.all(np.isnan(a[ibl][:, icend:])), (what, "padded tail touched", n, ibl)


def block_array(kind: str, per_direction: list):
    typ = B.Inputs if kind == "in" else B.Outputs
    return (typ * len(per_direction))(*[flat_block(kind, d) for d in per_direction])


def sanitizer_runtimes() -> bool:
    """the static AddressSanitizer and UndefinedBehaviorSanitizer runtimes an executable links"""
    for lib in ("libclang_rt.asan-x86_64.a", "libclang_rt.ubsan_standalone-x86_64.a"):
        try:
            p = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", f"-print-file-name={lib}"], capture_output=True, text=True, timeout=60).stdout.strip()
        except (OSError, subprocess.SubprocessError):
            return False
        if not (os.path.isabs(p) and os.path.exists(p)):
            return False
    return True
