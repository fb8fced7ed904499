"""Per-column parameter maps (C2F_PARMAP: what cloudsc2_{nl,tl,vjp}_launch_parmap run), compiled for the HOST.

The contract is bits: column c of every output, cover checkpoint, output tangent and field adjoint is what the scalar-parameter sweep
(tests/host_sweeps.py: the trajectory sweep, run_tl_par, run_vjp_par) gives at column c for a parameter block holding column c's four
values, and column c of the adjoint table is column c of that sweep's workspace.  It rests on the lane's derivation of its constants
(lane_consts) giving the BYTES of the host's make_consts + make_parlin, checked here in both precisions.  The sweeps run in the process's
precision; the fp64 process starts this module once more in the fp32 build.

Bounds.  None for the comparisons (bits).  1e-12 relative for the dot-product identity <TL(dx, dp), u> = <dx, xbar> + sum_c dp[c] pbar[c]
(the project's bound for this identity), and the parameter term must change it by more than 1e-9 (as tests/test_hostcheck_par.py
asserts): fp64 statements."""
from __future__ import annotations

import copy
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.host_sweeps import increments15, run_tl_par, run_vjp_par, trajectory_for_reverse
from tests.hostbuild import HOSTCHECK_DIR, build, precise  # noqa: F401
from tests.test_hostcheck_ens import FLAGS as ENS_FLAGS, rows_of
from tests.util import PARAM_NAMES, ROOT, B, bits, c2, flat_block, flat_fields, fp64_only, host_qsat, host_traj_blocks, increments_of, make_params

SHAPES = {"a": (24, 70), "b": (64, 200)}
_I, _D, _V = C.c_int, C.c_double, C.c_void_p
_PP, _PI, _PO, _PD = C.POINTER(B.Params), C.POINTER(B.Inputs), C.POINTER(B.Outputs), C.POINTER(C.c_double)
_G = [_PP, _D, _I, _I, _I]
PROTOTYPES = {
    "hostcheck_parmap_real_bytes": (_I, []),
    "hostcheck_parmap_lane_consts": (_I, [_PP, _D, _PD, _PD]),
    "hostcheck_parmap_nl": (_I, _G + [_V, _PI, _PO, _V]),
    "hostcheck_parmap_tl": (_I, _G + [_I, _V, _V, _PI, _PI, _PO]),
    "hostcheck_parmap_vjp": (_I, _G + [_I, _V, _PI, _PO, _PI, _PO, _V, _V]),
}
_libs: dict = {}


def parmap_lib(single: bool = B.SINGLE) -> C.CDLL:
    if single not in _libs:
        path = build(os.path.join(HOSTCHECK_DIR, "hostcheck_parmap.hip"),
                     os.path.join(HOSTCHECK_DIR, "libhostcheck_parmap" + ("_sp" if single else "") + ".so"), single=single)
        lib = C.CDLL(path)
        for fn, (restype, argtypes) in PROTOTYPES.items():
            getattr(lib, fn).restype = restype
            getattr(lib, fn).argtypes = argtypes
        _libs[single] = lib
    return _libs[single]


@pytest.fixture
def lib(precise):  # noqa: F811  (the process's precision, in the arithmetic mode of the other host libraries)
    lib = parmap_lib()
    lib.hostcheck_set_precise(int(precise))
    yield lib
    lib.hostcheck_set_precise(0)


def dvec(values):
    return (C.c_double * 4)(*[float(v) for v in values])


# ---- the lane's constants ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("flags", ENS_FLAGS, ids=lambda f: "-".join(k for k, v in f.items() if v) or "plain")
def test_a_lanes_constants_are_the_hosts_bytes(single, flags):
    lib = parmap_lib(single)
    assert lib.hostcheck_parmap_real_bytes() == (4 if single else 8)
    prm = make_params(c2.synthetic_table(), **flags)
    for ptsphy in (3600.0, 1234.5):
        for row in rows_of(prm):
            tangents = [0.01 * v / 3.0 for v in row]
            assert lib.hostcheck_parmap_lane_consts(C.byref(prm), ptsphy, dvec(row), dvec(tangents)) == 0, (flags, ptsphy, row, "tangents given")
            assert lib.hostcheck_parmap_lane_consts(C.byref(prm), ptsphy, dvec(row), None) == 0, (flags, ptsphy, row, "tangents NULL")


# ---- the sweeps -------------------------------------------------------------------------------------------------------------------

def case_state(shape):
    nproma, ngptot = SHAPES[shape]
    tab = c2.random_table(24, 100, seed=23) if shape == "a" else c2.synthetic_table()
    return tab, c2.state_from_table(tab, nproma, ngptot)


def value_map(prm, st, shape):
    """idx (ncols_pad,) and values (nvalues, 4): shape (a) a value of its own per column and parameter, shape (b) three values"""
    ncp = st.nblocks * st.nproma
    own = np.array([getattr(prm, n) for n in PARAM_NAMES])
    rng = np.random.default_rng(29)
    if shape == "a":
        idx = np.arange(ncp)
        vals = own * rng.uniform(0.6, 1.4, (ncp, 4))
        vals[:, 2] = own[2] + rng.uniform(-3.0, 3.0, ncp)  # rlptrc: an offset in K
    else:
        c = np.arange(ncp)
        idx = (c + c // st.nproma) % 3
        vals = np.array([own, own * [1.3, 0.8, 1.0, 1.1] + [0, 0, -2.0, 0], own * [0.7, 1.25, 1.0, 0.9] + [0, 0, 1.5, 0]])
    return idx, vals


def with_values(prm, row):
    p = copy.copy(prm)
    for n, v in zip(PARAM_NAMES, row):
        setattr(p, n, float(v))
    return p


def table_of(idx, vals, ngptot, scale=None):
    """(4, ncols_pad) doubles, NaN in the padded tail"""
    t = np.full((4, len(idx)), np.nan)
    t[:, :ngptot] = (vals[idx[:ngptot]] * (1.0 if scale is None else scale[:ngptot, None])).T
    return np.ascontiguousarray(t)


def cols(a, st):
    """(nblocks, nlevx, nproma) -> (nlevx, ncols_pad)"""
    return a.transpose(1, 0, 2).reshape(a.shape[1], -1)


def run_parmap(lib, prm, st, qsat, ptab, dtab, inc):
    """the three sweeps with the maps; everything they write is NaN-prefilled"""
    nb, nlev, nproma, ngptot = st.nblocks, st.nlev, st.nproma, st.ngptot
    i, _ = host_traj_blocks(st, qsat)
    out = flat_fields("out", nb, nlev, nproma, fill=np.nan)
    scratch = np.full((nb, nlev, nproma), np.nan, dtype=B.REAL)
    assert lib.hostcheck_parmap_nl(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, ptab.ctypes.data, C.byref(i), C.byref(flat_block("out", out)),
                                   scratch.ctypes.data) == 0
    tl = flat_fields("out", nb, nlev, nproma, fill=np.nan)
    assert lib.hostcheck_parmap_tl(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, int(qsat is None), ptab.ctypes.data, dtab.ctypes.data, C.byref(i),
                                   C.byref(flat_block("in", inc)), C.byref(flat_block("out", tl))) == 0
    xa = flat_fields("in", nb, nlev, nproma, fill=np.nan)
    if qsat is None:
        del xa["qsat"]
    u = {n: a.copy() for n, a in tl.items()}  # the cotangent: TL(dx, dp), NaN in its padded tail
    apar = np.full((4, nb * nproma), np.nan)
    assert lib.hostcheck_parmap_vjp(C.byref(prm), st.ptsphy, nproma, nlev, ngptot, int(qsat is None), ptab.ctypes.data, C.byref(i),
                                    C.byref(flat_block("out", out)), C.byref(flat_block("in", xa)), C.byref(flat_block("out", u)),
                                    scratch.ctypes.data, apar.ctypes.data) == 0
    for n in tl:
        assert np.array_equal(bits(u[n]), bits(tl[n])), ("output adjoint changed", n)
    return out, scratch, tl, xa, apar


@pytest.mark.parametrize("satur", [0, 1], ids=["qsat", "satur"])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True)], ids=["plain", "evap-regcl"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_distinct_maps_are_the_scalar_sweeps_column_by_column(lib, shape, flags, satur):
    tab, st = case_state(shape)
    prm = make_params(tab, **flags)
    evap = bool(prm.levapls2 or prm.ldrain1d)
    nproma, ngptot, ncp = st.nproma, st.ngptot, st.nblocks * st.nproma
    qsat = None if satur else host_qsat(st)
    inc = increments15(st) if satur else increments_of(st, qsat)
    idx, vals = value_map(prm, st, shape)
    rel = 0.01 * (1.0 + 0.5 * np.cos(idx))  # dp[c] = rel p[c], rel by value: in shape (a) a tangent of its own per column
    ptab, dtab = table_of(idx, vals, ngptot), table_of(idx, vals, ngptot, rel)
    out, scratch, tl, xa, apar = run_parmap(lib, prm, st, qsat, ptab, dtab, inc)

    active = np.arange(ncp) < ngptot
    # tails: every active element written, the padded tail untouched (PCOVPTOT's is zeroed, as its parent does)
    for what, arrays in (("out", out), ("tl", tl), ("xa", xa)):
        for n, a in arrays.items():
            c = cols(a, st)
            assert not np.any(np.isnan(c[:, active])), (what, "active element not written", n)
            if what == "out" and n == "covptot":
                assert np.all(c[:, ~active] == 0.0), "PCOVPTOT's padded tail"
            else:
                assert np.all(np.isnan(c[:, ~active])), (what, "padded tail touched", n)
    assert not np.any(np.isnan(apar[:, active])) and np.all(np.isnan(apar[:, ~active])), "adjoint table: active columns only"
    sc = cols(scratch, st)
    if evap:
        assert not np.any(np.isnan(sc[:, active])) and np.all(np.isnan(sc[:, ~active])), "cover checkpoint"
    else:
        assert np.all(np.isnan(sc)), "no cover checkpoint without the evaporation branch"

    # one scalar sweep of each kind per distinct value, taken at that value's columns
    u = {n: a.copy() for n, a in tl.items()}
    checked = 0
    for v in np.unique(idx[:ngptot]):
        at = active & (idx == v)
        c0 = int(np.flatnonzero(at)[0])
        if shape == "a":
            assert at.sum() == 1
        pv = with_values(prm, vals[v])
        fwd, scr = trajectory_for_reverse(pv, st, qsat)
        want_out = c2.op_outputs(fwd)
        for n in B.OUT_NAMES:
            assert np.array_equal(bits(np.ascontiguousarray(cols(out[n], st)[:, at])), bits(np.ascontiguousarray(cols(want_out[n], st)[:, at]))), ("output", n, v)
        if evap:
            assert np.array_equal(bits(np.ascontiguousarray(sc[:, at])), bits(np.ascontiguousarray(cols(scr, st)[:, at]))), ("cover checkpoint", v)
        want_tl = run_tl_par(pv, st, inc, dtab[:, c0], qsat)  # (the columns of a value share their tangents)
        for n in B.OUT_NAMES:
            assert np.array_equal(bits(np.ascontiguousarray(cols(tl[n], st)[:, at])), bits(np.ascontiguousarray(cols(want_tl[n], st)[:, at]))), ("tangent", n, v)
        want_xa, _, _, work = run_vjp_par(pv, st, fwd, scr, u, qsat)
        assert set(want_xa) == set(xa)
        for n in xa:
            assert np.array_equal(bits(np.ascontiguousarray(cols(xa[n], st)[:, at])), bits(np.ascontiguousarray(cols(want_xa[n], st)[:, at]))), ("field adjoint", n, v)
        assert np.array_equal(apar[:, at].view(np.int64), work[:, at].view(np.int64)), ("adjoint table against the workspace", v)
        checked += int(at.sum())
    assert checked == ngptot
    # the map reached the sweeps: columns differ from the sweep at prm's own values
    base, _ = trajectory_for_reverse(prm, st, qsat)
    assert not np.array_equal(cols(c2.op_outputs(base)["fplsl"], st)[:, active], cols(out["fplsl"], st)[:, active])
    assert np.all(np.any(apar[:3, active] != 0.0, axis=1)) and bool(np.any(apar[3, active] != 0.0)) == evap

    if not B.SINGLE:  # the dot-product identity, per column parameters included
        act3 = active.reshape(st.nblocks, 1, nproma)
        lhs = sum(float(np.sum(np.where(act3, tl[n], 0.0) ** 2)) for n in tl)
        fields = sum(float(np.sum(np.where(act3, inc[n] * xa[n], 0.0))) for n in xa)
        par = float(np.sum(dtab[:, active] * apar[:, active]))
        e, e0 = abs(lhs - (fields + par)) / abs(lhs), abs(lhs - fields) / abs(lhs)
        print(f"{shape} {flags} satur={satur}: identity {e:.3e}, without the parameter term {e0:.3e}")
        assert e <= 1e-12, (lhs, fields + par)
        assert e0 > 1e-9, "the parameter term must matter to the identity"


@fp64_only
def test_the_module_in_the_fp32_build():
    """this module once more with CLOUDSC2_PRECISION=single: one child, one time limit, no retry"""
    env = dict(os.environ, CLOUDSC2_PRECISION="single")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_hostcheck_parmap.py"), "-q", "-p", "no:cacheprovider",
                        "-m", "not gpu"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    lines = p.stdout.splitlines()
    print("\n".join(lines[-10:]))
    assert p.returncode == 0, (p.returncode, p.stdout[-6000:], p.stderr[-2000:])
    last = lines[-1] if lines else ""
    assert " passed" in last and "failed" not in last and "error" not in last, last
