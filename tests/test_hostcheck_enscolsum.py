"""The column sums of an ensemble's members (nl_column / tl_column / ad_reverse_column with C2F_MEMBER, and C2F_PARLIN together with
C2F_SPARSE | C2F_COLSUM: what cloudsc2_nl_launch_ens_colsum, cloudsc2_tl_launch_ens_colsum and cloudsc2_vjp_launch_ens_colsum run)
compiled for the HOST against their twins of the same library, member by member, every comparison bit for bit:

  sums                 the numpy fold ``acc = 0; acc = fl(acc + fl(w[k] * out[k]))`` over the dense planes of a run with row k's parameters;
  field gradients      the column-sum reverse sweep (hostcheck_colsum_vjp) with row k's parameters;
  parameter adjoints   ``ad_reverse_column<PARLIN>`` (hostcheck_vjp_par) fed the planes ``w[k] * ybar[c]``: every column's four sums and
                       their total;
  parameter tangents   ``tl_column<PARLIN>`` (hostcheck_tl_par) with zero planes for the absent tangents, folded.

The members' blocks are made by ``ens_member_args`` for K = 3 distinct rows (row 0 is prm's own); ``t`` is per member with a member stride
of two states, every other input is shared.  Masks are those of tests/sparse_patterns.py and, for the reverse sweep, the EMPTY gradient
mask with the parameter adjoints wanted.  Absent planes are NULL, written planes are NaN-prefilled."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest

from tests.host_sweeps import HALF, fold, table_of, weight_patterns
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.sparse_patterns import in_names, patterns
from tests.util import FLAGS, B, c2, flat_block, flat_fields, hfld, host_qsat, make_params, same_bits

PAR = ("rkconv", "rclcrit", "rlptrc", "rpecons")
# factors / offsets on prm's values (rlptrc: an offset in K): row 0 is prm's own
ROWS = [dict(rkconv=1.0, rclcrit=1.0, rlptrc=0.0, rpecons=1.0), dict(rkconv=1.3, rclcrit=0.8, rlptrc=-2.0, rpecons=1.1),
        dict(rkconv=0.7, rclcrit=1.25, rlptrc=1.5, rpecons=0.9)]
K = len(ROWS)


def flat_inputs(st, qsat) -> dict:
    return {n: np.ascontiguousarray(a, dtype=B.REAL) for n, a in c2.op_inputs(st, qsat).items()}


def with_row(prm, row):
    p = copy.copy(prm)
    for n, v in zip(PAR, row):
        setattr(p, n, float(v))
    return p


def member_block(kind: str, arrays: dict):
    """``arrays``: name -> (K, nb, nlevx, nproma) or (K, nb, nproma) contiguous, or a view of a larger buffer along axis 0; returns member
    0's block and the member strides in elements (shared 3-D / 2-D arrays of ``flat`` shape: stride 0)"""
    names = B.IN_NAMES if kind == "in" else B.OUT_NAMES
    blk = B.Inputs() if kind == "in" else B.Outputs()
    ms = (C.c_longlong * len(names))()
    for n, (a, per_member) in arrays.items():
        if per_member:
            f = B.Field()
            f.ptr = a[0].ctypes.data
            f.block_stride = int(np.prod(a.shape[2:]))
            assert a[0].flags["C_CONTIGUOUS"] and a.strides[0] % a.itemsize == 0
            setattr(blk, n, f)
            ms[names.index(n)] = a.strides[0] // a.itemsize
        else:
            setattr(blk, n, hfld(a))
    return blk, ms


def shared(arrays: dict) -> dict:
    return {n: (a, False) for n, a in arrays.items()}


def own(arrays: dict) -> dict:
    return {n: (a, True) for n, a in arrays.items()}


def active_mask(nb, nproma, ngptot, nlevx=None):
    a = (np.arange(nb * nproma) < ngptot).reshape(nb, nproma)
    return a if nlevx is None else a[:, None, :].repeat(nlevx, 1)


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "levapls2+lregcl", "ldrain1d", "lregcl"])
def test_members_are_the_bits_of_their_twins(precise, flags, satur):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)
    prm = make_params(tab, **flags)
    evap = bool(flags.get("levapls2") or flags.get("ldrain1d"))
    st = c2.state_from_table(tab, nproma, ngptot)
    nb = st.nblocks
    np_pad = nb * nproma
    lib, plib = host_lib("enscolsum"), host_lib("par")
    geom = lambda p: (C.byref(p), st.ptsphy, nproma, nlev, ngptot)  # noqa: E731
    ins = in_names(satur)
    x = flat_inputs(st, None if satur else host_qsat(st))
    x = {n: x[n] for n in ins}
    act = active_mask(nb, nproma, ngptot)
    rows = np.array([[getattr(prm, n) + r[n] if n == "rlptrc" else getattr(prm, n) * r[n] for n in PAR] for r in ROWS], dtype=np.float64)
    drows = np.array([[0.01 * rows[k, j] * (1.0 + 0.5 * k) for j in range(4)] for k in range(K)], dtype=np.float64)
    prms = [with_row(prm, rows[k]) for k in range(K)]
    pd = lambda a: a.ctypes.data  # noqa: E731

    # t: one state per member, a view with a member stride of two states (NaN between them); everything else shared
    tbuf = np.full((K, 2) + x["t"].shape, np.nan, dtype=B.REAL)
    for k in range(K):
        tbuf[k, 1] = x["t"] * B.REAL(1.0 + 5e-4 * k)
    t4 = tbuf[:, 1]
    xin = dict(shared({n: a for n, a in x.items() if n != "t"}), t=(t4, True))
    xb, xm = member_block("in", xin)
    xk = [dict(x, t=np.ascontiguousarray(t4[k])) for k in range(K)]
    all_shared_b, _ = member_block("in", shared(x))

    # ---- every member's dense run: the ten planes, the cover checkpoints
    planes, scratch = [], []
    for k in range(K):
        o = flat_fields("out", nb, nlev, nproma, fill=np.nan)
        sc = np.zeros((nb, nlev, nproma), dtype=B.REAL)
        assert lib.hostcheck_sparse_forward(*geom(prms[k]), C.byref(flat_block("in", xk[k])), C.byref(flat_block("out", o)), pd(sc)) == 0
        planes.append(o)
        scratch.append(sc)
    assert not same_bits(planes[0]["fplsl"], planes[1]["fplsl"]), "the rows do not differ in their outputs"

    # ---- forward: lean and with keep, for every weight pattern; once with every input shared
    for wname, weights in weight_patterns(nlev):
        table = table_of(weights, nlev)
        names = tuple(weights)
        for keep in (False, True):
            sums = {n: np.full((K, nb, nproma), np.nan, dtype=B.REAL) for n in names}
            sb, sm = member_block("out", own(sums))
            kept = {n: np.full((K, nb, nlev + 1, nproma), np.nan, dtype=B.REAL) for n in ("fplsl", "fplsn")}
            ck = np.full((K, nb, nlev, nproma), np.nan, dtype=B.REAL)
            kb, km = member_block("out", own(kept))
            assert lib.hostcheck_enscolsum_nl(*geom(prm), K, pd(rows), C.byref(xb), xm, pd(table), C.byref(sb), sm,
                                              C.byref(kb) if keep else None, km if keep else None, pd(ck) if keep else None,
                                              ck[0].size) == 0
            for k in range(K):
                for n in names:
                    want = fold(weights[n], planes[k][n])
                    assert not np.any(np.isnan(sums[n][k][act])), (wname, keep, k, n, "an active sum was not written")
                    assert same_bits(sums[n][k][act], want[act]), (wname, keep, k, n)
                    assert np.all(np.isnan(sums[n][k][~act])), (wname, keep, k, n, "the padded tail was touched")
                a3 = active_mask(nb, nproma, ngptot, nlev + 1)
                for n in kept:
                    if keep:
                        assert same_bits(kept[n][k][a3], planes[k][n][a3]) and np.all(np.isnan(kept[n][k][~a3])), (wname, k, n)
                    else:
                        assert np.all(np.isnan(kept[n])), (wname, n, "the lean form touched a plane")
                a3 = active_mask(nb, nproma, ngptot, nlev)
                if keep and evap:
                    assert same_bits(ck[k][a3], scratch[k][a3]) and np.all(np.isnan(ck[k][~a3])), (wname, k, "checkpoints")
                else:
                    assert np.all(np.isnan(ck)), (wname, "the cover checkpoints were touched")
    # every input shared: members differ by their rows alone
    wname, weights = weight_patterns(nlev)[0]
    table, names = table_of(weights, nlev), tuple(weights)
    sums = {n: np.full((K, nb, nproma), np.nan, dtype=B.REAL) for n in names}
    sb, sm = member_block("out", own(sums))
    assert lib.hostcheck_enscolsum_nl(*geom(prm), K, pd(rows), C.byref(all_shared_b), None, pd(table), C.byref(sb), sm, None, None, None, 0) == 0
    o0 = flat_fields("out", nb, nlev, nproma, fill=np.nan)
    sc0 = np.zeros((nb, nlev, nproma), dtype=B.REAL)
    assert lib.hostcheck_sparse_forward(*geom(prms[2]), C.byref(flat_block("in", x)), C.byref(flat_block("out", o0)), pd(sc0)) == 0
    for n in names:
        assert same_bits(sums[n][0][act], fold(weights[n], planes[0][n])[act]), ("shared", n)  # (member 0's t is the shared one)
        assert same_bits(sums[n][2][act], fold(weights[n], o0[n])[act]), ("shared", n)

    # ---- what the reverse sweeps re-read, per member: PFPLSL5 / PFPLSN5 and the checkpoints
    flux = {n: np.ascontiguousarray(np.stack([planes[k][n] for k in range(K)])) for n in ("fplsl", "fplsn")}
    fb, fm = member_block("out", own(flux))
    sc4 = np.ascontiguousarray(np.stack(scratch))
    allw = weight_patterns(nlev)[0][1]
    rng = np.random.default_rng(20261023)
    ybar_all = {n: rng.uniform(-1.0, 1.0, (K, nb, nproma)).astype(B.REAL) for n in B.OUT_NAMES}

    # ---- reverse sweep: the patterns of the sparse sweeps and the empty gradient mask
    pats = patterns(satur, nrandom=3) + [("parameters only", (), tuple(B.OUT_NAMES)), ("parameters only, surface", (), ("fplsl", "fplsn"))]
    par_ref: dict = {}
    for pname, pin, pout in pats:
        weights = {n: allw[n] for n in pout}
        table = table_of(weights, nlev)
        ybar = {n: ybar_all[n].copy() for n in pout}
        yb, ym = member_block("out", own(ybar))
        xa = {n: np.full((K,) + x[n].shape, np.nan, dtype=B.REAL) for n in pin}
        ab, am = member_block("in", own(xa))
        work = np.full((K, 4, np_pad), np.nan)
        par_adj = np.full((K, 4), np.nan)
        assert lib.hostcheck_enscolsum_vjp(*geom(prm), int(satur), K, pd(rows), C.byref(xb), xm, C.byref(fb), fm, C.byref(ab), am, pd(table),
                                           C.byref(yb), ym, pd(sc4), sc4[0].size, pd(work), pd(par_adj)) == 0
        for n in pout:
            assert same_bits(ybar[n], ybar_all[n]), (pname, "the reverse sweep changed a sum cotangent", n)
        for k in range(K):
            ok = flat_block("out", {n: flux[n][k] for n in flux})
            # field gradients: the column-sum reverse sweep with row k's parameters
            if pin:
                xw = {n: np.full(x[n].shape, np.nan, dtype=B.REAL) for n in pin}
                assert lib.hostcheck_colsum_vjp(*geom(prms[k]), int(satur), C.byref(flat_block("in", xk[k])), C.byref(ok),
                                                C.byref(flat_block("in", xw)), pd(table),
                                                C.byref(flat_block("out", {n: ybar[n][k] for n in pout})), pd(scratch[k])) == 0
                for n in pin:
                    a3 = active_mask(nb, nproma, ngptot, x[n].shape[1])
                    assert not np.any(np.isnan(xa[n][k][a3])), (pname, k, n, "an active element was not written")
                    assert same_bits(xa[n][k][a3], xw[n][a3]), (pname, k, n, "differs from the column-sum reverse sweep")
                    assert np.all(np.isnan(xa[n][k][~a3])), (pname, k, n, "the padded tail was touched")
            # parameter adjoints: the dense parameter form fed the planes w[k] * ybar[c]
            if (pout, k) not in par_ref:
                yplanes = {}
                for n in B.OUT_NAMES:
                    nlevx = nlev + (1 if n in HALF else 0)
                    yplanes[n] = (np.ascontiguousarray((weights[n][None, :, None] * ybar[n][k][:, None, :]).astype(B.REAL)) if n in pout
                                  else np.zeros((nb, nlevx, nproma), dtype=B.REAL))
                xd = {n: np.full(x[n].shape, np.nan, dtype=B.REAL) for n in ins}
                w1 = np.full((4, np_pad), np.nan)
                p1 = (C.c_double * 4)(*[np.nan] * 4)
                assert plib.hostcheck_vjp_par(*geom(prms[k]), int(satur), C.byref(flat_block("in", xk[k])), C.byref(ok),
                                              C.byref(flat_block("in", xd)), C.byref(flat_block("out", yplanes)), pd(scratch[k]),
                                              pd(w1), p1) == 0
                par_ref[(pout, k)] = (w1, np.array(p1[:]))
            w1, p1 = par_ref[(pout, k)]
            cols = np.arange(np_pad) < ngptot
            assert not np.any(np.isnan(work[k][:, cols])), (pname, k, "a column's parameter sums were not written")
            assert np.array_equal(work[k][:, cols].view(np.int64), w1[:, cols].view(np.int64)), (pname, k, "per-column parameter sums")
            assert np.all(np.isnan(work[k][:, ~cols])), (pname, k, "the padded tail of the workspace was touched")
            assert np.array_equal(par_adj[k].view(np.int64), p1.view(np.int64)), (pname, k, par_adj[k], p1)
        if not evap:
            assert np.all(par_adj[:, 3] == 0), "without the evaporation branch nothing depends on rpecons"
    assert any(np.any(p != 0) for _, p in par_ref.values())

    # ---- TL: the parameter tangents' source terms with absent field tangents
    inc = {n: np.ascontiguousarray(a * B.REAL(0.01)) for n, a in x.items()}
    dt4 = np.ascontiguousarray(np.stack([inc["t"] * B.REAL(1.0 + 0.25 * k) for k in range(K)]))
    for pname, pin, pout in patterns(satur, tl=True, nrandom=2):
        weights = {n: allw[n] for n in pout}
        table = table_of(weights, nlev)
        din = {n: ((dt4, True) if n == "t" else (inc[n], False)) for n in pin}
        db, dm = member_block("in", din)
        dsums = {n: np.full((K, nb, nproma), np.nan, dtype=B.REAL) for n in pout}
        sb, sm = member_block("out", own(dsums))
        assert lib.hostcheck_enscolsum_tl(*geom(prm), int(satur), K, pd(rows), pd(drows), C.byref(xb), xm, C.byref(db), dm, pd(table),
                                          C.byref(sb), sm) == 0
        for k in range(K):
            dk = {n: (np.ascontiguousarray(dt4[k]) if n == "t" else inc[n]) if n in pin else np.zeros_like(x[n]) for n in ins}
            dy = flat_fields("out", nb, nlev, nproma, fill=np.nan)
            dp = (C.c_double * 4)(*drows[k])
            assert plib.hostcheck_tl_par(*geom(prms[k]), int(satur), C.byref(flat_block("in", xk[k])), C.byref(flat_block("in", dk)), dp,
                                         C.byref(flat_block("out", dy))) == 0
            for n in pout:
                want = fold(weights[n], np.where(np.isnan(dy[n]), B.REAL(0), dy[n]))
                assert not np.any(np.isnan(dsums[n][k][act])), (pname, k, n, "an active tangent sum was not written")
                assert same_bits(dsums[n][k][act], want[act]), (pname, k, n, "differs from the fold over the parameter TL's planes")
                assert np.all(np.isnan(dsums[n][k][~act])), (pname, k, n, "the padded tail was touched")


def test_the_new_locate_function_is_a_bijection_onto_members_and_columns():
    members, wgs, block = 5, 3, 128
    m = np.empty(members * wgs * block, dtype=np.uint32)
    c = np.empty(members * wgs * block, dtype=np.int64)
    host_lib("enscolsum").hostcheck_enscolsum_locate(members, wgs, block, m.ctypes.data, c.ctypes.data)
    pairs = set(zip(m.tolist(), c.tolist()))
    assert pairs == {(k, j) for k in range(members) for j in range(wgs * block)}
    m = m.reshape(members * wgs, block)
    assert np.all(m == m[:, :1]), "a workgroup spans two members"
    assert np.all(np.diff(c.reshape(members * wgs, block), axis=1) == 1), "the lanes of a workgroup do not hold consecutive columns"
