"""The column-sum sweeps (nl_column / tl_column / ad_reverse_column with C2F_COLSUM: what cloudsc2_nl_launch_colsum,
cloudsc2_tl_launch_colsum and cloudsc2_vjp_launch_colsum run) compiled for the HOST against the dense and sparse host sweeps of the same
library.  A sum is the bits of the fold ``acc = 0; acc = fl(acc + fl(w[k] * out[k]))`` over the dense planes, done in numpy in the
library's real type; a gradient is the bits of the sparse reverse sweep fed the planes ``w[k] * ybar[c]``.  Absent sums, gradients and
tangents are NULL pointers, and the lean forward is given no output plane at all: a missing guard is a segmentation fault here, on
the CPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests.host_sweeps import HALF, fold, table_of, weight_patterns
from tests.hostbuild import host_lib, precise  # noqa: F401
from tests.sparse_patterns import NARROW, in_names
from tests.util import B, c2, flat_block, flat_fields, host_qsat, host_traj_blocks, increments_of, make_params, same_bits


def sums_block(names, nb: int, nproma: int, fill=np.nan):
    arrays = {n: np.full((nb, nproma), fill, dtype=B.REAL) for n in names}
    return arrays, flat_block("out", arrays)


def check_sums(got: dict, want: dict, nproma: int, ngptot: int, what) -> None:
    nb = next(iter(got.values())).shape[0]
    for n, g in got.items():
        for ibl in range(nb):
            icend = min(nproma, ngptot - ibl * nproma)
            assert not np.any(np.isnan(g[ibl, :icend])), (what, n, "an active sum was not written")
            assert same_bits(g[ibl, :icend], want[n][ibl, :icend]), (what, n, "differs from the fold over the planes")
            assert np.all(np.isnan(g[ibl, icend:])), (what, n, "the padded tail was touched")


def tangent_masks(satur: bool) -> list:
    ins = in_names(satur)
    rng = np.random.default_rng(20261021 + int(satur))
    return [ins, NARROW[0], (), ("paph", "lu"), tuple(n for n in ins if rng.random() < 0.4) or ("t",)]


@pytest.mark.parametrize("satur", [False, True], ids=["qsat", "satur"])
@pytest.mark.parametrize("flags", [dict(), dict(levapls2=True, lregcl=True), dict(ldrain1d=True), dict(lregcl=True)])
def test_column_sums_are_the_fold_over_the_planes(precise, flags, satur):
    nlev, nproma, ngptot = 137, 16, 30
    tab = c2.random_table(nlev, 30, seed=11)
    prm = make_params(tab, **flags)
    evap = bool(flags.get("levapls2") or flags.get("ldrain1d"))
    st = c2.state_from_table(tab, nproma, ngptot)
    nb = st.nblocks
    qsat = None if satur else host_qsat(st)
    ins = in_names(satur)
    lib = host_lib("colsum")
    geom = (C.byref(prm), st.ptsphy, nproma, nlev, ngptot)
    active = (np.arange(nb * nproma) < ngptot).reshape(nb, nproma)

    # the dense forward: the ten planes, and what the reverse sweep re-reads
    traj = st.copy()
    i, o = host_traj_blocks(traj, qsat)
    scratch = np.zeros((nb, nlev, nproma), dtype=B.REAL)
    assert lib.hostcheck_sparse_forward(*geom, C.byref(i), C.byref(o), scratch.ctypes.data) == 0
    S = nproma * nlev
    planes = {n: np.ascontiguousarray(a, dtype=B.REAL) for n, a in c2.op_outputs(traj).items()}
    assert planes["tent"].shape == (nb, nlev, nproma) and planes["fplsl"].shape == (nb, nlev + 1, nproma) and S

    inc = increments_of(st, host_qsat(st))  # v = 0.01 x
    rng = np.random.default_rng(20261022)
    ybar_all = {n: rng.uniform(-1.0, 1.0, (nb, nproma)).astype(B.REAL) for n in B.OUT_NAMES}

    for wname, weights in weight_patterns(nlev):
        table = table_of(weights, nlev)
        names = tuple(weights)
        want = {n: fold(weights[n], planes[n]) for n in names}

        # ---- forward, lean: no plane anywhere, a NaN-filled output block that is passed nowhere stays NaN
        bystander = flat_fields("out", nb, nlev, nproma, fill=np.nan)
        got, blk = sums_block(names, nb, nproma)
        assert lib.hostcheck_colsum_nl(*geom, C.byref(i), table.ctypes.data, C.byref(blk), None, None) == 0
        check_sums(got, want, nproma, ngptot, ("NL lean", wname))
        assert all(np.all(np.isnan(a)) for a in bystander.values())

        # ---- forward with keep: the two flux planes and the checkpoints are the trajectory pass's bits
        keep = {n: np.full((nb, nlev + 1, nproma), np.nan, dtype=B.REAL) for n in ("fplsl", "fplsn")}
        ck = np.full((nb, nlev, nproma), np.nan, dtype=B.REAL)
        got, blk = sums_block(names, nb, nproma)
        assert lib.hostcheck_colsum_nl(*geom, C.byref(i), table.ctypes.data, C.byref(blk), C.byref(flat_block("out", keep)), ck.ctypes.data) == 0
        check_sums(got, want, nproma, ngptot, ("NL keep", wname))
        for n in keep:
            assert same_bits(keep[n][active[:, None, :].repeat(nlev + 1, 1)], planes[n][active[:, None, :].repeat(nlev + 1, 1)]), (wname, n)
            assert np.all(np.isnan(keep[n][~active[:, None, :].repeat(nlev + 1, 1)])), (wname, n, "tail")
        act3 = active[:, None, :].repeat(nlev, 1)
        if evap:
            assert same_bits(ck[act3], scratch[act3]) and np.all(np.isnan(ck[~act3])), (wname, "checkpoints")
        else:
            assert np.all(np.isnan(ck)), (wname, "scratch was touched without the evaporation branch")

        # ---- TL: the sums of the sparse host TL's tangent planes
        tl_sum = {}
        for pin in tangent_masks(satur):
            din = {n: inc[n].copy() for n in pin}
            dy = flat_fields("out", nb, nlev, nproma, fill=np.nan)
            assert lib.hostcheck_sparse_tl(*geom, int(satur), 1, C.byref(i), C.byref(flat_block("in", din)), C.byref(flat_block("out", dy))) == 0
            dwant = {n: fold(weights[n], np.where(np.isnan(dy[n]), B.REAL(0), dy[n])) for n in names}
            got, blk = sums_block(names, nb, nproma)
            assert lib.hostcheck_colsum_tl(*geom, int(satur), C.byref(i), C.byref(flat_block("in", din)), table.ctypes.data, C.byref(blk)) == 0
            check_sums(got, dwant, nproma, ngptot, ("TL", wname, pin))
            for n in din:
                assert same_bits(din[n], inc[n]), ("TL changed a tangent", n)
            if pin == ins:
                tl_sum = got

        # ---- reverse: the sparse host reverse sweep fed the planes w[k] * ybar[c], zero planes for the absent sums
        ybar = {n: ybar_all[n].copy() for n in names}
        yplanes = {}
        for n in B.OUT_NAMES:
            nlevx = nlev + (1 if n in HALF else 0)
            if n in names:
                yplanes[n] = np.ascontiguousarray((weights[n][None, :, None] * ybar[n][:, None, :]).astype(B.REAL))
            else:
                yplanes[n] = np.zeros((nb, nlevx, nproma), dtype=B.REAL)
        vjp_all = {}
        for pin in [m for m in tangent_masks(satur) if m]:
            xw = {n: a for n, a in flat_fields("in", nb, nlev, nproma, fill=np.nan).items() if n in pin}
            assert lib.hostcheck_sparse_vjp(*geom, int(satur), 1, C.byref(i), C.byref(o), C.byref(flat_block("in", xw)),
                                            C.byref(flat_block("out", yplanes)), scratch.ctypes.data) == 0
            xa = {n: a for n, a in flat_fields("in", nb, nlev, nproma, fill=np.nan).items() if n in pin}
            assert lib.hostcheck_colsum_vjp(*geom, int(satur), C.byref(i), C.byref(o), C.byref(flat_block("in", xa)), table.ctypes.data,
                                            C.byref(flat_block("out", ybar)), scratch.ctypes.data) == 0
            for n in pin:
                nlevx = xa[n].shape[1]
                a3 = active[:, None, :].repeat(nlevx, 1)
                assert not np.any(np.isnan(xa[n][a3])), ("VJP", wname, n, "an active element was not written")
                assert same_bits(xa[n][a3], xw[n][a3]), ("VJP", wname, n, "differs from the sparse sweep fed the product planes")
                assert np.all(np.isnan(xa[n][~a3])), ("VJP", wname, n, "the padded tail was touched")
            for n in names:
                assert same_bits(ybar[n], ybar_all[n]), ("the reverse sweep changed a sum cotangent", n)
            if pin == ins:
                vjp_all = xa

        # ---- <ybar, TLsum(v)> = <VJPsum(ybar), v>: the bound of tests/test_hostcheck_satur_lin.py (fp64 only)
        if not B.SINGLE:
            lhs = [ybar[n][active] * tl_sum[n][active] for n in names]
            rhs = [vjp_all[n][active[:, None, :].repeat(vjp_all[n].shape[1], 1)] * inc[n][active[:, None, :].repeat(inc[n].shape[1], 1)] for n in ins]
            l, r = sum(float(x.sum()) for x in lhs), sum(float(x.sum()) for x in rhs)
            scale = sum(float(np.abs(x).sum()) for x in lhs) + sum(float(np.abs(x).sum()) for x in rhs)
            assert abs(l - r) <= 1e-12 * scale, (wname, l, r, scale)
