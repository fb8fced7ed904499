"""The column sums of an ensemble's members through the C ABI, run as a CHILD process by tests/test_gpu_autograd_enscolsum.py:
``[CLOUDSC2_OFF32=0|1] [CLOUDSC2_PRECISION=single] python tests/enscolsum_variant_checks.py OUT.npz``.

The launchers choose the addressing form of the kernels once per process (CLOUDSC2_OFF32), hence one child per form.  For the plain and
the evaporation flag set x math_mode 1 / 2 x qsat given / satur, at NPROMA 32 x 100 columns (four blocks, a padded tail of 28) and K = 3
rows (row 0 prm's own; ``t`` per member with a member stride of two states, everything else shared), cloudsc2_nl_launch_ens_colsum (lean
and with ``keep``), cloudsc2_tl_launch_ens_colsum and cloudsc2_vjp_launch_ens_colsum run next to their parents of the same process, each
parent called once per member with a host copy of prm holding that member's row:

  * member k's sums, kept flux planes and cover checkpoints are the bits of cloudsc2_nl_launch_colsum;
  * member k's field gradients are the bits of cloudsc2_vjp_launch_colsum, for all gradients, (q, t), (paph, lu) -- and for NO gradient
    plane, where only the parameter adjoints are formed;
  * row k of the parameter adjoints is the bits of cloudsc2_vjp_launch_par fed the planes ``w[k] * ybar[c]``;
  * member k's tangent sums are the bits of the torch fold (separate ``mul`` and ``add``) over cloudsc2_tl_launch_par's tangent planes,
    absent field tangents given as zero planes there;
  * absent sums and the padded tail keep their NaN prefill, what the launches read is unchanged, the launch log stays empty;
  * with a device: members x workgroups per member beyond the grid limit, and members < 1, are CLOUDSC2_EINVAL and launch nothing.

Two checksums of every compared array go to OUT.npz: the parent compares the two addressing forms.  Exit code 1 with the failures
printed if a check fails."""
from __future__ import annotations

import copy
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import offset_variant_checks as ov  # noqa: E402
from tests.colsum_variant_checks import Checks, fold, ptr, sums_blk, table_of, weight_patterns  # noqa: E402
from tests.sparse_patterns import NARROW, in_names  # noqa: E402
from tests.util import B, c2  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402

DEV = ov.DEV
FLAGSETS = (("plain", dict()), ("levapls2_lregcl", dict(levapls2=True, lregcl=True)))
MODES = (1, 2)
SHAPE = (32, 100)
NAN = float("nan")
P = c2.PARAM_NAMES
ROWS = [dict(rkconv=1.0, rclcrit=1.0, rlptrc=0.0, rpecons=1.0), dict(rkconv=1.3, rclcrit=0.8, rlptrc=-2.0, rpecons=1.1),
        dict(rkconv=0.7, rclcrit=1.25, rlptrc=1.5, rpecons=0.9)]
K = len(ROWS)
WEIGHTS = ("all", "surface", "tent,tenq")


def with_row(prm, row):
    p = copy.copy(prm)
    for n, v in zip(P, row):
        setattr(p, n, float(v))
    return p


def ens_blk(kind, ts, lay):
    b, ms = ag._ens_block(kind, ts, lay, K)
    return C.byref(b), ms


def ens_sums(ts, lay):
    b, ms = ag._ens_sums_block(ts, lay, K)
    return C.byref(b), ms


def launch(chk: Checks, key, fn, *args):
    """one call of a new launcher: it must succeed and leave the calling thread's launch log empty"""
    B.launch_log_reset()
    B.check(fn(*args))
    chk.log_empty(key)


WORST = {}  # kind -> the largest difference from the parent seen, relative to the parent's largest magnitude (printed, not asserted)


def measure(kind, got, want):
    d = (torch.nan_to_num(got) - torch.nan_to_num(want)).abs().max() / torch.nan_to_num(want).abs().max().clamp_min(1e-300)
    WORST[kind] = torch.maximum(WORST.get(kind, torch.zeros((), dtype=d.dtype, device=DEV)), d)


def per_member(shape, fill=NAN, dtype=None):
    return torch.full((K,) + tuple(shape), fill, dtype=dtype or ov.real(), device=DEV)


def run_case(chk: Checks, tag, tab, nproma, ngptot, flags, mode, satur):
    prm = c2.default_params(c2.ceta_from_table(tab), **flags)
    prm.math_mode = mode
    evap = bool(flags.get("levapls2") or flags.get("ldrain1d"))
    st = c2.state_from_table(tab, nproma, ngptot)
    lay = ag.Layout(st.nblocks, st.nlev, nproma, ngptot)
    nlev = lay.nlev
    ptsphy = float(st.ptsphy)
    G = ov.geom(prm, ptsphy, lay)
    flat = {n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in c2.op_inputs(st).items()}
    flat["qsat"] = ag.satur(flat["pap"], flat["t"], prm, ngptot)
    ins = in_names(satur)
    x = ov.packed("in", ins, lay, values=flat)
    dx = ov.packed("in", ins, lay, values=ov.seeded(B.IN_NAMES, lay, 100, scale=flat))
    rows = [[getattr(prm, n) + r[n] if n == "rlptrc" else getattr(prm, n) * r[n] for n in P] for r in ROWS]
    drows = [[0.01 * rows[k][j] * (1.0 + 0.5 * k) for j in range(len(P))] for k in range(K)]
    ptab = torch.tensor(rows, dtype=torch.float64, device=DEV)
    dptab = torch.tensor(drows, dtype=torch.float64, device=DEV)
    prms = [with_row(prm, rows[k]) for k in range(K)]
    for p in prms:
        p.math_mode = mode
    # t and its tangent: one state per member, views with a member stride of two states (NaN between them)
    tbuf, dtbuf = per_member((2,) + lay.shape("t")), per_member((2,) + lay.shape("t"))
    for k in range(K):
        tbuf[k, 1] = x["t"] * (1.0 + 5e-4 * k)
        dtbuf[k, 1] = dx["t"] * (1.0 + 0.25 * k)
    t4, dt4 = tbuf[:, 1], dtbuf[:, 1]
    xe = dict(x, t=t4)
    xk = [dict(x, t=t4[k]) for k in range(K)]
    work = ag._ens_workspace(K, lay, DEV)
    xb, xm = ens_blk("in", xe, lay)
    g = torch.Generator(device=DEV).manual_seed(300)
    ybar_all = {n: torch.randn((K, lay.nblocks, lay.nproma), generator=g, dtype=ov.real(), device=DEV) for n in B.OUT_NAMES}
    before = {k: {n: t.clone() for n, t in d.items()} for k, d in (("x", xe), ("dx", dx), ("ybar", ybar_all))}
    # every member's dense trajectory pass: what the parents' reverse sweeps re-read
    trajs = [ov.ad_forward(xk[k], prms[k], ptsphy, lay) for k in range(K)]
    masks = (ins, NARROW[0], ("paph", "lu"), ())

    for wname, weights in [w for w in weight_patterns(nlev) if w[0] in WEIGHTS]:
        table, names = table_of(weights, nlev), tuple(weights)
        key = f"{tag}.{wname}"
        # ---- NL: lean, then with keep
        for keep in (False, True):
            got = {n: per_member((lay.nblocks, lay.nproma)) for n in names}
            kept = {n: per_member(lay.shape(n)) for n in ("fplsl", "fplsn")}
            ck = per_member((lay.nblocks, lay.nlev, lay.nproma))
            sb, sm = ens_sums(got, lay)
            kb, km = ens_blk("out", kept, lay)
            launch(chk, f"{key}.nl", B.lib.cloudsc2_nl_launch_ens_colsum, *G, K, ptr(ptab), xb, xm, ptr(table), sb, sm, kb if keep else None,
                   km if keep else None, ptr(ck) if keep else None, ck.stride(0), ptr(work), ov.stream())
            for k in range(K):
                want = {n: torch.full((lay.nblocks, lay.nproma), NAN, dtype=ov.real(), device=DEV) for n in names}
                wkept = {n: torch.full(lay.shape(n), NAN, dtype=ov.real(), device=DEV) for n in kept}
                wck = ov.scratch_of(lay)
                GK = ov.geom(prms[k], ptsphy, lay)
                B.check(B.lib.cloudsc2_nl_launch_colsum(*GK, ov.blk("in", xk[k], lay), ptr(table), sums_blk(want, lay),
                                                        ov.blk("out", wkept, lay) if keep else None, ptr(wck) if keep else None, ov.stream()))
                what = "keep" if keep else "nl"
                for n in names:
                    chk.array(f"{key}.{what}.m{k}.{n}", got[n][k], want[n], lay)
                    if not keep:  # ... which are the fold over the member's dense planes
                        chk.array(f"{key}.fold.m{k}.{n}", got[n][k], fold(weights[n], trajs[k][0][n]), lay)
                if keep:
                    for n in kept:
                        chk.array(f"{key}.keep.plane.m{k}.{n}", kept[n][k], wkept[n], lay)
                    if evap:
                        chk.array(f"{key}.keep.scratch.m{k}", ck[k], wck, lay)
            if not keep:
                chk.untouched(f"{key}.nl.kept planes", torch.stack(list(kept.values())))
            if not (keep and evap):
                chk.untouched(f"{key}.{'keep' if keep else 'nl'}.scratch", ck)
        # ---- TL: the fold over the parameter TL launch's tangent planes (absent field tangents: zero planes there)
        for pin in masks:
            dxe = {n: (dt4 if n == "t" else dx[n]) for n in pin}
            got = {n: per_member((lay.nblocks, lay.nproma)) for n in names}
            sb, sm = ens_sums(got, lay)
            db, dm = ens_blk("in", dxe, lay)
            launch(chk, f"{key}.tl", B.lib.cloudsc2_tl_launch_ens_colsum, *G, int(satur), K, ptr(ptab), ptr(dptab), xb, xm, db, dm, ptr(table),
                   sb, sm, ptr(work), ov.stream())
            for k in range(K):
                dk = {n: ((dt4[k] if n == "t" else dx[n]) if n in pin else torch.zeros_like(x[n])) for n in ins}
                dy = ov.tl_par(xk[k], dk, drows[k], prms[k], ptsphy, lay, int(satur))
                for n in names:
                    chk.array(f"{key}.tl.{'+'.join(pin) if len(pin) < 3 else 'all'}.m{k}.{n}", got[n][k], fold(weights[n], torch.nan_to_num(dy[n])), lay)
        # ---- reverse sweep: the field gradients of the column-sum parent, the parameter adjoints of the parameter parent
        ybar = {n: ybar_all[n] for n in names}
        yb, ym = ens_sums(ybar, lay)
        fluxes = {n: torch.stack([trajs[k][0][n] for k in range(K)]) for n in ("fplsl", "fplsn")}
        sc4 = torch.stack([trajs[k][1] for k in range(K)])
        fb, fm = ens_blk("out", fluxes, lay)
        par_want = []
        for k in range(K):
            yplanes = {n: (torch.mul(weights[n][None, :, None], ybar[n][k][:, None, :]).contiguous() if n in names
                           else torch.zeros(lay.shape(n), dtype=ov.real(), device=DEV)) for n in B.OUT_NAMES}
            par_want.append(ov.vjp_par(xk[k], trajs[k][0], trajs[k][1], yplanes, prms[k], ptsphy, lay, int(satur))[2])
        for pin in masks:
            got_x = {n: per_member(lay.shape(n)) for n in pin}
            par_adj = per_member((len(P),), dtype=torch.float64)
            ab, am = ens_blk("in", got_x, lay)
            launch(chk, f"{key}.vjp", B.lib.cloudsc2_vjp_launch_ens_colsum, *G, int(satur), K, ptr(ptab), xb, xm, fb, fm, ab, am, ptr(table),
                   yb, ym, ptr(sc4), sc4.stride(0), ptr(work), ptr(par_adj), ov.stream())
            pname = "+".join(pin) if 0 < len(pin) < 3 else ("all" if pin else "none")
            for k in range(K):
                if pin:
                    want_x = ov.packed("in", pin, lay)
                    GK = ov.geom(prms[k], ptsphy, lay)
                    B.check(B.lib.cloudsc2_vjp_launch_colsum(*GK, int(satur), ov.blk("in", xk[k], lay), ov.blk("out", trajs[k][0], lay),
                                                             ov.blk("in", want_x, lay), ptr(table),
                                                             sums_blk({n: ybar[n][k] for n in names}, lay), ptr(trajs[k][1]), ov.stream()))
                    for n in pin:
                        measure("reverse sweep, field gradients", got_x[n][k], want_x[n])
                        chk.array(f"{key}.vjp.{pname}.m{k}.{n}", got_x[n][k], want_x[n], lay)
                measure("reverse sweep, parameter adjoints", par_adj[k], par_want[k])
                chk.flags.append((f"{key}.vjp.{pname}.m{k}.par_adj", (par_adj[k].view(torch.int64) == par_want[k].view(torch.int64)).all()))
                chk.keys.append(f"{key}.vjp.{pname}.m{k}.par_adj")
                chk.sums.append(torch.stack((par_adj[k].view(torch.int64).sum(), par_adj[k].view(torch.int64)[0])))
    for k, d in (("x", xe), ("dx", dx), ("ybar", ybar_all)):
        chk.unchanged(f"{tag}.{k}", d, before[k])
    chk.finish()


def refusals_with_a_device(chk: Checks, tab):
    """nothing may launch: the pointers are those of a 100-column state"""
    prm = c2.default_params(c2.ceta_from_table(tab))
    st = c2.state_from_table(tab, 128, 128)
    lay = ag.Layout(st.nblocks, st.nlev, 128, 128)
    x = {n: torch.zeros(lay.shape(n), dtype=ov.real(), device=DEV) for n in B.IN_NAMES}
    table = torch.ones((10, lay.nlev + 1), dtype=ov.real(), device=DEV)
    sums = {"fplsl": torch.zeros((K, 1, 128), dtype=ov.real(), device=DEV)}
    ptab = torch.ones((K, 4), dtype=torch.float64, device=DEV)
    work = ag._ens_workspace(K, lay, DEV)
    sb, sm = ens_sums(sums, lay)
    xb, xm = ens_blk("in", x, lay)
    big = 128 * 32769  # 32769 workgroups per member x 65535 members: one past the grid limit
    for members, ngptot, text in ((65535, big, b"cloudsc2_nl_launch_ens_colsum: ensemble: members x workgroups per member exceeds the grid limit"),
                                  (0, 128, b"cloudsc2_nl_launch_ens_colsum: ensemble: 1 <= members <= 65535 required")):
        rc = B.lib.cloudsc2_nl_launch_ens_colsum(C.byref(prm), float(st.ptsphy), 128, lay.nlev, ngptot, members, ptr(ptab), xb, xm, ptr(table),
                                                 sb, sm, None, None, None, 0, ptr(work), ov.stream())
        if rc != B.CLOUDSC2_EINVAL or B.lib.cloudsc2_last_error() != text:
            chk.failed.append(f"refusal with a device: members {members}, ngptot {ngptot}: {rc}, {B.lib.cloudsc2_last_error()!r}")


def main(path: str) -> int:
    assert B.device_available(), "no HIP device"
    tab = c2.random_table(137, 100, seed=21)  # non-zero supsat
    chk = Checks()
    refusals_with_a_device(chk, tab)
    cases = [(f"n{SHAPE[0]}x{SHAPE[1]}.m{mode}.{fname}.{'satur' if satur else 'qsat'}", *SHAPE, flags, mode, satur)
             for fname, flags in FLAGSETS for mode in MODES for satur in (False, True)]
    for tag, nproma, ngptot, flags, mode, satur in cases:
        run_case(chk, tag, tab, nproma, ngptot, flags, mode, satur)
    np.savez(path, keys=np.array(chk.keys), sums=torch.stack(chk.sums).cpu().numpy(), cases=np.array([c[0] for c in cases]),
             failed=np.array(chk.failed, dtype=str))
    print(f"{len(cases)} cases, {len(chk.keys)} arrays compared, CLOUDSC2_OFF32={os.environ.get('CLOUDSC2_OFF32')}")
    for kind, d in WORST.items():
        print(f"largest difference from the parent launcher, relative to the parent's largest magnitude: {kind}: {float(d):.3e}")
    if chk.failed:
        print(f"{len(chk.failed)} failures:", *chk.failed[:60], sep="\n  ")
    return 1 if chk.failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
