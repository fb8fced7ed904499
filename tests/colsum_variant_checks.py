"""The column-sum sweeps through the C ABI, run as a CHILD process by tests/test_gpu_autograd_colsum.py:
``[CLOUDSC2_OFF32=0|1] [CLOUDSC2_PRECISION=single] python tests/colsum_variant_checks.py OUT.npz [small]``.

The launchers choose the addressing form of the kernels once per process (CLOUDSC2_OFF32), hence one child per form.  For the plain and
the evaporation flag set x math_mode 1 / 2 x qsat given / satur, at NPROMA 32 x 100 columns (four blocks, a padded tail of 28), and for
one case at NPROMA 128 x 128 columns (no tail; not with ``small``), cloudsc2_nl_launch_colsum (lean and with ``keep``),
cloudsc2_tl_launch_colsum and cloudsc2_vjp_launch_colsum run next to the dense / sparse launchers of the same process:

  * a sum is the bits of ``acc = 0; acc = acc + w[k] * plane[k]`` done with separate torch ``mul`` and ``add`` over the dense forward's
    planes (TL: over the sparse TL launch's tangent planes); absent sums and the padded tail keep their NaN prefill;
  * with ``keep`` the two flux planes and the cover checkpoints are the trajectory pass's bits, without the evaporation branch the
    scratch plane is untouched;
  * a gradient is the bits of cloudsc2_vjp_launch_sparse fed the planes ``w[k] * ybar[c]``; the sum cotangents are unchanged;
  * what the launches read is unchanged and the calling thread's launch log stays empty.

Two checksums of every compared array go to OUT.npz: the parent compares the two addressing forms.  Exit code 1 with the failures
printed if a check fails."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import offset_variant_checks as ov  # noqa: E402
from tests.sparse_patterns import NARROW, in_names  # noqa: E402
from tests.sparse_variant_checks import tl_sparse, vjp_sparse  # noqa: E402
from tests.util import B, c2  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402

DEV = ov.DEV
FLAGSETS = (("plain", dict()), ("levapls2_lregcl", dict(levapls2=True, lregcl=True)))
MODES = (1, 2)
SHAPE, SHAPE2 = (32, 100), (128, 128)
INT = torch.int32 if B.SINGLE else torch.int64
NAN = float("nan")


def weight_patterns(nlev: int) -> list:
    """as in tests/test_hostcheck_colsum.py: all ten (negative entries, exact zeros, both ends non-zero), the surface fluxes, tent and
    tenq, covptot alone"""
    rng = np.random.default_rng(20261020)
    a = {}
    for n in B.OUT_NAMES:
        nlevx = nlev + (1 if n in ag.HALF_OUT else 0)
        w = rng.uniform(-1.0, 1.0, nlevx)
        w[rng.random(nlevx) < 0.2] = 0.0
        w[0], w[-1] = -0.75, 0.625
        a[n] = torch.from_numpy(w.astype(B.REAL)).to(DEV)
    surface = torch.zeros(nlev + 1, dtype=ov.real(), device=DEV)
    surface[-1] = 1.0
    return [("all", a), ("surface", {"fplsl": surface, "fplsn": surface.clone()}), ("tent,tenq", {n: a[n] for n in ("tent", "tenq")}),
            ("covptot", {"covptot": a["covptot"]})]


def table_of(weights: dict, nlev: int) -> torch.Tensor:
    t = torch.full((len(B.OUT_NAMES), nlev + 1), NAN, dtype=ov.real(), device=DEV)  # (rows and entries that must not be read: NaN)
    for n, w in weights.items():
        t[B.OUT_NAMES.index(n), :len(w)] = w
    return t


def fold(w: torch.Tensor, plane: torch.Tensor) -> torch.Tensor:
    acc = torch.zeros((plane.shape[0], plane.shape[2]), dtype=plane.dtype, device=DEV)
    for k in range(plane.shape[1]):
        acc = torch.add(acc, torch.mul(plane[:, k, :], w[k]))
    return acc


def sums_of(names, lay) -> dict:
    return {n: torch.full((lay.nblocks, lay.nproma), NAN, dtype=ov.real(), device=DEV) for n in names}


def sums_blk(ts: dict, lay):
    return C.byref(ag._sums_block(ts, lay))


def ptr(t):
    return C.c_void_p(t.data_ptr())


class Checks:
    """device-side verdicts of one case, read once at its end"""

    def __init__(self):
        self.flags, self.sums, self.keys, self.failed = [], [], [], []

    def array(self, key, got, want, lay):
        """got: (nblocks, [levels,] nproma): the active columns are want's bits, the padded tail is still NaN"""
        g, w = got.contiguous().view(INT), want.contiguous().view(INT)
        active = torch.ones((lay.nblocks,) + (1,) * (got.dim() - 2) + (lay.nproma,), dtype=torch.bool, device=DEV)
        active[-1, ..., lay.tail:] = False
        self.flags.append((key, ((g == w) | ~active).all() & (torch.isnan(got) | active).all() & ~(torch.isnan(got) & active).any()))
        v = g.to(torch.int64).flatten()
        self.keys.append(key)
        self.sums.append(torch.stack((v.sum(), (v * (2 * torch.arange(v.numel(), device=DEV) + 1)).sum())))

    def untouched(self, key, t):
        self.flags.append((f"{key} was touched", torch.isnan(t).all()))

    def unchanged(self, key, now: dict, before: dict):
        for n in now:
            self.flags.append((f"{key}.{n} changed", (now[n].contiguous().view(INT) == before[n].contiguous().view(INT)).all()))

    def log_empty(self, key):
        if B.lib.cloudsc2_debug_launch_log(None, None, 0) != 0:
            self.failed.append(f"{key}: the launch log is not empty after a column-sum launch")

    def finish(self):
        torch.cuda.synchronize()
        self.failed += [k for k, f in self.flags if not bool(f)]
        self.flags = []


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
    traj, sc = ov.ad_forward(x, prm, ptsphy, lay)  # the dense forward: the ten planes and what the reverse sweep re-reads
    g = torch.Generator(device=DEV).manual_seed(300)
    ybar_all = {n: torch.randn((lay.nblocks, lay.nproma), generator=g, dtype=ov.real(), device=DEV) for n in B.OUT_NAMES}
    before = {k: {n: t.clone() for n, t in d.items()} for k, d in (("x", x), ("dx", dx), ("traj", traj), ("ybar", ybar_all))}
    masks = (ins, NARROW[0], ("paph", "lu"))

    for wname, weights in weight_patterns(nlev):
        table, names = table_of(weights, nlev), tuple(weights)
        key = f"{tag}.{wname}"
        want = {n: fold(weights[n], traj[n]) for n in names}
        B.launch_log_reset()
        # ---- NL, lean
        got = sums_of(names, lay)
        B.check(B.lib.cloudsc2_nl_launch_colsum(*G, ov.blk("in", x, lay), ptr(table), sums_blk(got, lay), None, None, ov.stream()))
        for n in names:
            chk.array(f"{key}.nl.{n}", got[n], want[n], lay)
        # ---- NL with keep
        got = sums_of(names, lay)
        kept = {n: torch.full(lay.shape(n), NAN, dtype=ov.real(), device=DEV) for n in ("fplsl", "fplsn")}
        ck = ov.scratch_of(lay)
        B.check(B.lib.cloudsc2_nl_launch_colsum(*G, ov.blk("in", x, lay), ptr(table), sums_blk(got, lay), ov.blk("out", kept, lay), ptr(ck),
                                                ov.stream()))
        for n in names:
            chk.array(f"{key}.keep.{n}", got[n], want[n], lay)
        for n in kept:
            chk.array(f"{key}.keep.plane.{n}", kept[n], traj[n], lay)
        if evap:
            chk.array(f"{key}.keep.scratch", ck, sc, lay)
        else:
            chk.untouched(f"{key}.keep.scratch", ck)
        # ---- TL: the fold over the sparse TL launch's tangent planes
        for pin in masks + ((),):
            dy = ov.packed("out", B.OUT_NAMES, lay)
            tl_sparse(x, {n: dx[n] for n in pin}, dy, prm, ptsphy, lay, satur)
            got = sums_of(names, lay)
            B.check(B.lib.cloudsc2_tl_launch_colsum(*G, int(satur), ov.blk("in", x, lay), ov.blk("in", {n: dx[n] for n in pin}, lay), ptr(table),
                                                    sums_blk(got, lay), ov.stream()))
            for n in names:
                chk.array(f"{key}.tl.{'+'.join(pin) if len(pin) < 3 else 'all'}.{n}", got[n], fold(weights[n], torch.nan_to_num(dy[n])), lay)
        # ---- reverse: the sparse launch fed the planes w[k] * ybar[c]
        ybar = {n: ybar_all[n] for n in names}
        yplanes = {n: torch.mul(weights[n][None, :, None], ybar[n][:, None, :]).contiguous() for n in names}
        for pin in masks:
            want_x = ov.packed("in", pin, lay)
            vjp_sparse(x, traj, sc, want_x, yplanes, prm, ptsphy, lay, satur)
            got_x = ov.packed("in", pin, lay)
            B.check(B.lib.cloudsc2_vjp_launch_colsum(*G, int(satur), ov.blk("in", x, lay), ov.blk("out", traj, lay), ov.blk("in", got_x, lay),
                                                     ptr(table), sums_blk(ybar, lay), ptr(sc), ov.stream()))
            for n in pin:
                chk.array(f"{key}.vjp.{'+'.join(pin) if len(pin) < 3 else 'all'}.{n}", got_x[n], want_x[n], lay)
        chk.log_empty(key)
    for k, d in (("x", x), ("dx", dx), ("traj", traj), ("ybar", ybar_all)):
        chk.unchanged(f"{tag}.{k}", d, before[k])
    chk.finish()


def main(path: str, small: bool) -> int:
    assert B.device_available(), "no HIP device"
    tab = c2.random_table(137, 100, seed=21)  # non-zero supsat
    chk = Checks()
    cases = [(f"n{SHAPE[0]}x{SHAPE[1]}.m{mode}.{fname}.{'satur' if satur else 'qsat'}", *SHAPE, flags, mode, satur)
             for fname, flags in FLAGSETS for mode in MODES for satur in (False, True)]
    if not small:
        cases.append((f"n{SHAPE2[0]}x{SHAPE2[1]}.m1.levapls2_lregcl.satur", *SHAPE2, FLAGSETS[1][1], 1, True))
    for tag, nproma, ngptot, flags, mode, satur in cases:
        run_case(chk, tag, tab, nproma, ngptot, flags, mode, satur)
    np.savez(path, keys=np.array(chk.keys), sums=torch.stack(chk.sums).cpu().numpy(), cases=np.array([c[0] for c in cases]),
             failed=np.array(chk.failed, dtype=str))
    print(f"{len(cases)} cases, {len(chk.keys)} arrays compared, CLOUDSC2_OFF32={os.environ.get('CLOUDSC2_OFF32')}")
    if chk.failed:
        print(f"{len(chk.failed)} failures:", *chk.failed[:60], sep="\n  ")
    return 1 if chk.failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "small"))
