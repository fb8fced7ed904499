"""The sparse TL and reverse sweeps through the C ABI, run as a CHILD process by tests/test_gpu_autograd_sparse.py:
``[CLOUDSC2_OFF32=0|1] [CLOUDSC2_PRECISION=single] python tests/sparse_variant_checks.py OUT.npz [small]``.

The launchers choose the addressing form of the kernels once per process (CLOUDSC2_OFF32), hence one child per form.  For the four
FLAG_SETS of tests/util.py (those of tests/test_hostcheck_vjp.py) x math_mode 1 / 2 x qsat given / satur, at NPROMA 32 x 100 columns (four blocks, a padded
tail of 28), and for one case at NPROMA 128 x 128 columns (no tail; not with ``small``), every mask pattern of tests/sparse_patterns.py
is launched through cloudsc2_tl_launch_sparse and cloudsc2_vjp_launch_sparse next to the dense twin on zero planes:

  * every present plane has the dense launch's bits on the active columns, the padded tail (NaN-prefilled) is untouched;
  * what the launches read (trajectory, tangents, cotangents) is unchanged;
  * the calling thread's launch log stays empty across the sparse launches.

The tendencies and cloud planes are strided views of packed buffers, as in tests/offset_variant_checks.py, whose helpers run the dense
twins.  Two checksums of every present plane go to OUT.npz: the parent compares the two addressing forms.  Exit code 1 with the
failures printed if a check fails."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import offset_variant_checks as ov  # noqa: E402
from tests.sparse_patterns import in_names, patterns  # noqa: E402
from tests.util import B, c2  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402

DEV = ov.DEV
FLAGSETS = (("plain", dict()), ("levapls2_lregcl", dict(levapls2=True, lregcl=True)), ("ldrain1d", dict(ldrain1d=True)), ("lregcl", dict(lregcl=True)))
MODES = (1, 2)
SHAPE, SHAPE2 = (32, 100), (128, 128)
INT = torch.int32 if B.SINGLE else torch.int64


def tl_sparse(x, dx, dy, prm, ptsphy, lay, satur):
    B.check(B.lib.cloudsc2_tl_launch_sparse(*ov.geom(prm, ptsphy, lay), int(satur), ov.blk("in", x, lay), ov.blk("in", dx, lay), ov.blk("out", dy, lay),
                                            ov.stream()))


def vjp_sparse(x, traj, sc, xa, y, prm, ptsphy, lay, satur):
    B.check(B.lib.cloudsc2_vjp_launch_sparse(*ov.geom(prm, ptsphy, lay), int(satur), ov.blk("in", x, lay), ov.blk("out", traj, lay), ov.blk("in", xa, lay),
                                             ov.blk("out", y, lay), C.c_void_p(sc.data_ptr()), ov.stream()))


class Checks:
    """device-side verdicts of one case, read once at its end"""

    def __init__(self):
        self.flags, self.sums, self.keys, self.failed = [], [], [], []

    def plane(self, key, got, want, lay):
        g, w = got.contiguous().view(INT), want.contiguous().view(INT)
        active = torch.ones(lay.nblocks, 1, lay.nproma, dtype=torch.bool, device=DEV)
        active[-1, :, lay.tail:] = False
        same = ((g == w) | ~active).all()
        tail = (torch.isnan(got) | active).all()  # the padded tail: still the NaN it was prefilled with
        self.flags.append((key, same & tail))
        v = g.to(torch.int64).flatten()
        self.keys.append(key)
        self.sums.append(torch.stack((v.sum(), (v * (2 * torch.arange(v.numel(), device=DEV) + 1)).sum())))

    def unchanged(self, key, now: dict, before: dict):
        for n in now:
            self.flags.append((f"{key}.{n} changed", (now[n].contiguous().view(INT) == before[n].contiguous().view(INT)).all()))

    def log_empty(self, key):
        if B.lib.cloudsc2_debug_launch_log(None, None, 0) != 0:
            self.failed.append(f"{key}: the launch log is not empty after a sparse launch")

    def finish(self):
        torch.cuda.synchronize()
        self.failed += [k for k, f in self.flags if not bool(f)]
        self.flags = []


def run_case(chk: Checks, tag, tab, nproma, ngptot, flags, mode, satur):
    prm = c2.default_params(c2.ceta_from_table(tab), **flags)
    prm.math_mode = mode
    st = c2.state_from_table(tab, nproma, ngptot)
    lay = ag.Layout(st.nblocks, st.nlev, nproma, ngptot)
    ptsphy = float(st.ptsphy)
    flat = {n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in c2.op_inputs(st).items()}
    flat["qsat"] = ag.satur(flat["pap"], flat["t"], prm, ngptot)
    ins = in_names(satur)
    x = ov.packed("in", ins, lay, values=flat)
    dx = ov.packed("in", ins, lay, values=ov.seeded(B.IN_NAMES, lay, 100, scale=flat))
    zin = ov.packed("in", ins, lay, fill=0.0)
    u = ov.packed("out", B.OUT_NAMES, lay, values=ov.seeded(B.OUT_NAMES, lay, 200))
    zout = ov.packed("out", B.OUT_NAMES, lay, fill=0.0)
    traj, sc = ov.ad_forward(x, prm, ptsphy, lay)
    before = {k: {n: t.clone() for n, t in d.items()} for k, d in (("x", x), ("dx", dx), ("u", u), ("traj", traj))}
    before["sc"] = {"scratch": sc.clone()}
    B.launch_log_reset()

    for name, pin, pout in patterns(satur, tl=True):
        dz = {n: (dx[n] if n in pin else zin[n]) for n in ins}
        want = ov.tl_satur(x, dz, prm, ptsphy, lay) if satur else ov.tl(x, dz, prm, ptsphy, lay)
        B.launch_log_reset()
        got = ov.packed("out", pout, lay)
        tl_sparse(x, {n: dx[n] for n in pin}, got, prm, ptsphy, lay, satur)
        chk.log_empty(f"{tag}.tl.{name}")
        for n in pout:
            chk.plane(f"{tag}.tl.{name}.{n}", got[n], want[n], lay)
    for name, pin, pout in patterns(satur):
        yz = {n: (u[n] if n in pout else zout[n]) for n in B.OUT_NAMES}
        want = ov.vjp(x, traj, sc, yz, prm, ptsphy, lay, satur=satur)
        B.launch_log_reset()
        got = ov.packed("in", pin, lay)
        vjp_sparse(x, traj, sc, got, {n: u[n] for n in pout}, prm, ptsphy, lay, satur)
        chk.log_empty(f"{tag}.vjp.{name}")
        for n in pin:
            chk.plane(f"{tag}.vjp.{name}.{n}", got[n], want[n], lay)
    for k, d in (("x", x), ("dx", dx), ("u", u), ("traj", traj), ("sc", {"scratch": sc})):
        chk.unchanged(f"{tag}.{k}", d, before[k])
    chk.finish()


def main(path: str, small: bool) -> int:
    assert B.device_available(), "no HIP device"
    tab = c2.random_table(137, 100, seed=5)  # non-zero supsat
    chk = Checks()
    cases = [(f"n{SHAPE[0]}x{SHAPE[1]}.m{mode}.{fname}.{'satur' if satur else 'qsat'}", *SHAPE, flags, mode, satur)
             for fname, flags in FLAGSETS for mode in MODES for satur in (False, True)]
    if not small:
        cases.append((f"n{SHAPE2[0]}x{SHAPE2[1]}.m1.levapls2_lregcl.satur", *SHAPE2, FLAGSETS[1][1], 1, True))
    for tag, nproma, ngptot, flags, mode, satur in cases:
        run_case(chk, tag, tab, nproma, ngptot, flags, mode, satur)
    np.savez(path, keys=np.array(chk.keys), sums=torch.stack(chk.sums).cpu().numpy(), cases=np.array([c[0] for c in cases]),
             failed=np.array(chk.failed, dtype=str))
    print(f"{len(cases)} cases, {len(chk.keys)} present planes compared with the dense twins, CLOUDSC2_OFF32={os.environ.get('CLOUDSC2_OFF32')}")
    if chk.failed:
        print(f"{len(chk.failed)} failures:", *chk.failed[:40], sep="\n  ")
    return 1 if chk.failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], len(sys.argv) > 2 and sys.argv[2] == "small"))
