"""The parameter column-sum sweep through the C ABI, run as a CHILD process by tests/test_gpu_autograd_parcolsum.py:
``[CLOUDSC2_OFF32=0|1] [CLOUDSC2_PRECISION=single] python tests/parcolsum_variant_checks.py OUT.npz``.

The launchers choose the addressing form of the kernels once per process (CLOUDSC2_OFF32: the mechanism of tests/offset_variant_checks.py),
hence one child per form.  For the plain and the evaporation flag set x math_mode 1 / 2 x qsat given / SATUR in the sweep, at NPROMA 32 x
100 columns (four blocks, a padded tail of 28): cloudsc2_parjac_launch_colsum with all ten sums must give the bits of the fold of this
process's cloudsc2_tl_launch_parjac planes, the padded tail keeps its NaN prefill, and cloudsc2_parnormal_launch_colsum runs on seeded
residuals and weights.  Every sums array and the 14 doubles of every case go to OUT.npz: the parent compares the two forms bit for bit.
Exit code 1 with the failures printed if a check fails."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_autograd_parcolsum as T  # noqa: E402
from tests.util import B, c2  # noqa: E402

FLAGSETS = (("plain", dict()), ("levapls2_lregcl", dict(levapls2=True, lregcl=True)))
MODES = (1, 2)
SHAPE = (32, 100)


def main(path: str) -> int:
    assert B.device_available(), "no HIP device"
    tab = c2.random_table(137, 100, seed=21)
    weights = dict(T.level_weights())["all ten"]
    out, failed = {}, []
    for fname, flags in FLAGSETS:
        for mode in MODES:
            for satur in (False, True):
                tag = f"m{mode}.{fname}.{'satur' if satur else 'qsat'}"
                prm = T.params(tab, mode, **flags)
                x, ptsphy, lay = T.state(tab, *SHAPE, prm, satur)
                np_dirs = 4 if prm.levapls2 else 3
                want = T.folded(T.parjac_planes(x, prm, ptsphy, lay), np_dirs, weights)
                got = T.launch_sums(x, prm, ptsphy, lay, weights)
                try:
                    differ = T.check_sums(got, want, np_dirs, lay, tag)
                    if differ:
                        failed.append(f"{tag}: {differ} elements differ from the fold")
                except AssertionError as e:
                    failed.append(f"{tag}: {e}")
                r, w = T.observations(lay, tuple(weights), seed=51)
                normal, _ = T.launch_normal(x, prm, ptsphy, lay, weights, r, w)
                torch.cuda.synchronize()
                if not bool(torch.all(torch.isfinite(normal))):
                    failed.append(f"{tag}: the normal equations are not finite")
                out[f"{tag}.normal"] = normal.cpu().numpy()
                for k in range(np_dirs):
                    for n in T.PAR_SUMS:
                        out[f"{tag}.{T.P[k]}.{n}"] = T.act(got[k][n], lay).cpu().numpy()
    np.savez(path, **out)
    print(f"{len(out)} arrays, CLOUDSC2_OFF32={os.environ.get('CLOUDSC2_OFF32')}")
    if failed:
        print(f"{len(failed)} failures:", *failed[:40], sep="\n  ")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
