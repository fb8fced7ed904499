"""The parameter column-sum sweep through the C ABI, run as a CHILD process by tests/test_gpu_autograd_parcolsum.py:
``[CLOUDSC2_OFF32=0|1] [CLOUDSC2_PRECISION=single] python tests/parcolsum_variant_checks.py OUT.npz``.

The launchers choose the addressing form of the kernels once per process (CLOUDSC2_OFF32: the mechanism of tests/offset_variant_checks.py),
hence one child per form.  For the plain and the evaporation flag set x math_mode 1 / 2 x qsat given / SATUR in the sweep, at NPROMA 32 x
100 columns (four blocks, a padded tail of 28): cloudsc2_parjac_launch_colsum with all ten sums must give the bits of the fold of this
process's cloudsc2_tl_launch_parjac planes, the padded tail keeps its NaN prefill, and cloudsc2_parnormal_launch_colsum runs on seeded
residuals and weights.  Every sums array and the 14 doubles of every case go to OUT.npz: the parent compares the two forms bit for bit.
Exit code 1 with the failures printed if a check fails."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.gpu_util import DEV, new, params, state, stream  # noqa: E402
from tests.parcolsum_yardstick import PAR_SUMS  # noqa: E402
from tests.util import B, c2  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402

P = c2.PARAM_NAMES
NPAR = len(P)
NAN = float("nan")
GUARD = 64  # doubles after the workspace that must stay as they were
NLEV = 137
FLAGSETS = (("plain", dict()), ("levapls2_lregcl", dict(levapls2=True, lregcl=True)))
MODES = (1, 2)
SHAPE = (32, 100)


def level_weights() -> list:
    """(name, {sum: (nlevx,) weights}): the surface fluxes, all ten names (seeded: negative entries, exact zeros), one full-level sum"""
    rng = np.random.default_rng(20261020)
    every = {}
    for n in B.OUT_NAMES:
        nlevx = NLEV + (1 if n in ag.HALF_OUT else 0)
        w = rng.uniform(-1.0, 1.0, nlevx)
        w[rng.random(nlevx) < 0.2] = 0.0
        w[0], w[-1] = -0.75, 0.625
        every[n] = torch.from_numpy(w.astype(B.REAL)).to(DEV)
    surface = torch.zeros(NLEV + 1, dtype=B.torch_real(), device=DEV)
    surface[-1] = 1.0
    return [("surface", {"fplsl": surface, "fplsn": surface.clone()}), ("all ten", every), ("tenq", {"tenq": every["tenq"]})]


def table_of(weights: dict) -> torch.Tensor:
    t = torch.full((len(B.OUT_NAMES), NLEV + 1), NAN, dtype=B.torch_real(), device=DEV)  # (rows and entries that must not be read: NaN)
    for n, w in weights.items():
        t[B.OUT_NAMES.index(n), :len(w)] = w
    return t


def fold(w: torch.Tensor, plane: torch.Tensor) -> torch.Tensor:
    """the contract: acc = +0; acc = fl(acc + fl(w[k] * plane[:, k, :])), separate mul and add"""
    acc = torch.zeros((plane.shape[0], plane.shape[2]), dtype=plane.dtype, device=plane.device)
    for k in range(plane.shape[1]):
        acc = torch.add(acc, torch.mul(plane[:, k, :], w[k]))
    return acc


def parjac_planes(x, prm, ptsphy, lay):
    """cloudsc2_tl_launch_parjac, the parent: four blocks of ten planes (the rpecons block stays zero without the evaporation branch)"""
    sens = [new(B.OUT_NAMES, lay) for _ in P]
    blocks = (B.Outputs * NPAR)(*(ag._block("out", s, lay) for s in sens))
    B.check(B.lib.cloudsc2_tl_launch_parjac(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)), blocks, stream()))
    return sens


def folded(sens, np_dirs, weights):
    return [{n: fold(w, sens[k][n]) for n, w in weights.items()} for k in range(np_dirs)]


def launch_sums(x, prm, ptsphy, lay, weights: dict, names=None):
    """cloudsc2_parjac_launch_colsum into four NaN-prefilled blocks of (nblocks, nproma) sums"""
    names = tuple(weights) if names is None else names
    sums = [{n: torch.full((lay.nblocks, lay.nproma), NAN, dtype=B.torch_real(), device=DEV) for n in names} for _ in P]
    blocks = (B.Outputs * NPAR)(*(ag._sums_block(s, lay) for s in sums))
    B.check(B.lib.cloudsc2_parjac_launch_colsum(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                                C.c_void_p(table_of(weights).data_ptr()), blocks, stream()))
    return sums


def act(t, lay):
    """the active columns of a (nblocks, nproma) array in grid order"""
    return t.reshape(-1)[:lay.ngptot]


def check_sums(got, want, np_dirs, lay, label) -> int:
    """bits on the active columns, NaN prefill in the tail, the rpecons block untouched when it is not run -> the number of elements that
    differ (asserted zero by the caller, which prints it first)"""
    differ = 0
    for k, pname in enumerate(P):
        for n, g in got[k].items():
            if k >= np_dirs:
                assert bool(torch.all(torch.isnan(g))), (label, pname, n, "the rpecons block was written without the evaporation branch")
                continue
            a, w = act(g, lay), act(want[k][n], lay)
            assert bool(torch.all(torch.isfinite(a))), (label, pname, n, "an active sum was not written")
            assert bool(torch.all(torch.isnan(g.reshape(-1)[lay.ngptot:]))), (label, pname, n, "the padded tail was touched")
            bits = torch.int64 if a.dtype == torch.float64 else torch.int32
            differ += int((a.contiguous().view(bits) != w.contiguous().view(bits)).sum())
            if n not in PAR_SUMS:
                assert bool(torch.all(a == 0.0)), (label, pname, n, "must be exactly zero")
    return differ


def observations(lay, names, seed):
    """seeded residuals and positive weights per column, (nblocks, nproma), NaN in the padded tail"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r, w = {}, {}
    for n in names:
        r[n] = torch.randn((lay.nblocks, lay.nproma), generator=g, dtype=B.torch_real(), device=DEV)
        w[n] = torch.rand((lay.nblocks, lay.nproma), generator=g, dtype=B.torch_real(), device=DEV) * 1.5 + 0.5
        for t in (r[n], w[n]):
            t.view(-1)[lay.ngptot:] = NAN
    return r, w


def launch_normal(x, prm, ptsphy, lay, weights, r, w, work=None, normal=None):
    """cloudsc2_parnormal_launch_colsum -> (normal, work): 14 device doubles, and the NaN-prefilled workspace with its guard words.
    w None: the weight block itself is NULL; x without qsat: SATUR in the sweep"""
    n = C.c_longlong()
    B.check(B.lib.cloudsc2_parnormal_work_doubles(lay.nproma, lay.ngptot, C.byref(n)))
    work = work if work is not None else torch.full((n.value + GUARD,), NAN, dtype=torch.float64, device=DEV)
    normal = normal if normal is not None else torch.full((B.NNORMAL,), NAN, dtype=torch.float64, device=DEV)
    B.check(B.lib.cloudsc2_parnormal_launch_colsum(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                                   C.c_void_p(table_of(weights).data_ptr()), C.byref(ag._sums_block(r, lay)),
                                                   C.byref(ag._sums_block(w, lay)) if w is not None else None, C.c_void_p(work.data_ptr()),
                                                   C.c_void_p(normal.data_ptr()), stream()))
    return normal, work


def main(path: str) -> int:
    assert B.device_available(), "no HIP device"
    tab = c2.random_table(137, 100, seed=21)
    weights = dict(level_weights())["all ten"]
    out, failed = {}, []
    for fname, flags in FLAGSETS:
        for mode in MODES:
            for satur in (False, True):
                tag = f"m{mode}.{fname}.{'satur' if satur else 'qsat'}"
                prm = params(tab, mode, **flags)
                x, ptsphy, lay = state(tab, *SHAPE, prm, satur)
                np_dirs = 4 if prm.levapls2 else 3
                want = folded(parjac_planes(x, prm, ptsphy, lay), np_dirs, weights)
                got = launch_sums(x, prm, ptsphy, lay, weights)
                try:
                    differ = check_sums(got, want, np_dirs, lay, tag)
                    if differ:
                        failed.append(f"{tag}: {differ} elements differ from the fold")
                except AssertionError as e:
                    failed.append(f"{tag}: {e}")
                r, w = observations(lay, tuple(weights), seed=51)
                normal, _ = launch_normal(x, prm, ptsphy, lay, weights, r, w)
                torch.cuda.synchronize()
                if not bool(torch.all(torch.isfinite(normal))):
                    failed.append(f"{tag}: the normal equations are not finite")
                out[f"{tag}.normal"] = normal.cpu().numpy()
                for k in range(np_dirs):
                    for n in PAR_SUMS:
                        out[f"{tag}.{P[k]}.{n}"] = act(got[k][n], lay).cpu().numpy()
    np.savez(path, **out)
    print(f"{len(out)} arrays, CLOUDSC2_OFF32={os.environ.get('CLOUDSC2_OFF32')}")
    if failed:
        print(f"{len(failed)} failures:", *failed[:40], sep="\n  ")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
