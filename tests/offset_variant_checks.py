"""Every public sweep launcher through the C ABI, run as a CHILD process by tests/test_gpu_offset_variants.py:
``[CLOUDSC2_OFF32=0|1] [CLOUDSC2_PRECISION=single] python tests/offset_variant_checks.py OUT.npz [small]``.

The launchers choose between the 32-bit and the 64-bit byte offsets of every sweep kernel once per process (finish() in
csrc/cloudsc2_launch.hip reads CLOUDSC2_OFF32 once), hence one child per form.  The child runs NL (SATUR fused / qsat given), TL (fed,
self-increment, with trajectory stores), AD (accumulate, assign, forward + reverse), the vector-Jacobian product, the pairs with SATUR
differentiated and with the parameter derivative, the batched sweeps for 2..cloudsc2_batch_max() directions, the parameter Jacobian
and the Taylor sweep, for {} / {levapls2} / {ldrain1d} (NL only) times math_mode 1 and 2, at the two smallest shapes at which an offset
can go wrong:

  NPROMA 32 x 100 columns     four blocks, a ragged tail of 4, and a workgroup whose lanes cross blocks
  NPROMA 100 x 1000 columns   blocks that are no multiple of the wave, 8 workgroups

The tendencies and the cloud planes are strided views of packed (nblocks, 8, nlev, nproma) and (nblocks, 5, nlev, nproma) buffers, as
DeviceState lays them out (block stride != plane size; planes nobody may touch are NaN), the half-level fields have nlev + 1 rows, and
every output is NaN-prefilled.  It writes every output plane and the calling thread's launch log to one .npz and exits non-zero if an
active element of a written output is not finite.  ``small``: the first shape alone (the run of the fp32 library).

The launch helpers are also what the parent's tests of true >= 4 GiB spans call."""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.util import B, c2  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")
IN15 = tuple(n for n in B.IN_NAMES if n != "qsat")
P = c2.PARAM_NAMES
# the planes of DeviceState's B_CML / B_LOC (T A Q QL QI QR QS QV) and PCLV (QL QI QR QS QV)
PACKED_IN = (({"gtent": 0, "gtenq": 2, "gtenl": 3, "gteni": 4}, 8), ({"l": 0, "i": 1}, 5))
PACKED_OUT = (({"tent": 0, "tenq": 2, "tenl": 3, "teni": 4}, 8),)
SHAPES = ((32, 100), (100, 1000))
FLAGSETS = (("plain", dict(), False), ("levapls2", dict(levapls2=True), False), ("ldrain1d", dict(ldrain1d=True), True))  # name, flags, NL only
MODES = (1, 2)


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def real():
    return B.torch_real()


def packed(kind: str, names, lay, fill=NAN, values=None) -> dict:
    """the named fields of one argument block: tendencies and cloud planes as views of packed buffers, the rest flat"""
    out = {}
    for planes, n in (PACKED_IN if kind == "in" else PACKED_OUT):
        buf = torch.full((lay.nblocks, n, lay.nlev, lay.nproma), NAN if values is not None else fill, dtype=real(), device=DEV)
        out.update({name: buf[:, p] for name, p in planes.items()})
    for name in names:
        if name not in out:
            out[name] = torch.full(lay.shape(name), fill, dtype=real(), device=DEV)
        if values is not None:
            out[name].copy_(values[name])
    return {n: out[n] for n in names}


def zero_active(d: dict, lay) -> dict:
    """NaN-prefilled planes with the active columns zeroed: what an accumulating launcher adds to"""
    for t in d.values():
        t[:-1] = 0
        t[-1, :, :lay.tail] = 0
    return d


def seeded(names, lay, seed: int, scale=None) -> dict:
    """host-generated planes (the same bits in every process), zero in the padded tail; scale: a dict of planes to multiply by"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in names:
        a = rng.standard_normal(lay.shape(n)).astype(B.REAL)
        a[-1, :, lay.tail:] = 0
        t = torch.from_numpy(a).to(DEV)
        out[n] = t * scale[n] * 0.01 if scale is not None else t
    return out


def blk(kind, ts, lay):
    return C.byref(ag._block(kind, ts, lay))


def geom(prm, ptsphy, lay):
    return C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot


def scratch_of(lay):
    return torch.full((lay.nblocks, lay.nlev, lay.nproma), NAN, dtype=real(), device=DEV)


# ---- one helper per public launcher: NaN-prefilled outputs in, the launcher's return code checked -----------------------------------

def nl(x, prm, ptsphy, lay, out=None):
    out = out if out is not None else packed("out", B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_nl_launch(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", out, lay), B.Field(), 0.0, stream()))
    return out


def tl(x, dx, prm, ptsphy, lay, traj=None, dy=None):
    dy = dy if dy is not None else packed("out", B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_tl_launch(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", traj, lay) if traj is not None else C.byref(B.Outputs()),
                                     blk("in", dx, lay), blk("out", dy, lay), stream()))
    return dy


def tl_self(x, prm, ptsphy, lay):
    dy = packed("out", B.OUT_NAMES, lay)
    yy = torch.full((lay.nblocks * lay.nproma,), NAN, dtype=torch.float64, device=DEV)
    B.check(B.lib.cloudsc2_tl_launch_self(*geom(prm, ptsphy, lay), blk("in", x, lay), C.byref(B.Outputs()), 0.01, blk("out", dy, lay),
                                          C.c_void_p(yy.data_ptr()), stream()))
    return dy, yy


def ad(x, u, prm, ptsphy, lay, assign: bool):
    """cloudsc2_ad_launch / _assign -> input adjoints, the consumed output adjoints, trajectory outputs, cover checkpoints"""
    traj, sc = packed("out", B.OUT_NAMES, lay), scratch_of(lay)
    xa = packed("in", B.IN_NAMES, lay)
    if not assign:
        zero_active(xa, lay)
    y = packed("out", B.OUT_NAMES, lay, values=u)
    fn = B.lib.cloudsc2_ad_launch_assign if assign else B.lib.cloudsc2_ad_launch
    B.check(fn(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", traj, lay), blk("in", xa, lay), blk("out", y, lay), C.c_void_p(sc.data_ptr()),
               stream()))
    return xa, y, traj, sc


def ad_forward(x, prm, ptsphy, lay):
    traj, sc = packed("out", B.OUT_NAMES, lay), scratch_of(lay)
    B.check(B.lib.cloudsc2_ad_launch_forward(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", traj, lay), C.c_void_p(sc.data_ptr()), stream()))
    return traj, sc


def ad_reverse(x, traj, sc, u, prm, ptsphy, lay):
    xa = zero_active(packed("in", B.IN_NAMES, lay), lay)
    y = packed("out", B.OUT_NAMES, lay, values=u)
    B.check(B.lib.cloudsc2_ad_launch_reverse(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", traj, lay), blk("in", xa, lay), blk("out", y, lay),
                                             C.c_void_p(sc.data_ptr()), 0, stream()))
    return xa, y


def vjp(x, traj, sc, u, prm, ptsphy, lay, satur: bool = False, xa=None):
    """cloudsc2_vjp_launch (adjoints of all 16 inputs) or cloudsc2_vjp_launch_satur (x without qsat, 15 adjoints)"""
    xa = xa if xa is not None else packed("in", IN15 if satur else B.IN_NAMES, lay)
    fn = B.lib.cloudsc2_vjp_launch_satur if satur else B.lib.cloudsc2_vjp_launch
    B.check(fn(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", traj, lay), blk("in", xa, lay), blk("out", u, lay), C.c_void_p(sc.data_ptr()),
               stream()))
    return xa


def tl_satur(x, dx, prm, ptsphy, lay, dy=None):
    dy = dy if dy is not None else packed("out", B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_tl_launch_satur(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("in", dx, lay), blk("out", dy, lay), stream()))
    return dy


def tl_par(x, dx, dpar, prm, ptsphy, lay, satur: int, dy=None):
    dy = dy if dy is not None else packed("out", B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_tl_launch_par(*geom(prm, ptsphy, lay), int(satur), blk("in", x, lay), blk("in", dx, lay), (C.c_double * len(P))(*dpar),
                                         blk("out", dy, lay), stream()))
    return dy


def vjp_par(x, traj, sc, u, prm, ptsphy, lay, satur: int, xa=None):
    xa = xa if xa is not None else packed("in", IN15 if satur else B.IN_NAMES, lay)
    n = C.c_longlong()
    B.check(B.lib.cloudsc2_par_work_doubles(lay.nproma, lay.ngptot, C.byref(n)))
    work = torch.full((n.value,), NAN, dtype=torch.float64, device=DEV)
    par_adj = torch.full((len(P),), NAN, dtype=torch.float64, device=DEV)
    B.check(B.lib.cloudsc2_vjp_launch_par(*geom(prm, ptsphy, lay), int(satur), blk("in", x, lay), blk("out", traj, lay), blk("in", xa, lay),
                                          blk("out", u, lay), C.c_void_p(sc.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(par_adj.data_ptr()),
                                          stream()))
    return xa, work, par_adj


def tl_batch(x, dxs, prm, ptsphy, lay):
    dys = [packed("out", B.OUT_NAMES, lay) for _ in dxs]
    B.check(B.lib.cloudsc2_tl_launch_batch(*geom(prm, ptsphy, lay), blk("in", x, lay), len(dxs), ag._block_array("in", dxs, lay),
                                           ag._block_array("out", dys, lay), stream()))
    return dys


def vjp_batch(x, traj, sc, us, prm, ptsphy, lay):
    xas = [packed("in", B.IN_NAMES, lay) for _ in us]
    B.check(B.lib.cloudsc2_vjp_launch_batch(*geom(prm, ptsphy, lay), blk("in", x, lay), blk("out", traj, lay), len(us), ag._block_array("in", xas, lay),
                                            ag._block_array("out", us, lay), C.c_void_p(sc.data_ptr()), stream()))
    return xas


def parjac(x, prm, ptsphy, lay, sens=None):
    sens = sens if sens is not None else [packed("out", B.OUT_NAMES, lay) for _ in P]
    blocks = (B.Outputs * len(P))(*(ag._block("out", s, lay) for s in sens))
    B.check(B.lib.cloudsc2_tl_launch_parjac(*geom(prm, ptsphy, lay), blk("in", x, lay), blocks, stream()))
    return sens


def taylor(x, base, dy, prm, ptsphy, lay):
    n = C.c_longlong()
    B.check(B.lib.cloudsc2_taylor_sweep_work_doubles(lay.nproma, lay.ngptot, C.byref(n)))
    work = torch.full((n.value,), NAN, dtype=torch.float64, device=DEV)
    sums = torch.full((10, lay.nblocks, 10, 2), NAN, dtype=torch.float64, device=DEV)
    B.check(B.lib.cloudsc2_taylor_sweep_launch(*geom(prm, ptsphy, lay), lay.nproma, blk("in", x, lay), blk("out", base, lay), blk("out", dy, lay),
                                               C.c_void_p(work.data_ptr()), C.c_void_p(sums.data_ptr()), stream()))
    return sums, work


# ---- the child ----------------------------------------------------------------------------------------------------------------------

class Record:
    """the output planes of one case on the device, whether their active elements are finite, and the launch log"""

    def __init__(self):
        self.arrays, self.ok, self.bad = {}, None, []
        self.log_case, self.log_family, self.log_word = [], [], []

    def put(self, lay, key, value, check=True):
        if isinstance(value, dict):
            for n, t in value.items():
                self.put(lay, f"{key}.{n}", t, check)
            return
        if isinstance(value, (list, tuple)):
            for j, v in enumerate(value):
                self.put(lay, f"{key}.{j}", v, check)
            return
        assert key not in self.arrays, key
        self.arrays[key] = value
        if check:
            plane = value.dim() == 3 and value.shape[0] == lay.nblocks and value.shape[2] == lay.nproma  # (else: all of it is active)
            fine = torch.isfinite(value[:-1]).all() & torch.isfinite(value[-1, :, :lay.tail]).all() if plane else torch.isfinite(value).all()
            self.bad.append((key, fine))

    def take_log(self, case: int):
        for fam, word in B.launch_log():
            self.log_case.append(case)
            self.log_family.append(fam)
            self.log_word.append(word)
        B.launch_log_reset()


def run_case(rec: Record, tag: str, tab, nproma, ngptot, flags, mode, nl_only):
    prm = c2.default_params(c2.ceta_from_table(tab), **flags)
    prm.math_mode = mode
    st = c2.state_from_table(tab, nproma, ngptot)
    lay = ag.Layout(st.nblocks, st.nlev, nproma, ngptot)
    ptsphy = float(st.ptsphy)
    flat = {n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in c2.op_inputs(st).items()}
    flat["qsat"] = ag.satur(flat["pap"], flat["t"], prm, ngptot)  # (cloudsc2_satur_launch: not a sweep, not logged)
    x = packed("in", B.IN_NAMES, lay, values=flat)
    x15 = {n: x[n] for n in IN15}
    put = lambda key, value, check=True: rec.put(lay, f"{tag}.{key}", value, check)  # noqa: E731
    evap = bool(prm.levapls2 or prm.ldrain1d)

    put("nl_fused", nl(x15, prm, ptsphy, lay))
    base = nl(x, prm, ptsphy, lay)
    put("nl_qsat", base)
    if nl_only:
        return
    dx = seeded(B.IN_NAMES, lay, 100, scale=flat)
    dx = packed("in", B.IN_NAMES, lay, values=dx)
    dx15 = {n: dx[n] for n in IN15}
    u = packed("out", B.OUT_NAMES, lay, values=seeded(B.OUT_NAMES, lay, 200))
    dpar = [0.01 * getattr(prm, n) for n in P]

    put("tl_fed", tl(x, dx, prm, ptsphy, lay))
    dy_self, yy = tl_self(x, prm, ptsphy, lay)
    put("tl_self", dy_self)
    put("tl_self.yy", yy.view(lay.nblocks, 1, lay.nproma))
    traj = packed("out", B.OUT_NAMES, lay)
    put("tl_traj", tl(x, dx, prm, ptsphy, lay, traj=traj))
    put("tl_traj.traj", traj)

    for name, assign in (("ad_accumulate", False), ("ad_assign", True)):
        xa, y, tr, sc = ad(x, u, prm, ptsphy, lay, assign)
        put(name, xa)
        put(name + ".y", y)
        put(name + ".traj", tr)
        put(name + ".scratch", sc, check=evap)
    ftraj, fsc = ad_forward(x, prm, ptsphy, lay)
    put("ad_forward.traj", ftraj)
    put("ad_forward.scratch", fsc, check=evap)
    xa, y = ad_reverse(x, ftraj, fsc, u, prm, ptsphy, lay)
    put("ad_reverse", xa)
    put("ad_reverse.y", y)

    put("vjp", vjp(x, ftraj, fsc, u, prm, ptsphy, lay))
    straj, ssc = ad_forward(x15, prm, ptsphy, lay)  # the trajectory with SATUR evaluated in the sweep
    put("ad_forward_fused.traj", straj)
    put("ad_forward_fused.scratch", ssc, check=evap)
    put("vjp_fused_satur", vjp(x15, straj, ssc, u, prm, ptsphy, lay))  # traj_in->qsat NULL, adj_in->qsat an adjoint of its own

    put("tl_satur", tl_satur(x15, dx15, prm, ptsphy, lay))
    put("vjp_satur", vjp(x15, straj, ssc, u, prm, ptsphy, lay, satur=True))

    for satur in (0, 1):
        xs, dxs, tr, sc = (x15, dx15, straj, ssc) if satur else (x, dx, ftraj, fsc)
        put(f"tl_par{satur}", tl_par(xs, dxs, dpar, prm, ptsphy, lay, satur))
        xa, work, par_adj = vjp_par(xs, tr, sc, u, prm, ptsphy, lay, satur)
        put(f"vjp_par{satur}", xa)
        put(f"vjp_par{satur}.work", work.view(len(P), -1)[:, :ngptot])
        put(f"vjp_par{satur}.work_tail", work.view(len(P), -1)[:, ngptot:], check=False)
        put(f"vjp_par{satur}.par_adj", par_adj)

    kmax = B.lib.cloudsc2_batch_max()
    dxk = [dx] + [packed("in", B.IN_NAMES, lay, values=seeded(B.IN_NAMES, lay, 100 + j, scale=flat)) for j in range(1, kmax)]
    uk = [u] + [packed("out", B.OUT_NAMES, lay, values=seeded(B.OUT_NAMES, lay, 200 + j)) for j in range(1, kmax)]
    for k in range(2, kmax + 1):
        put(f"tl_batch{k}", tl_batch(x, dxk[:k], prm, ptsphy, lay))
        put(f"vjp_batch{k}", vjp_batch(x, ftraj, fsc, uk[:k], prm, ptsphy, lay))

    for name, xs in (("parjac_qsat", x), ("parjac_fused", x15)):
        sens = parjac(xs, prm, ptsphy, lay)
        put(name, sens[:3])
        put(name + ".3", sens[3], check=evap)  # without the evaporation branch the rpecons block is not written

    sums, work = taylor(x, base, dy_self, prm, ptsphy, lay)
    put("taylor.sums", sums)
    put("taylor.work", work, check=False)


def main(path: str, shapes=SHAPES) -> int:
    assert B.device_available(), "no HIP device"
    tab = c2.random_table(137, 100, seed=5)
    rec = Record()
    host = {}
    B.launch_log_reset()
    case = 0
    cases = []
    for nproma, ngptot in shapes:
        for mode in MODES:
            for fname, flags, nl_only in FLAGSETS:
                tag = f"n{nproma}x{ngptot}.m{mode}.{fname}"
                run_case(rec, tag, tab, nproma, ngptot, flags, mode, nl_only)
                torch.cuda.synchronize()
                rec.take_log(case)
                cases.append(tag)
                case += 1
                for k, t in rec.arrays.items():
                    host[k] = t.cpu().numpy()
                rec.arrays = {}
    bad = [k for k, fine in rec.bad if not bool(fine)]
    host["log_case"] = np.array(rec.log_case, dtype=np.int64)
    host["log_family"] = np.array(rec.log_family, dtype=np.int64)
    host["log_word"] = np.array(rec.log_word, dtype=np.int64)
    host["cases"] = np.array(cases)
    np.savez(path, **host)
    print(f"{len(host) - 4} planes, {len(rec.log_word)} sweep kernels logged, CLOUDSC2_OFF32={os.environ.get('CLOUDSC2_OFF32')}")
    if bad:
        print("not finite in an active element:", *bad[:20], sep="\n  ")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], SHAPES[:1] if sys.argv[2:] == ["small"] else SHAPES))
