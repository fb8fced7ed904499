"""Shared helpers of the tests that need torch or the device: the differentiable op's inputs, launchers and bit comparisons on cuda:0, the
parity tests' checker, and the inputs of the device-free argument and refusal tests.  Host-side numpy helpers are in tests/util.py, the
host sweeps' runners in tests/host_sweeps.py."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.util import ROOT, B, c2, flat_fields, refcall, relerr, set_lib_params
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

DEV = torch.device("cuda:0")
P = c2.PARAM_NAMES
NAN = float("nan")
KEYS15 = list(ag.SAT_NAMES)  # the inputs without qsat: SATUR in the sweep


# ---- the differentiable op on the device (tests/test_gpu_autograd*.py) ----
def make_inputs(tab, nproma, ngptot, prm):
    st = c2.state_from_table(tab, nproma, ngptot)
    x = {n: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for n, a in c2.op_inputs(st).items()}
    x["qsat"] = ag.satur(x["pap"], x["t"], prm, ngptot)
    return {n: x[n] for n in B.IN_NAMES}, float(st.ptsphy), ag.Layout(st.nblocks, st.nlev, nproma, ngptot)


def stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def new(names, lay, fill=0.0):
    return {n: torch.full(lay.shape(n), fill, dtype=B.torch_real(), device=DEV) for n in names}


def nl_launch(x, prm, ptsphy, lay):
    out = new(B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_nl_launch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                     C.byref(ag._block("out", out, lay)), B.Field(), 0.0, stream()))
    return out


def ad_assign_launch(x, u, prm, ptsphy, lay):
    traj, xa = new(B.OUT_NAMES, lay), new(B.IN_NAMES, lay)
    y = {n: u[n].clone() for n in B.OUT_NAMES}
    scratch = torch.zeros((lay.nblocks, lay.nlev, lay.nproma), dtype=B.torch_real(), device=DEV)
    B.check(B.lib.cloudsc2_ad_launch_assign(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                            C.byref(ag._block("out", traj, lay)), C.byref(ag._block("in", xa, lay)),
                                            C.byref(ag._block("out", y, lay)), C.c_void_p(scratch.data_ptr()), stream()))
    return xa


def tl_launch(x, dx, prm, ptsphy, lay):
    dy = new(B.OUT_NAMES, lay)
    B.check(B.lib.cloudsc2_tl_launch(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                     C.byref(B.Outputs()), C.byref(ag._block("in", dx, lay)), C.byref(ag._block("out", dy, lay)),
                                     stream()))
    return dy


def seeded(names, lay, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = {}
    for n in names:
        t = torch.randn(lay.shape(n), generator=g, dtype=B.torch_real(), device=DEV) * scale
        if lay.tail < lay.nproma:
            t[-1, :, lay.tail:] = 0
        out[n] = t
    return out


def same_bits(a, b):
    return torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                       b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))


def tail_zero(t, lay):
    return lay.tail == lay.nproma or bool(torch.all(t[-1, :, lay.tail:] == 0))


def params(tab, math_mode=0, **flags):
    prm = c2.default_params(c2.ceta_from_table(tab), **flags)
    prm.math_mode = math_mode
    return prm


def names_of(satur):
    return KEYS15 if satur else list(B.IN_NAMES)


def state(tab, nproma, ngptot, prm, satur):
    x, ptsphy, lay = make_inputs(tab, nproma, ngptot, prm)
    return {n: x[n] for n in names_of(satur)}, ptsphy, lay


def rel_err(got: torch.Tensor, want: torch.Tensor) -> float:
    d = float(torch.max(torch.abs(got - want)))
    m = float(torch.max(torch.abs(want)))
    return 0.0 if d == 0.0 else d / m if m > 0.0 else float("inf")


def parjac(x, prm, ptsphy, lay, sens=None, null_last=False):
    """cloudsc2_tl_launch_parjac into four NaN-prefilled blocks (``null_last``: the rpecons block all NULL); x without qsat: SATUR in the sweep"""
    sens = sens if sens is not None else [new(B.OUT_NAMES, lay, fill=NAN) for _ in P]
    blocks = (B.Outputs * len(P))(*(ag._block("out", s, lay) for s in (sens[:-1] if null_last else sens)))
    B.check(B.lib.cloudsc2_tl_launch_parjac(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, C.byref(ag._block("in", x, lay)),
                                            blocks, stream()))
    return sens


def single(x, zero, k, prm, ptsphy, lay):
    """cloudsc2_tl_launch_par (satur = 0) on zero-filled tangent planes with dpar = e_k, into NaN-prefilled outputs"""
    dy = new(B.OUT_NAMES, lay, fill=NAN)
    e = [0.0] * len(P)
    e[k] = 1.0
    B.check(B.lib.cloudsc2_tl_launch_par(C.byref(prm), ptsphy, lay.nproma, lay.nlev, lay.ngptot, 0, C.byref(ag._block("in", x, lay)),
                                         C.byref(ag._block("in", zero, lay)), (C.c_double * len(P))(*e), C.byref(ag._block("out", dy, lay)),
                                         stream()))
    return dy


def active(t, lay):
    """the active columns of every block as one (nlevx, ngptot) view-free tensor"""
    return t.transpose(0, 1).reshape(t.shape[1], -1)[:, :lay.ngptot]


def hip_runtime():
    """the HIP runtime this process already uses (the file torch mapped), for the graph queries torch does not wrap"""
    with open("/proc/self/maps") as maps:
        paths = sorted({line.split()[-1] for line in maps if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = C.CDLL(paths[0])
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipGraphGetEdges.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    return hip


# ---- the CPU checker of the parity tests (tests/test_gpu_parity.py; tools/fuzz_case.py) ----
def checker():
    if refcall.have_ref():
        return refcall.RefLib()
    return refcall.OracleLib()


def ref_qsat(chk, st):
    qsat = np.zeros_like(st.PAP)
    for ibl in range(st.nblocks):
        icend = min(st.nproma, st.ngptot - ibl * st.nproma)
        qsat[ibl] = chk.satur(np.ascontiguousarray(st.PAP[ibl]), np.ascontiguousarray(st.PT[ibl]), kfdia=icend)
        qsat[ibl][:, icend:] = 0.0
    return qsat


def ref_nl_state(chk, st, prm, qsat=None):
    """Reference outputs for a whole state: per-block SATUR + CLOUDSC2 exactly like cloudsc_driver_mod.F90:82-111."""
    out = st.copy()
    out.PCOVPTOT[...] = 0.0
    out.B_LOC[:, 7] = 0.0
    for ibl in range(st.nblocks):
        icend = min(st.nproma, st.ngptot - ibl * st.nproma)
        qs = qsat[ibl] if qsat is not None else chk.satur(np.ascontiguousarray(st.PAP[ibl]), np.ascontiguousarray(st.PT[ibl]), kfdia=icend)
        o = chk.cloudsc2(st.ptsphy, refcall.block_inputs(st, ibl, qs), kfdia=icend, ldrain1d=bool(prm.ldrain1d))
        for n, a in refcall.state_outputs_block(out, ibl).items():
            a[:, :icend] = o[n][:, :icend]
    return out


def assert_outputs_close(ref_st, got_st, tol):
    for n, r in ref_st.outputs().items():
        g = got_st.outputs()[n]
        assert np.all(np.isfinite(g)), n
        assert relerr(r, g) <= tol, (n, relerr(r, g))
        assert c2.validate_l1(r, g) <= tol, (n, c2.validate_l1(r, g))


def _device_tl_ad(tab, nproma, ngptot, flags):
    """Run TL then AD on the GPU at kernel level (device pointers) and with the checker; returns both result sets."""
    prm = c2.default_params(c2.ceta_from_table(tab), **flags)
    st = c2.state_from_table(tab, nproma, ngptot)
    nb, nlev = st.nblocks, st.nlev
    chk = checker()
    set_lib_params(chk, prm)
    qsat = ref_qsat(chk, st)

    ds = c2.DeviceState(st, "cuda:0")
    ds.satur(prm)
    torch.cuda.synchronize()
    q_dev = ds.QSAT.cpu().numpy()
    for ibl in range(nb):
        icend = min(nproma, ngptot - ibl * nproma)
        assert relerr(qsat[ibl][:, :icend], q_dev[ibl][:, :icend]) < 1e-14
    inc = ds.increments()
    tl_out = c2.FlatFields("out", nb, nlev, nproma, ds.device)
    ds.tl(prm, inc, tl_out)
    torch.cuda.synchronize()
    tl_dev = {n: t.cpu().numpy() for n, t in tl_out.t.items()}
    traj_dev = ds.download(st.copy())

    # checker TL
    inc_h = {n: t.cpu().numpy() for n, t in inc.t.items()}
    tl_ref = flat_fields("out", nb, nlev, nproma)
    traj_ref = st.copy()
    for ibl in range(nb):
        icend = min(nproma, ngptot - ibl * nproma)
        dinp = {n: np.ascontiguousarray(inc_h[n][ibl]) for n in inc_h}
        inp = refcall.block_inputs(st, ibl, qsat[ibl])
        for d in (inp, dinp):  # keep the checker away from the uninitialised tail
            for a in d.values():
                a[:, icend:] = 1.0
        o5, do = chk.cloudsc2tl(st.ptsphy, inp, dinp, kfdia=icend, ldrain1d=bool(prm.ldrain1d))
        for n in do:
            tl_ref[n][ibl][:, :icend] = do[n][:, :icend]
        for n, a in refcall.state_outputs_block(traj_ref, ibl).items():
            a[:, :icend] = o5[n][:, :icend]

    # AD with y = TL output (the adjoint test's choice, cloudsc_driver_ad_mod.F90:216-237), x pre-filled with a
    # non-zero background to check accumulation
    rng = np.random.default_rng(5)
    x0 = {n: rng.standard_normal(a.shape) * (np.abs(a).max() + 1e-30) for n, a in inc_h.items()}
    adj_in = c2.FlatFields("in", nb, nlev, nproma, ds.device)
    for n in x0:
        adj_in.t[n].copy_(torch.from_numpy(x0[n]))
    scratch = ds.new_scratch()
    ds.ad(prm, adj_in, tl_out, scratch)
    torch.cuda.synchronize()
    x_dev = {n: t.cpu().numpy() for n, t in adj_in.t.items()}
    y_after = {n: t.cpu().numpy() for n, t in tl_out.t.items()}

    x_ref = {n: a.copy() for n, a in x0.items()}
    for ibl in range(nb):
        icend = min(nproma, ngptot - ibl * nproma)
        inp = refcall.block_inputs(st, ibl, qsat[ibl])
        for a in inp.values():
            a[:, icend:] = 1.0
        ain = {n: x_ref[n][ibl].copy() for n in x_ref}
        aout = {n: tl_ref[n][ibl].copy() for n in tl_ref}  # consumed (zeroed) by the AD
        chk.cloudsc2ad(st.ptsphy, inp, ain, aout, kfdia=icend, ldrain1d=bool(prm.ldrain1d))
        for n in ain:
            x_ref[n][ibl][:, :icend] = ain[n][:, :icend]
    return dict(st=st, tl_dev=tl_dev, tl_ref=tl_ref, traj_dev=traj_dev, traj_ref=traj_ref, x_dev=x_dev, x_ref=x_ref,
                x0=x0, y_after=y_after, inc=inc_h)


def _run_fortran(exe, *args, cwd=None, env=None):
    path = os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "fortran", "build", exe)
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: run __graft_entry__.build()")
    full = None if env is None else {k: v for k, v in {**os.environ, **env}.items() if v != ""}  # (a variable set to "" is removed)
    r = subprocess.run([path, *map(str, args)], capture_output=True, text=True, timeout=300, cwd=cwd, env=full)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, r.stderr


# ---- the device-free argument tests (tests/test_autograd_*args.py): CPU and meta tensors ----
ARG_NB, ARG_NLEV, ARG_NPROMA = 3, 137, 32
K = 3  # members of the ensemble arguments


def arg_inputs(device="cpu", nb=ARG_NB, nlev=ARG_NLEV, nproma=ARG_NPROMA, dtype=None):
    dtype = dtype or B.torch_real()
    return {n: torch.ones((nb, nlev + (1 if n == "paph" else 0), nproma), dtype=dtype, device=device) for n in B.IN_NAMES}


def arg_params(nlev=ARG_NLEV, **kw):
    return c2.default_params(np.linspace(0.01, 1.0, nlev), **kw)


def bad_cases():
    x = arg_inputs(); x["t"] = x["t"].to(torch.float32 if not B.SINGLE else torch.float64)
    yield "dtype", x, arg_params(), "dtype"
    x = arg_inputs(); x["q"] = torch.ones((ARG_NB, ARG_NLEV - 1, ARG_NPROMA), dtype=B.torch_real())
    yield "nlev mismatch", x, arg_params(), "shape"
    yield "prm.nlev mismatch", arg_inputs(), arg_params(ARG_NLEV - 1), "prm.nlev"
    x = arg_inputs(); x["mfu"] = torch.ones((ARG_NB, ARG_NPROMA, ARG_NLEV), dtype=B.torch_real()).transpose(1, 2)
    yield "column stride", x, arg_params(), "column stride"
    x = arg_inputs(); x["lude"] = torch.ones((ARG_NB, ARG_NLEV, 2 * ARG_NPROMA), dtype=B.torch_real())[:, :, ::2]
    yield "column stride 2", x, arg_params(), "column stride"
    x = arg_inputs(); x["l"] = torch.ones(ARG_NB * ARG_NLEV * ARG_NPROMA, dtype=B.torch_real()).as_strided((ARG_NB, ARG_NLEV, ARG_NPROMA), (7, ARG_NPROMA, 1))
    yield "overlapping blocks", x, arg_params(), "overlap"
    yield "nlev > 200", arg_inputs(nlev=B.CLOUDSC2_MAX_NLEV + 1), arg_params(), "nlev"
    yield "lphylin = 0", arg_inputs(), _no_lphylin(), "lphylin"
    x = arg_inputs(); del x["supsat"]
    yield "missing name", x, arg_params(), "names"
    yield "ngptot", arg_inputs(), arg_params(), "ngptot"


def _no_lphylin():
    p = arg_params()
    p.lphylin = 0
    return p


def weights(device="cpu", names=("fplsl", "tent")):
    return {n: torch.ones(ARG_NLEV + (1 if n in ag.HALF_OUT else 0), dtype=B.torch_real(), device=device) for n in names}


def bad_weights(device):
    """(id, weights, what the message must contain)"""
    yield "not a mapping", [torch.ones(ARG_NLEV, dtype=B.torch_real(), device=device)], "weights must map"
    yield "none", None, "weights must map"
    yield "empty", {}, "weights is empty"
    w = weights(device); w["rain"] = w["tent"]
    yield "unknown name", w, "'rain'"
    w = weights(device); w["tent"] = [1.0] * ARG_NLEV
    yield "not a tensor", w, "weights['tent'] is not a tensor"
    w = weights(device); w["tent"] = torch.ones((1, ARG_NLEV), dtype=B.torch_real(), device=device)
    yield "not 1-D", w, "weights['tent'] must be 1-D"
    w = weights(device); w["tent"] = torch.ones(ARG_NLEV + 1, dtype=B.torch_real(), device=device)
    yield "full-level length", w, f"weights['tent'] has length {ARG_NLEV + 1}, expected {ARG_NLEV}"
    w = weights(device); w["fplsl"] = torch.ones(ARG_NLEV, dtype=B.torch_real(), device=device)
    yield "half-level length", w, f"weights['fplsl'] has length {ARG_NLEV}, expected {ARG_NLEV + 1}"
    w = weights(device); w["fplsl"] = w["fplsl"].to((torch.float32 if not B.SINGLE else torch.float64))
    yield "dtype", w, "weights['fplsl'] has dtype"
    if device == "cpu":
        w = weights(device); w["tent"] = w["tent"].clone().requires_grad_(True)
        yield "requires grad", w, "weights['tent'] requires grad"
        w = weights(device); w["tent"] = torch.ones(ARG_NLEV, dtype=B.torch_real(), device="meta")
        yield "other device", w, "weights['tent'] is on meta"


def pk(k=K, dtype=torch.float64, **kw):
    return torch.linspace(1.0, 2.0, k, dtype=torch.float64).to(dtype).requires_grad_(kw.get("requires_grad", False))


def four_d(t, k=K):
    return t.unsqueeze(0).repeat(k, 1, 1, 1)


def bad_params():
    yield {}, "empty"
    yield {"rlmin": pk()}, "unknown name"
    yield {"rkconv": pk(), "ptsphy": pk()}, "unknown name"
    yield {"rkconv": torch.tensor(1.0, dtype=torch.float64)}, "1-d"
    yield {"rkconv": torch.ones(K, 2, dtype=torch.float64)}, "1-d"
    yield {"rkconv": torch.ones(0, dtype=torch.float64)}, "1-d"
    yield {"rkconv": pk(dtype=torch.float32)}, "dtype"
    yield {"rkconv": torch.ones(K, dtype=torch.int64)}, "dtype"
    yield {"rkconv": pk(), "rlptrc": pk(K + 1)}, "common length"
    yield {"rlptrc": [250.0] * K}, "not a tensor"
    yield [("rkconv", pk())], "must map"
    yield None, "must map"


# ---- the launcher-refusal tests (tests/test_*refusals.py): two blocks, the second with a padded tail ----
R_NPROMA, R_NLEV, R_NGPTOT, R_NB = 8, 4, 12, 2
S, SH = R_NPROMA * R_NLEV, R_NPROMA * (R_NLEV + 1)  # block strides of the full-level and the half-level fields
R_HALF = ("paph", "fplsl", "fplsn", "fhpsl", "fhpsn")


def refusal_params(**kw) -> B.Params:
    p = c2.default_params(np.linspace(0.01, 1.0, R_NLEV))
    for n, v in kw.items():
        setattr(p, n, v)
    return p


class World:
    """The pointers of the calls: dummies without a device, else device memory allocated once and kept (4 x the extent of a field
    per field, so that a stride of a mismatch case stays inside too)."""

    def __init__(self, device: bool):
        self.device = device
        self.kept = {}

    def mem(self, key, n: int, real: bool = True) -> int:
        if not self.device:
            return 256
        if key not in self.kept:
            self.kept[key] = torch.zeros(n, dtype=B.torch_real() if real else torch.float64, device="cuda:0")
        return self.kept[key].data_ptr()

    def field(self, key, half: bool = False, stride: int | None = None) -> B.Field:
        f = B.Field()
        f.ptr = self.mem(key, 4 * R_NB * SH)
        f.block_stride = stride if stride is not None else (SH if half else S)
        return f

    def block(self, cls, names, tag, only=None, **edit):
        """edit[name] = None: a NULL field; an integer: that block stride.  only: the other fields are NULL."""
        blk = cls()
        for n in names:
            if (only is not None and n not in only) or (n in edit and edit[n] is None):
                continue
            setattr(blk, n, self.field((tag, n), n in R_HALF, edit.get(n)))
        return blk

    def ins(self, tag="traj", **edit) -> B.Inputs:
        return self.block(B.Inputs, B.IN_NAMES, tag, **edit)

    def outs(self, tag="traj", **edit) -> B.Outputs:
        return self.block(B.Outputs, B.OUT_NAMES, tag, **edit)

    def dbl(self, key, n: int = 128 * R_NB * R_NPROMA) -> C.c_void_p:
        return C.c_void_p(self.mem(key, n, real=False))

    def real(self, key, n: int = 4 * R_NB * SH) -> C.c_void_p:
        return C.c_void_p(self.mem(key, n))


class DistinctWorld(World):
    """World whose dummies differ from field to field: the sparse launchers refuse a written plane that is given twice"""

    def mem(self, key, n: int, real: bool = True) -> int:
        if self.device:
            return super().mem(key, n, real)
        return 4096 * (1 + self.kept.setdefault(key, len(self.kept)))


class SumWorld(DistinctWorld):
    def sums(self, tag, only=("fplsl", "fplsn"), **edit) -> B.Outputs:
        """a block of (nblocks, nproma) sums: block stride R_NPROMA unless edited"""
        blk = B.Outputs()
        for n in only:
            f = B.Field()
            f.ptr = self.mem((tag, n), 4 * 2 * SH)
            f.block_stride = edit.get(n, R_NPROMA)
            setattr(blk, n, f)
        return blk
