"""CLOUDSC2 as a differentiable PyTorch operation: the NL sweep forward, the TL sweep as its jvp, the reverse sweep of the adjoint
(in its vector-Jacobian form, ``cloudsc2_vjp_launch``) as its backward.

    out = cloudsc2(inputs, prm, ptsphy, ngptot=None)

``inputs`` maps every name of ``binding.IN_NAMES`` to a device tensor; ``out`` is a :class:`Cloudsc2Outputs` namedtuple over
``binding.OUT_NAMES``.  ``torch.autograd.grad`` / ``.backward()``, ``torch.autograd.forward_ad`` and ``torch.func.jvp`` / ``vjp`` /
``grad`` all work; double backward, vmap and gradients with respect to ``prm`` / ``ptsphy`` do not.

Layout.  Full-level fields are ``(nblocks, nlev, nproma)``, ``paph`` and the four fluxes ``(nblocks, nlev+1, nproma)``, in the
library's dtype (``binding.torch_real()``) on one HIP device, with column stride 1 and level stride ``nproma``: the blocked
``(NPROMA, NLEV, NBLOCKS)`` arrays of the reference.  Views are accepted, e.g. planes of a packed tendency buffer.  The kernels take
one block stride per layout group -- full-level (``pap q qsat t lude lu mfu mfd supsat``), ``PGTEN*`` (``gtent gtenq gtenl
gteni``), ``l i``, half-level (``paph``) -- and the outputs, which this op allocates contiguous, share the full-level and
half-level ones; a group that does not fit is copied contiguous first (the copy is an ordinary differentiable torch op).
Incoming gradients and tangents are treated the same way.  ``ngptot`` (default ``nblocks * nproma``) is the number of active
columns; the padded tail of the last block is zero in every output, gradient and tangent the op returns.

Semantics.
  * The derivatives are those of CLOUDSC2TL / CLOUDSC2AD, which linearise the LPHYLIN form of the scheme: ``prm.lphylin = 0`` is
    refused, because the forward would then not be the function its derivatives belong to.
  * With ``prm.lregcl`` the jvp and backward are the reference's *regularised* linearisation (cloudsc2tl.F90:575,657,754,794,998),
    not the exact derivative of the forward.
  * ``qsat`` is an ordinary differentiable input, as in CLOUDSC2TL / CLOUDSC2AD.  :func:`satur` computes it from ``pap`` and ``t``
    without a gradient: its result enters the op as a constant.
  * The ``supsat`` gradient is the true derivative (coefficient 1 in ZQP1, cloudsc2tl.F90:345), not CLOUDSC2AD's PTSPHY*ZQP1
    (cloudsc2ad.F90:1733); every other gradient equals ``cloudsc2_ad_launch_assign``'s input adjoint bit for bit.

Device and stream.  Every launch runs on the inputs' device, on ``torch.cuda.current_stream()``.  The first use on a device calls
``cloudsc2_device_prepare`` (a synchronous probe of the dispatcher).  Capturing the op in ``torch.cuda.graph`` therefore needs one
eager call first, with the same CETA: it runs that probe and uploads the per-level CETA table, neither of which may happen during
capture.
"""
from __future__ import annotations

import ctypes as C
import threading
from collections import namedtuple

import torch
from torch._C import _functorch
from torch.autograd.function import once_differentiable

from . import binding as B

Cloudsc2Outputs = namedtuple("Cloudsc2Outputs", B.OUT_NAMES)

HALF_IN = ("paph",)
HALF_OUT = ("fplsl", "fplsn", "fhpsl", "fhpsn")
# layout groups of the C ABI (resolve_in / resolve_out in csrc/cloudsc2_launch.hip): one block stride each; the output groups
# "full" and "half" must have the input groups' strides, "loc" is free
IN_GROUPS = {"full": ("pap", "q", "qsat", "t", "lude", "lu", "mfu", "mfd", "supsat"), "half": ("paph",),
             "cml": ("gtent", "gtenq", "gtenl", "gteni"), "clv": ("l", "i")}
OUT_GROUPS = {"loc": ("tent", "tenq", "tenl", "teni"), "full": ("clc", "covptot"), "half": HALF_OUT}


class Layout(namedtuple("Layout", "nblocks nlev nproma ngptot")):
    """Blocking of one call."""

    def nlevx(self, name: str) -> int:
        return self.nlev + (1 if name in HALF_IN or name in HALF_OUT else 0)

    def shape(self, name: str) -> tuple:
        return (self.nblocks, self.nlevx(name), self.nproma)

    @property
    def tail(self) -> int:
        """first padded column of the last block (nproma: no padding)"""
        return self.ngptot - (self.nblocks - 1) * self.nproma


def _block_stride(t: torch.Tensor, lay: Layout, name: str) -> int:
    # a dimension of size 1 has no meaningful stride: the kernels never step over it
    return t.stride(0) if lay.nblocks > 1 else lay.nlevx(name) * lay.nproma


def _fits(t: torch.Tensor, lay: Layout, name: str) -> bool:
    """column stride 1 and level stride nproma (the kernels' in-block addressing)"""
    return (lay.nproma == 1 or t.stride(2) == 1) and t.stride(1) == lay.nproma


def check_layout(inputs, prm: B.Params, ngptot: int | None = None) -> Layout:
    """Every check of :func:`cloudsc2` that needs no device: names, dtype, shapes, strides, ``ngptot``, ``nlev`` and the parameters.
    Runs on CPU or meta tensors; raises ``ValueError``."""
    names = set(inputs.keys()) if hasattr(inputs, "keys") else None
    if names is None or names != set(B.IN_NAMES):
        raise ValueError(f"inputs must map exactly the names {B.IN_NAMES}; got {sorted(names) if names is not None else type(inputs)}")
    dtype = B.torch_real()
    for n in B.IN_NAMES:
        t = inputs[n]
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"inputs[{n!r}] is not a tensor")
        if t.dtype != dtype:
            raise ValueError(f"inputs[{n!r}] has dtype {t.dtype}; this library works on {dtype} (CLOUDSC2_PRECISION)")
        if t.dim() != 3:
            raise ValueError(f"inputs[{n!r}] must be 3-D (nblocks, nlev{'+1' if n in HALF_IN else ''}, nproma); got shape {tuple(t.shape)}")
    nb, nlev, nproma = (int(s) for s in inputs["pap"].shape)
    if nb < 1 or nproma < 1:
        raise ValueError(f"empty inputs: shape {tuple(inputs['pap'].shape)}")
    if nlev < 2 or nlev > B.CLOUDSC2_MAX_NLEV:
        raise ValueError(f"nlev = {nlev}: 2 <= nlev <= {B.CLOUDSC2_MAX_NLEV} (CLOUDSC2_MAX_NLEV) required")
    lay = Layout(nb, nlev, nproma, nb * nproma if ngptot is None else int(ngptot))
    if not (nb - 1) * nproma < lay.ngptot <= nb * nproma:
        raise ValueError(f"ngptot = {lay.ngptot} does not fit {nb} blocks of nproma = {nproma} (the last block must hold 1..nproma columns)")
    for n in B.IN_NAMES:
        t = inputs[n]
        if tuple(t.shape) != lay.shape(n):
            raise ValueError(f"inputs[{n!r}] has shape {tuple(t.shape)}, expected {lay.shape(n)} (from pap: nblocks, nlev, nproma)")
        if not _fits(t, lay, n):
            raise ValueError(f"inputs[{n!r}] has strides {t.stride()}: column stride 1 and level stride nproma = {nproma} are required")
        if lay.nblocks > 1 and t.stride(0) < lay.nlevx(n) * nproma:
            raise ValueError(f"inputs[{n!r}] has block stride {t.stride(0)} < {lay.nlevx(n) * nproma}: its blocks overlap")
    if int(prm.nlev) != nlev:
        raise ValueError(f"prm.nlev = {prm.nlev} does not match the inputs' nlev = {nlev}")
    if not prm.lphylin:
        raise ValueError("prm.lphylin = 0: CLOUDSC2TL / CLOUDSC2AD linearise the LPHYLIN form only, the forward would not match its derivatives")
    if prm.math_mode not in (0, 1, 2):
        raise ValueError(f"prm.math_mode = {prm.math_mode}: 0, 1 or 2")
    return lay


def check_device(tensors) -> torch.device:
    """All tensors on one HIP device (the library has no CPU path); returns it.  Raises ``ValueError``."""
    devs = {t.device for t in tensors}
    if len(devs) != 1:
        raise ValueError(f"all tensors must be on one device; got {sorted(str(d) for d in devs)}")
    dev = devs.pop()
    if dev.type != "cuda":
        raise ValueError(f"tensors are on {dev}: CLOUDSC2 runs on a HIP device only (no CPU path)")
    return dev


def _group_fits(ts: dict, lay: Layout, names, want: int | None) -> bool:
    strides = {_block_stride(ts[n], lay, n) for n in names}
    if len(strides) != 1 or not all(_fits(ts[n], lay, n) for n in names):
        return False
    return want is None or strides.pop() == want


def normalize(ts: dict, lay: Layout, groups: dict) -> dict:
    """Copy contiguous every group of ``ts`` the launchers cannot take as it is: members of a group with different block strides, or
    a full-level / half-level group whose stride is not that of the contiguous arrays the op allocates (or a member without the
    in-block layout: expanded, zero-strided)."""
    out = dict(ts)
    for g, names in groups.items():
        want = lay.nlev * lay.nproma if g == "full" else (lay.nlev + 1) * lay.nproma if g == "half" else None
        if not _group_fits(out, lay, names, want):
            for n in names:
                out[n] = out[n].contiguous()
    return out


def _raw(t: torch.Tensor) -> torch.Tensor:
    """the plain tensor inside torch.func's wrappers (its transforms hand jvp / backward wrapped tensors, which have no data pointer
    of their own; the wrapper's value shares the storage)"""
    while _functorch.is_functorch_wrapped_tensor(t):
        t = _functorch.get_unwrapped(t)
    return t


def _field(t: torch.Tensor | None, lay: Layout, name: str) -> B.Field:
    f = B.Field()
    if t is not None:
        t = _raw(t)
        f.ptr = t.data_ptr()
        f.block_stride = _block_stride(t, lay, name)
    return f


def _block(kind: str, ts: dict, lay: Layout):
    blk = B.Inputs() if kind == "in" else B.Outputs()
    for n, t in ts.items():
        setattr(blk, n, _field(t, lay, n))
    return blk


def _new(names, lay: Layout, like: torch.Tensor) -> dict:
    """fresh contiguous arrays, padded tail zeroed (that slice only)"""
    out = {}
    for n in names:
        t = torch.empty(lay.shape(n), dtype=like.dtype, device=like.device)
        if lay.tail < lay.nproma:
            t[-1, :, lay.tail:] = 0
        out[n] = t
    return out


_prepared: set = set()
_prepare_lock = threading.Lock()


def _prepare(dev: torch.device) -> None:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _prepared:
        return
    with _prepare_lock:
        if idx not in _prepared:
            with torch.cuda.device(idx):
                B.check(B.lib.cloudsc2_device_prepare())
            _prepared.add(idx)


def _stream(dev: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _evap(prm: B.Params) -> bool:
    return bool(prm.levapls2 or prm.ldrain1d)


class _Cloudsc2(torch.autograd.Function):
    # forward(prm, ptsphy, layout, *16 inputs in IN_NAMES order) -> 10 outputs + the cover-checkpoint scratch (non-differentiable)

    @staticmethod
    def forward(prm, ptsphy, lay, *xs):
        x = dict(zip(B.IN_NAMES, xs))
        like = x["pap"]
        dev = like.device
        out = _new(B.OUT_NAMES, lay, like)
        scratch = torch.empty((lay.nblocks, lay.nlev, lay.nproma) if _evap(prm) else (0,), dtype=like.dtype, device=dev)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                     C.byref(_block("in", x, lay)), C.byref(_block("out", out, lay)),
                                                     C.c_void_p(_raw(scratch).data_ptr() if scratch.numel() else None), _stream(dev)))
        return tuple(out[n] for n in B.OUT_NAMES) + (scratch,)

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, *xs = inputs
        out = dict(zip(B.OUT_NAMES, output[:-1]))
        scratch = output[-1]
        ctx.mark_non_differentiable(scratch)
        ctx.save_for_backward(*xs, out["fplsl"], out["fplsn"], scratch)
        ctx.save_for_forward(*xs)
        ctx.prm, ctx.ptsphy, ctx.lay = prm, ptsphy, lay

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        x = dict(zip(B.IN_NAMES, saved[:16]))
        fplsl, fplsn, scratch = saved[16:]
        lay, like = ctx.lay, x["pap"]
        dev = like.device
        need = ctx.needs_input_grad[3:]
        if not any(need):
            return (None, None, None) + (None,) * 16
        y = {}
        zeros = {}
        for n, g in zip(B.OUT_NAMES, grads[:10]):
            if g is None:  # an output that took no part in the loss: a zero adjoint (read only, so one plane per shape serves all)
                key = lay.nlevx(n)
                if key not in zeros:
                    zeros[key] = torch.zeros(lay.shape(n), dtype=like.dtype, device=dev)
                g = zeros[key]
            y[n] = g
        y = normalize(y, lay, OUT_GROUPS)
        xa = _new(B.IN_NAMES, lay, like)
        traj_out = B.Outputs()
        traj_out.fplsl, traj_out.fplsn = _field(fplsl, lay, "fplsl"), _field(fplsn, lay, "fplsn")
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch(C.byref(ctx.prm), float(ctx.ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                              C.byref(_block("in", x, lay)), C.byref(traj_out), C.byref(_block("in", xa, lay)),
                                              C.byref(_block("out", y, lay)),
                                              C.c_void_p(_raw(scratch).data_ptr() if scratch.numel() else None), _stream(dev)))
        return (None, None, None) + tuple(xa[n] if nd else None for n, nd in zip(B.IN_NAMES, need))

    @staticmethod
    def jvp(ctx, *tangents):
        x = dict(zip(B.IN_NAMES, ctx.saved_tensors))
        lay, like = ctx.lay, x["pap"]
        dev = like.device
        dx = {}
        zeros = {}
        for n, t in zip(B.IN_NAMES, tangents[3:]):
            if t is None:  # no tangent: zero (read only, one plane per shape)
                key = lay.nlevx(n)
                if key not in zeros:
                    zeros[key] = torch.zeros(lay.shape(n), dtype=like.dtype, device=dev)
                t = zeros[key]
            dx[n] = t
        dx = normalize(dx, lay, IN_GROUPS)
        dy = _new(B.OUT_NAMES, lay, like)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch(C.byref(ctx.prm), float(ctx.ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                             C.byref(_block("in", x, lay)), C.byref(B.Outputs()),  # no trajectory stores
                                             C.byref(_block("in", dx, lay)), C.byref(_block("out", dy, lay)), _stream(dev)))
        return tuple(dy[n] for n in B.OUT_NAMES) + (None,)


def cloudsc2(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None) -> Cloudsc2Outputs:
    """SATUR-free CLOUDSC2 (``qsat`` is an input) over all blocks as a differentiable op; see the module docstring."""
    lay = check_layout(inputs, prm, ngptot)
    dev = check_device(inputs[n] for n in B.IN_NAMES)
    _prepare(dev)
    x = normalize({n: inputs[n] for n in B.IN_NAMES}, lay, IN_GROUPS)
    out = _Cloudsc2.apply(prm, float(ptsphy), lay, *(x[n] for n in B.IN_NAMES))
    return Cloudsc2Outputs(*out[:10])


def satur(pap: torch.Tensor, t: torch.Tensor, prm: B.Params, ngptot: int | None = None) -> torch.Tensor:
    """SATUR (satur.F90:106-123, the LPHYLIN branch the drivers call) into a new ``(nblocks, nlev, nproma)`` tensor, with NO
    gradient: passed to :func:`cloudsc2` as ``qsat`` it is a constant input there (differentiate through ``qsat`` only as an input
    of its own, as CLOUDSC2TL / CLOUDSC2AD do)."""
    for n, a in (("pap", pap), ("t", t)):
        if not isinstance(a, torch.Tensor) or a.dtype != B.torch_real() or a.dim() != 3:
            raise ValueError(f"{n} must be a 3-D {B.torch_real()} tensor")
    if tuple(pap.shape) != tuple(t.shape):
        raise ValueError(f"pap {tuple(pap.shape)} and t {tuple(t.shape)} differ in shape")
    nb, nlev, nproma = (int(s) for s in pap.shape)
    lay = Layout(nb, nlev, nproma, nb * nproma if ngptot is None else int(ngptot))
    if not (nb - 1) * nproma < lay.ngptot <= nb * nproma or not 2 <= nlev <= B.CLOUDSC2_MAX_NLEV or int(prm.nlev) != nlev:
        raise ValueError(f"satur: shape {tuple(pap.shape)}, ngptot {lay.ngptot} and prm.nlev {prm.nlev} do not fit together")
    dev = check_device((pap, t))
    with torch.no_grad():
        pap, t = pap.detach().contiguous(), t.detach().contiguous()
        q = _new(("qsat",), lay, pap)["qsat"]
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_satur_launch(C.byref(prm), nproma, nlev, lay.ngptot, _field(pap, lay, "pap"), _field(t, lay, "t"),
                                                _field(q, lay, "qsat"), _stream(dev)))
    return q
