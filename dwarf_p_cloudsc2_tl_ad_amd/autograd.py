"""CLOUDSC2 as a differentiable PyTorch operation: the NL sweep forward, the TL sweep as its jvp, the reverse sweep of the adjoint
(in its vector-Jacobian form, ``cloudsc2_vjp_launch``) as its backward.

    out = cloudsc2(inputs, prm, ptsphy, ngptot=None, satur=False, params=None, sparse=False)

``inputs`` maps every name of ``binding.IN_NAMES`` to a device tensor (with ``satur=True``: every name but ``qsat``); ``out`` is a :class:`Cloudsc2Outputs` namedtuple over
``binding.OUT_NAMES``.  ``torch.autograd.grad`` / ``.backward()``, ``torch.autograd.forward_ad`` and ``torch.func.jvp`` / ``vjp`` /
``grad`` / ``vmap`` / ``jacfwd`` / ``jacrev`` all work; double backward, nested vmap, ``torch.autograd.grad(...,
is_grads_batched=True)`` (use ``torch.func.vmap`` of the vjp function instead) and gradients with respect to ``ptsphy`` do not.

Parameters.  ``params`` maps any subset of ``PARAM_NAMES`` (``rkconv``, ``rclcrit``, ``rlptrc``, ``rpecons``: the four constants of
``prm`` that enter CLOUDSC2 smoothly) to 0-d ``float64`` tensors, on the CPU or on the inputs' device.  Their values override those
fields of a *copy* of ``prm`` -- the forward is bit for bit ``cloudsc2(inputs, prm_with_those_values, ...)`` -- and the op is
differentiable with respect to them: ``loss(out).backward()`` leaves a 0-d float64 ``.grad`` on each parameter's device next to the
field gradients (which are the bits of the op without ``params``), ``torch.func.grad`` / ``vjp``, ``forward_ad`` and
``torch.func.jvp`` work.  Backward is one ``cloudsc2_vjp_launch_par`` (the reverse sweep sums each column's contributions in four
doubles, a second kernel folds them in a fixed order: the same bits from run to run), or today's launch when no parameter needs a
gradient; jvp is one ``cloudsc2_tl_launch_par``.  The constants travel in the kernel-argument segment, so the parameters' values
(and, in forward mode, their tangents) are read on the HOST: that synchronises when they live on the device, returning a gradient
to a CPU parameter copies four doubles back, and the op refuses ``params`` while the stream is capturing.  Any ``torch.func.vmap``
level over the op with ``params`` (so also ``jacfwd`` / ``jacrev``) raises ``NotImplementedError``: use the unbatched calls, one
direction at a time.  With the evaporation branch ``rpecons`` must not be 0.  The whole parameter Jacobian -- ``d out / d p`` for
all four parameters, what a Gauss-Newton or Levenberg-Marquardt calibration needs -- is :func:`param_jacobian`: one
``cloudsc2_tl_launch_parjac``, the trajectory read once and no tangent plane read, every entry the ``torch.func.jvp`` of the op
with a unit tangent on that parameter.  Such a step itself needs only ``J^T W J`` and ``J^T W r``: :func:`param_normal_equations` forms
them in one ``cloudsc2_parnormal_launch`` without the Jacobian ever being written.

Ensembles.  ``cloudsc2_ensemble(inputs, prm, ptsphy, ngptot, satur, params={name: (K,) device tensor})`` runs K parameter sets -- a
perturbed-parameter ensemble, over one shared state or over one 4-D state per member -- in one launch per sweep and reads the
parameters ON THE DEVICE: each member has an argument block of its own in device memory, whose constants a small kernel derives from
the member's row of a ``(K, 4)`` table (``cloudsc2_nl_launch_ens`` / ``cloudsc2_tl_launch_ens`` / ``cloudsc2_vjp_launch_ens``).  So it
neither synchronises nor refuses stream capture, and the ensemble is the batch that ``vmap`` over ``params`` does not give; every
member is the bits of the 0-d ``params`` call with its row.  The 0-d ``params`` path above keeps its host read on purpose: it is
the one launch whose constants sit in the kernel-argument segment, its bits, launch log and refusals are what callers and tests rely
on, and a single parameter set has no table to derive on the device.

Parameter maps.  ``cloudsc2_param_maps(inputs, prm, ptsphy, ngptot, satur, params={name: (nblocks, nproma) device tensor})`` is the
spatial counterpart of the ensemble: the four constants are FIELDS, a value per column.  Before the level loop a lane loads its four
doubles from a ``(4, nblocks, nproma)`` table and derives its constants with the host's expressions in their order
(``cloudsc2_nl_launch_parmap`` / ``cloudsc2_tl_launch_parmap`` / ``cloudsc2_vjp_launch_parmap``); the gradient of a map is the lane's
four parameter adjoints, stored per column with no fold.  Nothing is read on the host, so it captures in a graph like the ensemble;
column c of every output and field gradient is the bits of the 0-d ``params`` call with column c's values.

Sparse losses.  A loss usually touches a few outputs (surface precipitation, the ``t`` / ``q`` tendencies) and wants a few gradients
(``t``, ``q``), yet the dense backward reads ten cotangent planes -- zeros allocated for the outputs that took no part -- and writes
all 16 gradients before ``needs_input_grad`` throws most away.  ``cloudsc2(..., sparse=True)`` is the same forward with gradients
left unmaterialised: backward is one ``cloudsc2_vjp_launch_sparse`` over the cotangents that exist and the gradients that are
wanted (nothing else is allocated, read or written; the other inputs get ``None``), jvp one ``cloudsc2_tl_launch_sparse`` over the
tangents that exist (all ten output tangents are stored).  Every plane is the bits of ``sparse=False``.  With every plane present
the dense sweeps run; with no cotangent nothing is launched; batched directions under ``vmap`` / ``jacfwd`` / ``jacrev`` go through
the dense batched rules on zero-filled planes; where ``torch.func`` hands over materialised zeros the op moves more planes and returns
the same bits.  Not with ``params`` (``NotImplementedError``); the default stays ``sparse=False``.

Batches.  Under ``torch.func.vmap`` the op distinguishes two cases.  Several tangents or cotangents over ONE state -- ``jacfwd``,
``jacrev``, ``vmap(jvp)``, ``vmap(vjp_fn)`` -- are one ``cloudsc2_tl_launch_batch`` / ``cloudsc2_vjp_launch_batch`` call: the
trajectory is read once per ``cloudsc2_batch_max()`` directions instead of once per direction, and every direction's result is the
bits of the unbatched call.  A batch of STATES (``vmap`` of the op itself, with or without batched directions) is
folded into the block dimension, columns being independent: one launch over ``K * nblocks`` blocks when the blocks are full, one
launch per state when ``ngptot`` leaves a padded tail (which must stay zero, and uncomputed, in every member).

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
  * The parameter derivative is the library's own (the reference has none).  Its local partials are exact derivatives of the
    forward; the resulting perturbation travels down the column through the same linearisation as the field tangents.  So with
    ``prm.lregcl`` it is regularised exactly where CLOUDSC2TL is and is not the exact derivative; with ``lregcl = 0`` it is.
    ``d zfwat / d rlptrc = -d zfwat / dT`` at cold points, 0 elsewhere.  Exact zeros: ``clc`` and ``covptot`` depend on none of the
    four; without the evaporation branch nothing depends on ``rpecons``; with it ``teni`` does not depend on ``rclcrit``.
  * ``qsat`` is an ordinary differentiable input, as in CLOUDSC2TL / CLOUDSC2AD.  :func:`satur` computes it from ``pap`` and ``t``
    without a gradient by default: its result then enters the op as a constant.
  * ``satur=True`` differentiates what the drivers compute, ``pap, t -> SATUR -> CLOUDSC2`` (cloudsc_driver_mod.F90:91): ``inputs``
    has no ``qsat``, SATUR (satur.F90:106-123) and its two partial derivatives are evaluated inside the sweeps
    (``cloudsc2_tl_launch_satur`` / ``cloudsc2_vjp_launch_satur``; no qsat plane is read, written or saved), and the ``pap`` / ``t``
    gradients carry the saturation humidity's share.  The reference has no SATURTL / SATURAD: this derivative is the library's
    own.  ``satur(pap, t, prm, differentiable=True)`` fed to the plain op is the same function unfused (three more planes, a launch
    and torch's chain rule) for a caller who needs ``qsat`` itself; the two routes agree to 1e-11 of a field's maximum.  Batched
    directions over one state (``jacfwd``, ``jacrev``, ``vmap(jvp)``, ``vmap(vjp_fn)``) of the ``satur=True`` op run by composition
    -- one ``cloudsc2_satur_lin_launch``, the chain rule in torch, the batched sweeps with ``qsat`` as a plane -- so for them the
    promise is that tolerance, not the bits of the unbatched fused call; a batch of states folds into the blocks as always.
  * The ``supsat`` gradient is the true derivative (coefficient 1 in ZQP1, cloudsc2tl.F90:345), not CLOUDSC2AD's PTSPHY*ZQP1
    (cloudsc2ad.F90:1733); every other gradient equals ``cloudsc2_ad_launch_assign``'s input adjoint bit for bit.

Device and stream.  Every launch runs on the inputs' device, on ``torch.cuda.current_stream()``.  The first use on a device calls
``cloudsc2_device_prepare`` (a synchronous probe of the dispatcher).  Capturing the op in ``torch.cuda.graph`` therefore needs one
eager call first, with the same CETA: it runs that probe and uploads the per-level CETA table, neither of which may happen during
capture.

Column sums.  ``cloudsc2_column_sums(inputs, prm, ptsphy, ngptot, weights={name: w}, satur=...)`` returns per-column weighted level
sums ``y_n[c] = sum_k w_n[k] out_n[k, c]`` of the outputs, formed in the sweeps (``cloudsc2_{nl,tl,vjp}_launch_colsum``): neither the
output planes nor their cotangent or tangent planes exist.  Its docstring has the contract.
"""
from __future__ import annotations

import copy
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
# satur=True: SATUR is evaluated and differentiated inside the sweeps, qsat exists on no side
SAT_NAMES = tuple(n for n in B.IN_NAMES if n != "qsat")
SAT_GROUPS = {g: tuple(n for n in names if n != "qsat") for g, names in IN_GROUPS.items()}
PARAM_NAMES = B.PARAM_NAMES  # the constants of prm that cloudsc2(..., params=...) differentiates
FPLSL, FPLSN = B.OUT_NAMES.index("fplsl"), B.OUT_NAMES.index("fplsn")  # the two outputs the reverse sweep re-reads


def _names(satur: bool):
    return (SAT_NAMES, SAT_GROUPS) if satur else (B.IN_NAMES, IN_GROUPS)


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


def _check_names(inputs, satur: bool) -> tuple:
    """``inputs`` maps exactly the names of this form of the op, which are returned; raises ``ValueError``"""
    IN_NAMES = SAT_NAMES if satur else B.IN_NAMES
    names = set(inputs.keys()) if hasattr(inputs, "keys") else None
    if satur and names is not None and "qsat" in names:
        raise ValueError("satur=True: SATUR is evaluated and differentiated inside the op, inputs must not have a 'qsat'")
    if names is None or names != set(IN_NAMES):
        raise ValueError(f"inputs must map exactly the names {IN_NAMES}; got {sorted(names) if names is not None else type(inputs)}")
    return IN_NAMES


def check_layout(inputs, prm: B.Params, ngptot: int | None = None, satur: bool = False) -> Layout:
    """Every check of :func:`cloudsc2` that needs no device: names, dtype, shapes, strides, ``ngptot``, ``nlev`` and the parameters.
    Runs on CPU or meta tensors; raises ``ValueError``.  ``satur``: the names are those of ``SAT_NAMES`` (no ``qsat``)."""
    IN_NAMES = _check_names(inputs, satur)
    dtype = B.torch_real()
    for n in IN_NAMES:
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
    for n in IN_NAMES:
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


def _member0(t: torch.Tensor) -> torch.Tensor:
    """the first member of a 4-D ensemble tensor ``(K, nblocks, nlevx, nproma)``; a 3-D tensor as it is"""
    return t[0] if t.dim() == 4 else t


def _group_fits(ts: dict, lay: Layout, names, want: int | None) -> bool:
    ts = {n: _member0(ts[n]) for n in names}
    strides = {_block_stride(ts[n], lay, n) for n in names}
    if len(strides) != 1 or not all(_fits(ts[n], lay, n) for n in names):
        return False
    return want is None or strides.pop() == want


def normalize(ts: dict, lay: Layout, groups: dict) -> dict:
    """Copy contiguous every group of ``ts`` the launchers cannot take as it is: members of a group with different block strides, or
    a full-level / half-level group whose stride is not that of the contiguous arrays the op allocates (or a member without the
    in-block layout: expanded, zero-strided).  The tensors of an ensemble are 3-D (shared) or 4-D (one per member): its launchers
    take one block stride per layout group and any member stride per field."""
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
    while True:
        if _functorch.is_batchedtensor(t) or _functorch.is_legacy_batchedtensor(t):
            # a batch dimension the vmap rules below have not taken off: a nested vmap, or the legacy batching of
            # torch.autograd.grad(..., is_grads_batched=True), which does not go through them -- its data pointer is not a field's
            raise NotImplementedError("cloudsc2: a batched tensor reached a launcher (nested vmap and is_grads_batched=True are not "
                                      "supported; use one level of torch.func.vmap / jacfwd / jacrev)")
        if not _functorch.is_functorch_wrapped_tensor(t):
            return t
        t = _functorch.get_unwrapped(t)


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


def _new(names, lay: Layout, like: torch.Tensor, batch: int | None = None) -> dict:
    """fresh contiguous arrays, padded tail zeroed (that slice only); batch: ``(batch, *shape)``, one member per direction"""
    out = {}
    for n in names:
        t = torch.empty(((batch,) if batch is not None else ()) + lay.shape(n), dtype=like.dtype, device=like.device)
        if lay.tail < lay.nproma:
            t[..., -1, :, lay.tail:] = 0
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


def _scratch_ptr(scratch: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(_raw(scratch).data_ptr() if scratch.numel() else None)


def _zero_filled(names, ts, lay: Layout, like: torch.Tensor) -> dict:
    """``ts`` by name with a zero plane for every None (no tangent / an output that took no part in the loss): read only, so one
    plane per shape serves all"""
    out, zeros = {}, {}
    for n, t in zip(names, ts):
        if t is None:
            key = lay.nlevx(n)
            if key not in zeros:
                zeros[key] = torch.zeros(lay.shape(n), dtype=like.dtype, device=like.device)
            t = zeros[key]
        out[n] = t
    return out


def _forward_launch(prm, ptsphy, lay: Layout, x: dict) -> tuple:
    """the forward of every form of the op: ``cloudsc2_ad_launch_forward`` over the inputs ``x`` (with ``qsat``, or without it: SATUR
    evaluated in the sweep) -> the 10 outputs and the cover-checkpoint scratch (empty without the evaporation branch)"""
    like = x["pap"]
    dev = like.device
    out = _new(B.OUT_NAMES, lay, like)
    scratch = torch.empty((lay.nblocks, lay.nlev, lay.nproma) if _evap(prm) else (0,), dtype=like.dtype, device=dev)
    with torch.cuda.device(dev):
        B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                 C.byref(_block("in", x, lay)), C.byref(_block("out", out, lay)),
                                                 _scratch_ptr(scratch), _stream(dev)))
    return tuple(out[n] for n in B.OUT_NAMES) + (scratch,)


# ---- what the vmap rules share --------------------------------------------------------------------------------------------------
# torch.func.vmap hands a rule its operands with the batch level taken off and ``in_dims`` (None: not batched).  The three functions
# below share one treatment.  ``traj`` operands batched: a batch of states (_fold).  Only direction operands batched: one batched
# launch.  Nothing batched: the plain call.

def _batch_size(in_dims, ts) -> int | None:
    sizes = {t.shape[d] for t, d in zip(ts, in_dims) if d is not None}
    if len(sizes) > 1:
        raise ValueError(f"cloudsc2 under vmap: operands with different batch sizes {sorted(sizes)}")
    return sizes.pop() if sizes else None


def _refuse_nested(ts) -> None:
    for t in ts:
        if isinstance(t, torch.Tensor) and (_functorch.is_batchedtensor(_peel_grad(t)) or _functorch.is_legacy_batchedtensor(t)):
            raise NotImplementedError("cloudsc2: nested vmap is not supported (one level of torch.func.vmap / jacfwd / jacrev is)")


def _peel_grad(t: torch.Tensor) -> torch.Tensor:
    while _functorch.is_gradtrackingtensor(t):
        t = _functorch.get_unwrapped(t)
    return t


def _front(t: torch.Tensor, d: int | None) -> torch.Tensor:
    return t if d is None else t.movedim(d, 0)


def _fold(fn, lay: Layout, names, ts, in_dims, out_names):
    """A batch of K states through ``fn(layout, tensors) -> tuple`` (the unbatched call).  Columns are independent, so with full
    blocks the batch is folded into the block dimension -- ``(K * nblocks, nlevx, nproma)``, unbatched operands expanded -- and run
    as one call.  With a padded tail (``ngptot < nblocks * nproma``) the tail of every member would lie in the middle of the folded
    array, where it has to stay zero and uncomputed: then one call per state.  Returns the outputs stacked, ``(K, *shape)``;
    members of ``out_names`` that are None name outputs without the field layout (the empty cover scratch), returned as they are."""
    K = _batch_size(in_dims, ts)
    ts = [_front(t, d) for t, d in zip(ts, in_dims)]
    if lay.tail == lay.nproma:
        folded = Layout(K * lay.nblocks, lay.nlev, lay.nproma, K * lay.nblocks * lay.nproma)
        flat = []
        for n, t, d in zip(names, ts, in_dims):
            if t.dim() != 3 + (d is not None):  # (the empty cover scratch of a call without the evaporation branch)
                flat.append(t)
                continue
            t = t if d is not None else t.unsqueeze(0).expand(K, *t.shape)
            flat.append(t.reshape(K * lay.nblocks, *t.shape[2:]))
        outs = fn(folded, flat)
        return tuple(o if n is None else o.reshape(K, lay.nblocks, *o.shape[1:]) for n, o in zip(out_names, outs))
    per_state = [fn(lay, [t if d is None else t[k] for t, d in zip(ts, in_dims)]) for k in range(K)]
    return tuple(per_state[0][j] if n is None else torch.stack([r[j] for r in per_state]) for j, n in enumerate(out_names))


def _directions(names, ts, in_dims, K: int, lay: Layout, groups: dict) -> list:
    """K dicts name -> tensor, one per direction: member k of a batched operand, the shared tensor of an unbatched one; each
    direction's groups normalized (all alike: the members of one batched tensor share their strides)"""
    ts = [_front(t, d) for t, d in zip(ts, in_dims)]
    return [normalize({n: (t if d is None else t[k]) for n, t, d in zip(names, ts, in_dims)}, lay, groups) for k in range(K)]


def _block_array(kind: str, per_direction: list, lay: Layout):
    typ = B.Inputs if kind == "in" else B.Outputs
    return (typ * len(per_direction))(*[_block(kind, d, lay) for d in per_direction])


def _vmap_states(cls, in_dims, prm, ptsphy, lay: Layout, satur: bool, xs):
    """The vmap rule of an op-level Function ``cls`` with the operands ``(prm, ptsphy, layout, satur, *inputs)``: nothing batched is
    the plain call, a batch of states is folded into the blocks (:func:`_fold`); the cover scratch is batched only where it exists."""
    _refuse_nested(xs)
    names, groups = _names(satur)
    dims = in_dims[4:]
    if _batch_size(dims, xs) is None:
        return cls.apply(prm, ptsphy, lay, satur, *xs), (None,) * 11

    def one(l, flat):
        x = normalize(dict(zip(names, flat)), l, groups)
        return cls.apply(prm, ptsphy, l, satur, *(x[n] for n in names))
    evap = _evap(prm)
    outs = _fold(one, lay, names, xs, dims, B.OUT_NAMES + ("scratch" if evap else None,))
    return outs, (0,) * 10 + (0 if evap else None,)


# ---- what the Function classes share ---------------------------------------------------------------------------------------------
# An op-level Function (_Cloudsc2, _Cloudsc2Par, _Cloudsc2Sparse, _Cloudsc2Ens, _Cloudsc2Colsum) is the forward launch; its jvp and
# backward each apply an inner Function (...Tl, ...Vjp), which is one launcher of the C ABI.

def _inner(raises: str | None):
    """Class decorator of an inner Function: what differentiating it again does.  ``raises=None`` (dense, par, sparse): its outputs
    are marked non-differentiable, and it is reached under ``once_differentiable``.  ``raises=message`` (ens, colsum): its
    ``backward`` and ``jvp`` raise ``NotImplementedError(message)``."""
    def decorate(cls):
        if raises is None:
            def setup_context(ctx, inputs, output):
                ctx.mark_non_differentiable(*output)
        else:
            def setup_context(ctx, inputs, output):
                pass

            def refuse(ctx, *args):
                raise NotImplementedError(raises)
            cls.backward = cls.jvp = staticmethod(refuse)
        cls.setup_context = staticmethod(setup_context)
        return cls
    return decorate


def _no_vmap(message: str):
    """Class decorator of a Function of a family without vmap rules: ``vmap`` raises ``NotImplementedError(message)``"""
    def decorate(cls):
        def vmap(info, in_dims, *args):
            raise NotImplementedError(message)
        cls.vmap = staticmethod(vmap)
        return cls
    return decorate


def _split(names, ts) -> tuple:
    """the tensor operands of a ...Vjp Function: the trajectory inputs by name, PFPLSL5, PFPLSN5, the cover scratch, the cotangents"""
    n = len(names)
    return (dict(zip(names, ts[:n])), *ts[n:n + 3], ts[n + 3:])


def _traj_out(fplsl, fplsn, lay: Layout) -> B.Outputs:
    """the trajectory outputs the reverse sweeps re-read: the two precipitation fluxes, every other field NULL"""
    out = B.Outputs()
    out.fplsl, out.fplsn = _field(fplsl, lay, "fplsl"), _field(fplsn, lay, "fplsn")
    return out


def _save_trajectory(ctx, xs, fplsl, fplsn, scratch, table=None, fluxes_are_outputs: bool = True, materialize: bool = True, **attrs) -> None:
    """The ``setup_context`` of the op-level Functions: the inputs, PFPLSL5, PFPLSN5 and the cover scratch saved for backward, the
    inputs for jvp, behind the family's device table where it has one; the scratch (and the fluxes, where they are kept planes and
    not outputs) non-differentiable; ``materialize=False``: backward sees None for an output that took no part in the loss;
    ``attrs`` are set on ``ctx``."""
    lead = () if table is None else (table,)
    ctx.mark_non_differentiable(*(() if fluxes_are_outputs else (fplsl, fplsn)), scratch)
    if not materialize:
        ctx.set_materialize_grads(False)
    ctx.save_for_backward(*lead, *xs, fplsl, fplsn, scratch)
    ctx.save_for_forward(*lead, *xs)
    for k, v in attrs.items():
        setattr(ctx, k, v)


def _enter(inputs, prm: B.Params, ngptot, satur: bool, check=None, *more) -> tuple:
    """What the public entry points begin with: the names and layout groups of this form, the device-free checks (``check``:
    :func:`check_layout`, or the entry point's own, which ends in it) and the device check -> (names, groups, what ``check``
    returned, device)"""
    names, groups = _names(satur)
    checked = (check or check_layout)(inputs, prm, ngptot, bool(satur), *more)
    return names, groups, checked, check_device(inputs[n] for n in names)


def _apply(cls, lead: tuple, inputs, names, groups: dict, lay: Layout) -> tuple:
    """What the public entry points end with: the groups the launchers cannot take copied contiguous, then the Function"""
    x = normalize({n: inputs[n] for n in names}, lay, groups)
    return cls.apply(*lead, *(x[n] for n in names))


# ---- satur=True: pap, t -> SATUR -> CLOUDSC2, differentiated through SATUR inside the sweeps -------------------------------------

def _satur_planes(prm, lay: Layout, pap: torch.Tensor, t: torch.Tensor, want_qsat: bool = True):
    """``cloudsc2_satur_lin_launch``: (qsat or None, dqs/dpap, dqs/dt) as new contiguous planes, padded tail zero"""
    dev = pap.device
    pap, t = pap.contiguous(), t.contiguous()
    new = _new(("qsat", "dqs_dpap", "dqs_dt") if want_qsat else ("dqs_dpap", "dqs_dt"), lay, pap)
    with torch.cuda.device(dev):
        B.check(B.lib.cloudsc2_satur_lin_launch(C.byref(prm), lay.nproma, lay.nlev, lay.ngptot, _field(pap, lay, "pap"), _field(t, lay, "t"),
                                                _field(new.get("qsat"), lay, "qsat"), _field(new["dqs_dpap"], lay, "pap"),
                                                _field(new["dqs_dt"], lay, "pap"), _stream(dev)))
    return new.get("qsat"), new["dqs_dpap"], new["dqs_dt"]


def _with_qsat(x15: dict, qsat) -> list:
    return [qsat if n == "qsat" else x15[n] for n in B.IN_NAMES]


# ---- the dense op: every plane of every cotangent and tangent, with qsat as an input or (satur) SATUR in the sweeps -----------------
# Batched directions over ONE state are one batched launch over the 16 inputs.  With satur they run by composition: SATUR's partials
# once (cloudsc2_satur_lin_launch), the chain rule in torch, the batched sweep with qsat as a plane.

def _tl_batch(prm, ptsphy, lay: Layout, x: dict, dts, ddims, K: int) -> tuple:
    """K tangents (``dts`` in IN_NAMES order, batched where ``ddims`` says) over one state ``x``: one ``cloudsc2_tl_launch_batch``
    -> the 10 output tangents ``(K, ...)``"""
    like = x["pap"]
    dev = like.device
    dxs = _directions(B.IN_NAMES, dts, ddims, K, lay, IN_GROUPS)
    dy = _new(B.OUT_NAMES, lay, like, batch=K)
    dys = [{n: dy[n][k] for n in B.OUT_NAMES} for k in range(K)]
    with torch.cuda.device(dev):
        B.check(B.lib.cloudsc2_tl_launch_batch(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                               C.byref(_block("in", x, lay)), K, _block_array("in", dxs, lay),
                                               _block_array("out", dys, lay), _stream(dev)))
    return tuple(dy[n] for n in B.OUT_NAMES)


def _vjp_batch(prm, ptsphy, lay: Layout, x: dict, fplsl, fplsn, scratch, ys, ydims, K: int) -> tuple:
    """K cotangents (``ys`` in OUT_NAMES order, batched where ``ydims`` says) over one state ``x``: one
    ``cloudsc2_vjp_launch_batch`` -> the 16 input adjoints ``(K, ...)``"""
    like = x["pap"]
    dev = like.device
    ys = _directions(B.OUT_NAMES, ys, ydims, K, lay, OUT_GROUPS)
    xa = _new(B.IN_NAMES, lay, like, batch=K)
    xas = [{n: xa[n][k] for n in B.IN_NAMES} for k in range(K)]
    with torch.cuda.device(dev):
        B.check(B.lib.cloudsc2_vjp_launch_batch(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                C.byref(_block("in", x, lay)), C.byref(_traj_out(fplsl, fplsn, lay)), K,
                                                _block_array("in", xas, lay), _block_array("out", ys, lay), _scratch_ptr(scratch),
                                                _stream(dev)))
    return tuple(xa[n] for n in B.IN_NAMES)


@_inner(raises=None)
class _Cloudsc2Tl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, *n trajectory inputs, *n tangents) -> 10 output tangents: the TL sweep without trajectory
    stores, ``cloudsc2_tl_launch`` (n = 16) or ``cloudsc2_tl_launch_satur`` (n = 15).  Not differentiable (no double backward)."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = normalize(dict(zip(names, ts[n:])), lay, groups)
        dy = _new(B.OUT_NAMES, lay, like)
        with torch.cuda.device(dev):
            if satur:
                B.check(B.lib.cloudsc2_tl_launch_satur(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                       C.byref(_block("in", x, lay)), C.byref(_block("in", dx, lay)),
                                                       C.byref(_block("out", dy, lay)), _stream(dev)))
            else:
                B.check(B.lib.cloudsc2_tl_launch(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                 C.byref(_block("in", x, lay)), C.byref(B.Outputs()),  # no trajectory stores
                                                 C.byref(_block("in", dx, lay)), C.byref(_block("out", dy, lay)), _stream(dev)))
        return tuple(dy[k] for k in B.OUT_NAMES)

    @staticmethod
    def vmap(info, in_dims, prm, ptsphy, lay, satur, *ts):
        _refuse_nested(ts)
        names, groups = _names(satur)
        n = len(names)
        dims = in_dims[4:]
        K = _batch_size(dims, ts)
        if K is None:
            return _Cloudsc2Tl.apply(prm, ptsphy, lay, satur, *ts), (None,) * 10
        if any(d is not None for d in dims[:n]):  # a batch of states
            def one(l, flat):
                x = normalize(dict(zip(names, flat[:n])), l, groups)
                return _Cloudsc2Tl.apply(prm, ptsphy, l, satur, *(x[k] for k in names), *flat[n:])
            return _fold(one, lay, names * 2, ts, dims, B.OUT_NAMES), (0,) * 10
        x, dts, ddims = dict(zip(names, ts[:n])), ts[n:], dims[n:]
        if satur:  # SATUR's partials once, the tangent of qsat of every direction in torch, the batched TL sweep with qsat as a plane
            dx = {k: _front(t, d) for k, t, d in zip(names, dts, ddims)}
            ddim = dict(zip(names, (None if d is None else 0 for d in ddims)))
            qsat, dqp, dqt = _satur_planes(prm, lay, x["pap"], x["t"])
            dx["qsat"] = dqp * dx["pap"] + dqt * dx["t"]
            ddim["qsat"] = None if ddim["pap"] is None and ddim["t"] is None else 0
            x = normalize(dict(zip(B.IN_NAMES, _with_qsat(x, qsat))), lay, IN_GROUPS)
            dts, ddims = [dx[k] for k in B.IN_NAMES], [ddim[k] for k in B.IN_NAMES]
        return _tl_batch(prm, ptsphy, lay, x, dts, ddims, K), (0,) * 10


@_inner(raises=None)
class _Cloudsc2Vjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, *n trajectory inputs, PFPLSL5, PFPLSN5, cover scratch, *10 output adjoints) -> n input
    adjoints: the reverse sweep in its vector-Jacobian form, ``cloudsc2_vjp_launch`` (n = 16) or ``cloudsc2_vjp_launch_satur``
    (n = 15).  Not differentiable (no double backward)."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = normalize(dict(zip(B.OUT_NAMES, ys)), lay, OUT_GROUPS)
        xa = _new(names, lay, like)
        launch = B.lib.cloudsc2_vjp_launch_satur if satur else B.lib.cloudsc2_vjp_launch
        with torch.cuda.device(dev):
            B.check(launch(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                           C.byref(_block("in", x, lay)), C.byref(_traj_out(fplsl, fplsn, lay)), C.byref(_block("in", xa, lay)),
                           C.byref(_block("out", y, lay)), _scratch_ptr(scratch), _stream(dev)))
        return tuple(xa[k] for k in names)

    @staticmethod
    def vmap(info, in_dims, prm, ptsphy, lay, satur, *ts):
        _refuse_nested(ts)
        names, groups = _names(satur)
        n = len(names)
        dims = in_dims[4:]
        K = _batch_size(dims, ts)
        if K is None:
            return _Cloudsc2Vjp.apply(prm, ptsphy, lay, satur, *ts), (None,) * n
        if any(d is not None for d in dims[:n + 3]):  # a batch of states
            def one(l, flat):
                x = normalize(dict(zip(names, flat[:n])), l, groups)
                fl = [t if _fits(t, l, "fplsl") and _block_stride(t, l, "fplsl") == (l.nlev + 1) * l.nproma else t.contiguous() for t in flat[n:n + 2]]
                sc = flat[n + 2].contiguous()
                return _Cloudsc2Vjp.apply(prm, ptsphy, l, satur, *(x[k] for k in names), *fl, sc, *flat[n + 3:])
            return _fold(one, lay, names + ("fplsl", "fplsn", "scratch") + B.OUT_NAMES, ts, dims, names), (0,) * n
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        if not satur:
            return _vjp_batch(prm, ptsphy, lay, x, fplsl, fplsn, scratch, ys, dims[n + 3:], K), (0,) * n
        # the batched reverse sweep with qsat as a plane, then SATUR's transpose in torch
        qsat, dqp, dqt = _satur_planes(prm, lay, x["pap"], x["t"])
        x16 = normalize(dict(zip(B.IN_NAMES, _with_qsat(x, qsat))), lay, IN_GROUPS)
        xa = dict(zip(B.IN_NAMES, _vjp_batch(prm, ptsphy, lay, x16, fplsl, fplsn, scratch, ys, dims[n + 3:], K)))
        xa["pap"] = xa["pap"] + dqp * xa["qsat"]
        xa["t"] = xa["t"] + dqt * xa["qsat"]
        return tuple(xa[k] for k in names), (0,) * n


class _Cloudsc2(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, *n inputs in the order of the names) -> 10 outputs + the cover-checkpoint scratch
    # (non-differentiable): the NL sweep, with SATUR fused when satur (n = 15: one plane less is saved).  Its jvp and backward are the
    # two functions above, whose vmap rules carry batched tangents and cotangents.

    @staticmethod
    def forward(prm, ptsphy, lay, satur, *xs):
        return _forward_launch(prm, ptsphy, lay, dict(zip(_names(satur)[0], xs)))

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, *xs = inputs
        _save_trajectory(ctx, xs, output[FPLSL], output[FPLSN], output[-1], prm=prm, ptsphy=ptsphy, lay=lay, satur=satur)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        lay, like = ctx.lay, saved[0]
        need = ctx.needs_input_grad[4:]
        if not any(need):
            return (None,) * (4 + len(need))
        y = _zero_filled(B.OUT_NAMES, grads[:10], lay, like)
        xa = _Cloudsc2Vjp.apply(ctx.prm, ctx.ptsphy, lay, ctx.satur, *saved, *(y[n] for n in B.OUT_NAMES))
        return (None,) * 4 + tuple(a if nd else None for a, nd in zip(xa, need))

    @staticmethod
    def jvp(ctx, *tangents):
        names, _ = _names(ctx.satur)
        xs = ctx.saved_tensors
        dx = _zero_filled(names, tangents[4:], ctx.lay, xs[0])
        dy = _Cloudsc2Tl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, *xs, *(dx[n] for n in names))
        return tuple(dy) + (None,)

    @staticmethod
    def vmap(info, in_dims, prm, ptsphy, lay, satur, *xs):
        return _vmap_states(_Cloudsc2, in_dims, prm, ptsphy, lay, satur, xs)


class _Satur(torch.autograd.Function):
    # forward(prm, layout, pap, t) -> qsat, dqs/dpap, dqs/dt (the partials non-differentiable, saved): SATUR with first-order
    # derivatives, both elementwise products with the partial planes

    @staticmethod
    def forward(prm, lay, pap, t):
        return _satur_planes(prm, lay, pap, t)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _, dqp, dqt = output
        ctx.mark_non_differentiable(dqp, dqt)
        ctx.save_for_backward(dqp, dqt)
        ctx.save_for_forward(dqp, dqt)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gp, _gt):
        dqp, dqt = ctx.saved_tensors
        need = ctx.needs_input_grad
        return None, None, (g * dqp if need[2] else None), (g * dqt if need[3] else None)

    @staticmethod
    def jvp(ctx, _prm, _lay, dpap, dt):
        dqp, dqt = ctx.saved_tensors
        dq = None
        for part, d in ((dqp, dpap), (dqt, dt)):
            if d is not None:
                dq = part * d if dq is None else dq + part * d
        return dq if dq is not None else torch.zeros_like(dqp), None, None

    @staticmethod
    def vmap(info, in_dims, prm, lay, pap, t):
        raise NotImplementedError("satur(differentiable=True): torch.func.vmap is not supported (differentiate the op with "
                                  "satur=True, whose vmap rules carry batches)")


# ---- params=...: the derivative with respect to the tunable parameters next to the one with respect to the fields ----------------

_NO_VMAP = ("cloudsc2 with params: torch.func.vmap, jacfwd and jacrev are not supported (batched parameter directions are not built); "
            "use .backward() / torch.autograd.grad / torch.func.grad / torch.func.vjp, or torch.autograd.forward_ad / torch.func.jvp, "
            "one direction at a time")


def check_params(params, prm: B.Params) -> tuple:
    """The checks of ``cloudsc2(..., params=...)`` that need no device; returns the given names in ``PARAM_NAMES`` order.  Runs on CPU
    tensors; raises ``ValueError``."""
    if not hasattr(params, "keys"):
        raise ValueError(f"params must map names of {PARAM_NAMES} to 0-d float64 tensors; got {type(params)}")
    unknown = sorted(set(params.keys()) - set(PARAM_NAMES))
    if unknown:
        raise ValueError(f"params: unknown name(s) {unknown}; the differentiable parameters are {PARAM_NAMES}")
    for n in params.keys():
        p = params[n]
        if not isinstance(p, torch.Tensor):
            raise ValueError(f"params[{n!r}] is not a tensor")
        if p.dtype != torch.float64:
            raise ValueError(f"params[{n!r}] has dtype {p.dtype}; parameters are float64 in both builds (the constants of cloudsc2_params are C doubles)")
        if p.dim() != 0:
            raise ValueError(f"params[{n!r}] must be a 0-d tensor; got shape {tuple(p.shape)}")
    if not prm.lphylin:
        raise ValueError("params with prm.lphylin = 0: the parameter derivative belongs to the LPHYLIN form of the scheme")
    return tuple(n for n in PARAM_NAMES if n in params.keys())


def _batched_inside(t) -> bool:
    """a vmap level anywhere under torch.func's wrappers (jacfwd hands the op a dual whose primal has been batched with its tangent)"""
    while isinstance(t, torch.Tensor):
        if _functorch.is_batchedtensor(t) or _functorch.is_legacy_batchedtensor(t):
            return True
        if not _functorch.is_functorch_wrapped_tensor(t):
            return False
        t = _functorch.get_unwrapped(t)
    return False


def _refuse_batched(ts, message: str = _NO_VMAP) -> None:
    if any(_batched_inside(t) for t in ts):
        raise NotImplementedError(message)


def _host_value(t: torch.Tensor | None) -> float:
    return 0.0 if t is None else float(_raw(t).detach())


def _check_param_devices(pnames, ps, dev: torch.device) -> None:
    for n, p in zip(pnames, ps):
        if p.device.type != "cpu" and p.device != dev:
            raise ValueError(f"params[{n!r}] is on {p.device}: parameters live on the CPU or on the inputs' device {dev}")


def _with_host_values(prm: B.Params, pnames, ps, who: str) -> B.Params:
    """a copy of ``prm`` that holds the parameters' values, read on the HOST; with the evaporation branch ``rpecons`` must not be 0"""
    prm = copy.copy(prm)  # (a ctypes structure: a copy of its bytes)
    for n, p in zip(pnames, ps):
        setattr(prm, n, _host_value(p))  # synchronises when the parameter lives on the device
    if _evap(prm) and prm.rpecons == 0.0:
        raise ValueError(f"{who} with the evaporation branch (levapls2 / ldrain1d): rpecons must not be 0")
    return prm


@_no_vmap(_NO_VMAP)
@_inner(raises=None)
class _Cloudsc2ParTl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, (4 parameter tangents), *n trajectory inputs, *n tangents) -> 10 output tangents:
    ``cloudsc2_tl_launch_par`` (n = 16, or 15 with satur).  Not differentiable."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, dpar, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = normalize(dict(zip(names, ts[n:])), lay, groups)
        dy = _new(B.OUT_NAMES, lay, like)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch_par(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur),
                                                 C.byref(_block("in", x, lay)), C.byref(_block("in", dx, lay)),
                                                 (C.c_double * len(PARAM_NAMES))(*dpar), C.byref(_block("out", dy, lay)), _stream(dev)))
        return tuple(dy[k] for k in B.OUT_NAMES)


@_no_vmap(_NO_VMAP)
@_inner(raises=None)
class _Cloudsc2ParVjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, *n trajectory inputs, PFPLSL5, PFPLSN5, cover scratch, *10 output adjoints) -> n input
    adjoints and the 4 parameter adjoints (device float64): ``cloudsc2_vjp_launch_par``.  Not differentiable."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = normalize(dict(zip(B.OUT_NAMES, ys)), lay, OUT_GROUPS)
        xa = _new(names, lay, like)
        nwork = C.c_longlong()
        B.check(B.lib.cloudsc2_par_work_doubles(lay.nproma, lay.ngptot, C.byref(nwork)))
        work = torch.empty(nwork.value, dtype=torch.float64, device=dev)
        par_adj = torch.empty(len(PARAM_NAMES), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch_par(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur),
                                                  C.byref(_block("in", x, lay)), C.byref(_traj_out(fplsl, fplsn, lay)),
                                                  C.byref(_block("in", xa, lay)), C.byref(_block("out", y, lay)), _scratch_ptr(scratch),
                                                  C.c_void_p(work.data_ptr()), C.c_void_p(par_adj.data_ptr()), _stream(dev)))
        return tuple(xa[k] for k in names) + (par_adj,)


@_no_vmap(_NO_VMAP)
class _Cloudsc2Par(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, parameter names, *their 0-d tensors, *n inputs) -> 10 outputs + the cover-checkpoint scratch:
    # prm already holds the parameters' values, so the forward is the NL sweep of _Cloudsc2; the tensors are operands for autograd's
    # sake.  backward: one cloudsc2_vjp_launch_par (today's launch when no parameter needs a gradient); jvp: one
    # cloudsc2_tl_launch_par.

    @staticmethod
    def forward(prm, ptsphy, lay, satur, pnames, *ts):
        return _forward_launch(prm, ptsphy, lay, dict(zip(_names(satur)[0], ts[len(pnames):])))

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, pnames, *ts = inputs
        _save_trajectory(ctx, ts[len(pnames):], output[FPLSL], output[FPLSN], output[-1], prm=prm, ptsphy=ptsphy, lay=lay, satur=satur,
                         pnames=pnames, pdevs=tuple(p.device for p in ts[:len(pnames)]))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        _refuse_batched(grads)
        saved = ctx.saved_tensors
        lay, like, P = ctx.lay, saved[0], len(ctx.pnames)
        need_p, need_x = ctx.needs_input_grad[5:5 + P], ctx.needs_input_grad[5 + P:]
        if not any(need_p) and not any(need_x):
            return (None,) * (5 + P + len(need_x))
        y = _zero_filled(B.OUT_NAMES, grads[:10], lay, like)
        if not any(need_p):  # the field gradients alone: today's launch
            xa = _Cloudsc2Vjp.apply(ctx.prm, ctx.ptsphy, lay, ctx.satur, *saved, *(y[n] for n in B.OUT_NAMES))
            return (None,) * (5 + P) + tuple(a if nd else None for a, nd in zip(xa, need_x))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("cloudsc2 with params: the backward cannot run while the stream is capturing")
        *xa, par_adj = _Cloudsc2ParVjp.apply(ctx.prm, ctx.ptsphy, lay, ctx.satur, *saved, *(y[n] for n in B.OUT_NAMES))
        gp = tuple(par_adj[PARAM_NAMES.index(n)].to(d) if nd else None for n, d, nd in zip(ctx.pnames, ctx.pdevs, need_p))
        return (None,) * 5 + gp + tuple(a if nd else None for a, nd in zip(xa, need_x))

    @staticmethod
    def jvp(ctx, *tangents):
        _refuse_batched(tangents)
        names, _ = _names(ctx.satur)
        P = len(ctx.pnames)
        xs = ctx.saved_tensors
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("cloudsc2 with params: the parameter tangents are read on the host, which cannot happen while the stream is capturing")
        dpar = [0.0] * len(PARAM_NAMES)
        for n, t in zip(ctx.pnames, tangents[5:5 + P]):
            dpar[PARAM_NAMES.index(n)] = _host_value(t)
        dx = _zero_filled(names, tangents[5 + P:], ctx.lay, xs[0])
        dy = _Cloudsc2ParTl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, tuple(dpar), *xs, *(dx[n] for n in names))
        return tuple(dy) + (None,)


def _cloudsc2_par(inputs, prm: B.Params, ptsphy: float, ngptot, satur: bool, params) -> Cloudsc2Outputs:
    names, groups = _names(satur)
    lay = check_layout(inputs, prm, ngptot, satur=satur)
    pnames = check_params(params, prm)
    dev = check_device(inputs[n] for n in names)
    ps = tuple(params[n] for n in pnames)
    _refuse_batched(ps + tuple(inputs[n] for n in names))
    _check_param_devices(pnames, ps, dev)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("cloudsc2 with params: the parameters' values are read on the host (they travel in the kernel-argument "
                           "segment), which cannot happen while the stream is capturing")
    _prepare(dev)
    prm = _with_host_values(prm, pnames, ps, "params")
    return Cloudsc2Outputs(*_apply(_Cloudsc2Par, (prm, float(ptsphy), lay, bool(satur), pnames, *ps), inputs, names, groups, lay)[:10])


# ---- sparse=True: the derivative side moves only the planes a loss touches -----------------------------------------------------------
# The forward is the dense op's launch.  Backward and jvp hand the cotangents / tangents that exist (not None) and the gradients that
# are wanted (needs_input_grad) to cloudsc2_vjp_launch_sparse / cloudsc2_tl_launch_sparse: no zero plane is allocated or read, no
# unwanted gradient is allocated or written.  With every plane present they call the dense inner functions (the same bits, and the
# measured path).  Batched directions under vmap hand over to the dense batched rules with zero-filled planes.

def _present(names, ts) -> dict:
    return {n: t for n, t in zip(names, ts) if t is not None}


def _normalize_present(ts: dict, lay: Layout, groups: dict) -> dict:
    """:func:`normalize` for a subset of the fields: every layout group's present members"""
    return normalize(ts, lay, {g: tuple(n for n in names if n in ts) for g, names in groups.items() if any(n in ts for n in names)})


@_inner(raises=None)
class _Cloudsc2SparseTl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, *n trajectory inputs, *n tangents or None) -> 10 output tangents:
    ``cloudsc2_tl_launch_sparse`` (n = 16, or 15 with satur); a None tangent is a zero tangent that is not read.  Not differentiable."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = _normalize_present(_present(names, ts[n:]), lay, groups)
        dy = _new(B.OUT_NAMES, lay, like)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch_sparse(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur),
                                                    C.byref(_block("in", x, lay)), C.byref(_block("in", dx, lay)),
                                                    C.byref(_block("out", dy, lay)), _stream(dev)))
        return tuple(dy[k] for k in B.OUT_NAMES)

    @staticmethod
    def vmap(info, in_dims, prm, ptsphy, lay, satur, *ts):
        # the dense rules on zero-filled planes: every direction is the bits of the dense call
        names, _ = _names(satur)
        n = len(names)
        dims = in_dims[4:]
        dx = _zero_filled(names, ts[n:], lay, ts[0])
        ddims = tuple(None if t is None else d for t, d in zip(ts[n:], dims[n:]))
        return _Cloudsc2Tl.vmap(info, (None,) * 4 + tuple(dims[:n]) + ddims, prm, ptsphy, lay, satur, *ts[:n], *(dx[k] for k in names))


@_inner(raises=None)
class _Cloudsc2SparseVjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, want, *n trajectory inputs, PFPLSL5, PFPLSN5, cover scratch, *10 output adjoints or None)
    -> the input adjoints named in ``want``, in that order: ``cloudsc2_vjp_launch_sparse``; a None adjoint is a zero cotangent that is
    not read, an input not in ``want`` gets no plane.  Not differentiable."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, want, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = _normalize_present(_present(B.OUT_NAMES, ys), lay, OUT_GROUPS)
        xa = _new(want, lay, like)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch_sparse(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur),
                                                     C.byref(_block("in", x, lay)), C.byref(_traj_out(fplsl, fplsn, lay)),
                                                     C.byref(_block("in", xa, lay)), C.byref(_block("out", y, lay)),
                                                     _scratch_ptr(scratch), _stream(dev)))
        return tuple(xa[k] for k in want)

    @staticmethod
    def vmap(info, in_dims, prm, ptsphy, lay, satur, want, *ts):
        # the dense rules on zero-filled planes: every direction is the bits of the dense call; the unwanted adjoints are dropped
        names, _ = _names(satur)
        n = len(names)
        dims = in_dims[5:]
        y = _zero_filled(B.OUT_NAMES, ts[n + 3:], lay, ts[0])
        ydims = tuple(None if t is None else d for t, d in zip(ts[n + 3:], dims[n + 3:]))
        xa, od = _Cloudsc2Vjp.vmap(info, (None,) * 4 + tuple(dims[:n + 3]) + ydims, prm, ptsphy, lay, satur, *ts[:n + 3],
                                   *(y[k] for k in B.OUT_NAMES))
        sel = [names.index(k) for k in want]
        return tuple(xa[j] for j in sel), tuple(od[j] for j in sel)


class _Cloudsc2Sparse(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, *n inputs) -> 10 outputs + the cover-checkpoint scratch: the launch of _Cloudsc2;
    # gradients are not materialised, so backward sees None for an output that took no part in the loss

    @staticmethod
    def forward(prm, ptsphy, lay, satur, *xs):
        return _forward_launch(prm, ptsphy, lay, dict(zip(_names(satur)[0], xs)))

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, *xs = inputs
        _save_trajectory(ctx, xs, output[FPLSL], output[FPLSN], output[-1], materialize=False, prm=prm, ptsphy=ptsphy, lay=lay, satur=satur)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        names, _ = _names(ctx.satur)
        need = ctx.needs_input_grad[4:]
        ys = grads[:10]
        if not any(need) or all(g is None for g in ys):
            return (None,) * (4 + len(names))
        if all(need) and all(g is not None for g in ys):  # everything present: the dense sweep (the same bits)
            return (None,) * 4 + tuple(_Cloudsc2Vjp.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, *saved, *ys))
        want = tuple(n for n, nd in zip(names, need) if nd)
        xa = dict(zip(want, _Cloudsc2SparseVjp.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, want, *saved, *ys)))
        return (None,) * 4 + tuple(xa.get(n) for n in names)

    @staticmethod
    def jvp(ctx, *tangents):
        xs = ctx.saved_tensors
        dts = tangents[4:]
        if all(t is not None for t in dts):  # everything present: the dense sweep (the same bits)
            dy = _Cloudsc2Tl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, *xs, *dts)
        else:  # (all ten output tangents are stored: autograd cannot say which will be used)
            dy = _Cloudsc2SparseTl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, *xs, *dts)
        return tuple(dy) + (None,)

    @staticmethod
    def vmap(info, in_dims, prm, ptsphy, lay, satur, *xs):
        return _vmap_states(_Cloudsc2Sparse, in_dims, prm, ptsphy, lay, satur, xs)


def cloudsc2(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, satur: bool = False, params=None,
             sparse: bool = False) -> Cloudsc2Outputs:
    """CLOUDSC2 over all blocks as a differentiable op, SATUR-free (``qsat`` is an input) or, with ``satur=True``, with SATUR
    evaluated and differentiated inside (``inputs`` without ``qsat``); ``params``: a mapping of names of ``PARAM_NAMES`` to 0-d
    float64 tensors that override those constants of (a copy of) ``prm`` and are differentiated too; ``sparse=True``: backward and
    jvp move only the cotangent / tangent planes that exist and the gradients that are wanted (not with ``params``); see the module
    docstring."""
    if sparse and params is not None:
        raise NotImplementedError("cloudsc2: sparse=True with params= is not built (the parameter sweeps have no sparse form); "
                                  "use sparse=False with params")
    if params is not None:
        return _cloudsc2_par(inputs, prm, ptsphy, ngptot, satur, params)
    names, groups, lay, dev = _enter(inputs, prm, ngptot, satur)
    _prepare(dev)
    cls = _Cloudsc2Sparse if sparse else _Cloudsc2
    return Cloudsc2Outputs(*_apply(cls, (prm, float(ptsphy), lay, bool(satur)), inputs, names, groups, lay)[:10])


def param_jacobian(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, satur: bool = False, params=None) -> dict:
    """The whole parameter Jacobian of :func:`cloudsc2` at one state: a dict ``name -> Cloudsc2Outputs`` holding ``d out / d name``
    for every name of ``PARAM_NAMES`` (``params=None``: at ``prm``'s values), or for the names of ``params`` (a mapping as for
    ``cloudsc2(..., params=...)``, whose values override a copy of ``prm``).  One ``cloudsc2_tl_launch_parjac``: the trajectory is
    read once and no tangent plane exists, where ``torch.func.jvp`` of the op with a unit tangent on one parameter is a launch per
    parameter over zero-filled tangent planes; every entry is that jvp's result.  ``inputs`` as for :func:`cloudsc2` (without ``qsat``
    when ``satur=True``: SATUR is then evaluated in the sweep; none of the parameters enters it).  The result is plain contiguous
    tensors without a graph, padded tails zero; without the evaporation branch the ``rpecons`` entry is zero tensors."""
    names, groups = _names(satur)
    lay = check_layout(inputs, prm, ngptot, satur=satur)
    pnames = PARAM_NAMES if params is None else check_params(params, prm)
    dev = check_device(inputs[n] for n in names)
    ps = () if params is None else tuple(params[n] for n in pnames)
    if any(_batched_inside(t) for t in ps + tuple(inputs[n] for n in names)):
        raise NotImplementedError("param_jacobian: batched (vmap-wrapped) operands are not supported; call it once per state")
    _check_param_devices(pnames, ps, dev)
    if any(p.device.type != "cpu" for p in ps) and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("param_jacobian: the parameters' values are read on the host (they travel in the kernel-argument segment), "
                           "which cannot happen for device tensors while the stream is capturing")
    _prepare(dev)
    prm = _with_host_values(prm, pnames, ps, "param_jacobian")
    evap = _evap(prm)
    with torch.no_grad():
        x = normalize({n: _raw(inputs[n]).detach() for n in names}, lay, groups)
        like = x["pap"]
        ran = PARAM_NAMES if evap else PARAM_NAMES[:-1]  # (nothing depends on rpecons without the evaporation branch: not run)
        dy = {n: _new(B.OUT_NAMES, lay, like) for n in ran}
        if any(n in ran for n in pnames):
            blocks = (B.Outputs * len(PARAM_NAMES))(*(_block("out", dy[n], lay) for n in ran))
            with torch.cuda.device(dev):
                B.check(B.lib.cloudsc2_tl_launch_parjac(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                        C.byref(_block("in", x, lay)), blocks, _stream(dev)))
        return {n: Cloudsc2Outputs(*(dy[n][k] if n in ran else torch.zeros(lay.shape(k), dtype=like.dtype, device=dev) for k in B.OUT_NAMES))
                for n in pnames}


NormalEquations = namedtuple("NormalEquations", "names jtj jtr")


def normal_row(a: int, b: int) -> int:
    """where ``cloudsc2_parnormal_launch`` leaves ``(J^T W J)[a][b]``: the upper triangle row by row in ``PARAM_NAMES`` order"""
    a, b = min(a, b), max(a, b)
    return a * len(PARAM_NAMES) - a * (a - 1) // 2 + (b - a)


def check_residual(residual, weights, lay: Layout) -> tuple:
    """The checks of :func:`param_normal_equations` on its residuals and weights that need no device; raises ``ValueError``.
    ``residual``: a non-empty mapping of names of ``binding.OUT_NAMES`` (the observed outputs) to tensors of that output's shape in the
    library's dtype; ``weights``: ``None`` or a mapping over a subset of ``residual``'s names with the same shapes (a missing name is
    weight 1).  Returns ``(residual, weights)`` as dicts the launcher can take: it wants one block stride per layout group, the same
    for residuals and weights, so a group that does not fit is copied contiguous (:func:`normalize`)."""
    if not hasattr(residual, "keys") or (weights is not None and not hasattr(weights, "keys")):
        raise ValueError(f"residual (and weights, if given) must map names of {B.OUT_NAMES} to tensors; got {type(residual)}, {type(weights)}")
    if len(residual.keys()) == 0:
        raise ValueError("residual is empty: at least one output must be observed")
    weights = {} if weights is None else weights
    for what, d in (("residual", residual), ("weights", weights)):
        unknown = sorted(set(d.keys()) - set(B.OUT_NAMES), key=str)
        if unknown:
            raise ValueError(f"{what}: unknown name(s) {unknown}; the outputs are {B.OUT_NAMES}")
    unobserved = sorted(set(weights.keys()) - set(residual.keys()))
    if unobserved:
        raise ValueError(f"weights given for output(s) {unobserved} that are not observed (no residual)")
    dtype = B.torch_real()
    for what, d in (("residual", residual), ("weights", weights)):
        for n, t in d.items():
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what}[{n!r}] is not a tensor")
            if t.dtype != dtype:
                raise ValueError(f"{what}[{n!r}] has dtype {t.dtype}; this library works on {dtype} (CLOUDSC2_PRECISION)")
            if tuple(t.shape) != lay.shape(n):
                raise ValueError(f"{what}[{n!r}] has shape {tuple(t.shape)}, expected {lay.shape(n)}")
    r = {n: residual[n] for n in B.OUT_NAMES if n in residual.keys()}
    w = {n: weights[n] for n in B.OUT_NAMES if n in weights.keys()}
    # (group keys other than "full" / "half": any common stride will do, not only that of contiguous arrays)
    r = normalize(r, lay, {"r_" + g: tuple(n for n in names if n in r) for g, names in OUT_GROUPS.items()})
    w = normalize(w, lay, {"w_" + g: tuple(n for n in names if n in w) for g, names in OUT_GROUPS.items()})
    for names in OUT_GROUPS.values():
        rn, wn = [n for n in names if n in r], [n for n in names if n in w]
        if wn and _block_stride(r[rn[0]], lay, rn[0]) != _block_stride(w[wn[0]], lay, wn[0]):
            for n in rn:
                r[n] = r[n].contiguous()
            for n in wn:
                w[n] = w[n].contiguous()
    return r, w


def param_normal_equations(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, residual=None, weights=None,
                           satur: bool = False, params=None) -> NormalEquations:
    """The Gauss-Newton normal equations of the parameters at one state: ``NormalEquations(names, jtj, jtr)`` with ``jtj = J^T W J``
    (``(len(names), len(names))`` float64, symmetric: the upper triangle mirrored bit for bit) and ``jtr = J^T W r``
    (``(len(names),)`` float64) on the inputs' device, where ``J = d out / d names`` is :func:`param_jacobian`'s, ``r`` the
    ``residual`` (model - observation; a mapping of the observed outputs' names to tensors of their shape) and ``W`` the diagonal
    ``weights`` (``None``, or a mapping over a subset of ``residual``'s names; a missing name is weight 1).  The sums run over every
    active column, level and observed output.  One ``cloudsc2_parnormal_launch``: the sensitivities never exist in memory, the sums
    are formed in double in a fixed order and are the same bits from run to run.  ``names`` is ``PARAM_NAMES`` (``params=None``: at
    ``prm``'s values) or the names of ``params`` in that order (a mapping as for ``cloudsc2(..., params=...)``, whose values override
    a copy of ``prm``); the rules for ``params``, ``satur``, batched operands and ``rpecons`` are :func:`param_jacobian`'s.  Without
    the evaporation branch every entry with ``rpecons`` is exactly zero.  The result is plain tensors without a graph.  With
    ``params=None`` or CPU parameters the call can be captured in ``torch.cuda.graph`` after one eager call."""
    names, groups = _names(satur)
    lay = check_layout(inputs, prm, ngptot, satur=satur)
    pnames = PARAM_NAMES if params is None else check_params(params, prm)
    r, w = check_residual(residual, weights, lay)
    dev = check_device([inputs[n] for n in names] + list(r.values()) + list(w.values()))
    ps = () if params is None else tuple(params[n] for n in pnames)
    if any(_batched_inside(t) for t in ps + tuple(inputs[n] for n in names) + tuple(r.values()) + tuple(w.values())):
        raise NotImplementedError("param_normal_equations: batched (vmap-wrapped) operands are not supported; call it once per state")
    _check_param_devices(pnames, ps, dev)
    if any(p.device.type != "cpu" for p in ps) and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("param_normal_equations: the parameters' values are read on the host (they travel in the kernel-argument "
                           "segment), which cannot happen for device tensors while the stream is capturing")
    _prepare(dev)
    prm = _with_host_values(prm, pnames, ps, "param_normal_equations")
    with torch.no_grad():
        if not pnames:
            return NormalEquations((), torch.zeros((0, 0), dtype=torch.float64, device=dev), torch.zeros((0,), dtype=torch.float64, device=dev))
        x = normalize({n: _raw(inputs[n]).detach() for n in names}, lay, groups)
        r = {n: _raw(t).detach() for n, t in r.items()}
        w = {n: _raw(t).detach() for n, t in w.items()}
        work = torch.empty(B.NNORMAL * lay.nblocks * lay.nproma, dtype=torch.float64, device=dev)
        normal = torch.empty(B.NNORMAL, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_parnormal_launch(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                    C.byref(_block("in", x, lay)), C.byref(_block("out", r, lay)),
                                                    C.byref(_block("out", w, lay)) if w else None, C.c_void_p(work.data_ptr()),
                                                    C.c_void_p(normal.data_ptr()), _stream(dev)))
        idx = [PARAM_NAMES.index(n) for n in pnames]
        jtj = torch.stack([normal[normal_row(a, b)] for a in idx for b in idx]).reshape(len(idx), len(idx))
        jtr = torch.stack([normal[B.NNORMAL - len(PARAM_NAMES) + a] for a in idx])
        return NormalEquations(tuple(pnames), jtj, jtr)


# ---- cloudsc2_ensemble: K parameter sets in one launch, the parameters read on the device -------------------------------------------

_NO_VMAP_ENS = ("cloudsc2_ensemble: torch.func.vmap, jacfwd and jacrev are not supported (the ensemble is the batch: give the members' "
                "parameters as (K,) tensors and per-member states as 4-D inputs); use .backward() / torch.autograd.grad / "
                "torch.func.grad / torch.func.vjp, or torch.autograd.forward_ad / torch.func.jvp")


_NO_SECOND_ENS = ("cloudsc2_ensemble: double backward (and forward-over-reverse, reverse-over-forward) is not supported: the sweeps are "
                  "first-order derivatives of CLOUDSC2")


def check_ensemble(inputs, prm: B.Params, ngptot: int | None = None, satur: bool = False, params=None) -> tuple:
    """Every check of :func:`cloudsc2_ensemble` that needs no device; returns ``(layout, K, the given names in PARAM_NAMES order)``.
    Runs on CPU tensors; raises ``ValueError``."""
    if not hasattr(params, "keys"):
        raise ValueError(f"params must map names of {PARAM_NAMES} to 1-d float64 tensors of one length K; got {type(params)}")
    if len(params.keys()) == 0:
        raise ValueError(f"params is empty: an ensemble varies at least one of {PARAM_NAMES}")
    unknown = sorted(set(params.keys()) - set(PARAM_NAMES), key=str)
    if unknown:
        raise ValueError(f"params: unknown name(s) {unknown}; the differentiable parameters are {PARAM_NAMES}")
    pnames = tuple(n for n in PARAM_NAMES if n in params.keys())
    K = None
    for n in pnames:
        p = params[n]
        if not isinstance(p, torch.Tensor):
            raise ValueError(f"params[{n!r}] is not a tensor")
        if p.dtype != torch.float64:
            raise ValueError(f"params[{n!r}] has dtype {p.dtype}; parameters are float64 in both builds (the constants of cloudsc2_params are C doubles)")
        if p.dim() != 1 or p.shape[0] < 1:
            raise ValueError(f"params[{n!r}] must be a 1-d tensor with one value per member (K >= 1); got shape {tuple(p.shape)}")
        if K is None:
            K = int(p.shape[0])
        elif int(p.shape[0]) != K:
            raise ValueError(f"params[{n!r}] has {p.shape[0]} members, params[{pnames[0]!r}] has {K}: one common length K is required")
    IN_NAMES = _check_names(inputs, satur)
    member0 = {}
    for n in IN_NAMES:
        t = inputs[n]
        if isinstance(t, torch.Tensor) and t.dim() == 4:
            if int(t.shape[0]) != K:
                raise ValueError(f"inputs[{n!r}] is 4-D with leading size {t.shape[0]}: a per-member input has one state for each of the K = {K} members")
            t = t[0]
        elif isinstance(t, torch.Tensor) and t.dim() != 3:
            raise ValueError(f"inputs[{n!r}] must be 3-D (shared by all members) or 4-D (K, nblocks, nlev{'+1' if n in HALF_IN else ''}, nproma); "
                             f"got shape {tuple(t.shape)}")
        member0[n] = t
    return check_layout(member0, prm, ngptot, satur=satur), K, pnames


def _ens_block(kind: str, ts: dict, lay: Layout, K: int):
    """member 0's argument block and the member strides (elements; 0: shared) of ``ts``: name -> 3-D or 4-D tensor"""
    blk, names = (B.Inputs(), B.IN_NAMES) if kind == "in" else (B.Outputs(), B.OUT_NAMES)
    ms = (C.c_longlong * len(names))()
    for n, t in ts.items():
        t = _raw(t)
        setattr(blk, n, _field(_member0(t), lay, n))
        ms[names.index(n)] = t.stride(0) if t.dim() == 4 and K > 1 else 0
    return blk, ms


def _ens_workspace(K: int, lay: Layout, dev: torch.device) -> torch.Tensor:
    nbytes = B.lib.cloudsc2_ens_workspace_bytes(K, lay.nproma, lay.nlev, lay.ngptot)
    if nbytes < 0:
        B.check(int(nbytes))
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(_raw(t).data_ptr())


def _table(t: torch.Tensor) -> torch.Tensor:
    """a (K, 4) parameter table as the launchers read it: plain, contiguous"""
    return _raw(t).detach().contiguous()


@_no_vmap(_NO_VMAP_ENS)
@_inner(raises=_NO_SECOND_ENS)
class _Cloudsc2EnsTl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, K, (K, 4) parameters, (K, 4) parameter tangents, *n trajectory inputs, *n tangents) -> 10
    output tangents ``(K, ...)``: ``cloudsc2_tl_launch_ens``.  Inputs and tangents are 3-D (shared) or 4-D.  Differentiating it again
    raises ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, K, ptab, dptab, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = normalize(dict(zip(names, ts[n:])), lay, groups)
        dy = _new(B.OUT_NAMES, lay, like, batch=K)
        ptab, dptab = _table(ptab), _table(dptab)
        work = _ens_workspace(K, lay, dev)
        (xb, xm), (db, dm), (yb, ym) = _ens_block("in", x, lay, K), _ens_block("in", dx, lay, K), _ens_block("out", dy, lay, K)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch_ens(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur), K, _ptr(ptab),
                                                 _ptr(dptab), C.byref(xb), xm, C.byref(db), dm, C.byref(yb), ym, _ptr(work), _stream(dev)))
        return tuple(dy[k] for k in B.OUT_NAMES)


@_no_vmap(_NO_VMAP_ENS)
@_inner(raises=_NO_SECOND_ENS)
class _Cloudsc2EnsVjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, K, (K, 4) parameters, *n trajectory inputs, PFPLSL5, PFPLSN5, cover scratch, *10 output
    adjoints) -> n input adjoints ``(K, ...)`` and the ``(K, 4)`` parameter adjoints: ``cloudsc2_vjp_launch_ens``.  Differentiating it
    again (double backward) raises ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, K, ptab, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = normalize(dict(zip(B.OUT_NAMES, ys)), lay, OUT_GROUPS)
        xa = _new(names, lay, like, batch=K)
        ptab = _table(ptab)
        work = _ens_workspace(K, lay, dev)
        par_adj = torch.empty((K, len(PARAM_NAMES)), dtype=torch.float64, device=dev)
        (xb, xm), (ab, am), (yb, ym) = _ens_block("in", x, lay, K), _ens_block("in", xa, lay, K), _ens_block("out", y, lay, K)
        tb, tm = _ens_block("out", {"fplsl": fplsl, "fplsn": fplsn}, lay, K)
        sc = _raw(scratch)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch_ens(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur), K, _ptr(ptab),
                                                  C.byref(xb), xm, C.byref(tb), tm, C.byref(ab), am, C.byref(yb), ym, _scratch_ptr(scratch),
                                                  sc.stride(0) if sc.dim() == 4 and K > 1 else 0, _ptr(work), _ptr(par_adj), _stream(dev)))
        return tuple(xa[k] for k in names) + (par_adj,)


@_no_vmap(_NO_VMAP_ENS)
class _Cloudsc2Ens(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, K, the (K, 4) parameter table, *n inputs, 3-D or 4-D) -> 10 outputs (K, ...) + the members'
    # cover-checkpoint scratch: cloudsc2_nl_launch_ens.  prm holds the values of the parameters that are not given; the table is a device
    # tensor nobody reads on the host.  backward: one cloudsc2_vjp_launch_ens; jvp: one cloudsc2_tl_launch_ens.

    @staticmethod
    def forward(prm, ptsphy, lay, satur, K, ptab, *xs):
        names, _ = _names(satur)
        x = dict(zip(names, xs))
        like = x["pap"]
        dev = like.device
        out = _new(B.OUT_NAMES, lay, like, batch=K)
        evap = _evap(prm)
        scratch = torch.empty((K, lay.nblocks, lay.nlev, lay.nproma) if evap else (0,), dtype=like.dtype, device=dev)
        ptab = _table(ptab)
        work = _ens_workspace(K, lay, dev)
        (xb, xm), (ob, om) = _ens_block("in", x, lay, K), _ens_block("out", out, lay, K)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_nl_launch_ens(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, K, _ptr(ptab), C.byref(xb), xm,
                                                 C.byref(ob), om, _scratch_ptr(scratch), scratch.stride(0) if evap and K > 1 else 0,
                                                 _ptr(work), _stream(dev)))
        return tuple(out[n] for n in B.OUT_NAMES) + (scratch,)

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, K, ptab, *xs = inputs
        _save_trajectory(ctx, xs, output[FPLSL], output[FPLSN], output[-1], table=ptab, prm=prm, ptsphy=ptsphy, lay=lay, satur=satur, K=K)

    @staticmethod
    def backward(ctx, *grads):
        _refuse_batched(grads, _NO_VMAP_ENS)
        ptab, *saved = ctx.saved_tensors
        lay, like = ctx.lay, saved[0]
        need_p, need_x = ctx.needs_input_grad[5], ctx.needs_input_grad[6:]
        if not need_p and not any(need_x):
            return (None,) * (6 + len(need_x))
        y = _zero_filled(B.OUT_NAMES, grads[:10], lay, like)  # (an output that took no part: one shared zero plane)
        *xa, par_adj = _Cloudsc2EnsVjp.apply(ctx.prm, ctx.ptsphy, lay, ctx.satur, ctx.K, ptab, *saved, *(y[n] for n in B.OUT_NAMES))
        # a per-member input gets its members' gradients, a shared one their sum
        gx = tuple((a if x.dim() == 4 else a.sum(0)) if nd else None for a, x, nd in zip(xa, saved, need_x))
        return (None,) * 5 + (par_adj if need_p else None,) + gx

    @staticmethod
    def jvp(ctx, *tangents):
        _refuse_batched(tangents, _NO_VMAP_ENS)
        names, _ = _names(ctx.satur)
        ptab, *xs = ctx.saved_tensors
        dptab = tangents[5] if tangents[5] is not None else torch.zeros_like(ptab)
        dx = _zero_filled(names, tangents[6:], ctx.lay, xs[0])  # (no tangent: one shared zero plane)
        dy = _Cloudsc2EnsTl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, ctx.K, ptab, dptab, *xs, *(dx[n] for n in names))
        return tuple(dy) + (None,)


def cloudsc2_ensemble(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, satur: bool = False, params=None) -> Cloudsc2Outputs:
    """A perturbed-parameter ensemble of CLOUDSC2 in one launch: K parameter sets over one state, or over one state each.

    ``params`` maps a non-empty subset of ``PARAM_NAMES`` to 1-d ``float64`` tensors of one common length K >= 1 ON THE INPUTS' DEVICE;
    a name that is not given keeps ``prm``'s value in every member.  Nothing is read on the host: the ``(K, 4)`` table is assembled
    with torch ops and a small kernel derives every member's constants from its row on the device, so the call does not synchronise,
    and after one eager call with the same CETA the forward and ``torch.autograd.grad`` of it can be captured in ``torch.cuda.graph`` --
    a replay after ``params[name].copy_(new)`` computes with the new values.

    ``inputs``: the names of :func:`cloudsc2` (without ``qsat`` when ``satur=True``); each tensor is 3-D in that op's layout and
    shared by all members, or 4-D ``(K, nblocks, nlevx, nproma)`` with one state per member and any member stride ``t.stride(0)``.
    The in-block layout rules are :func:`cloudsc2`'s: one block stride per layout group, a group that does not fit is copied contiguous.

    Returns a :class:`Cloudsc2Outputs` of ``(K, nblocks, nlevx, nproma)`` tensors, the padded tail zero in every member.
    ``.backward()``, ``torch.autograd.grad``, ``torch.func.grad`` / ``vjp``, ``forward_ad`` and ``torch.func.jvp`` differentiate with
    respect to the ``(K,)`` parameters (gradient ``(K,)``, float64, on the device) and the fields (a 4-D input gets per-member
    gradients, a 3-D shared input the sum over the members); ``torch.func.vmap`` / ``jacfwd`` / ``jacrev`` raise
    ``NotImplementedError``, and so does double backward (differentiating a gradient made with ``create_graph=True``, or a tangent).  ``prm.lphylin = 0`` is refused.  With the
    evaporation branch (``levapls2`` / ``ldrain1d``) every member's ``rpecons`` must be non-zero: a value given in ``params`` lives on
    the device and is NOT checked (a zero gives non-finite ``rpecons`` derivatives); ``prm``'s own value is checked when it is used.

    Promise: member k of every output, every per-member field gradient, every output tangent and every parameter gradient is bit for
    bit what ``cloudsc2(inputs_k, prm, ptsphy, ngptot, satur=..., params={the four 0-d values of row k})`` gives forward, in
    ``backward`` and in ``jvp``.  The gradient of a shared input is the members' sum (``xa.sum(0)``): equal to the sum of those
    calls' gradients up to the order of summation, not to the bit."""
    names, groups, (lay, K, pnames), dev = _enter(inputs, prm, ngptot, satur, check_ensemble, params)
    ptab = _ens_table(inputs, names, prm, params, pnames, K, dev, _NO_VMAP_ENS)
    return Cloudsc2Outputs(*_apply(_Cloudsc2Ens, (prm, float(ptsphy), lay, bool(satur), K, ptab), inputs, names, groups, lay)[:10])


def _ens_table(inputs, names, prm: B.Params, params, pnames, K: int, dev: torch.device, no_vmap: str, more=()) -> torch.Tensor:
    """What the ensemble entry points do between their checks and their Function: the refusals that need the device's name, the device
    prepared, and the ``(K, 4)`` parameter table assembled with torch ops (a name not given: ``prm``'s value in every member)"""
    ps = tuple(params[n] for n in pnames)
    _refuse_batched(ps + tuple(inputs[n] for n in names) + tuple(more), no_vmap)
    for n, p in zip(pnames, ps):
        if p.device != dev:
            raise ValueError(f"params[{n!r}] is on {p.device}: the parameters of an ensemble live on the inputs' device {dev} (they are read there)")
    if _evap(prm) and "rpecons" not in pnames and prm.rpecons == 0.0:
        raise ValueError("cloudsc2_ensemble with the evaporation branch (levapls2 / ldrain1d): rpecons must not be 0")
    _prepare(dev)
    given = dict(zip(pnames, ps))
    return torch.stack([given[n] if n in given else torch.full((K,), float(getattr(prm, n)), dtype=torch.float64, device=dev)
                        for n in PARAM_NAMES], dim=1)


# ---- cloudsc2_param_maps: the four parameters as (nblocks, nproma) fields, read on the device ---------------------------------------------

_NO_VMAP_PARMAP = ("cloudsc2_param_maps: torch.func.vmap, jacfwd, jacrev and is_grads_batched=True are not supported (batched "
                   "directions of the parameter-map sweeps are not built); use .backward() / torch.autograd.grad / torch.func.grad / "
                   "torch.func.vjp, or torch.autograd.forward_ad / torch.func.jvp, one direction at a time")

_NO_SECOND_PARMAP = ("cloudsc2_param_maps: double backward (and forward-over-reverse, reverse-over-forward) is not supported: the sweeps "
                     "are first-order derivatives of CLOUDSC2")


def check_param_maps(inputs, prm: B.Params, ngptot: int | None = None, satur: bool = False, params=None) -> tuple:
    """Every check of :func:`cloudsc2_param_maps` that needs no device; returns ``(layout, the given names in PARAM_NAMES order)``.
    Runs on CPU tensors; raises ``ValueError``."""
    if not hasattr(params, "keys"):
        raise ValueError(f"params must map names of {PARAM_NAMES} to (nblocks, nproma) float64 tensors; got {type(params)}")
    if len(params.keys()) == 0:
        raise ValueError(f"params is empty: a parameter map gives at least one of {PARAM_NAMES}")
    unknown = sorted(set(params.keys()) - set(PARAM_NAMES), key=str)
    if unknown:
        raise ValueError(f"params: unknown name(s) {unknown}; the differentiable parameters are {PARAM_NAMES}")
    pnames = tuple(n for n in PARAM_NAMES if n in params.keys())
    for n in pnames:
        p = params[n]
        if not isinstance(p, torch.Tensor):
            raise ValueError(f"params[{n!r}] is not a tensor")
        if p.dim() < 2:
            raise ValueError(f"params[{n!r}] has shape {tuple(p.shape)}: a parameter map is a 2-d (nblocks, nproma) tensor with one value per "
                             "column; one value for all columns is cloudsc2(..., params={name: 0-d tensor}), one value per member "
                             "cloudsc2_ensemble(..., params={name: (K,) tensor})")
        if p.dtype != torch.float64:
            raise ValueError(f"params[{n!r}] has dtype {p.dtype}; parameters are float64 in both builds (the constants of cloudsc2_params are C doubles)")
    lay = check_layout(inputs, prm, ngptot, satur=satur)
    for n in pnames:
        if tuple(params[n].shape) != (lay.nblocks, lay.nproma):
            raise ValueError(f"params[{n!r}] has shape {tuple(params[n].shape)}, expected (nblocks, nproma) = {(lay.nblocks, lay.nproma)}")
    return lay, pnames


def _map_table(t: torch.Tensor) -> torch.Tensor:
    """a (4, nblocks, nproma) table as the launchers read it -- (CLOUDSC2_NPAR, ncols_pad) doubles by padded column: plain, contiguous"""
    return _raw(t).detach().contiguous()


@_no_vmap(_NO_VMAP_PARMAP)
@_inner(raises=_NO_SECOND_PARMAP)
class _Cloudsc2ParmapTl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, (4, nblocks, nproma) values, (4, nblocks, nproma) tangents, *n trajectory inputs, *n tangents)
    -> 10 output tangents: ``cloudsc2_tl_launch_parmap``.  Differentiating it again raises ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, ptab, dptab, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = normalize(dict(zip(names, ts[n:])), lay, groups)
        dy = _new(B.OUT_NAMES, lay, like)
        ptab, dptab = _map_table(ptab), _map_table(dptab)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch_parmap(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur), _ptr(ptab),
                                                    _ptr(dptab), C.byref(_block("in", x, lay)), C.byref(_block("in", dx, lay)),
                                                    C.byref(_block("out", dy, lay)), _stream(dev)))
        return tuple(dy[k] for k in B.OUT_NAMES)


@_no_vmap(_NO_VMAP_PARMAP)
@_inner(raises=_NO_SECOND_PARMAP)
class _Cloudsc2ParmapVjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, (4, nblocks, nproma) values, *n trajectory inputs, PFPLSL5, PFPLSN5, cover scratch, *10 output
    adjoints) -> n input adjoints and the ``(4, nblocks, nproma)`` parameter adjoints, padded tail zero: ``cloudsc2_vjp_launch_parmap``.
    Differentiating it again (double backward) raises ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, ptab, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = normalize(dict(zip(B.OUT_NAMES, ys)), lay, OUT_GROUPS)
        xa = _new(names, lay, like)
        ptab = _map_table(ptab)
        par_adj = torch.empty((len(PARAM_NAMES), lay.nblocks, lay.nproma), dtype=torch.float64, device=dev)
        if lay.tail < lay.nproma:
            par_adj[:, -1, lay.tail:] = 0  # (the sweep assigns the active columns)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch_parmap(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur), _ptr(ptab),
                                                     C.byref(_block("in", x, lay)), C.byref(_traj_out(fplsl, fplsn, lay)),
                                                     C.byref(_block("in", xa, lay)), C.byref(_block("out", y, lay)), _scratch_ptr(scratch),
                                                     _ptr(par_adj), _stream(dev)))
        return tuple(xa[k] for k in names) + (par_adj,)


@_no_vmap(_NO_VMAP_PARMAP)
class _Cloudsc2Parmap(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, the (4, nblocks, nproma) value table, *n inputs) -> 10 outputs + the cover-checkpoint scratch:
    # cloudsc2_nl_launch_parmap.  The table is a device tensor nobody reads on the host.  backward: one cloudsc2_vjp_launch_parmap; jvp:
    # one cloudsc2_tl_launch_parmap.

    @staticmethod
    def forward(prm, ptsphy, lay, satur, ptab, *xs):
        names, _ = _names(satur)
        x = dict(zip(names, xs))
        like = x["pap"]
        dev = like.device
        out = _new(B.OUT_NAMES, lay, like)
        scratch = torch.empty((lay.nblocks, lay.nlev, lay.nproma) if _evap(prm) else (0,), dtype=like.dtype, device=dev)
        ptab = _map_table(ptab)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_nl_launch_parmap(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, _ptr(ptab),
                                                    C.byref(_block("in", x, lay)), C.byref(_block("out", out, lay)), _scratch_ptr(scratch),
                                                    _stream(dev)))
        return tuple(out[n] for n in B.OUT_NAMES) + (scratch,)

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, ptab, *xs = inputs
        _save_trajectory(ctx, xs, output[FPLSL], output[FPLSN], output[-1], table=ptab, prm=prm, ptsphy=ptsphy, lay=lay, satur=satur)

    @staticmethod
    def backward(ctx, *grads):
        _refuse_batched(grads, _NO_VMAP_PARMAP)
        ptab, *saved = ctx.saved_tensors
        lay, like = ctx.lay, saved[0]
        need_p, need_x = ctx.needs_input_grad[4], ctx.needs_input_grad[5:]
        if not need_p and not any(need_x):
            return (None,) * (5 + len(need_x))
        y = _zero_filled(B.OUT_NAMES, grads[:10], lay, like)  # (an output that took no part: one shared zero plane)
        *xa, par_adj = _Cloudsc2ParmapVjp.apply(ctx.prm, ctx.ptsphy, lay, ctx.satur, ptab, *saved, *(y[n] for n in B.OUT_NAMES))
        return (None,) * 4 + (par_adj if need_p else None,) + tuple(a if nd else None for a, nd in zip(xa, need_x))

    @staticmethod
    def jvp(ctx, *tangents):
        _refuse_batched(tangents, _NO_VMAP_PARMAP)
        names, _ = _names(ctx.satur)
        ptab, *xs = ctx.saved_tensors
        dptab = tangents[4] if tangents[4] is not None else torch.zeros_like(ptab)
        dx = _zero_filled(names, tangents[5:], ctx.lay, xs[0])  # (no tangent: one shared zero plane)
        dy = _Cloudsc2ParmapTl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, ptab, dptab, *xs, *(dx[n] for n in names))
        return tuple(dy) + (None,)


def cloudsc2_param_maps(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, satur: bool = False, params=None) -> Cloudsc2Outputs:
    """CLOUDSC2 with ``rkconv``, ``rclcrit``, ``rlptrc``, ``rpecons`` as FIELDS: a value per column, read on the device.

    ``params`` maps a non-empty subset of ``PARAM_NAMES`` to ``(nblocks, nproma)`` ``float64`` tensors ON THE INPUTS' DEVICE (float64 in
    both builds); a name that is not given keeps ``prm``'s value in every column.  Nothing is read on the host: the
    ``(4, nblocks, nproma)`` table is assembled with torch ops and every lane derives its constants from its column of it, so the call
    does not synchronise, and after one eager call with the same CETA the forward and ``torch.autograd.grad`` of it can be captured in
    ``torch.cuda.graph`` -- a replay after ``params[name].copy_(new)`` computes with the new values.  The values in the padded tail of a
    map are not read.

    ``inputs`` and ``satur`` are those of :func:`cloudsc2`.  Returns a :class:`Cloudsc2Outputs`.  ``.backward()``,
    ``torch.autograd.grad``, ``torch.func.grad`` / ``vjp``, ``forward_ad`` and ``torch.func.jvp`` (with tangent maps) differentiate with
    respect to the maps -- the gradient of a map is ``(nblocks, nproma)`` float64 on the device, column c holding d loss / d p[c], the
    padded tail zero -- and the fields; ``torch.func.vmap`` / ``jacfwd`` / ``jacrev`` and ``is_grads_batched`` raise
    ``NotImplementedError``, and so does double backward.  ``prm.lphylin = 0`` is refused.  It is not combined with ``sparse``, the
    column-sum ops or the ensemble ops.  With the evaporation branch (``levapls2`` / ``ldrain1d``) every column's ``rpecons`` must be
    non-zero: a map lives on the device and is NOT checked (a zero gives non-finite ``rpecons`` derivatives); ``prm``'s own value is
    checked when it is used.

    Promise: column c of every output, output tangent and field gradient is bit for bit what
    ``cloudsc2(inputs, prm, ptsphy, ngptot, satur=..., params={the four 0-d values of column c})`` gives at that column; columns are
    independent.  The gradient of a map is, per active column, that column's contribution to the 0-d parameter gradient of that call
    (the row of ``cloudsc2_vjp_launch_par``'s workspace) before its fold."""
    names, groups, (lay, pnames), dev = _enter(inputs, prm, ngptot, satur, check_param_maps, params)
    ps = tuple(params[n] for n in pnames)
    _refuse_batched(ps + tuple(inputs[n] for n in names), _NO_VMAP_PARMAP)
    for n, p in zip(pnames, ps):
        if p.device != dev:
            raise ValueError(f"params[{n!r}] is on {p.device}: parameter maps live on the inputs' device {dev} (they are read there)")
    if _evap(prm) and "rpecons" not in pnames and prm.rpecons == 0.0:
        raise ValueError("cloudsc2_param_maps with the evaporation branch (levapls2 / ldrain1d): rpecons must not be 0")
    _prepare(dev)
    given = dict(zip(pnames, ps))
    ptab = torch.stack([given[n] if n in given else torch.full((lay.nblocks, lay.nproma), float(getattr(prm, n)), dtype=torch.float64, device=dev)
                        for n in PARAM_NAMES], dim=0)
    return Cloudsc2Outputs(*_apply(_Cloudsc2Parmap, (prm, float(ptsphy), lay, bool(satur), ptab), inputs, names, groups, lay)[:10])


# ---- cloudsc2_column_sums: per-column weighted level sums of the outputs, formed in the sweeps ------------------------------------------

_NO_VMAP_COLSUM = ("cloudsc2_column_sums: torch.func.vmap, jacfwd, jacrev and is_grads_batched=True are not supported (batched "
                   "directions of the column-sum sweeps are not built); use .backward() / torch.autograd.grad / torch.func.grad / "
                   "torch.func.vjp, or torch.autograd.forward_ad / torch.func.jvp, one direction at a time")

_NO_SECOND_COLSUM = ("cloudsc2_column_sums: double backward (and forward-over-reverse, reverse-over-forward) is not supported: the sweeps "
                     "are first-order derivatives of CLOUDSC2")


def check_column_sums(inputs, prm: B.Params, ngptot: int | None = None, satur: bool = False, weights=None) -> tuple:
    """Every check of :func:`cloudsc2_column_sums` that needs no device; returns ``(layout, the given names in OUT_NAMES order)``.
    Runs on CPU or meta tensors; raises ``ValueError``."""
    lay = check_layout(inputs, prm, ngptot, satur=bool(satur))
    return lay, check_weights(weights, lay, inputs["pap"].device)


def check_weights(weights, lay: Layout, dev: torch.device) -> tuple:
    """The checks of the ``weights`` of the column-sum ops for a layout and the inputs' device; returns the given names in OUT_NAMES
    order.  Raises ``ValueError``."""
    if not hasattr(weights, "keys"):
        raise ValueError(f"weights must map names of {B.OUT_NAMES} to 1-D tensors of per-level weights; got {type(weights)}")
    if len(weights.keys()) == 0:
        raise ValueError(f"weights is empty: give a weight vector for at least one of {B.OUT_NAMES}")
    unknown = sorted((k for k in weights.keys() if k not in B.OUT_NAMES), key=str)
    if unknown:
        raise ValueError(f"weights: unknown name(s) {unknown}; the outputs are {B.OUT_NAMES}")
    dtype = B.torch_real()
    wnames = tuple(n for n in B.OUT_NAMES if n in weights.keys())
    for n in wnames:
        w = weights[n]
        if not isinstance(w, torch.Tensor):
            raise ValueError(f"weights[{n!r}] is not a tensor")
        if w.dim() != 1:
            raise ValueError(f"weights[{n!r}] must be 1-D, one weight per level of the plane; got shape {tuple(w.shape)}")
        if int(w.shape[0]) != lay.nlevx(n):
            raise ValueError(f"weights[{n!r}] has length {w.shape[0]}, expected {lay.nlevx(n)} (nlev{' + 1: the half levels, k = 0 the top' if n in HALF_OUT else ''})")
        if w.dtype != dtype:
            raise ValueError(f"weights[{n!r}] has dtype {w.dtype}; this library works on {dtype} (CLOUDSC2_PRECISION)")
        if w.requires_grad:
            raise ValueError(f"weights[{n!r}] requires grad: the weights are constants (the derivative with respect to a weight is the "
                             "output plane, which this op exists not to form); detach it")
        if w.device != dev:
            raise ValueError(f"weights[{n!r}] is on {w.device}: the weights live on the inputs' device {dev}")
    return wnames


def _new_sums(names, lay: Layout, like: torch.Tensor, batch: int | None = None) -> dict:
    """fresh contiguous (nblocks, nproma) arrays, padded tail zeroed (that slice only); batch: ``(batch, nblocks, nproma)``"""
    out = {}
    for n in names:
        t = torch.empty(((batch,) if batch is not None else ()) + (lay.nblocks, lay.nproma), dtype=like.dtype, device=like.device)
        if lay.tail < lay.nproma:
            t[..., -1, lay.tail:] = 0
        out[n] = t
    return out


def _weight_table(weights, wnames, lay: Layout, like: torch.Tensor) -> torch.Tensor:
    """the launchers' table: ten rows of nlev + 1 in the order of OUT_NAMES, device ops only"""
    with torch.no_grad():
        table = torch.zeros((len(B.OUT_NAMES), lay.nlev + 1), dtype=like.dtype, device=like.device)
        for n in wnames:
            table[B.OUT_NAMES.index(n), :lay.nlevx(n)].copy_(weights[n])
    return table


def _sums_block(ts: dict, lay: Layout):
    """contiguous (nblocks, nproma) tensors by name -> the launchers' block of sums (block stride nproma)"""
    blk = B.Outputs()
    for n, t in ts.items():
        f = B.Field()
        f.ptr = _raw(t).data_ptr()
        f.block_stride = lay.nproma
        setattr(blk, n, f)
    return blk


@_no_vmap(_NO_VMAP_COLSUM)
@_inner(raises=_NO_SECOND_COLSUM)
class _Cloudsc2ColsumTl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, names, table, *n trajectory inputs, *n tangents or None) -> the sums of the output tangents
    named: ``cloudsc2_tl_launch_colsum``; a None tangent is a zero tangent that is not read.  Differentiating it again raises
    ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, wnames, table, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = _normalize_present(_present(names, ts[n:]), lay, groups)
        dy = _new_sums(wnames, lay, like)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur),
                                                    C.byref(_block("in", x, lay)), C.byref(_block("in", dx, lay)), _ptr(table),
                                                    C.byref(_sums_block(dy, lay)), _stream(dev)))
        return tuple(dy[k] for k in wnames)


@_no_vmap(_NO_VMAP_COLSUM)
@_inner(raises=_NO_SECOND_COLSUM)
class _Cloudsc2ColsumVjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, want, names, table, *n trajectory inputs, PFPLSL5, PFPLSN5, cover scratch, *the cotangents of
    the sums named or None) -> the input adjoints named in ``want``, in that order: ``cloudsc2_vjp_launch_colsum``; a None cotangent
    is a zero one that is not read, an input not in ``want`` gets no plane.  Differentiating it again raises ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, want, wnames, table, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = {k: t.contiguous() for k, t in _present(wnames, ys).items()}
        xa = _new(want, lay, like)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur),
                                                     C.byref(_block("in", x, lay)), C.byref(_traj_out(fplsl, fplsn, lay)),
                                                     C.byref(_block("in", xa, lay)), _ptr(table), C.byref(_sums_block(y, lay)),
                                                     _scratch_ptr(scratch), _stream(dev)))
        return tuple(xa[k] for k in want)


@_no_vmap(_NO_VMAP_COLSUM)
class _Cloudsc2Colsum(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, names, keep, table, *n inputs) -> the sums named + PFPLSL5, PFPLSN5 and the cover-checkpoint
    # scratch (all three empty without `keep`): one cloudsc2_nl_launch_colsum.  keep: the call tracks gradients, so the forward keeps what
    # the reverse sweep re-reads; else it allocates no plane at all.  backward: one cloudsc2_vjp_launch_colsum; jvp: one
    # cloudsc2_tl_launch_colsum.  Gradients are not materialised: a sum that took no part in the loss is a None cotangent.

    @staticmethod
    def forward(prm, ptsphy, lay, satur, wnames, keep, table, *xs):
        names, _ = _names(satur)
        x = dict(zip(names, xs))
        like = x["pap"]
        dev = like.device
        sums = _new_sums(wnames, lay, like)
        none = torch.empty((0,), dtype=like.dtype, device=dev)
        kept, keep_blk, scratch = {"fplsl": none, "fplsn": none}, None, none
        if keep:
            kept = _new(("fplsl", "fplsn"), lay, like)
            keep_blk = C.byref(_block("out", kept, lay))
            if _evap(prm):
                scratch = torch.empty((lay.nblocks, lay.nlev, lay.nproma), dtype=like.dtype, device=dev)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_nl_launch_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                    C.byref(_block("in", x, lay)), _ptr(table), C.byref(_sums_block(sums, lay)), keep_blk,
                                                    _scratch_ptr(scratch), _stream(dev)))
        return tuple(sums[k] for k in wnames) + (kept["fplsl"], kept["fplsn"], scratch)

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, wnames, keep, table, *xs = inputs
        _save_trajectory(ctx, xs, *output[-3:], table=table, fluxes_are_outputs=False, materialize=False, prm=prm, ptsphy=ptsphy, lay=lay,
                         satur=satur, wnames=wnames, keep=keep)

    @staticmethod
    def backward(ctx, *grads):
        names, _ = _names(ctx.satur)
        need = ctx.needs_input_grad[7:]
        ys = grads[:len(ctx.wnames)]
        nothing = (None,) * (7 + len(names))
        if not any(need) or all(g is None for g in ys):
            return nothing
        _refuse_batched(ys, _NO_VMAP_COLSUM)
        if not ctx.keep:
            raise RuntimeError("cloudsc2_column_sums: backward of a forward that tracked no gradient (nothing was kept for the reverse sweep)")
        table, *saved = ctx.saved_tensors
        want = tuple(n for n, nd in zip(names, need) if nd)
        xa = dict(zip(want, _Cloudsc2ColsumVjp.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, want, ctx.wnames, table, *saved, *ys)))
        return (None,) * 7 + tuple(xa.get(n) for n in names)

    @staticmethod
    def jvp(ctx, *tangents):
        _refuse_batched(tangents, _NO_VMAP_COLSUM)
        table, *xs = ctx.saved_tensors
        dy = _Cloudsc2ColsumTl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, ctx.wnames, table, *xs, *tangents[7:])
        return tuple(dy) + (None, None, None)


def cloudsc2_column_sums(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, weights=None,
                         satur: bool = False) -> Cloudsc2Outputs:
    """Per-column weighted level sums of the outputs of :func:`cloudsc2`, formed inside the sweeps: no output plane, no cotangent plane
    and no tangent plane exists on this route.

    ``inputs``, ``prm``, ``ptsphy``, ``ngptot`` and ``satur`` are those of :func:`cloudsc2`.  ``weights`` maps a non-empty subset of
    ``binding.OUT_NAMES`` to 1-D tensors of length ``nlevx(name)`` in the library's dtype on the inputs' device (any stride); index ``k``
    is the plane's level index, for the four fluxes ``k = 0`` is the top half level.  They are constants (a weight that requires grad
    is refused) and must be finite, which is not checked: the op packs them into one device table with device ops, reads nothing on
    the host and does not synchronise, so after one eager call the forward and ``torch.autograd.grad`` of it can be captured in
    ``torch.cuda.graph``.

    Returns a :class:`Cloudsc2Outputs` holding a ``(nblocks, nproma)`` tensor for every name of ``weights`` and ``None`` for the others.
    Contract, to the bit, for every active column: ``acc = +0; for k: acc = fl(acc + fl(w[k] * out[k]))`` with ``out`` the bits of
    ``cloudsc2(inputs, ..., satur=satur)`` -- the product is rounded before the add.  The padded tail is zero.  A hybrid-level mass
    integral ``sum_k (dA_k + dB_k ps) x_k`` is two sums, ``weights dA`` and ``weights dB``, combined per column afterwards.

    Differentiable with respect to the inputs: ``.backward()``, ``torch.autograd.grad``, ``torch.func.grad`` / ``vjp`` / ``jvp`` and
    ``forward_ad``.  A call that tracks gradients (grad mode on and an input that requires grad) keeps the two flux planes and the
    cover checkpoints the reverse sweep re-reads; any other call allocates no plane.  Backward allocates and writes only the gradients
    that are wanted (``None`` elsewhere) and launches nothing without a cotangent; every gradient is the bits of
    ``cloudsc2(..., sparse=True)`` differentiated through the same fold written in torch.  ``torch.func.vmap`` / ``jacfwd`` /
    ``jacrev`` / ``is_grads_batched`` and double backward raise ``NotImplementedError``."""
    names, groups, (lay, wnames), dev = _enter(inputs, prm, ngptot, satur, check_column_sums, weights)
    xs = tuple(inputs[n] for n in names)
    _refuse_batched(xs + tuple(weights[n] for n in wnames), _NO_VMAP_COLSUM)
    _prepare(dev)
    table = _weight_table(weights, wnames, lay, inputs["pap"])
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in xs)
    out = dict(zip(wnames, _apply(_Cloudsc2Colsum, (prm, float(ptsphy), lay, bool(satur), wnames, bool(keep), table), inputs, names, groups, lay)))
    return Cloudsc2Outputs(*(out.get(n) for n in B.OUT_NAMES))


# ---- the parameter Jacobian and the normal equations of the column sums, one sweep, no sensitivity plane -----------------------------

_PAR_SUMS = tuple(n for n in B.OUT_NAMES if n not in ("clc", "covptot"))  # the outputs that depend on a parameter


def check_sum_residual(residual, weights, wnames, lay: Layout) -> tuple:
    """The checks of :func:`param_normal_equations_column_sums` on its residuals and weights that need no device; raises
    ``ValueError``.  ``residual``: a non-empty mapping of names among ``wnames`` (the names of ``level_weights``) to ``(nblocks, nproma)``
    tensors in the library's dtype; ``weights``: ``None`` or a mapping over a subset of ``residual``'s names with the same shape (a
    missing name is weight 1).  Returns ``(residual, weights)`` as dicts in ``OUT_NAMES`` order."""
    if not hasattr(residual, "keys") or (weights is not None and not hasattr(weights, "keys")):
        raise ValueError(f"residual (and weights, if given) must map names of {B.OUT_NAMES} to tensors; got {type(residual)}, {type(weights)}")
    if len(residual.keys()) == 0:
        raise ValueError("residual is empty: at least one column sum must be observed")
    weights = {} if weights is None else weights
    for what, d in (("residual", residual), ("weights", weights)):
        unknown = sorted(set(d.keys()) - set(B.OUT_NAMES), key=str)
        if unknown:
            raise ValueError(f"{what}: unknown name(s) {unknown}; the outputs are {B.OUT_NAMES}")
    unsummed = sorted(set(residual.keys()) - set(wnames))
    if unsummed:
        raise ValueError(f"residual given for sum(s) {unsummed} that have no level weights (level_weights names {tuple(wnames)})")
    unobserved = sorted(set(weights.keys()) - set(residual.keys()))
    if unobserved:
        raise ValueError(f"weights given for sum(s) {unobserved} that are not observed (no residual)")
    dtype = B.torch_real()
    shape = (lay.nblocks, lay.nproma)
    for what, d in (("residual", residual), ("weights", weights)):
        for n, t in d.items():
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{what}[{n!r}] is not a tensor")
            if t.dtype != dtype:
                raise ValueError(f"{what}[{n!r}] has dtype {t.dtype}; this library works on {dtype} (CLOUDSC2_PRECISION)")
            if tuple(t.shape) != shape:
                raise ValueError(f"{what}[{n!r}] has shape {tuple(t.shape)}, expected {shape} (one value per column)")
    return ({n: residual[n] for n in B.OUT_NAMES if n in residual.keys()}, {n: weights[n] for n in B.OUT_NAMES if n in weights.keys()})


def _enter_parcolsum(inputs, prm: B.Params, ngptot, satur: bool, params, level_weights) -> tuple:
    """what the two functions below check first, as :func:`param_jacobian` does: the layout, the weights' and the parameters' names"""
    names, groups = _names(satur)
    lay = check_layout(inputs, prm, ngptot, satur=satur)
    wnames = check_weights(level_weights, lay, inputs["pap"].device)
    pnames = PARAM_NAMES if params is None else check_params(params, prm)
    ps = () if params is None else tuple(params[n] for n in pnames)
    return names, groups, lay, wnames, pnames, ps


def _finish_parcolsum(who: str, prm: B.Params, pnames, ps, operands) -> tuple:
    """... and then: the operands' device, the refusals of batched operands and of device parameters under capture, ``prm`` with the values"""
    dev = check_device(operands)
    if any(_batched_inside(t) for t in tuple(ps) + tuple(operands)):
        raise NotImplementedError(f"{who}: batched (vmap-wrapped) operands are not supported; call it once per state")
    _check_param_devices(pnames, ps, dev)
    if any(p.device.type != "cpu" for p in ps) and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{who}: the parameters' values are read on the host (they travel in the kernel-argument segment), "
                           "which cannot happen for device tensors while the stream is capturing")
    _prepare(dev)
    return dev, _with_host_values(prm, pnames, ps, who)


def param_jacobian_column_sums(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, level_weights=None, satur: bool = False,
                               params=None) -> dict:
    """The parameter Jacobian of the column sums of :func:`cloudsc2_column_sums` at one state: a dict ``name -> Cloudsc2Outputs`` holding,
    for every name of ``level_weights``, the ``(nblocks, nproma)`` tensor ``s[c] = sum_k w[k] * (d out / d name)[k, c]`` (``None`` for the
    other outputs), for every name of ``PARAM_NAMES`` or of ``params``.  One ``cloudsc2_parjac_launch_colsum``: the sweep of
    :func:`param_jacobian` with its sensitivities folded into per-lane accumulators, no sensitivity plane exists.  Every sum is the
    bits of the fold ``acc = +0; acc = fl(acc + fl(w[k] * J[k]))`` over :func:`param_jacobian`'s planes.

    ``level_weights`` is the ``weights`` of :func:`cloudsc2_column_sums` (packed into a device table with device ops: no host read);
    ``params``, ``satur``, batched operands and stream capture follow :func:`param_jacobian`.  The result is plain tensors without a
    graph, padded tails zero; without the evaporation branch the ``rpecons`` entry is zero tensors; ``clc`` and ``covptot`` depend on
    no parameter: their entries are zero tensors and their weights are accepted and not used."""
    who = "param_jacobian_column_sums"
    names, groups, lay, wnames, pnames, ps = _enter_parcolsum(inputs, prm, ngptot, satur, params, level_weights)
    dev, prm = _finish_parcolsum(who, prm, pnames, ps, [inputs[n] for n in names] + [level_weights[n] for n in wnames])
    evap = _evap(prm)
    with torch.no_grad():
        x = normalize({n: _raw(inputs[n]).detach() for n in names}, lay, groups)
        like = x["pap"]
        ran = PARAM_NAMES if evap else PARAM_NAMES[:-1]  # (nothing depends on rpecons without the evaporation branch: not run)
        swept = tuple(n for n in wnames if n in _PAR_SUMS)
        launch = bool(swept) and any(n in ran for n in pnames)
        dy = {n: _new_sums(swept, lay, like) for n in ran} if launch else {}
        if launch:
            table = _weight_table(level_weights, swept, lay, like)
            blocks = (B.Outputs * len(PARAM_NAMES))(*(_sums_block(dy[n], lay) for n in ran))
            with torch.cuda.device(dev):
                B.check(B.lib.cloudsc2_parjac_launch_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                            C.byref(_block("in", x, lay)), _ptr(table), blocks, _stream(dev)))

        def entry(p, k):
            if k not in wnames:
                return None
            if p in dy and k in dy[p]:
                return dy[p][k]
            return torch.zeros((lay.nblocks, lay.nproma), dtype=like.dtype, device=dev)

        return {p: Cloudsc2Outputs(*(entry(p, k) for k in B.OUT_NAMES)) for p in pnames}


def param_normal_equations_column_sums(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, level_weights=None, residual=None,
                                       weights=None, satur: bool = False, params=None) -> NormalEquations:
    """The Gauss-Newton normal equations of the parameters against observed COLUMN SUMS: ``NormalEquations(names, jtj, jtr)`` as
    :func:`param_normal_equations` returns them, with ``J`` the Jacobian of :func:`param_jacobian_column_sums` (one row per active
    column and observed sum), ``r`` the ``residual`` (model sum - observed sum, from :func:`cloudsc2_column_sums`; a mapping of names
    of ``level_weights`` to ``(nblocks, nproma)`` tensors) and ``W`` the diagonal ``weights`` (``None``, or a mapping over a subset of
    ``residual``'s names, same shape; a missing name is weight 1).  One ``cloudsc2_parnormal_launch_colsum``: neither a sensitivity
    plane nor a sensitivity sum exists in memory; the products are summed in double in a fixed order, the same bits from run to run.
    ``jtj`` is the upper triangle mirrored bit for bit.  The values of ``residual`` and ``weights`` in a padded tail are not read.
    The rules for ``params``, ``satur``, batched operands, ``rpecons`` and stream capture are :func:`param_normal_equations`'s."""
    who = "param_normal_equations_column_sums"
    names, groups, lay, wnames, pnames, ps = _enter_parcolsum(inputs, prm, ngptot, satur, params, level_weights)
    r, w = check_sum_residual(residual, weights, wnames, lay)
    dev, prm = _finish_parcolsum(who, prm, pnames, ps,
                                 [inputs[n] for n in names] + [level_weights[n] for n in wnames] + list(r.values()) + list(w.values()))
    with torch.no_grad():
        if not pnames:
            return NormalEquations((), torch.zeros((0, 0), dtype=torch.float64, device=dev), torch.zeros((0,), dtype=torch.float64, device=dev))
        x = normalize({n: _raw(inputs[n]).detach() for n in names}, lay, groups)
        r = {n: _raw(t).detach().contiguous() for n, t in r.items()}
        w = {n: _raw(t).detach().contiguous() for n, t in w.items()}
        table = _weight_table(level_weights, tuple(n for n in r if n in _PAR_SUMS), lay, x["pap"])
        work = torch.empty(B.NNORMAL * lay.nblocks * lay.nproma, dtype=torch.float64, device=dev)
        normal = torch.empty(B.NNORMAL, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_parnormal_launch_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot,
                                                           C.byref(_block("in", x, lay)), _ptr(table), C.byref(_sums_block(r, lay)),
                                                           C.byref(_sums_block(w, lay)) if w else None, C.c_void_p(work.data_ptr()),
                                                           C.c_void_p(normal.data_ptr()), _stream(dev)))
        idx = [PARAM_NAMES.index(n) for n in pnames]
        jtj = torch.stack([normal[normal_row(a, b)] for a in idx for b in idx]).reshape(len(idx), len(idx))
        jtr = torch.stack([normal[B.NNORMAL - len(PARAM_NAMES) + a] for a in idx])
        return NormalEquations(tuple(pnames), jtj, jtr)


# ---- cloudsc2_ensemble_column_sums: the column sums of K members in one launch, no output plane -------------------------------------

_NO_VMAP_ENSCOLSUM = ("cloudsc2_ensemble_column_sums: torch.func.vmap, jacfwd, jacrev and is_grads_batched=True are not supported (the "
                      "ensemble is the batch: give the members' parameters as (K,) tensors and per-member states as 4-D inputs); use "
                      ".backward() / torch.autograd.grad / torch.func.grad / torch.func.vjp, or torch.autograd.forward_ad / torch.func.jvp")

_NO_SECOND_ENSCOLSUM = ("cloudsc2_ensemble_column_sums: double backward (and forward-over-reverse, reverse-over-forward) is not supported: "
                        "the sweeps are first-order derivatives of CLOUDSC2")


def check_ensemble_column_sums(inputs, prm: B.Params, ngptot: int | None = None, satur: bool = False, params=None, weights=None) -> tuple:
    """Every check of :func:`cloudsc2_ensemble_column_sums` that needs no device: :func:`check_ensemble`, then the weight checks of
    :func:`check_column_sums`; returns ``(layout, K, the given parameter names, the given weight names)``.  Raises ``ValueError``."""
    lay, K, pnames = check_ensemble(inputs, prm, ngptot, satur, params)
    return lay, K, pnames, check_weights(weights, lay, inputs["pap"].device)


def _ens_sums_block(ts: dict, lay: Layout, K: int):
    """contiguous (K, nblocks, nproma) tensors by name -> member 0's block of sums and the member strides"""
    ms = (C.c_longlong * len(B.OUT_NAMES))()
    for n, t in ts.items():
        ms[B.OUT_NAMES.index(n)] = _raw(t).stride(0) if K > 1 else 0
    return _sums_block({n: _raw(t)[0] for n, t in ts.items()}, lay), ms


def _mstride(t: torch.Tensor, K: int) -> int:
    t = _raw(t)
    return t.stride(0) if t.dim() == 4 and K > 1 else 0


@_no_vmap(_NO_VMAP_ENSCOLSUM)
@_inner(raises=_NO_SECOND_ENSCOLSUM)
class _Cloudsc2EnsColsumTl(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, K, names, table, (K, 4) parameters, (K, 4) parameter tangents, *n trajectory inputs, *n
    tangents or None) -> the ``(K, nblocks, nproma)`` sums of the output tangents named: ``cloudsc2_tl_launch_ens_colsum``; a None
    tangent is a zero tangent that is not read.  Differentiating it again raises ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, K, wnames, table, ptab, dptab, *ts):
        names, groups = _names(satur)
        n = len(names)
        x = dict(zip(names, ts[:n]))
        like = x["pap"]
        dev = like.device
        dx = _normalize_present(_present(names, ts[n:]), lay, groups)
        dy = _new_sums(wnames, lay, like, batch=K)
        ptab, dptab = _table(ptab), _table(dptab)
        work = _ens_workspace(K, lay, dev)
        (xb, xm), (db, dm), (yb, ym) = _ens_block("in", x, lay, K), _ens_block("in", dx, lay, K), _ens_sums_block(dy, lay, K)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_tl_launch_ens_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur), K,
                                                        _ptr(ptab), _ptr(dptab), C.byref(xb), xm, C.byref(db), dm, _ptr(table),
                                                        C.byref(yb), ym, _ptr(work), _stream(dev)))
        return tuple(dy[k] for k in wnames)


@_no_vmap(_NO_VMAP_ENSCOLSUM)
@_inner(raises=_NO_SECOND_ENSCOLSUM)
class _Cloudsc2EnsColsumVjp(torch.autograd.Function):
    """forward(prm, ptsphy, layout, satur, K, want, names, table, (K, 4) parameters, *n trajectory inputs, PFPLSL5, PFPLSN5, cover
    scratch, *the cotangents of the sums named or None) -> the ``(K, ...)`` input adjoints named in ``want`` (possibly none: no plane is
    allocated or written) and the ``(K, 4)`` parameter adjoints: ``cloudsc2_vjp_launch_ens_colsum``.  Differentiating it again raises
    ``NotImplementedError``."""

    @staticmethod
    def forward(prm, ptsphy, lay, satur, K, want, wnames, table, ptab, *ts):
        names, _ = _names(satur)
        x, fplsl, fplsn, scratch, ys = _split(names, ts)
        like = x["pap"]
        dev = like.device
        y = {k: t.contiguous() for k, t in _present(wnames, ys).items()}
        xa = _new(want, lay, like, batch=K)
        ptab = _table(ptab)
        work = _ens_workspace(K, lay, dev)
        par_adj = torch.empty((K, len(PARAM_NAMES)), dtype=torch.float64, device=dev)
        (xb, xm), (ab, am), (yb, ym) = _ens_block("in", x, lay, K), _ens_block("in", xa, lay, K), _ens_sums_block(y, lay, K)
        tb, tm = _ens_block("out", {"fplsl": fplsl, "fplsn": fplsn}, lay, K)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_vjp_launch_ens_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, int(satur), K,
                                                         _ptr(ptab), C.byref(xb), xm, C.byref(tb), tm, C.byref(ab), am, _ptr(table),
                                                         C.byref(yb), ym, _scratch_ptr(scratch), _mstride(scratch, K), _ptr(work),
                                                         _ptr(par_adj), _stream(dev)))
        return tuple(xa[k] for k in want) + (par_adj,)


@_no_vmap(_NO_VMAP_ENSCOLSUM)
class _Cloudsc2EnsColsum(torch.autograd.Function):
    # forward(prm, ptsphy, layout, satur, K, names, keep, table, the (K, 4) parameter table, *n inputs, 3-D or 4-D) -> the (K, nblocks,
    # nproma) sums named + the members' PFPLSL5, PFPLSN5 and cover-checkpoint scratch (all three empty without `keep`): one
    # cloudsc2_nl_launch_ens_colsum.  backward: one cloudsc2_vjp_launch_ens_colsum, which allocates the field gradients wanted and nothing
    # else; jvp: one cloudsc2_tl_launch_ens_colsum.  Gradients are not materialised: a sum that took no part in the loss is a None cotangent.

    @staticmethod
    def forward(prm, ptsphy, lay, satur, K, wnames, keep, table, ptab, *xs):
        names, _ = _names(satur)
        x = dict(zip(names, xs))
        like = x["pap"]
        dev = like.device
        sums = _new_sums(wnames, lay, like, batch=K)
        none = torch.empty((0,), dtype=like.dtype, device=dev)
        kept, keep_blk, keep_ms, scratch = {"fplsl": none, "fplsn": none}, None, None, none
        if keep:
            kept = _new(("fplsl", "fplsn"), lay, like, batch=K)
            kb, keep_ms = _ens_block("out", kept, lay, K)
            keep_blk = C.byref(kb)
            if _evap(prm):
                scratch = torch.empty((K, lay.nblocks, lay.nlev, lay.nproma), dtype=like.dtype, device=dev)
        ptab = _table(ptab)
        work = _ens_workspace(K, lay, dev)
        (xb, xm), (sb, sm) = _ens_block("in", x, lay, K), _ens_sums_block(sums, lay, K)
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_nl_launch_ens_colsum(C.byref(prm), float(ptsphy), lay.nproma, lay.nlev, lay.ngptot, K, _ptr(ptab),
                                                        C.byref(xb), xm, _ptr(table), C.byref(sb), sm, keep_blk, keep_ms,
                                                        _scratch_ptr(scratch), _mstride(scratch, K), _ptr(work), _stream(dev)))
        return tuple(sums[k] for k in wnames) + (kept["fplsl"], kept["fplsn"], scratch)

    @staticmethod
    def setup_context(ctx, inputs, output):
        prm, ptsphy, lay, satur, K, wnames, keep, table, ptab, *xs = inputs
        _save_trajectory(ctx, (ptab, *xs), *output[-3:], table=table, fluxes_are_outputs=False, materialize=False, prm=prm, ptsphy=ptsphy,
                         lay=lay, satur=satur, K=K, wnames=wnames, keep=keep)

    @staticmethod
    def backward(ctx, *grads):
        names, _ = _names(ctx.satur)
        need_p, need = ctx.needs_input_grad[8], ctx.needs_input_grad[9:]
        ys = grads[:len(ctx.wnames)]
        nothing = (None,) * (9 + len(names))
        if (not need_p and not any(need)) or all(g is None for g in ys):
            return nothing
        _refuse_batched(ys, _NO_VMAP_ENSCOLSUM)
        if not ctx.keep:
            raise RuntimeError("cloudsc2_ensemble_column_sums: backward of a forward that tracked no gradient (nothing was kept for the "
                               "reverse sweep)")
        table, ptab, *saved = ctx.saved_tensors
        want = tuple(n for n, nd in zip(names, need) if nd)
        *xa, par_adj = _Cloudsc2EnsColsumVjp.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, ctx.K, want, ctx.wnames, table, ptab, *saved, *ys)
        xa = dict(zip(want, xa))
        # a per-member input gets its members' gradients, a shared one their sum
        gx = tuple((xa[n] if x.dim() == 4 else xa[n].sum(0)) if n in xa else None for n, x in zip(names, saved))
        return (None,) * 8 + (par_adj if need_p else None,) + gx

    @staticmethod
    def jvp(ctx, *tangents):
        _refuse_batched(tangents, _NO_VMAP_ENSCOLSUM)
        table, ptab, *xs = ctx.saved_tensors
        dptab = tangents[8] if tangents[8] is not None else torch.zeros_like(ptab)
        dy = _Cloudsc2EnsColsumTl.apply(ctx.prm, ctx.ptsphy, ctx.lay, ctx.satur, ctx.K, ctx.wnames, table, ptab, dptab, *xs, *tangents[9:])
        return tuple(dy) + (None, None, None)


def cloudsc2_ensemble_column_sums(inputs, prm: B.Params, ptsphy: float, ngptot: int | None = None, weights=None, params=None,
                                  satur: bool = False) -> Cloudsc2Outputs:
    """The column sums of a perturbed-parameter ensemble in one launch: :func:`cloudsc2_ensemble` and :func:`cloudsc2_column_sums` at
    once, which is what a calibration needs -- K members' surface precipitation or column-integrated tendencies and their gradient with
    respect to the parameters -- without an output, cotangent or tangent plane for any member.

    ``inputs``, ``params``, ``satur``, ``prm`` and ``ngptot`` are those of :func:`cloudsc2_ensemble` (3-D shared or 4-D per-member
    inputs with any member stride; ``(K,)`` float64 parameters on the inputs' device, a name not given keeps ``prm``'s value; the same
    refusals).  ``weights`` is that of :func:`cloudsc2_column_sums`, shared by all members.  Nothing is read on the host and nothing
    synchronises: after one eager call the forward and ``torch.autograd.grad`` of it can be captured in ``torch.cuda.graph``, and a
    replay after ``params[name].copy_(new)`` computes with the new values.

    Returns a :class:`Cloudsc2Outputs` holding a ``(K, nblocks, nproma)`` tensor for every name of ``weights`` and ``None`` for the
    others, the padded tail zero.  Member k of every sum is the bits of ``cloudsc2_column_sums`` for a ``prm`` holding row k.

    ``.backward()``, ``torch.autograd.grad``, ``torch.func.grad`` / ``vjp`` / ``jvp`` and ``forward_ad`` differentiate with respect to
    the ``(K,)`` parameters (gradient ``(K,)``, float64, on the device: the bits of ``cloudsc2(..., params=row k)`` differentiated
    through the same fold written in torch) and the fields (a 4-D input gets per-member gradients, the bits of
    ``cloudsc2_column_sums``'s; a 3-D shared input their sum over the members).  A call that tracks no gradient allocates no plane; one
    that does keeps, per member, the two flux planes and (evaporation branch) the cover checkpoint.  Backward allocates the field
    gradients that are wanted and nothing else: with only parameter gradients wanted it allocates no plane at all.
    ``torch.func.vmap`` / ``jacfwd`` / ``jacrev`` / ``is_grads_batched`` and double backward raise ``NotImplementedError``."""
    names, groups, (lay, K, pnames, wnames), dev = _enter(inputs, prm, ngptot, satur, check_ensemble_column_sums, params, weights)
    ptab = _ens_table(inputs, names, prm, params, pnames, K, dev, _NO_VMAP_ENSCOLSUM, more=tuple(weights[n] for n in wnames))
    table = _weight_table(weights, wnames, lay, inputs["pap"])
    keep = torch.is_grad_enabled() and (ptab.requires_grad or any(inputs[n].requires_grad for n in names))
    lead = (prm, float(ptsphy), lay, bool(satur), K, wnames, bool(keep), table, ptab)
    out = dict(zip(wnames, _apply(_Cloudsc2EnsColsum, lead, inputs, names, groups, lay)))
    return Cloudsc2Outputs(*(out.get(n) for n in B.OUT_NAMES))


def satur(pap: torch.Tensor, t: torch.Tensor, prm: B.Params, ngptot: int | None = None, differentiable: bool = False) -> torch.Tensor:
    """SATUR (satur.F90:106-123, the LPHYLIN branch the drivers call) into a new ``(nblocks, nlev, nproma)`` tensor.  By default
    with NO gradient: passed to :func:`cloudsc2` as ``qsat`` it is a constant input there (differentiate through ``qsat`` only as
    an input of its own, as CLOUDSC2TL / CLOUDSC2AD do).  ``differentiable=True``: the result carries first-order derivatives with
    respect to ``pap`` and ``t`` (``cloudsc2_satur_lin_launch``: the two partial planes are saved, backward and jvp are elementwise
    products with them; no double backward, no vmap) -- the unfused counterpart of ``cloudsc2(..., satur=True)``."""
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
    if differentiable:
        return _Satur.apply(prm, lay, pap, t)[0]
    with torch.no_grad():
        pap, t = pap.detach().contiguous(), t.detach().contiguous()
        q = _new(("qsat",), lay, pap)["qsat"]
        with torch.cuda.device(dev):
            B.check(B.lib.cloudsc2_satur_launch(C.byref(prm), nproma, nlev, lay.ngptot, _field(pap, lay, "pap"), _field(t, lay, "t"),
                                                _field(q, lay, "qsat"), _stream(dev)))
    return q
