#!/usr/bin/env python3
"""The differentiable op (dwarf_p_cloudsc2_tl_ad_amd.autograd) at 160 000 columns, NPROMA 128, fp64: forward, backward and jvp
through torch, the VJP kernel alone, and the route the op replaces for a backward (clone the 10 grad_outputs, then
cloudsc2_ad_launch_reverse with assign=1, which zeroes its output adjoints).  Prints ONE JSON object: median times over REPS
event-timed calls after warm-up, the bytes per column each moves (loads + stores of the sweeps as written, counted below) and
the fraction of 8 TB/s that is.
    python tools/autograd_timing.py [NGPTOT [REPS]]"""
import ctypes as C
import json
import sys

import timing_harness as th
import torch

from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
from dwarf_p_cloudsc2_tl_ad_amd import binding as B

ngptot = int(sys.argv[1]) if len(sys.argv) > 1 else 160000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
nproma, nlev = 128, 137

case = th.setup(ngptot, nproma, nlev, prepare=False)
prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
xs = {n: t.detach().requires_grad_() for n, t in x.items()}  # views of the state's arena: no copies in the op
assert all(t.data_ptr() == ag.normalize(x, lay, ag.IN_GROUPS)[n].data_ptr() for n, t in x.items()), "inputs would be copied"
g = torch.Generator(device=dev).manual_seed(0)
u = {n: torch.randn(lay.shape(n), generator=g, dtype=torch.float64, device=dev) for n in B.OUT_NAMES}
v = {n: 0.01 * t for n, t in x.items()}
st = lambda: th.stream(dev)  # noqa: E731
new = lambda names: th.new(names, lay, dev)  # noqa: E731
timed = lambda step, pre=None: th.median_ms(step, reps, pre=pre)  # noqa: E731

# forward / backward / jvp through torch
fwd_ms = timed(lambda: ag.cloudsc2(xs, prm, ptsphy, ngptot))
out = ag.cloudsc2(xs, prm, ptsphy, ngptot)
outs, ins, us = list(out), [xs[n] for n in B.IN_NAMES], [u[n] for n in B.OUT_NAMES]
bwd_ms = timed(lambda: torch.autograd.grad(outs, ins, us, retain_graph=True))
keys = list(B.IN_NAMES)
# forward-mode AD gives the BASE of a view a tangent too (a zero fill of the whole state arena per call): the jvp is timed on
# separate arrays, as a caller of torch.func.jvp would hold them
xc = {n: t.clone() for n, t in x.items()}
jvp_ms = timed(lambda: torch.func.jvp(lambda *a: tuple(ag.cloudsc2(dict(zip(keys, a)), prm, ptsphy, ngptot)),
                                      tuple(xc[n] for n in keys), tuple(v[n] for n in keys)))

# the kernels alone, on preallocated buffers
traj = new(B.OUT_NAMES)
B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), ptsphy, nproma, nlev, ngptot, C.byref(ag._block("in", x, lay)),
                                         C.byref(ag._block("out", traj, lay)), None, st()))
xa, y = new(B.IN_NAMES), new(B.OUT_NAMES)
blk = lambda: (C.byref(prm), ptsphy, nproma, nlev, ngptot, C.byref(ag._block("in", x, lay)), C.byref(ag._block("out", traj, lay)),  # noqa: E731
               C.byref(ag._block("in", xa, lay)))
refill = lambda: [y[n].copy_(u[n]) for n in B.OUT_NAMES]  # noqa: E731
vjp_kernel_ms = timed(lambda: B.check(B.lib.cloudsc2_vjp_launch(*blk(), C.byref(ag._block("out", u, lay)), None, st())))
reverse_kernel_ms = timed(lambda: B.check(B.lib.cloudsc2_ad_launch_reverse(*blk(), C.byref(ag._block("out", y, lay)), None, 1, st())),
                          pre=refill)


def clone_route():
    yc = {n: u[n].clone() for n in B.OUT_NAMES}
    B.check(B.lib.cloudsc2_ad_launch_reverse(*blk(), C.byref(ag._block("out", yc, lay)), None, 1, st()))


clone_route_ms = timed(clone_route)
dy = new(B.OUT_NAMES)
tl_kernel_ms = timed(lambda: B.check(B.lib.cloudsc2_tl_launch(C.byref(prm), ptsphy, nproma, nlev, ngptot, C.byref(ag._block("in", x, lay)),
                                                             C.byref(B.Outputs()), C.byref(ag._block("in", v, lay)),
                                                             C.byref(ag._block("out", dy, lay)), st())))

# bytes per column: reals loaded + stored by each sweep as written (no evaporation branch: no cover checkpoints)
R, H = nlev, nlev + 1  # one full-level / half-level plane
traj_in = 15 * R + H          # 15 full-level inputs and PAPHP1
outs10 = 6 * R + 4 * H        # 4 tendencies, PCLC, PCOVPTOT, 4 fluxes
fwd_b = 8 * (traj_in + outs10)
# reverse sweep: the trajectory inputs, PFPLSL5 / PFPLSN5 and the 10 output adjoints in (the fluxes' top level not read), the 16
# input adjoints out; the assign form also stores zeros over the 10 output adjoints
rev_in = traj_in + 2 * R + 6 * R + 4 * R
vjp_b = 8 * (rev_in + traj_in)
rev_b = 8 * (rev_in + traj_in + outs10)
clone_b = 8 * 2 * outs10 + rev_b
tl_b = 8 * (2 * traj_in + outs10)
jvp_b = fwd_b + tl_b

row = lambda ms, b: th.row(ms, b, ngptot)  # noqa: E731

print(json.dumps({
    "ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp64", "reps": reps, "device": torch.cuda.get_device_name(dev),
    "forward": row(fwd_ms, fwd_b),
    "backward": row(bwd_ms, vjp_b),
    "jvp_forward_plus_tl": row(jvp_ms, jvp_b),
    "vjp_kernel": row(vjp_kernel_ms, vjp_b),
    "reverse_assign_kernel": row(reverse_kernel_ms, rev_b),
    "clone_plus_reverse_assign": row(clone_route_ms, clone_b),
    "tl_kernel_no_traj": row(tl_kernel_ms, tl_b),
    "vjp_over_reverse_assign": round(vjp_kernel_ms / reverse_kernel_ms, 3),
    "backward_over_clone_route": round(bwd_ms / clone_route_ms, 3),
}))
