#!/usr/bin/env python3
"""What the Gauss-Newton normal equations of the parameters cost: one cloudsc2_parnormal_launch (J^T W J and J^T W r summed in the
sweep, no sensitivity plane) against cloudsc2_tl_launch_parjac alone (which only writes the planes) and against ``c2.param_jacobian``
followed by the contraction in torch (per output: stack the NP planes, multiply by the weight, two matrix products); all ten outputs
observed and weighted, fp64, NPROMA 128, in ONE process: the state placed by the library's allocator (as bench.py does), warmed, then
the three forms in rotating order, device events around each.  NP = 3, or 4 with the evaporation branch.
    python tools/autograd_parnormal_timing.py run [NGPTOT [REPS [evap]]]     ONE JSON object with the three median times
Bytes per column (NLEV 137, fp64): 17 544 + 2 x 10 992 + 14 x 8 = 39 640 against 17 544 + NP x 10 992 written by the parameter Jacobian
alone, and at least 127 464 with a contraction that read every plane exactly once.  It writes nothing but that line."""
import ctypes as C
import json
import statistics
import sys

import timing_harness as th
import torch

import dwarf_p_cloudsc2_tl_ad_amd as c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
from dwarf_p_cloudsc2_tl_ad_amd import binding as B

args = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]
ngptot = int(args[0]) if len(args) > 0 else 160000
reps = int(args[1]) if len(args) > 1 else 30
evap = len(args) > 2 and args[2] == "evap"
nproma, nlev = 128, 137
NPAR = len(c2.PARAM_NAMES)
np_run = NPAR if evap else NPAR - 1

case = th.setup(ngptot, nproma, nlev, prepare=False, fp64=False, levapls2=evap)
prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
dtype = B.torch_real()
st = lambda: th.stream(dev)  # noqa: E731
new = lambda names: th.new(names, lay, dev)  # noqa: E731

gen = torch.Generator(device=dev).manual_seed(1)
resid = {n: torch.randn(lay.shape(n), generator=gen, dtype=dtype, device=dev) for n in B.OUT_NAMES}
weight = {n: torch.rand(lay.shape(n), generator=gen, dtype=dtype, device=dev) + 0.5 for n in B.OUT_NAMES}
for t in resid.values():  # (the padded tail: the sweep does not read it, the torch contraction multiplies it by zero sensitivities)
    if lay.tail < lay.nproma:
        t[-1, :, lay.tail:] = 0
sens = [new(B.OUT_NAMES) for _ in range(np_run)]
work = torch.empty(B.NNORMAL * lay.nblocks * nproma, dtype=torch.float64, device=dev)
normal = torch.empty(B.NNORMAL, dtype=torch.float64, device=dev)
head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
bx, br, bw = ag._block("in", x, lay), ag._block("out", resid, lay), ag._block("out", weight, lay)
blocks = (B.Outputs * NPAR)(*(ag._block("out", s, lay) for s in sens))


def abi_parnormal():
    B.check(B.lib.cloudsc2_parnormal_launch(*head, C.byref(bx), C.byref(br), C.byref(bw), C.c_void_p(work.data_ptr()),
                                            C.c_void_p(normal.data_ptr()), st()))


def abi_parjac():
    B.check(B.lib.cloudsc2_tl_launch_parjac(*head, C.byref(bx), blocks, st()))


def torch_contraction():
    jac = c2.param_jacobian(x, prm, ptsphy, ngptot)
    jtj = torch.zeros((np_run, np_run), dtype=torch.float64, device=dev)
    jtr = torch.zeros(np_run, dtype=torch.float64, device=dev)
    for k, n in enumerate(B.OUT_NAMES):
        J = torch.stack([jac[p][k] for p in c2.PARAM_NAMES[:np_run]]).flatten(1).to(torch.float64)
        wJ = J * weight[n].flatten().to(torch.float64)
        jtj += wJ @ J.T
        jtr += wJ @ resid[n].flatten().to(torch.float64)
    return jtj, jtr


forms = {"parnormal": abi_parnormal, "parjac_alone": abi_parjac, "param_jacobian_then_torch": torch_contraction}
for _ in range(3):
    for step in forms.values():
        step()
torch.cuda.synchronize()
jtj, jtr = torch_contraction()
got = normal.cpu().tolist()
agree = max(abs(got[B.NNORMAL - NPAR + a] - float(jtr[a])) / max(abs(float(jtr[a])), 1e-300) for a in range(np_run))

ms = th.rotated(forms, reps, th.event_ms, 3)

res = {"ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp32" if B.SINGLE else "fp64", "reps": reps, "evap": evap,
       "directions": np_run, "device": torch.cuda.get_device_name(dev), "jtr_relative_difference_from_torch": agree}
for k, t in ms.items():
    res[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
print(json.dumps(res))
