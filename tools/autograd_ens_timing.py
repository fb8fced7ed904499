#!/usr/bin/env python3
"""What a perturbed-parameter ensemble costs: ``c2.cloudsc2_ensemble`` with K members over ONE shared state (one launch per sweep, the
parameters read on the device) against the loop it replaces, K calls of ``c2.cloudsc2(..., params={0-d device tensors})`` (each reads
its parameters on the host: a synchronisation per call); fp64, NPROMA 128, in ONE process: the state placed by the library's allocator
(as bench.py does), warmed, then the forms in rotating order.  Two steps are timed: the forward alone, and the forward with the
backward of a loss over tent, fplsl and covptot with respect to the parameters and the shared ``t``.  The loop's host reads are part of
its cost, so the times are wall clock between two device synchronisations.
    python tools/autograd_ens_timing.py run [NGPTOT [K [REPS [evap]]]]     ONE JSON object with the median times
It writes nothing but that line."""
import json
import statistics
import sys

import timing_harness as th
import torch

import dwarf_p_cloudsc2_tl_ad_amd as c2
from dwarf_p_cloudsc2_tl_ad_amd import binding as B

args = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]
ngptot = int(args[0]) if len(args) > 0 else 160000
K = int(args[1]) if len(args) > 1 else 8
reps = int(args[2]) if len(args) > 2 else 10
evap = len(args) > 3 and args[3] == "evap"
nproma, nlev = 128, 137
LOSS = ("tent", "fplsl", "covptot")

case = th.setup(ngptot, nproma, nlev, prepare=False, fp64=False, levapls2=evap)
prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
dtype = B.torch_real()

factors = torch.linspace(0.8, 1.2, K, dtype=torch.float64, device=dev)
members = {n: (getattr(prm, n) * factors).requires_grad_() for n in c2.PARAM_NAMES}
singles = [{n: members[n][k].detach().clone().requires_grad_() for n in c2.PARAM_NAMES} for k in range(K)]
xt = dict(x, t=x["t"].detach().clone().requires_grad_())
gen = torch.Generator(device=dev).manual_seed(1)
w = {n: torch.randn(lay.shape(n), generator=gen, dtype=dtype, device=dev) for n in LOSS}
wk = {n: w[n].unsqueeze(0).expand(K, *w[n].shape) for n in LOSS}


def ens_forward():
    with torch.no_grad():
        return c2.cloudsc2_ensemble(x, prm, ptsphy, ngptot, params={n: p.detach() for n, p in members.items()})


def loop_forward():
    with torch.no_grad():
        return [c2.cloudsc2(x, prm, ptsphy, ngptot, params={n: p.detach() for n, p in s.items()}) for s in singles]


def ens_backward():
    out = c2.cloudsc2_ensemble(xt, prm, ptsphy, ngptot, params=members)
    return torch.autograd.grad([getattr(out, n) for n in LOSS], list(members.values()) + [xt["t"]], [wk[n] for n in LOSS])


def loop_backward():
    grads = []
    for s in singles:
        out = c2.cloudsc2(xt, prm, ptsphy, ngptot, params=s)
        grads.append(torch.autograd.grad([getattr(out, n) for n in LOSS], list(s.values()) + [xt["t"]], [w[n] for n in LOSS]))
    return grads


forms = {"ensemble_forward": ens_forward, "loop_forward": loop_forward, "ensemble_forward_backward": ens_backward,
         "loop_forward_backward": loop_backward}
for _ in range(2):
    for step in forms.values():
        step()
torch.cuda.synchronize()
ge, gl = ens_backward(), loop_backward()
torch.cuda.synchronize()
same = all(bool(ge[i][k] == gl[k][i]) for k in range(K) for i in range(len(c2.PARAM_NAMES)))
del ge, gl

ms = th.rotated(forms, reps, th.wall_ms, 4)

res = {"ngptot": ngptot, "members": K, "nproma": nproma, "nlev": nlev, "precision": "fp32" if B.SINGLE else "fp64", "reps": reps,
       "evap": evap, "device": torch.cuda.get_device_name(dev), "clock": "wall, between device synchronisations",
       "parameter_gradients_equal_the_loops": same}
for k, t in ms.items():
    res[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
print(json.dumps(res))
