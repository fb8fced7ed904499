#!/usr/bin/env python3
"""What the parameter Jacobian costs: one cloudsc2_tl_launch_parjac against NP calls of cloudsc2_tl_launch_par (zero-filled tangent
planes, dpar = e_k), and ``c2.param_jacobian`` against the Python loop of NP ``torch.func.jvp`` calls with a unit tangent on one
parameter; fp64, NPROMA 128, in ONE process: the state placed by the library's allocator (as bench.py does), warmed, then the two forms
in alternating order, device events around each.  NP = 3, or 4 with the evaporation branch.
    python tools/autograd_parjac_timing.py run [NGPTOT [REPS [evap]]]     ONE JSON object
Bytes per column (NLEV 137, fp64): 17 544 + NP x 10 992 against NP x 46 080, i.e. 0.37 (NP = 3) and 0.33 (NP = 4).  Run it in three
fresh processes and take the median of the medians (profiles/autograd_parjac_timing.json)."""
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

# one zero plane per tangent field, as a caller without the new launcher has them (the single launcher reads all 16)
zero = {n: torch.zeros(lay.shape(n), dtype=dtype, device=dev) for n in B.IN_NAMES}
sens = [new(B.OUT_NAMES) for _ in range(np_run)]
loop_out = [new(B.OUT_NAMES) for _ in range(np_run)]
head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
bx, bz = ag._block("in", x, lay), ag._block("in", zero, lay)
blocks = (B.Outputs * NPAR)(*(ag._block("out", s, lay) for s in sens))
loop_blocks = [ag._block("out", o, lay) for o in loop_out]
units = [(C.c_double * NPAR)(*[1.0 if j == k else 0.0 for j in range(NPAR)]) for k in range(np_run)]
one = torch.tensor(1.0, dtype=torch.float64)


def abi_loop():
    for k in range(np_run):
        B.check(B.lib.cloudsc2_tl_launch_par(*head, 0, C.byref(bx), C.byref(bz), units[k], C.byref(loop_blocks[k]), st()))


def abi_parjac():
    B.check(B.lib.cloudsc2_tl_launch_parjac(*head, C.byref(bx), blocks, st()))


def torch_loop():
    out = []
    for name in c2.PARAM_NAMES[:np_run]:
        f = lambda p, name=name: tuple(c2.cloudsc2(x, prm, ptsphy, ngptot, params={name: p}))  # noqa: E731
        out.append(torch.func.jvp(f, (torch.tensor(getattr(prm, name), dtype=torch.float64),), (one,))[1])
    return out


def torch_parjac():
    return c2.param_jacobian(x, prm, ptsphy, ngptot)


pairs = {"abi": (abi_loop, abi_parjac), "torch": (torch_loop, torch_parjac)}
for _ in range(3):
    for loop, fused in pairs.values():
        loop()
        fused()
torch.cuda.synchronize()
same = all(torch.equal(sens[k][n].view(torch.int64), loop_out[k][n].view(torch.int64)) for k in range(np_run) for n in B.OUT_NAMES) \
    if not B.SINGLE else None

ms = {f"{k}_{form}": [] for k in pairs for form in ("loop", "parjac")}
for r in range(reps):
    for k, (loop, fused) in pairs.items():
        order = (("loop", loop), ("parjac", fused)) if r % 2 == 0 else (("parjac", fused), ("loop", loop))
        for form, step in order:
            ms[f"{k}_{form}"].append(th.event_ms(step))

res = {"ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp32" if B.SINGLE else "fp64", "reps": reps, "evap": evap,
       "directions": np_run, "device": torch.cuda.get_device_name(dev), "same_bits_as_the_loop": same,
       "byte_ratio": round((17544 + np_run * 10992) / (np_run * 46080), 4)}
for k, t in ms.items():
    res[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
for k in pairs:
    res[f"{k}_ratio"] = round(res[f"{k}_parjac"]["median_ms"] / res[f"{k}_loop"]["median_ms"], 4)
print(json.dumps(res))
