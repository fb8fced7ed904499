#!/usr/bin/env python3
"""What the parameter gradients cost: cloudsc2_vjp_launch_par (reverse sweep + fold of the workspace) against the PARENT commit's
cloudsc2_vjp_launch, and cloudsc2_tl_launch_par against the parent's cloudsc2_tl_launch without trajectory stores, fp64, NPROMA 128,
in ONE process: both libraries loaded, the state placed by this library's allocator (as bench.py does), warmed, then the four
launchers in alternation, device events around each launch.
    python tools/autograd_par_timing.py run PARENT_LIB.so [NGPTOT [REPS [evap]]]     ONE JSON object
PARENT_LIB.so: libcloudsc2_hip.so built from the parent commit (make -C dwarf_p_cloudsc2_tl_ad_amd/csrc in a checkout of it).
Accepted when the new launch's median is no more than the parent's median * (1 + the parent's own spread in this call, (max - min) /
median of its repeats, + 0.02 for the added instructions and registers)."""
import ctypes as C
import json
import os
import statistics
import sys

import timing_harness as th
import torch

import dwarf_p_cloudsc2_tl_ad_amd as c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
from dwarf_p_cloudsc2_tl_ad_amd import binding as B

args = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]
parent = C.CDLL(os.path.abspath(args[0]))
ngptot = int(args[1]) if len(args) > 1 else 160000
reps = int(args[2]) if len(args) > 2 else 25
evap = len(args) > 3 and args[3] == "evap"
nproma, nlev = 128, 137
for name in ("cloudsc2_vjp_launch", "cloudsc2_tl_launch"):
    getattr(parent, name).argtypes = getattr(B.lib, name).argtypes
    getattr(parent, name).restype = C.c_int

case = th.setup(ngptot, nproma, nlev, prepare=False, fp64=False, levapls2=evap)
prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
dtype = B.torch_real()
g = torch.Generator(device=dev).manual_seed(0)
u = {n: torch.randn(lay.shape(n), generator=g, dtype=dtype, device=dev) for n in B.OUT_NAMES}
v = {n: 0.01 * t for n, t in x.items()}
st = lambda: th.stream(dev)  # noqa: E731
new = lambda names: th.new(names, lay, dev)  # noqa: E731

traj, xa, dy = new(B.OUT_NAMES), new(B.IN_NAMES), new(B.OUT_NAMES)
scratch = torch.zeros((lay.nblocks, nlev, nproma), dtype=dtype, device=dev)
head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
B.check(B.lib.cloudsc2_ad_launch_forward(*head, C.byref(ag._block("in", x, lay)), C.byref(ag._block("out", traj, lay)),
                                         C.c_void_p(scratch.data_ptr()), st()))
nwork = C.c_longlong()
B.check(B.lib.cloudsc2_par_work_doubles(nproma, ngptot, C.byref(nwork)))
work = torch.empty(nwork.value, dtype=torch.float64, device=dev)
par_adj = torch.empty(4, dtype=torch.float64, device=dev)
dpar = (C.c_double * 4)(*[0.01 * getattr(prm, n) for n in c2.PARAM_NAMES])
bx, bt, bxa, bu, bv, bdy, none = (ag._block("in", x, lay), ag._block("out", traj, lay), ag._block("in", xa, lay), ag._block("out", u, lay),
                                  ag._block("in", v, lay), ag._block("out", dy, lay), B.Outputs())
sc, wk, pa = C.c_void_p(scratch.data_ptr()), C.c_void_p(work.data_ptr()), C.c_void_p(par_adj.data_ptr())


def ok(rc):
    assert rc == 0, rc


steps = {
    "vjp_parent": lambda: ok(parent.cloudsc2_vjp_launch(*head, C.byref(bx), C.byref(bt), C.byref(bxa), C.byref(bu), sc, st())),
    "vjp_par": lambda: B.check(B.lib.cloudsc2_vjp_launch_par(*head, 0, C.byref(bx), C.byref(bt), C.byref(bxa), C.byref(bu), sc, wk, pa, st())),
    "tl_parent": lambda: ok(parent.cloudsc2_tl_launch(*head, C.byref(bx), C.byref(none), C.byref(bv), C.byref(bdy), st())),
    "tl_par": lambda: B.check(B.lib.cloudsc2_tl_launch_par(*head, 0, C.byref(bx), C.byref(bv), dpar, C.byref(bdy), st())),
}
for _ in range(5):
    for step in steps.values():
        step()
torch.cuda.synchronize()
ms = th.rotated(steps, reps, th.event_ms, 1)  # (the same order in every repetition)

res = {"ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp32" if B.SINGLE else "fp64", "reps": reps, "evap": evap,
       "device": torch.cuda.get_device_name(dev), "par_adj": par_adj.cpu().tolist()}
for k, t in ms.items():
    res[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
              "spread": round((max(t) - min(t)) / statistics.median(t), 4)}
for fam in ("vjp", "tl"):
    p, n = res[fam + "_parent"], res[fam + "_par"]
    res[fam + "_ratio"] = round(n["median_ms"] / p["median_ms"], 4)
    res[fam + "_accepted"] = bool(n["median_ms"] <= p["median_ms"] * (1.0 + p["spread"] + 0.02))
print(json.dumps(res))
