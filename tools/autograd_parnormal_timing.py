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
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dwarf_p_cloudsc2_tl_ad_amd as c2  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import binding as B  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd.state import PLANE_Q, PLANE_QI, PLANE_QL, PLANE_T  # noqa: E402

args = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]
ngptot = int(args[0]) if len(args) > 0 else 160000
reps = int(args[1]) if len(args) > 1 else 30
evap = len(args) > 2 and args[2] == "evap"
nproma, nlev = 128, 137
NPAR = len(c2.PARAM_NAMES)
np_run = NPAR if evap else NPAR - 1

tab = c2.synthetic_table(nlev)
prm = c2.default_params(c2.ceta_from_table(tab), lregcl=True, levapls2=evap)
ds = c2.DeviceState.from_table(tab, nproma, ngptot)
ds.satur(prm)
x = {"paph": ds.PAPH, "pap": ds.PAP, "q": ds.PQ, "qsat": ds.QSAT, "t": ds.PT, "l": ds.PCLV[:, 0], "i": ds.PCLV[:, 1],
     "lude": ds.PLUDE, "lu": ds.PLU, "mfu": ds.PMFU, "mfd": ds.PMFD, "gtent": ds.B_CML[:, PLANE_T], "gtenq": ds.B_CML[:, PLANE_Q],
     "gtenl": ds.B_CML[:, PLANE_QL], "gteni": ds.B_CML[:, PLANE_QI], "supsat": ds.PSUPSAT}
lay = ag.check_layout(x, prm, ngptot)
ptsphy = float(ds.ptsphy)
dev = ds.device
dtype = B.torch_real()
st = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
new = lambda names: {n: torch.empty(lay.shape(n), dtype=dtype, device=dev) for n in names}  # noqa: E731

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


def timed(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


ms = {k: [] for k in forms}
names = list(forms)
for r in range(reps):
    for k in names[r % 3:] + names[:r % 3]:
        ms[k].append(timed(forms[k]))

res = {"ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp32" if B.SINGLE else "fp64", "reps": reps, "evap": evap,
       "directions": np_run, "device": torch.cuda.get_device_name(dev), "jtr_relative_difference_from_torch": agree}
for k, t in ms.items():
    res[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
print(json.dumps(res))
