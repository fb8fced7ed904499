#!/usr/bin/env python3
"""The differentiable op with SATUR inside (cloudsc2(..., satur=True)) at 160 000 columns, NPROMA 128, fp64 (fp32 with
CLOUDSC2_PRECISION=single, for the record): the two fused sweeps alone (cloudsc2_tl_launch_satur, cloudsc2_vjp_launch_satur) next to
the sweeps they replace (cloudsc2_tl_launch without trajectory stores, cloudsc2_vjp_launch, qsat as a plane), and backward / jvp of
the fused op through torch next to the unfused route (satur(differentiable=True) + cloudsc2 + torch's chain rule).
    python tools/autograd_satur_timing.py run [NGPTOT [REPS]]        ONE JSON object: event medians after warm-up, bytes per column
                                                                     (loads + stores of the sweeps as written, counted below)
    python tools/autograd_satur_timing.py summarise OUT.json PARENT.jsonl NEW.jsonl
        PARENT.jsonl: lines of tools/autograd_timing.py run on the parent commit, NEW.jsonl: lines of `run`, fresh processes in
        alternation; writes the medians, the spreads and the ratios"""
import ctypes as C
import json
import statistics
import sys

import timing_harness as th


def summarise(out_path, parent_path, new_path):
    parent = [json.loads(line) for line in open(parent_path) if line.startswith("{")]
    new = [json.loads(line) for line in open(new_path) if line.startswith("{")]
    med = lambda rows, k: statistics.median(r[k]["ms"] for r in rows)  # noqa: E731
    spread = lambda rows, k: th.spread(rows, (k, "ms"))  # noqa: E731
    res = {"pairs": min(len(parent), len(new)), "ngptot": new[0]["ngptot"], "nproma": new[0]["nproma"], "precision": new[0]["precision"],
           "device": new[0]["device"], "runs_parent": parent, "runs_new": new}
    for name, pk, nk in (("tl", "tl_kernel_no_traj", "tl_kernel_satur"), ("vjp", "vjp_kernel", "vjp_kernel_satur")):
        res[name] = {"parent_ms": round(med(parent, pk), 4), "parent_spread": spread(parent, pk),
                     "fused_ms": round(med(new, nk), 4), "fused_spread": spread(new, nk),
                     "ratio": round(med(new, nk) / med(parent, pk), 4),
                     "byte_ratio": round(new[0][nk]["bytes_per_column"] / parent[0][pk]["bytes_per_column"], 4),
                     "same_commit_unfused_ms": round(med(new, pk), 4)}
        res[name]["not_slower_than_parent_by_more_than_its_spread"] = bool(
            med(new, nk) <= med(parent, pk) * (1.0 + spread(parent, pk)))
    for k in ("backward_fused_over_unfused", "jvp_fused_over_unfused"):
        res[k] = round(statistics.median(r[k] for r in new), 4)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.startswith("runs_")}))


if len(sys.argv) > 1 and sys.argv[1] == "summarise":
    summarise(*sys.argv[2:5])
    sys.exit(0)

import torch  # noqa: E402

from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag  # noqa: E402
from dwarf_p_cloudsc2_tl_ad_amd import binding as B  # noqa: E402

args = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]
ngptot = int(args[0]) if len(args) > 0 else 160000
reps = int(args[1]) if len(args) > 1 else 30
nproma, nlev = 128, 137
RB = B.REAL_BYTES

case = th.setup(ngptot, nproma, nlev, prepare=False, fp64=False)
prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
x15 = {n: x[n] for n in ag.SAT_NAMES}
dtype = B.torch_real()
assert all(t.data_ptr() == ag.normalize(x15, lay, ag.SAT_GROUPS)[n].data_ptr() for n, t in x15.items()), "inputs would be copied"
g = torch.Generator(device=dev).manual_seed(0)
u = {n: torch.randn(lay.shape(n), generator=g, dtype=dtype, device=dev) for n in B.OUT_NAMES}
v = {n: 0.01 * t for n, t in x.items()}
v15 = {n: v[n] for n in ag.SAT_NAMES}
st = lambda: th.stream(dev)  # noqa: E731
new = lambda names: th.new(names, lay, dev)  # noqa: E731
timed = lambda step: th.median_ms(step, reps)  # noqa: E731

# the kernels alone, on preallocated buffers
traj = new(B.OUT_NAMES)
B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), ptsphy, nproma, nlev, ngptot, C.byref(ag._block("in", x, lay)),
                                         C.byref(ag._block("out", traj, lay)), None, st()))
head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
xa, xa15, dy = new(B.IN_NAMES), new(ag.SAT_NAMES), new(B.OUT_NAMES)
vjp_kernel_ms = timed(lambda: B.check(B.lib.cloudsc2_vjp_launch(*head, C.byref(ag._block("in", x, lay)), C.byref(ag._block("out", traj, lay)),
                                                                C.byref(ag._block("in", xa, lay)), C.byref(ag._block("out", u, lay)), None, st())))
vjp_satur_ms = timed(lambda: B.check(B.lib.cloudsc2_vjp_launch_satur(*head, C.byref(ag._block("in", x15, lay)), C.byref(ag._block("out", traj, lay)),
                                                                     C.byref(ag._block("in", xa15, lay)), C.byref(ag._block("out", u, lay)), None,
                                                                     st())))
tl_kernel_ms = timed(lambda: B.check(B.lib.cloudsc2_tl_launch(*head, C.byref(ag._block("in", x, lay)), C.byref(B.Outputs()),
                                                              C.byref(ag._block("in", v, lay)), C.byref(ag._block("out", dy, lay)), st())))
tl_satur_ms = timed(lambda: B.check(B.lib.cloudsc2_tl_launch_satur(*head, C.byref(ag._block("in", x15, lay)), C.byref(ag._block("in", v15, lay)),
                                                                   C.byref(ag._block("out", dy, lay)), st())))
# the existing sweep with SATUR fused for the trajectory only (traj_in->qsat NULL, the qsat tangent a plane): what SATUR's own
# arithmetic costs a sweep at one wave per SIMD, apart from the partials
tl_fusedtraj_ms = timed(lambda: B.check(B.lib.cloudsc2_tl_launch(*head, C.byref(ag._block("in", x15, lay)), C.byref(B.Outputs()),
                                                                 C.byref(ag._block("in", v, lay)), C.byref(ag._block("out", dy, lay)), st())))
q, dqp, dqt = new(("qsat",))["qsat"], new(("pap",))["pap"], new(("pap",))["pap"]
f = lambda t: ag._field(t, lay, "pap")  # noqa: E731
satur_ms = timed(lambda: B.check(B.lib.cloudsc2_satur_launch(C.byref(prm), nproma, nlev, ngptot, f(x["pap"]), f(x["t"]), f(q), st())))
satur_lin_ms = timed(lambda: B.check(B.lib.cloudsc2_satur_lin_launch(C.byref(prm), nproma, nlev, ngptot, f(x["pap"]), f(x["t"]), f(q), f(dqp),
                                                                     f(dqt), st())))

# the whole gradient through torch: the fused op against what a user would otherwise write
keys = list(ag.SAT_NAMES)
us = [u[n] for n in B.OUT_NAMES]


def fused(*a):
    return tuple(ag.cloudsc2(dict(zip(keys, a)), prm, ptsphy, ngptot, satur=True))


def unfused(*a):
    xx = dict(zip(keys, a))
    xx["qsat"] = ag.satur(xx["pap"], xx["t"], prm, ngptot, differentiable=True)
    return tuple(ag.cloudsc2(xx, prm, ptsphy, ngptot))


res = {}
xc = {n: t.clone() for n, t in x15.items()}  # (forward-mode AD gives the BASE of a view a tangent too: separate arrays, as in autograd_timing.py)
for name, fn in (("fused", fused), ("unfused", unfused)):
    xs = [x15[n].detach().requires_grad_() for n in keys]
    res["forward_" + name] = timed(lambda: fn(*xs))
    outs = list(fn(*xs))
    res["backward_" + name] = timed(lambda: torch.autograd.grad(outs, xs, us, retain_graph=True))
    res["jvp_" + name] = timed(lambda: torch.func.jvp(fn, tuple(xc[n] for n in keys), tuple(v15[n] for n in keys)))
    del outs

# bytes per column: reals loaded + stored by each sweep as written (no evaporation branch: no cover checkpoints)
R, H = nlev, nlev + 1             # one full-level / half-level plane
traj_in = 15 * R + H              # 15 full-level inputs and PAPHP1
outs10 = 6 * R + 4 * H            # 4 tendencies, PCLC, PCOVPTOT, 4 fluxes
rev_in = traj_in + 2 * R + 6 * R + 4 * R  # + PFPLSL5 / PFPLSN5 and the 10 output adjoints (the fluxes' top level not read)
tl_b = RB * (2 * traj_in + outs10)
vjp_b = RB * (rev_in + traj_in)
tl_s_b = tl_b - RB * 2 * R        # no qsat trajectory plane, no qsat tangent plane
vjp_s_b = vjp_b - RB * 2 * R      # no qsat trajectory plane, no qsat adjoint plane
sat_b, sat_lin_b = RB * 3 * R, RB * 5 * R

row = lambda ms, b: th.row(ms, b, ngptot)  # noqa: E731

print(json.dumps({
    "ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp32" if B.SINGLE else "fp64", "reps": reps,
    "device": torch.cuda.get_device_name(dev),
    "tl_kernel_no_traj": row(tl_kernel_ms, tl_b), "tl_kernel_satur": row(tl_satur_ms, tl_s_b),
    "tl_kernel_satur_trajectory_only": row(tl_fusedtraj_ms, tl_b - RB * R),
    "vjp_kernel": row(vjp_kernel_ms, vjp_b), "vjp_kernel_satur": row(vjp_satur_ms, vjp_s_b),
    "satur_kernel": row(satur_ms, sat_b), "satur_lin_kernel": row(satur_lin_ms, sat_lin_b),
    "tl_satur_over_tl": round(tl_satur_ms / tl_kernel_ms, 4), "vjp_satur_over_vjp": round(vjp_satur_ms / vjp_kernel_ms, 4),
    **{k + "_ms": round(ms, 4) for k, ms in res.items()},
    "backward_fused_over_unfused": round(res["backward_fused"] / res["backward_unfused"], 4),
    "jvp_fused_over_unfused": round(res["jvp_fused"] / res["jvp_unfused"], 4),
}))
