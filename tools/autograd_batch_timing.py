#!/usr/bin/env python3
"""Batched tangents / cotangents at 160 000 columns, NPROMA 128, fp64: one cloudsc2_tl_launch_batch / cloudsc2_vjp_launch_batch call
with K directions against the yardstick, K back-to-back cloudsc2_tl_launch (no trajectory stores) / cloudsc2_vjp_launch calls on the
same state and the same direction arrays in the same process, for K = kBatchMax and 2 * kBatchMax; and through torch, vmap(jvp) with
K directions against the Python loop of K jvp calls.  HIP events on the launch stream, medians over REPS after warm-up.

    python tools/autograd_batch_timing.py run loop|batch [NGPTOT [REPS]]     one fresh process; `loop|batch`: which of the two is
                                                                             measured first (the second of a pair reads slower)
    python tools/autograd_batch_timing.py summarise RUN.json...              the runs of both orders -> ONE JSON object: per pair
                                                                             the ratio batch / loop, the yardstick's own spread
                                                                             over the processes, and the byte ratio
CLOUDSC2_PACE=0 in the environment of a `run` gives the unpaced leg of the pacing A/B."""
import ctypes as C
import json
import os
import statistics
import sys

import timing_harness as th

NLEV = 137
R, H = NLEV, NLEV + 1
TRAJ_IN = 8 * (15 * R + H)                    # bytes per column: 15 full-level inputs and PAPHP1
OUTS10 = 8 * (6 * R + 4 * H)                  # 4 tendencies, PCLC, PCOVPTOT, 4 fluxes
TL_ONE = 2 * TRAJ_IN + OUTS10                 # trajectory in + tangent in + tangent out
VJP_REST = 8 * (2 * R)                        # PFPLSL5 / PFPLSN5
VJP_DIR = 8 * (6 * R + 4 * R) + TRAJ_IN       # 10 output adjoints in (the fluxes' top level not read) + 16 input adjoints out
VJP_ONE = TRAJ_IN + VJP_REST + VJP_DIR


def chunks(k, kmax):
    n = -(-k // kmax)
    return [k // n + (1 if c < k % n else 0) for c in range(n)]


def byte_ratio(sweep, k, kmax):
    shared, per_dir, one = (TRAJ_IN, TL_ONE - TRAJ_IN, TL_ONE) if sweep == "tl" else (TRAJ_IN + VJP_REST, VJP_DIR, VJP_ONE)
    return sum(shared + per_dir * c for c in chunks(k, kmax)) / (k * one)


def run(first, ngptot, reps):
    import torch

    from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    nproma, nlev = 128, NLEV
    kmax = B.lib.cloudsc2_batch_max()
    case = th.setup(ngptot, nproma, nlev, prepare=False)
    prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
    st = lambda: th.stream(dev)  # noqa: E731
    new = lambda names: th.new(names, lay, dev)  # noqa: E731
    timed = lambda step: th.median_ms(step, reps)  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(0)
    K2 = 2 * kmax
    vs = [{n: t * (0.01 * (j + 1)) for n, t in x.items()} for j in range(K2)]
    us = [{n: torch.randn(lay.shape(n), generator=gen, dtype=torch.float64, device=dev) for n in B.OUT_NAMES} for _ in range(K2)]
    dys, xas = [new(B.OUT_NAMES) for _ in range(K2)], [new(B.IN_NAMES) for _ in range(K2)]
    traj = new(B.OUT_NAMES)
    xb = ag._block("in", x, lay)
    B.check(B.lib.cloudsc2_ad_launch_forward(C.byref(prm), ptsphy, nproma, nlev, ngptot, C.byref(xb), C.byref(ag._block("out", traj, lay)),
                                             None, st()))
    tb = ag._block("out", {"fplsl": traj["fplsl"], "fplsn": traj["fplsn"]}, lay)
    vb, ub = [ag._block("in", v, lay) for v in vs], [ag._block("out", u, lay) for u in us]
    dyb, xab = [ag._block("out", d, lay) for d in dys], [ag._block("in", a, lay) for a in xas]
    none = B.Outputs()
    head = (C.byref(prm), ptsphy, nproma, nlev, ngptot, C.byref(xb))

    def legs(k):
        vin, dout = (B.Inputs * k)(*vb[:k]), (B.Outputs * k)(*dyb[:k])
        ain, uout = (B.Inputs * k)(*xab[:k]), (B.Outputs * k)(*ub[:k])

        def tl_loop():
            for j in range(k):
                B.check(B.lib.cloudsc2_tl_launch(*head, C.byref(none), C.byref(vb[j]), C.byref(dyb[j]), st()))

        def vjp_loop():
            for j in range(k):
                B.check(B.lib.cloudsc2_vjp_launch(*head, C.byref(tb), C.byref(xab[j]), C.byref(ub[j]), None, st()))

        return {"tl": {"loop": tl_loop, "batch": lambda: B.check(B.lib.cloudsc2_tl_launch_batch(*head, k, vin, dout, st()))},
                "vjp": {"loop": vjp_loop, "batch": lambda: B.check(B.lib.cloudsc2_vjp_launch_batch(*head, C.byref(tb), k, ain, uout, None, st()))}}

    order = [first, "batch" if first == "loop" else "loop"]
    out = {"first": first, "ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp64", "reps": reps, "batch_max": kmax,
           "pace": os.environ.get("CLOUDSC2_PACE", "default"), "device": torch.cuda.get_device_name(dev), "kernels": {}, "torch": {}}
    for k in (kmax, K2):
        for sweep, two in legs(k).items():
            ms = {which: timed(two[which]) for which in order}
            out["kernels"][f"{sweep}_K{k}"] = {"loop_ms": round(ms["loop"], 4), "batch_ms": round(ms["batch"], 4),
                                               "ratio": round(ms["batch"] / ms["loop"], 4)}
    # through torch: vmap(jvp) with K directions against the Python loop of K jvp calls (each of them: the forward + one TL sweep;
    # the vmap: ONE forward + the batched TL sweep)
    keys = list(B.IN_NAMES)
    xc = tuple(x[n].clone() for n in keys)
    f = lambda *a: tuple(ag.cloudsc2(dict(zip(keys, a)), prm, ptsphy, ngptot))  # noqa: E731
    for k in (kmax, K2):
        V = tuple(torch.stack([vs[j][n] for j in range(k)]) for n in keys)
        two = {"loop": lambda: [torch.func.jvp(f, xc, tuple(vs[j][n] for n in keys))[1] for j in range(k)],
               "batch": lambda: torch.func.vmap(lambda *v: torch.func.jvp(f, xc, v)[1])(*V)}
        ms = {which: timed(two[which]) for which in order}
        out["torch"][f"vmap_jvp_K{k}"] = {"loop_ms": round(ms["loop"], 4), "batch_ms": round(ms["batch"], 4),
                                          "ratio": round(ms["batch"] / ms["loop"], 4)}
        del V
    print(json.dumps(out))


def summarise(files):
    runs = [json.loads(open(f).read().strip().splitlines()[-1]) for f in files]
    kmax = runs[0]["batch_max"]
    out = {k: runs[0][k] for k in ("ngptot", "nproma", "nlev", "precision", "reps", "batch_max", "device")}
    out["processes"] = {"loop_first": sum(r["first"] == "loop" for r in runs), "batch_first": sum(r["first"] == "batch" for r in runs)}
    for group in ("kernels", "torch"):
        out[group] = {}
        for name in runs[0][group]:
            rows = [r[group][name] for r in runs]
            loops = [r["loop_ms"] for r in rows]
            spread = th.spread(rows, ("loop_ms",))
            ratios = [r["ratio"] for r in rows]
            e = {"loop_ms": loops, "batch_ms": [r["batch_ms"] for r in rows], "first": [r["first"] for r in runs], "ratio": ratios,
                 "ratio_median": round(statistics.median(ratios), 4), "yardstick_spread": spread,
                 "beats_the_yardstick_by_more_than_its_spread_in_every_pair": all(1.0 - q > spread for q in ratios)}
            if group == "kernels":
                sweep, k = name.split("_K")
                e["byte_ratio"] = round(byte_ratio(sweep, int(k), kmax), 4)
            out[group][name] = e
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run" and sys.argv[2] in ("loop", "batch"):
        run(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 160000, int(sys.argv[4]) if len(sys.argv) > 4 else 30)
    elif len(sys.argv) >= 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2:])
    else:
        sys.exit(__doc__)
