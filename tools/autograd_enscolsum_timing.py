#!/usr/bin/env python3
"""What the column sums of a perturbed-parameter ensemble cost: ``c2.cloudsc2_ensemble_column_sums`` with K members over ONE shared state
against the route it replaces, ``c2.cloudsc2_ensemble`` followed by the fold in torch as one ``einsum`` per sum; the two surface sums
(fplsl and fplsn at the lowest half level), fp64, NPROMA 128.  One route per PROCESS: the state placed by the library's allocator (as
bench.py does), warmed, then three steps in rotating order -- the forward alone (no gradient tracked), the forward with the backward to
the parameters only, and the forward with the backward to ``t``, ``q`` and the parameters -- each timed as wall clock between two device
synchronisations, and once more for its peak memory in full-level planes (NGPTOT x NLEV reals).
    python tools/autograd_enscolsum_timing.py run ROUTE [NGPTOT [K [REPS [evap]]]]    ROUTE: sums | dense; ONE JSON object
    python tools/autograd_enscolsum_timing.py alternate [NGPTOT [K [ROUNDS [REPS]]]]  fresh processes of the two routes in alternation,
        each under its own time limit, none started after one that failed; ONE JSON object: per route and step the median of the
        processes' medians and their spread (min, max), the peak memory, and the largest K that fits each route, computed from the
        measured peaks and the device's free memory (not tried)
    python tools/autograd_enscolsum_timing.py order LIB [NGPTOT [ROUNDS [REPS]]]      the forward of the sums route at K = 8 and 32 with
        the library of the tree and with LIB (CLOUDSC2_LIB: an experiment build with another workgroup order) in alternation
It writes nothing but that line."""
import json
import os
import statistics
import subprocess
import sys

import timing_harness as th

STEPS = ("forward", "forward_backward_params", "forward_backward_t_q_params")


def run(route, ngptot, K, reps, evap):
    import torch

    import dwarf_p_cloudsc2_tl_ad_amd as c2
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    nproma, nlev = 128, 137
    case = th.setup(ngptot, nproma, nlev, prepare=False, fp64=False, levapls2=evap)
    prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
    dtype = B.torch_real()
    plane = lay.nblocks * lay.nlev * lay.nproma * torch.empty((), dtype=dtype).element_size()

    factors = torch.linspace(0.8, 1.2, K, dtype=torch.float64, device=dev)
    members = {n: (getattr(prm, n) * factors).requires_grad_() for n in c2.PARAM_NAMES}
    frozen = {n: p.detach() for n, p in members.items()}
    xg = dict(x, t=x["t"].detach().clone().requires_grad_(), q=x["q"].detach().clone().requires_grad_())
    surface = torch.zeros(lay.nlev + 1, dtype=dtype, device=dev)
    surface[-1] = 1
    weights = {"fplsl": surface, "fplsn": surface.clone()}
    gen = torch.Generator(device=dev).manual_seed(1)
    u = [torch.randn((K, lay.nblocks, lay.nproma), generator=gen, dtype=dtype, device=dev) for _ in weights]

    if route == "sums":
        def sums(xs, ps):
            ys = c2.cloudsc2_ensemble_column_sums(xs, prm, ptsphy, ngptot, weights=weights, params=ps)
            return [ys.fplsl, ys.fplsn]
    else:
        def sums(xs, ps):
            out = c2.cloudsc2_ensemble(xs, prm, ptsphy, ngptot, params=ps)
            return [torch.einsum("k,mbkc->mbc", weights[n], getattr(out, n)) for n in weights]

    def forward():
        with torch.no_grad():
            return sums(x, frozen)

    def backward_params():
        return torch.autograd.grad(sums(x, members), list(members.values()), u)

    def backward_all():
        return torch.autograd.grad(sums(xg, members), list(members.values()) + [xg["t"], xg["q"]], u)

    forms = dict(zip(STEPS, (forward, backward_params, backward_all)))
    for _ in range(2):
        for step in forms.values():
            step()
    torch.cuda.synchronize()

    def peak(step):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        r = step()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated(dev) - before
        del r
        return rise / plane

    ms = th.rotated(forms, reps, th.wall_ms, 3)
    y = forward()
    gp = backward_params()
    torch.cuda.synchronize()
    sums_check, grads_check = [int(t.view(torch.int64).sum().item()) for t in y], [int(t.view(torch.int64).sum().item()) for t in gp]
    del y, gp
    torch.cuda.empty_cache()  # (what torch's allocator has cached is free memory to the question "what fits")
    free, total = torch.cuda.mem_get_info(dev)
    res = {"route": route, "library": os.environ.get("CLOUDSC2_LIB", "tree"), "ngptot": ngptot, "members": K, "nproma": nproma, "nlev": nlev,
           "precision": "fp32" if B.SINGLE else "fp64", "reps": reps, "evap": evap, "device": torch.cuda.get_device_name(dev),
           "clock": "wall, between device synchronisations", "plane_bytes": plane, "free_bytes_with_the_state_resident": int(free),
           "checksum_sums": sums_check, "checksum_parameter_gradients": grads_check}
    for k, t in ms.items():
        res[k] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                  "peak_planes": round(peak(forms[k]), 3)}
    return res


def child(argv, env=None, limit=300):
    """one fresh process under its own time limit -> (its JSON object or None, what it printed)"""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "run"] + [str(a) for a in argv], env={**os.environ, **(env or {})},
                           capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        return None, f"time limit: {e}"
    if r.returncode != 0:
        return None, f"return code {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stdout


def spread(runs, step):
    med = [r[step]["median_ms"] for r in runs]
    return {"median_ms": round(statistics.median(med), 4), "min_ms": min(med), "max_ms": max(med), "processes": len(med),
            "peak_planes": max(r[step]["peak_planes"] for r in runs)}


def alternate(ngptot, K, rounds, reps):
    runs = {"sums": [], "dense": []}
    for _ in range(rounds):
        for route in ("dense", "sums"):
            res, text = child([route, ngptot, K, reps])
            if res is None:  # nothing more is started
                return {"failed": route, "output": text}
            runs[route].append(res)
    out = {"ngptot": ngptot, "members": K, "rounds": rounds, "reps": reps, "device": runs["sums"][0]["device"], "precision": runs["sums"][0]["precision"],
           "protocol": "fresh processes of the two routes in alternation; per step the median of the processes' medians, min and max of them",
           "sums_equal_in_every_process": len({tuple(r["checksum_sums"]) for r in runs["sums"]}) == 1}
    for route, rs in runs.items():
        out[route] = {s: spread(rs, s) for s in STEPS}
        # peak = fixed + K x per member: the route's peaks are whole multiples of K up to its small arrays
        r0 = rs[0]
        per_member = max(r0[s]["peak_planes"] for s in STEPS) * r0["plane_bytes"] / K
        budget = r0["free_bytes_with_the_state_resident"]
        out[route]["largest_K_that_fits"] = {s: int(budget // max(r0[s]["peak_planes"] * r0["plane_bytes"] / K, 1.0)) for s in STEPS}
        out[route]["bytes_per_member_at_the_largest_peak"] = int(per_member)
    out["ratio_sums_over_dense"] = {s: round(out["sums"][s]["median_ms"] / out["dense"][s]["median_ms"], 4) for s in STEPS}
    return out


def order(lib, ngptot, rounds, reps):
    out = {"ngptot": ngptot, "rounds": rounds, "reps": reps, "experiment_library": os.path.basename(lib),
           "protocol": "fresh processes of the two builds in alternation; the forward of the sums route; median of the processes' medians, min, max"}
    for K in (8, 32):
        runs = {"member_major": [], "member_interleaved": []}
        for _ in range(rounds):
            for name, env in (("member_major", {}), ("member_interleaved", {"CLOUDSC2_LIB": lib})):
                res, text = child(["sums", ngptot, K, reps], env)
                if res is None:
                    out["failed"] = {"build": name, "members": K, "output": text}
                    return out
                runs[name].append(res)
        out[f"K{K}"] = {name: spread(rs, "forward") for name, rs in runs.items()}
        out[f"K{K}"]["identical_bits"] = len({tuple(r["checksum_sums"]) for rs in runs.values() for r in rs}) == 1
    return out


if __name__ == "__main__":
    mode, args = (sys.argv[1], sys.argv[2:]) if len(sys.argv) > 1 else ("alternate", [])
    num = lambda i, d, a=None: int((a if a is not None else args)[i]) if len(a if a is not None else args) > i else d  # noqa: E731
    if mode == "run":
        print(json.dumps(run(args[0], num(1, 160000), num(2, 8), num(3, 10), len(args) > 4 and args[4] == "evap")))
    elif mode == "alternate":
        print(json.dumps(alternate(num(0, 160000), num(1, 8), num(2, 3), num(3, 10))))
    elif mode == "order":
        print(json.dumps(order(os.path.abspath(args[0]), num(1, 160000), num(2, 3), num(3, 10))))
    else:
        sys.exit(__doc__)
