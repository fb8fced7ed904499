#!/usr/bin/env python3
"""What per-column parameter maps cost, fp64, NPROMA 128, 160 000 columns by default, no evaporation branch.
Same process: each new launcher against its scalar parent on the same state, in rotating order, timed between two events --
``cloudsc2_nl_launch_parmap`` / ``cloudsc2_ad_launch_forward``, ``cloudsc2_tl_launch_parmap`` / ``cloudsc2_tl_launch_par``,
``cloudsc2_vjp_launch_parmap`` / ``cloudsc2_vjp_launch_par`` (the parent's time includes its fold kernel).
Through torch, one route per PROCESS: a two-valued (land / sea) ``rclcrit`` map through ``c2.cloudsc2_param_maps``, forward and forward +
backward to ``t``, ``q`` and the map, against the only route without the op: two ``c2.cloudsc2(params={"rclcrit": 0-d})`` calls joined by
``torch.where`` over the ten planes, backward to ``t``, ``q`` and the two values; wall clock between two device synchronisations,
because that route's host reads are part of its cost.
    python tools/autograd_parmap_timing.py run ROUTE [NGPTOT [REPS]]      ROUTE: launchers | maps | where; ONE JSON object
    python tools/autograd_parmap_timing.py alternate [NGPTOT [ROUNDS [REPS]]]  fresh processes of the three routes in alternation, each
        under its own time limit, none started after one that failed; ONE JSON object: per route and step the median of the processes'
        medians and their spread (min, max)
It writes nothing but that line."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

import timing_harness as th

STEPS = ("forward", "forward_backward_t_q_map")
PAIRS = ("nl_parmap", "ad_forward", "tl_parmap", "tl_par", "vjp_parmap", "vjp_par")


def summary(ms):
    return {k: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)} for k, t in ms.items()}


def launchers(case, reps):
    import torch

    from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
    L, p, geo, st = B.lib, C.byref(prm), (lay.nproma, lay.nlev, lay.ngptot), (lambda: th.stream(dev))
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    like = x["pap"]
    out, dy, xa = ag._new(B.OUT_NAMES, lay, like), ag._new(B.OUT_NAMES, lay, like), ag._new(B.IN_NAMES, lay, like)
    dx = {n: (0.01 * t).contiguous() for n, t in x.items()}
    gen = torch.Generator(device=dev).manual_seed(1)
    y = {n: torch.randn(lay.shape(n), generator=gen, dtype=like.dtype, device=dev) for n in B.OUT_NAMES}
    own = [float(getattr(prm, n)) for n in B.PARAM_NAMES]
    ptab = torch.tensor(own, dtype=torch.float64, device=dev)[:, None, None].expand(4, lay.nblocks, lay.nproma).contiguous()
    dptab, apar = (0.01 * ptab).contiguous(), torch.empty_like(ptab)
    dpar = (C.c_double * 4)(*[0.01 * v for v in own])
    nwork = C.c_longlong()
    B.check(L.cloudsc2_par_work_doubles(lay.nproma, lay.ngptot, C.byref(nwork)))
    work, par_adj = torch.empty(nwork.value, dtype=torch.float64, device=dev), torch.empty(4, dtype=torch.float64, device=dev)
    xb, ob, dxb, dyb = ag._block("in", x, lay), ag._block("out", out, lay), ag._block("in", dx, lay), ag._block("out", dy, lay)
    ab, yb, tb = ag._block("in", xa, lay), ag._block("out", y, lay), ag._traj_out(out["fplsl"], out["fplsn"], lay)
    r = C.byref
    forms = {
        "nl_parmap": lambda: B.check(L.cloudsc2_nl_launch_parmap(p, ptsphy, *geo, ptr(ptab), r(xb), r(ob), None, st())),
        "ad_forward": lambda: B.check(L.cloudsc2_ad_launch_forward(p, ptsphy, *geo, r(xb), r(ob), None, st())),
        "tl_parmap": lambda: B.check(L.cloudsc2_tl_launch_parmap(p, ptsphy, *geo, 0, ptr(ptab), ptr(dptab), r(xb), r(dxb), r(dyb), st())),
        "tl_par": lambda: B.check(L.cloudsc2_tl_launch_par(p, ptsphy, *geo, 0, r(xb), r(dxb), dpar, r(dyb), st())),
        "vjp_parmap": lambda: B.check(L.cloudsc2_vjp_launch_parmap(p, ptsphy, *geo, 0, ptr(ptab), r(xb), r(tb), r(ab), r(yb), None, ptr(apar), st())),
        "vjp_par": lambda: B.check(L.cloudsc2_vjp_launch_par(p, ptsphy, *geo, 0, r(xb), r(tb), r(ab), r(yb), None, ptr(work), ptr(par_adj), st())),
    }
    assert tuple(forms) == PAIRS
    for _ in range(3):
        for step in forms.values():
            step()
    torch.cuda.synchronize()
    res = summary(th.rotated(forms, reps, th.event_ms, len(forms)))
    res["bytes_per_column_of_the_tables"] = {"nl": 32, "tl": 64, "vjp": 64}
    res["clock"] = "events on the stream"
    return res


def through_torch(case, route, reps):
    import torch

    import dwarf_p_cloudsc2_tl_ad_amd as c2
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    prm, x, lay, ptsphy, dev, ngptot = case.prm, case.x, case.lay, case.ptsphy, case.dev, case.lay.ngptot
    land = (torch.arange(lay.nblocks * lay.nproma, device=dev).reshape(lay.nblocks, lay.nproma) * 7919 % 10) < 3  # 30 % land
    values = (float(prm.rclcrit), 0.6 * float(prm.rclcrit))  # sea, land
    xg = dict(x, t=x["t"].detach().clone().requires_grad_(), q=x["q"].detach().clone().requires_grad_())
    gen = torch.Generator(device=dev).manual_seed(1)
    u = [torch.randn(lay.shape(n), generator=gen, dtype=B.torch_real(), device=dev) for n in B.OUT_NAMES]
    if route == "maps":
        sea, lnd = (torch.tensor(v, dtype=torch.float64, device=dev) for v in values)
        rc = torch.where(land, lnd, sea).requires_grad_()
        leaves = [rc]

        def outputs(xs, grad):
            return list(c2.cloudsc2_param_maps(xs, prm, ptsphy, ngptot, params={"rclcrit": rc if grad else rc.detach()}))
    else:
        sea, lnd = (torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for v in values)
        leaves, mask = [sea, lnd], land[:, None, :]

        def outputs(xs, grad):
            a = c2.cloudsc2(xs, prm, ptsphy, ngptot, params={"rclcrit": sea if grad else sea.detach()})
            b = c2.cloudsc2(xs, prm, ptsphy, ngptot, params={"rclcrit": lnd if grad else lnd.detach()})
            return [torch.where(mask, tb, ta) for ta, tb in zip(a, b)]

    def forward():
        with torch.no_grad():
            return outputs(x, False)

    def backward():
        return torch.autograd.grad(outputs(xg, True), leaves + [xg["t"], xg["q"]], u)

    forms = dict(zip(STEPS, (forward, backward)))
    for _ in range(2):
        for step in forms.values():
            step()
    torch.cuda.synchronize()
    res = summary(th.rotated(forms, reps, th.wall_ms, 2))
    res["checksum_fplsl"] = int(forward()[B.OUT_NAMES.index("fplsl")].view(torch.int64).sum().item())
    res["clock"] = "wall, between device synchronisations"
    return res


def run(route, ngptot, reps):
    import torch

    case = th.setup(ngptot, 128, 137, prepare=True, fp64=True)
    res = launchers(case, reps) if route == "launchers" else through_torch(case, route, reps)
    res.update(route=route, ngptot=ngptot, nproma=128, nlev=137, precision="fp64", reps=reps, device=torch.cuda.get_device_name(case.dev))
    return res


def child(argv, limit=300):
    """one fresh process under its own time limit -> (its JSON object or None, what it printed)"""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "run"] + [str(a) for a in argv], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        return None, f"time limit: {e}"
    if r.returncode != 0:
        return None, f"return code {r.returncode}\n{r.stdout[-2000:]}{r.stderr[-2000:]}"
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stdout


def spread(runs, step):
    med = [r[step]["median_ms"] for r in runs]
    return {"median_ms": round(statistics.median(med), 4), "min_ms": min(med), "max_ms": max(med), "processes": len(med)}


def alternate(ngptot, rounds, reps):
    runs = {"where": [], "maps": [], "launchers": []}
    for _ in range(rounds):
        for route in runs:
            res, text = child([route, ngptot, reps])
            if res is None:  # nothing more is started
                return {"failed": route, "output": text}
            runs[route].append(res)
    out = {"ngptot": ngptot, "rounds": rounds, "reps": reps, "device": runs["maps"][0]["device"], "precision": "fp64",
           "protocol": "fresh processes of the routes in alternation; per step the median of the processes' medians, min and max of them",
           "the_two_routes_give_the_same_fplsl": len({r["checksum_fplsl"] for r in runs["maps"] + runs["where"]}) == 1}
    for route in ("maps", "where"):
        out[route] = {s: spread(runs[route], s) for s in STEPS}
    out["launchers"] = {k: spread(runs["launchers"], k) for k in PAIRS}
    out["ratio_maps_over_where"] = {s: round(out["maps"][s]["median_ms"] / out["where"][s]["median_ms"], 4) for s in STEPS}
    out["spread_of_where_over_its_processes"] = {s: round((out["where"][s]["max_ms"] - out["where"][s]["min_ms"]) / out["where"][s]["median_ms"], 4)
                                                 for s in STEPS}
    out["ratio_launcher_over_parent"] = {a: round(out["launchers"][a]["median_ms"] / out["launchers"][b]["median_ms"], 4)
                                         for a, b in zip(PAIRS[::2], PAIRS[1::2])}
    return out


if __name__ == "__main__":
    mode, args = (sys.argv[1], sys.argv[2:]) if len(sys.argv) > 1 else ("alternate", [])
    num = lambda i, d: int(args[i]) if len(args) > i else d  # noqa: E731
    if mode == "run":
        print(json.dumps(run(args[0], num(1, 160000), num(2, 10))))
    elif mode == "alternate":
        print(json.dumps(alternate(num(0, 160000), num(1, 3), num(2, 10))))
    else:
        sys.exit(__doc__)
