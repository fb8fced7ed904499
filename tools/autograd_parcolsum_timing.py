#!/usr/bin/env python3
"""The parameter column-sum sweep (cloudsc2_parjac_launch_colsum, cloudsc2_parnormal_launch_colsum; param_jacobian_column_sums,
param_normal_equations_column_sums) against the route it replaces, at 160 000 columns, NPROMA 128, fp64, the evaporation branch (four
directions), the two surface sums observed and weighted: medians of REPS event-timed calls after warm-up.

    python tools/autograd_parcolsum_timing.py run new|route [NGPTOT [REPS]]
        one process, ONE JSON object.
        route: the parent commit's route, which needs nothing of this sweep -- param_jacobian (61 512 B per column written), every
               plane folded over the levels in torch (one einsum per parameter and sum), the folded sums contracted in torch in float64;
               and cloudsc2_tl_launch_parjac alone.
        new:   param_normal_equations_column_sums and param_jacobian_column_sums through torch, the two launchers alone, and
               cloudsc2_tl_launch_parjac alone in the same process (the same arithmetic with every sensitivity stored).
    python tools/autograd_parcolsum_timing.py alternate [NGPTOT [REPS]]
        fresh processes of `run route` and `run new` alternating, three pairs per order; every process's JSON goes to
        profiles/autograd_parcolsum_timing.json, the route's own spread over its processes is printed first."""
import ctypes as C
import json
import os
import statistics
import sys

import timing_harness as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternate(rest):
    runs = th.children({which: ([sys.executable, os.path.abspath(__file__), "run", which, *rest], ROOT) for which in ("route", "new")})
    if isinstance(runs, int):
        return runs
    med = lambda which, k: statistics.median(p["result"]["rows"][k]["ms"] for p in runs if p["which"] == which)  # noqa: E731
    y = [p["result"]["rows"] for p in runs if p["which"] == "route"]
    spread = {k: th.spread(y, (k, "ms")) for k in y[0]}
    print("route spread over its processes:", json.dumps(spread))
    summary = {"route_normal_equations_ms": med("route", "normal_equations_route"), "route_sums_ms": med("route", "sums_route"),
               "route_parjac_kernel_ms": med("route", "parjac_kernel"), "new_normal_equations_ms": med("new", "normal_equations"),
               "new_sums_ms": med("new", "sums"), "new_normal_launcher_ms": med("new", "normal_launcher"),
               "new_sums_launcher_ms": med("new", "sums_launcher"), "new_parjac_kernel_ms": med("new", "parjac_kernel")}
    print(json.dumps(summary))
    with open(os.path.join(ROOT, "profiles", "autograd_parcolsum_timing.json"), "w") as f:
        json.dump({"route_spread": spread, "medians_over_processes": summary, "processes": runs}, f)
    return 0


def run(which, rest):
    import torch

    import dwarf_p_cloudsc2_tl_ad_amd as c2
    from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    ngptot = int(rest[0]) if len(rest) > 0 else 160000
    reps = int(rest[1]) if len(rest) > 1 else 30
    nproma, nlev = 128, 137
    case = th.setup(ngptot, nproma, nlev, levapls2=True)
    prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
    st = lambda: th.stream(dev)  # noqa: E731
    timed = lambda step: th.median_ms(step, reps, ndigits=4)  # noqa: E731

    surface = torch.zeros(nlev + 1, dtype=torch.float64, device=dev)
    surface[-1] = 1
    wsurf = {"fplsl": surface, "fplsn": surface.clone()}
    g = torch.Generator(device=dev).manual_seed(0)
    r = {n: torch.randn((lay.nblocks, nproma), generator=g, dtype=torch.float64, device=dev) for n in wsurf}
    w = {n: torch.rand((lay.nblocks, nproma), generator=g, dtype=torch.float64, device=dev) + 0.5 for n in wsurf}
    head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
    xb = C.byref(ag._block("in", x, lay))
    P = c2.PARAM_NAMES
    rows = {}

    sens = [{n: torch.empty(lay.shape(n), dtype=torch.float64, device=dev) for n in B.OUT_NAMES} for _ in P]
    blocks = (B.Outputs * len(P))(*(ag._block("out", s, lay) for s in sens))
    rows["parjac_kernel"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_tl_launch_parjac(*head, xb, blocks, st()))), "bytes_per_column": 17544 + 4 * 10992}
    del sens, blocks

    if which == "route":
        def sums_route():
            J = c2.param_jacobian(x, prm, ptsphy, ngptot)
            return {p: {n: torch.einsum("k,bkc->bc", wsurf[n], getattr(J[p], n)) for n in wsurf} for p in P}

        def normal_route():
            s = sums_route()
            S = torch.stack([torch.stack([s[p][n].reshape(-1)[:ngptot] for n in wsurf]).reshape(-1) for p in P])  # (4, 2 * ngptot)
            W = torch.stack([w[n].reshape(-1)[:ngptot] for n in wsurf]).reshape(-1)
            R = torch.stack([r[n].reshape(-1)[:ngptot] for n in wsurf]).reshape(-1)
            SW = S * W
            return SW @ S.T, SW @ R
        rows["sums_route"] = {"ms": timed(sums_route), "bytes_per_column": 17544 + 4 * 10992 + 8 * 8 * (nlev + 1) + 8 * 8}
        rows["normal_equations_route"] = {"ms": timed(normal_route)}
    else:
        table = torch.zeros((10, nlev + 1), dtype=torch.float64, device=dev)
        for n, a in wsurf.items():
            table[B.OUT_NAMES.index(n), :len(a)] = a
        sums = [{n: torch.zeros((lay.nblocks, nproma), dtype=torch.float64, device=dev) for n in wsurf} for _ in P]
        sblocks = (B.Outputs * len(P))(*(ag._sums_block(s, lay) for s in sums))
        tp = C.c_void_p(table.data_ptr())
        rows["sums_launcher"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_parjac_launch_colsum(*head, xb, tp, sblocks, st()))),
                                 "bytes_per_column": 17544 + 8 * 8}
        work = torch.empty(B.NNORMAL * lay.nblocks * nproma, dtype=torch.float64, device=dev)
        normal = torch.empty(B.NNORMAL, dtype=torch.float64, device=dev)
        rb, wb = C.byref(ag._sums_block(r, lay)), C.byref(ag._sums_block(w, lay))
        rows["normal_launcher"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_parnormal_launch_colsum(
            *head, xb, tp, rb, wb, C.c_void_p(work.data_ptr()), C.c_void_p(normal.data_ptr()), st()))),
            "bytes_per_column": 17544 + 4 * 8 + 2 * 14 * 8}
        rows["sums"] = {"ms": timed(lambda: c2.param_jacobian_column_sums(x, prm, ptsphy, ngptot, level_weights=wsurf))}
        rows["normal_equations"] = {"ms": timed(lambda: c2.param_normal_equations_column_sums(x, prm, ptsphy, ngptot, level_weights=wsurf,
                                                                                             residual=r, weights=w))}
        for k in ("sums_launcher", "normal_launcher"):
            rows[k]["over_parjac_kernel"] = round(rows[k]["ms"] / rows["parjac_kernel"]["ms"], 3)
    print(json.dumps({"which": which, "ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp64", "reps": reps,
                      "evaporation": True, "device": torch.cuda.get_device_name(dev), "rows": rows}))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "alternate":
        sys.exit(alternate(sys.argv[2:]))
    sys.exit(run(sys.argv[2], sys.argv[3:]))
