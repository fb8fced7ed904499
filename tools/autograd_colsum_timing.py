#!/usr/bin/env python3
"""The column-sum sweeps (cloudsc2_{nl,tl,vjp}_launch_colsum; cloudsc2_column_sums) against the dense and sparse ones at 160 000 columns,
NPROMA 128, fp64: medians of REPS event-timed calls after warm-up, and peak memory of both routes.

    python tools/autograd_colsum_timing.py run [NGPTOT [REPS [evap]]]
        one process, ONE JSON object:
        (i)   the lean forward kernel (surface sums; all ten sums) and the keep form against cloudsc2_nl_launch / _ad_launch_forward;
        (ii)  the reverse and TL column-sum kernels against their dense and sparse twins (narrow case and everything);
        (iii) through torch, the narrow case (surface rain and snow -> t, q): forward, forward + backward, jvp of cloudsc2_column_sums
              against cloudsc2 + the fold as one einsum per sum, and its backward;
        (iv)  peak memory of both routes across forward + backward, in bytes and in full-level planes.
    python tools/autograd_colsum_timing.py alternate YARDSTICK_TREE [NGPTOT [REPS [evap]]]
        fresh processes of `run` alternating with YARDSTICK_TREE/tools/autograd_timing.py (a built checkout of the parent commit), three
        pairs per order; every process's JSON goes to profiles/autograd_colsum_timing.json, the yardstick's own spread over its
        processes is printed first."""
import ctypes as C
import json
import os
import sys

import timing_harness as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def alternate(tree, rest):
    runs = th.children({"yardstick": ([sys.executable, os.path.join(tree, "tools", "autograd_timing.py"), *rest[:2]], tree),
                        "colsum": ([sys.executable, os.path.abspath(__file__), "run", *rest], ROOT)})
    if isinstance(runs, int):
        return runs
    y = [r["result"] for r in runs if r["which"] == "yardstick"]
    spread = {k: th.spread(y, (k, "ms")) for k in ("forward", "backward", "vjp_kernel", "tl_kernel_no_traj")}
    print("yardstick spread over its processes:", json.dumps(spread))
    with open(os.path.join(ROOT, "profiles", "autograd_colsum_timing.json"), "w") as f:
        json.dump({"yardstick_spread": spread, "processes": runs}, f)
    return 0


def run(rest):
    import torch

    from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
    from dwarf_p_cloudsc2_tl_ad_amd import binding as B

    ngptot = int(rest[0]) if len(rest) > 0 else 160000
    reps = int(rest[1]) if len(rest) > 1 else 30
    evap = len(rest) > 2 and rest[2] == "evap"
    nproma, nlev = 128, 137
    case = th.setup(ngptot, nproma, nlev, levapls2=evap)
    prm, x, lay, ptsphy, dev = case.prm, case.x, case.lay, case.ptsphy, case.dev
    st = lambda: th.stream(dev)  # noqa: E731
    HALF = ("paph", "fplsl", "fplsn", "fhpsl", "fhpsn")
    R, H = 8 * nlev, 8 * (nlev + 1)
    plane_bytes = lambda names: sum(H if n in HALF else R for n in names)  # noqa: E731
    traj_b = plane_bytes(B.IN_NAMES)
    kept_b = 2 * R + (R if evap else 0)  # what the keep form stores and the reverse sweep re-reads (the fluxes' top level apart)

    timed = lambda step: th.median_ms(step, reps, ndigits=4)  # noqa: E731
    new = lambda names: th.new(names, lay, dev)  # noqa: E731
    sums = lambda names: {n: torch.zeros((lay.nblocks, nproma), dtype=torch.float64, device=dev) for n in names}  # noqa: E731
    g = torch.Generator(device=dev).manual_seed(0)
    w = {n: 2 * torch.rand(lay.nlevx(n), generator=g, dtype=torch.float64, device=dev) - 1 for n in B.OUT_NAMES}
    surface = torch.zeros(nlev + 1, dtype=torch.float64, device=dev)
    surface[-1] = 1
    wsurf = {"fplsl": surface, "fplsn": surface.clone()}

    def table(weights):
        t = torch.zeros((10, nlev + 1), dtype=torch.float64, device=dev)
        for n, a in weights.items():
            t[B.OUT_NAMES.index(n), :len(a)] = a
        return t
    head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
    xb = C.byref(ag._block("in", x, lay))
    out, scratch = new(B.OUT_NAMES), torch.empty((lay.nblocks, nlev, nproma) if evap else (0,), dtype=torch.float64, device=dev)
    sc = C.c_void_p(scratch.data_ptr() if evap else None)
    ob = C.byref(ag._block("out", out, lay))
    rows = {}
    # (i) forward
    rows["nl_dense"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_nl_launch(*head, xb, ob, B.Field(), 0.0, st()))),
                        "bytes_per_column": traj_b + plane_bytes(B.OUT_NAMES)}
    rows["nl_trajectory_pass"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_ad_launch_forward(*head, xb, ob, sc, st()))),
                                  "bytes_per_column": traj_b + plane_bytes(B.OUT_NAMES) + (R if evap else 0)}
    for name, weights in (("surface", wsurf), ("all_ten", w)):
        t, y = table(weights), sums(weights)
        yb = C.byref(ag._sums_block(y, lay))
        rows[f"nl_colsum_lean_{name}"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_nl_launch_colsum(*head, xb, C.c_void_p(t.data_ptr()), yb, None, None, st()))),
                                          "bytes_per_column": traj_b + 8 * len(weights)}
        kb = C.byref(ag._block("out", {n: out[n] for n in ("fplsl", "fplsn")}, lay))
        rows[f"nl_colsum_keep_{name}"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_nl_launch_colsum(*head, xb, C.c_void_p(t.data_ptr()), yb, kb, sc, st()))),
                                          "bytes_per_column": traj_b + 8 * len(weights) + kept_b + 16}
    # (ii) reverse and TL: dense, sparse, column sums; the narrow case (surface sums <-> t, q) and everything
    B.check(B.lib.cloudsc2_ad_launch_forward(*head, xb, ob, sc, st()))
    u = {n: torch.randn(lay.shape(n), generator=g, dtype=torch.float64, device=dev) for n in B.OUT_NAMES}
    ybar = {n: torch.randn((lay.nblocks, nproma), generator=g, dtype=torch.float64, device=dev) for n in B.OUT_NAMES}
    v = {n: 0.01 * a for n, a in x.items()}
    xa, dy, dsum = new(B.IN_NAMES), new(B.OUT_NAMES), sums(B.OUT_NAMES)
    rows["vjp_dense"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_vjp_launch(*head, xb, ob, C.byref(ag._block("in", xa, lay)),
                                                                                C.byref(ag._block("out", u, lay)), sc, st()))),
                         "bytes_per_column": traj_b + kept_b + 10 * R + plane_bytes(B.IN_NAMES)}
    rows["tl_dense"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_tl_launch(*head, xb, C.byref(B.Outputs()), C.byref(ag._block("in", v, lay)),
                                                                              C.byref(ag._block("out", dy, lay)), st()))),
                        "bytes_per_column": 2 * traj_b + plane_bytes(B.OUT_NAMES)}
    for name, pin, pout, weights in (("narrow", ("q", "t"), ("fplsl", "fplsn"), wsurf), ("everything", B.IN_NAMES, B.OUT_NAMES, w)):
        t = C.c_void_p(table(weights).data_ptr())
        ai = C.byref(ag._block("in", {n: xa[n] for n in pin}, lay))
        rows[f"vjp_sparse_{name}"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_vjp_launch_sparse(
            *head, 0, xb, ob, ai, C.byref(ag._block("out", {n: u[n] for n in pout}, lay)), sc, st()))),
            "bytes_per_column": traj_b + kept_b + len(pout) * R + plane_bytes(pin)}
        rows[f"vjp_colsum_{name}"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_vjp_launch_colsum(
            *head, 0, xb, ob, ai, t, C.byref(ag._sums_block({n: ybar[n] for n in pout}, lay)), sc, st()))),
            "bytes_per_column": traj_b + kept_b + 8 * len(pout) + plane_bytes(pin)}
        di = C.byref(ag._block("in", {n: v[n] for n in pin}, lay))
        rows[f"tl_sparse_{name}"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_tl_launch_sparse(
            *head, 0, xb, di, C.byref(ag._block("out", {n: dy[n] for n in pout}, lay)), st()))),
            "bytes_per_column": traj_b + plane_bytes(pin) + plane_bytes(pout)}
        rows[f"tl_colsum_{name}"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_tl_launch_colsum(
            *head, 0, xb, di, t, C.byref(ag._sums_block({n: dsum[n] for n in pout}, lay)), st()))),
            "bytes_per_column": traj_b + plane_bytes(pin) + 8 * len(pout)}
    del u, dy, xa, out
    # (iii) and (iv) through torch: the narrow case, separate arrays
    xc = {n: a.clone() for n, a in x.items()}
    yb2 = [ybar["fplsl"], ybar["fplsn"]]
    plane = lay.nblocks * nlev * nproma * 8

    def colsum_route(xs):
        ys = ag.cloudsc2_column_sums(xs, prm, ptsphy, ngptot, weights=wsurf)
        return [ys.fplsl, ys.fplsn]

    def einsum_route(xs):
        o = ag.cloudsc2(xs, prm, ptsphy, ngptot, sparse=True)
        return [torch.einsum("k,bkc->bc", wsurf["fplsl"], o.fplsl), torch.einsum("k,bkc->bc", wsurf["fplsn"], o.fplsn)]
    for name, route in (("colsum", colsum_route), ("einsum", einsum_route)):
        with torch.no_grad():
            rows[f"forward_nograd_{name}"] = {"ms": timed(lambda: route(xc))}

        def fwd_bwd():
            xs = {n: (a.requires_grad_() if n in ("q", "t") else a) for n, a in xc.items()}
            return torch.autograd.grad(route(xs), [xs["q"], xs["t"]], yb2)
        rows[f"forward_backward_{name}"] = {"ms": timed(fwd_bwd)}

        def f(q, t):
            a = dict(xc)
            a.update(q=q, t=t)
            return tuple(route(a))
        for a in xc.values():
            a.requires_grad_(False)
        rows[f"jvp_{name}"] = {"ms": timed(lambda: torch.func.jvp(f, (xc["q"], xc["t"]), (v["q"], v["t"])))}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        keep = fwd_bwd()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        rows[f"peak_forward_backward_{name}"] = {"bytes": peak, "full_level_planes": round(peak / plane, 2)}
        del keep
        for a in xc.values():
            a.requires_grad_(False)
    for a, b in (("nl_colsum_lean_surface", "nl_dense"), ("nl_colsum_lean_all_ten", "nl_dense"), ("nl_colsum_keep_surface", "nl_trajectory_pass"),
                 ("vjp_colsum_narrow", "vjp_sparse_narrow"), ("vjp_colsum_everything", "vjp_dense"), ("tl_colsum_narrow", "tl_sparse_narrow"),
                 ("tl_colsum_everything", "tl_dense"), ("forward_nograd_colsum", "forward_nograd_einsum"),
                 ("forward_backward_colsum", "forward_backward_einsum"), ("jvp_colsum", "jvp_einsum")):
        rows[a]["over_" + b] = round(rows[a]["ms"] / rows[b]["ms"], 3)
    print(json.dumps({"ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp64", "reps": reps, "evaporation": evap,
                      "device": torch.cuda.get_device_name(dev), "rows": rows}))
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "alternate":
        sys.exit(alternate(os.path.abspath(sys.argv[2]), sys.argv[3:]))
    sys.exit(run(sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "run" else sys.argv[1:]))
