#!/usr/bin/env python3
"""The sparse derivative sweeps (cloudsc2_tl_launch_sparse, cloudsc2_vjp_launch_sparse; cloudsc2(..., sparse=True)) against the dense
ones at 160 000 columns, NPROMA 128, fp64: medians of REPS event-timed calls after warm-up.  Three mask cases,
    (a) everything present,
    (b) the narrow case: cotangents fplsl, fplsn -> gradients of t, q (TL: tangents of t, q, all ten output tangents stored),
    (c) one cotangent (fplsl), all 16 gradients (TL: one tangent, t, all ten output tangents),
each without and with the evaporation branch (levapls2), for the TL and the reverse sweep on preallocated buffers; then the narrow
backward and jvp through torch, dense op against sparse op.  Prints ONE JSON object with the bytes per column each launch moves.
    python tools/autograd_sparse_timing.py [NGPTOT [REPS]]"""
import ctypes as C
import json
import sys

import timing_harness as th
import torch

import dwarf_p_cloudsc2_tl_ad_amd as c2
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag
from dwarf_p_cloudsc2_tl_ad_amd import binding as B

ngptot = int(sys.argv[1]) if len(sys.argv) > 1 else 160000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
nproma, nlev = 128, 137

case = th.setup(ngptot, nproma, nlev)  # (one state under both parameter sets: QSAT is filled again per set below)
tab, ds, x, lay, ptsphy, dev = case.tab, case.ds, case.x, case.lay, case.ptsphy, case.dev
st = lambda: th.stream(dev)  # noqa: E731
new = lambda names: th.new(names, lay, dev)  # noqa: E731
timed = lambda step: th.median_ms(step, reps, ndigits=4)  # noqa: E731
HALF = ("paph", "fplsl", "fplsn", "fhpsl", "fhpsn")
R, H = 8 * nlev, 8 * (nlev + 1)  # bytes per column of a full-level plane and of a half-level plane written whole


def plane_bytes(names):
    return sum(H if n in HALF else R for n in names)


CASES = {  # name: (input side, output side) of the derivative blocks
    "a_everything": (B.IN_NAMES, B.OUT_NAMES),
    "b_narrow": (("q", "t"), ("fplsl", "fplsn")),
    "c_one_cotangent": (B.IN_NAMES, ("fplsl",)),
}
TL_CASES = {"a_everything": (B.IN_NAMES, B.OUT_NAMES), "b_narrow": (("q", "t"), B.OUT_NAMES), "c_one_tangent": (("t",), B.OUT_NAMES)}
result = {"ngptot": ngptot, "nproma": nproma, "nlev": nlev, "precision": "fp64", "reps": reps, "device": torch.cuda.get_device_name(dev)}

for evap in (False, True):
    prm = c2.default_params(c2.ceta_from_table(tab), lregcl=True, levapls2=evap)
    ds.satur(prm)
    g = torch.Generator(device=dev).manual_seed(0)
    u = {n: torch.randn(lay.shape(n), generator=g, dtype=torch.float64, device=dev) for n in B.OUT_NAMES}
    v = {n: 0.01 * t for n, t in x.items()}
    traj, scratch = new(B.OUT_NAMES), torch.empty((lay.nblocks, nlev, nproma) if evap else (0,), dtype=torch.float64, device=dev)
    sc = C.c_void_p(scratch.data_ptr() if evap else None)
    head = (C.byref(prm), ptsphy, nproma, nlev, ngptot)
    xb = C.byref(ag._block("in", x, lay))
    B.check(B.lib.cloudsc2_ad_launch_forward(*head, xb, C.byref(ag._block("out", traj, lay)), sc, st()))
    tb = C.byref(ag._block("out", traj, lay))
    xa, dy = new(B.IN_NAMES), new(B.OUT_NAMES)
    rows = {}
    traj_b = plane_bytes(B.IN_NAMES)
    rows["vjp_dense"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_vjp_launch(*head, xb, tb, C.byref(ag._block("in", xa, lay)),
                                                                                C.byref(ag._block("out", u, lay)), sc, st()))),
                         "bytes_per_column": traj_b + (3 if evap else 2) * R + 10 * R + 16 * R + H - R}
    rows["tl_dense"] = {"ms": timed(lambda: B.check(B.lib.cloudsc2_tl_launch(*head, xb, C.byref(B.Outputs()), C.byref(ag._block("in", v, lay)),
                                                                              C.byref(ag._block("out", dy, lay)), st()))),
                        "bytes_per_column": 2 * traj_b + plane_bytes(B.OUT_NAMES)}
    for name, (pin, pout) in CASES.items():
        ai = C.byref(ag._block("in", {n: xa[n] for n in pin}, lay))
        ao = C.byref(ag._block("out", {n: u[n] for n in pout}, lay))
        rows[f"vjp_sparse_{name}"] = {
            "ms": timed(lambda: B.check(B.lib.cloudsc2_vjp_launch_sparse(*head, 0, xb, tb, ai, ao, sc, st()))),
            "bytes_per_column": traj_b + (3 if evap else 2) * R + len(pout) * R + plane_bytes(pin)}
    for name, (pin, pout) in TL_CASES.items():
        di = C.byref(ag._block("in", {n: v[n] for n in pin}, lay))
        do = C.byref(ag._block("out", {n: dy[n] for n in pout}, lay))
        rows[f"tl_sparse_{name}"] = {
            "ms": timed(lambda: B.check(B.lib.cloudsc2_tl_launch_sparse(*head, 0, xb, di, do, st()))),
            "bytes_per_column": traj_b + plane_bytes(pin) + plane_bytes(pout)}
    # through torch: the narrow loss, separate arrays (forward-mode AD gives the base of a view a tangent too)
    xc = {n: t.clone() for n, t in x.items()}
    for sparse in (False, True):
        xs = {n: (t.clone().requires_grad_() if n in ("q", "t") else t) for n, t in xc.items()}
        out = ag.cloudsc2(xs, prm, ptsphy, ngptot, sparse=sparse)
        rows[f"backward_narrow_{'sparse' if sparse else 'dense'}"] = {"ms": timed(lambda: torch.autograd.grad(
            [out.fplsl, out.fplsn], [xs["q"], xs["t"]], [u["fplsl"], u["fplsn"]], retain_graph=True))}

        def f(q, t):
            a = dict(xc)
            a.update(q=q, t=t)
            return tuple(ag.cloudsc2(a, prm, ptsphy, ngptot, sparse=sparse))
        rows[f"jvp_narrow_{'sparse' if sparse else 'dense'}"] = {"ms": timed(lambda: torch.func.jvp(f, (xc["q"], xc["t"]), (v["q"], v["t"])))}
    for k in ("a_everything", "b_narrow", "c_one_cotangent"):
        rows[f"vjp_sparse_{k}"]["over_dense"] = round(rows[f"vjp_sparse_{k}"]["ms"] / rows["vjp_dense"]["ms"], 3)
    for k in TL_CASES:
        rows[f"tl_sparse_{k}"]["over_dense"] = round(rows[f"tl_sparse_{k}"]["ms"] / rows["tl_dense"]["ms"], 3)
    for k in ("backward", "jvp"):
        rows[f"{k}_narrow_sparse"]["over_dense"] = round(rows[f"{k}_narrow_sparse"]["ms"] / rows[f"{k}_narrow_dense"]["ms"], 3)
    result["evaporation" if evap else "plain"] = rows

print(json.dumps(result))
