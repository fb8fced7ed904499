"""What the launchers of csrc/cloudsc2_launch.hip refuse, pinned: the return code and the text of ``cloudsc2_last_error()`` of every
refusal each entry point can produce, recorded in ``launcher_refusals.json`` in two columns -- ``cpu`` (no device: everything that is
checked before the device is looked for, CLOUDSC2_ENODEVICE for the rest) and ``gpu`` (with a device).  A few cases carry two faults,
so that which of them is reported is pinned too.

Geometry of every case whose fault is not the geometry: NPROMA 8, NLEV 4, NGPTOT 12 -- two blocks, the second with a padded tail.

Without a device the pointers are dummies: nothing can launch.  With one, a refusal lost by mistake must not become a kernel on memory
that is not there: every non-NULL pointer is device memory of (more than) the extent the geometry implies, and only cases whose loss
would still be a valid small launch have a ``gpu`` column (stride mismatches, satur, rpecons, lphylin, partial traj_out, qsat given
with SATUR in the sweep, a weight without a residual, a written field two members share, nproma_stat < 1, pert_lambda without LPHYLIN).
A NULL field or block, a missing checkpoint plane and a bad geometry are cases of the ``cpu`` column alone.

``python -m tests.test_launcher_refusals cpu|gpu`` records a column."""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

import pytest

from tests.gpu_util import R_NB as NB, R_NGPTOT as NGPTOT, R_NLEV as NLEV, R_NPROMA as NPROMA, S, SH, World, refusal_params as params
from tests.util import B

JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "launcher_refusals.json")
NCOLS = NB * NPROMA
K = 2  # members of the ensemble cases
RP, DP = C.POINTER(B.c_real), C.POINTER(C.c_double)


def cases(W: World):
    """(id, whether it has a gpu column, the call) of every case"""
    L, r, out = B.lib, C.byref, []

    def case(name, gpu, fn):
        assert name not in [c[0] for c in out], name
        out.append((name, gpu, fn))

    p, pe, pe0, p0 = params(), params(levapls2=1), params(levapls2=1, rpecons=0.0), params(lphylin=0)
    G = (NPROMA, NLEV, NGPTOT)
    G0 = (0, NLEV, NGPTOT)

    def h(q=p, g=G):  # the arguments every sweep launcher begins with
        return (r(q) if q is not None else None, 3600.0, *g)

    no_field = B.Field()
    ti, to, scr = W.ins(), W.outs(), W.real("scratch")
    di, do = W.ins("pert"), W.outs("pert")
    ti_q0, di_q0 = W.ins(qsat=None), W.ins("pert", qsat=None)
    none_out = B.Outputs()
    pap, t, qs, d1, d2 = (W.field(("satur", n)) for n in ("pap", "t", "qsat", "dqs_dpap", "dqs_dt"))
    odd = W.field(("satur", "odd"), stride=2 * S)

    # ---- the launch log ----
    case("launch_log/max<0", True, lambda: L.cloudsc2_debug_launch_log(None, None, -1))
    case("launch_log/no_arrays", True, lambda: L.cloudsc2_debug_launch_log(None, None, 1))

    # ---- SATUR: everything check_geom checks, in its order ----
    sat = lambda q=p, g=G, a=pap, b=t, c=qs: L.cloudsc2_satur_launch(r(q) if q is not None else None, *g, a, b, c, None)  # noqa: E731
    case("satur/prm_null", False, lambda: sat(q=None))
    case("satur/nproma=0", False, lambda: sat(g=G0))
    case("satur/nlev=1", False, lambda: sat(q=params(nlev=1), g=(NPROMA, 1, NGPTOT)))
    case("satur/ngptot=0", False, lambda: sat(g=(NPROMA, NLEV, 0)))
    case("satur/nlev>max", False, lambda: sat(g=(NPROMA, B.CLOUDSC2_MAX_NLEV + 1, NGPTOT)))
    case("satur/prm.nlev", False, lambda: sat(q=params(nlev=NLEV + 1)))
    case("satur/math_mode", False, lambda: sat(q=params(math_mode=3)))
    case("satur/prm_null+nproma=0", False, lambda: sat(q=None, g=G0))
    case("satur/null_field", False, lambda: sat(c=no_field))
    case("satur/stride", True, lambda: sat(b=odd))
    satl = lambda a=pap, b=t, c=qs, d=d1, e=d2, g=G: L.cloudsc2_satur_lin_launch(r(p), *g, a, b, c, d, e, None)  # noqa: E731
    case("satur_lin/nproma=0", False, lambda: satl(g=G0))
    case("satur_lin/null_field", False, lambda: satl(d=no_field))
    case("satur_lin/stride", True, lambda: satl(e=odd))
    case("satur_lin/stride_qsat", True, lambda: satl(c=odd))

    # ---- NL ----
    nl = lambda q=p, g=G, i=ti, o=to, lam=0.0: L.cloudsc2_nl_launch(*h(q, g), r(i) if i else None, r(o) if o else None, no_field, lam, None)  # noqa: E731
    case("nl/null_block", False, lambda: nl(o=None))
    case("nl/null_block+nproma=0", False, lambda: nl(i=None, g=G0))
    case("nl/nproma=0", False, lambda: nl(g=G0))
    case("nl/input_null", False, lambda: nl(i=W.ins(supsat=None)))
    case("nl/output_null", False, lambda: nl(o=W.outs(covptot=None)))
    case("nl/in_stride_full", True, lambda: nl(i=W.ins(mfd=2 * S)))
    case("nl/in_stride_cml", True, lambda: nl(i=W.ins(gteni=2 * S)))
    case("nl/in_stride_clv", True, lambda: nl(i=W.ins(i=2 * S)))
    case("nl/out_stride_loc", True, lambda: nl(o=W.outs(tenq=2 * S)))
    case("nl/out_stride_half", True, lambda: nl(o=W.outs(fhpsn=2 * SH)))
    case("nl/out_full_vs_in", True, lambda: nl(o=W.outs(clc=2 * S, covptot=2 * S)))
    case("nl/out_half_vs_paph", True, lambda: nl(o=W.outs(fplsl=2 * SH, fplsn=2 * SH, fhpsl=2 * SH, fhpsn=2 * SH)))
    case("nl/in_stride+out_stride", True, lambda: nl(i=W.ins(lu=2 * S), o=W.outs(teni=2 * S)))
    case("nl/nolin+pert_lambda", True, lambda: nl(q=p0, lam=0.1))

    # ---- TL ----
    tl = lambda q=p, g=G, i=ti, o=none_out, x=di, y=do: L.cloudsc2_tl_launch(  # noqa: E731
        *h(q, g), r(i) if i else None, r(o) if o else None, r(x) if x else None, r(y) if y else None, None)
    case("tl/pert_in_null", False, lambda: tl(x=None))
    case("tl/pert_in_null+nproma=0", False, lambda: tl(x=None, g=G0))
    case("tl/null_block", False, lambda: tl(y=None))
    case("tl/nproma=0", False, lambda: tl(g=G0))
    case("tl/partial_traj_out", True, lambda: tl(o=W.outs(only=("tent", "clc"))))
    case("tl/traj_in_null_field", False, lambda: tl(i=W.ins(t=None)))
    case("tl/pert_in_null_field", False, lambda: tl(x=W.ins("pert", lude=None)))
    case("tl/pert_in_qsat_null", False, lambda: tl(x=di_q0))
    case("tl/pert_out_null_field", False, lambda: tl(y=W.outs("pert", fplsl=None)))
    case("tl/pert_in_stride", True, lambda: tl(x=W.ins("pert", q=2 * S)))
    case("tl/pert_out_stride", True, lambda: tl(y=W.outs("pert", tenl=2 * S)))
    case("tl/pert_out_full_vs_pert_in", True, lambda: tl(y=W.outs("pert", clc=2 * S, covptot=2 * S)))
    case("tl/traj_out_stride", True, lambda: tl(o=W.outs(fplsn=2 * SH)))
    tls = lambda g=G, i=ti, o=to, y=do: L.cloudsc2_tl_launch_self(  # noqa: E731
        *h(p, g), r(i) if i else None, r(o) if o else None, 0.01, r(y) if y else None, None, None)
    case("tl_self/null_block", False, lambda: tls(i=None))
    case("tl_self/nproma=0", False, lambda: tls(g=G0))
    case("tl_self/partial_traj_out", True, lambda: tls(o=W.outs(covptot=None)))
    case("tl_self/pert_out_null_field", False, lambda: tls(y=W.outs("pert", tent=None)))
    case("tl_self/pert_out_stride", True, lambda: tls(y=W.outs("pert", teni=2 * S)))
    tlsat = lambda g=G, i=ti_q0, x=di_q0, y=do: L.cloudsc2_tl_launch_satur(*h(p, g), r(i) if i else None, r(x) if x else None, r(y), None)  # noqa: E731
    case("tl_satur/pert_in_null", False, lambda: tlsat(x=None))
    case("tl_satur/null_block", False, lambda: tlsat(i=None))
    case("tl_satur/nproma=0", False, lambda: tlsat(g=G0))
    case("tl_satur/traj_qsat_given", True, lambda: tlsat(i=ti))
    case("tl_satur/pert_qsat_given", True, lambda: tlsat(x=di))
    case("tl_satur/pert_in_stride", True, lambda: tlsat(x=W.ins("pert", qsat=None, t=2 * S)))

    # ---- AD: both sweeps, each alone, the vector-Jacobian product ----
    for name, fn in (("ad", L.cloudsc2_ad_launch), ("ad_assign", L.cloudsc2_ad_launch_assign), ("vjp", L.cloudsc2_vjp_launch),
                     ("vjp_satur", L.cloudsc2_vjp_launch_satur)):
        sl = name == "vjp_satur"
        a_ti, a_di = (ti_q0, di_q0) if sl else (ti, di)
        ad = lambda q=p, g=G, i=a_ti, o=to, x=a_di, y=do, s=scr, fn=fn: fn(  # noqa: E731
            *h(q, g), r(i) if i else None, r(o), r(x) if x else None, r(y), s, None)
        case(f"{name}/null_block", False, lambda ad=ad: ad(x=None))
        case(f"{name}/nproma=0", False, lambda ad=ad: ad(g=G0))
        case(f"{name}/traj_in_null_field", False, lambda ad=ad, sl=sl: ad(i=W.ins(qsat=None, pap=None) if sl else W.ins(pap=None)))
        case(f"{name}/adj_in_stride", True, lambda ad=ad, sl=sl: ad(x=W.ins("pert", mfu=2 * S, **({"qsat": None} if sl else {}))))
        case(f"{name}/adj_out_stride", True, lambda ad=ad: ad(y=W.outs("pert", fhpsl=2 * SH)))
        case(f"{name}/adj_out_null_field", False, lambda ad=ad: ad(y=W.outs("pert", clc=None)))
        case(f"{name}/no_checkpoint_plane", False, lambda ad=ad: ad(q=pe, s=None))
        if name.startswith("ad"):
            case(f"{name}/traj_out_null_field", False, lambda ad=ad: ad(o=W.outs(tent=None)))
        else:
            case(f"{name}/traj_out_no_flux", False, lambda ad=ad: ad(o=W.outs(fplsn=None)))
        if not sl:
            case(f"{name}/adj_in_qsat_null", False, lambda ad=ad: ad(x=di_q0))
    case("vjp_satur/traj_qsat_given", True, lambda: L.cloudsc2_vjp_launch_satur(*h(), r(ti), r(to), r(di_q0), r(do), scr, None))
    case("vjp_satur/adj_qsat_given", True, lambda: L.cloudsc2_vjp_launch_satur(*h(), r(ti_q0), r(to), r(di), r(do), scr, None))
    fwd = lambda g=G, i=ti, o=to, q=p, s=scr: L.cloudsc2_ad_launch_forward(*h(q, g), r(i) if i else None, r(o), s, None)  # noqa: E731
    case("ad_forward/null_block", False, lambda: fwd(i=None))
    case("ad_forward/nproma=0", False, lambda: fwd(g=G0))
    case("ad_forward/traj_out_null_field", False, lambda: fwd(o=W.outs(fhpsl=None)))
    case("ad_forward/in_stride", True, lambda: fwd(i=W.ins(lude=2 * S)))
    case("ad_forward/no_checkpoint_plane", False, lambda: fwd(q=pe, s=None))
    rev = lambda g=G, o=to, x=di, y=do, q=p, s=scr, a=1: L.cloudsc2_ad_launch_reverse(  # noqa: E731
        *h(q, g), r(ti), r(o), r(x) if x else None, r(y), s, a, None)
    case("ad_reverse/null_block", False, lambda: rev(x=None))
    case("ad_reverse/nproma=0", False, lambda: rev(g=G0))
    case("ad_reverse/traj_out_no_flux", False, lambda: rev(o=W.outs(only=("fplsn",))))
    case("ad_reverse/adj_in_stride", True, lambda: rev(x=W.ins("pert", gtenq=2 * S), a=0))
    case("ad_reverse/flux_vs_paph", True, lambda: rev(o=W.outs(only=("fplsl", "fplsn"), fplsl=2 * SH, fplsn=2 * SH)))
    case("ad_reverse/no_checkpoint_plane", False, lambda: rev(q=pe, s=None))
    norms, gmax = W.dbl("norms", 3 * NCOLS), W.dbl("gmax", 1)
    rn = lambda q=p, g=G, n=norms, m=gmax, x=di: L.cloudsc2_ad_launch_reverse_norms(*h(q, g), r(ti), r(to), r(x), r(do), n, m, None)  # noqa: E731
    case("ad_reverse_norms/norms_null", False, lambda: rn(n=None))
    case("ad_reverse_norms/norms_null+nproma=0", False, lambda: rn(m=None, g=G0))
    case("ad_reverse_norms/nproma=0", False, lambda: rn(g=G0))
    case("ad_reverse_norms/evaporation", False, lambda: rn(q=pe))  # (no checkpoint plane: that is what a device reports first)
    case("ad_reverse_norms/adj_in_stride", True, lambda: rn(x=W.ins("pert", supsat=2 * S)))

    # ---- the parameter forms ----
    n_out = C.c_longlong(0)
    for name, fn in (("par", L.cloudsc2_par_work_doubles), ("parnormal", L.cloudsc2_parnormal_work_doubles),
                     ("taylor_sweep", L.cloudsc2_taylor_sweep_work_doubles)):
        case(f"{name}_work_doubles/nproma=0", True, lambda fn=fn: fn(0, NGPTOT, r(n_out)))
        case(f"{name}_work_doubles/ngptot=0", True, lambda fn=fn: fn(NPROMA, 0, r(n_out)))
        case(f"{name}_work_doubles/result_null", True, lambda fn=fn: fn(NPROMA, NGPTOT, None))
    dpar = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    tlp = lambda q=p, g=G, sat=0, i=ti, x=di, d=dpar, y=do: L.cloudsc2_tl_launch_par(  # noqa: E731
        *h(q, g), sat, r(i) if i else None, r(x) if x else None, d, r(y), None)
    case("tl_par/satur=2", True, lambda: tlp(sat=2))
    case("tl_par/satur=2+rpecons=0", True, lambda: tlp(sat=2, q=pe0))
    case("tl_par/rpecons=0", True, lambda: tlp(q=pe0))
    case("tl_par/rpecons=0_ldrain1d", True, lambda: tlp(q=params(ldrain1d=1, rpecons=0.0)))
    case("tl_par/pert_in_null", False, lambda: tlp(x=None))
    case("tl_par/dpar_null", False, lambda: tlp(d=None))
    case("tl_par/satur=0_without_qsat", False, lambda: tlp(i=ti_q0))
    case("tl_par/satur=1_with_qsat", True, lambda: tlp(sat=1, x=di_q0))
    case("tl_par/traj_in_null", False, lambda: tlp(i=None))
    case("tl_par/nproma=0", False, lambda: tlp(g=G0))
    case("tl_par/pert_out_stride", True, lambda: tlp(y=W.outs("pert", fplsl=2 * SH)))
    work, padj = W.dbl("work"), W.dbl("par_adj", 4 * K)
    vjpp = lambda q=p, g=G, sat=0, i=ti, x=di, w=work, a=padj, s=scr: L.cloudsc2_vjp_launch_par(  # noqa: E731
        *h(q, g), sat, r(i) if i else None, r(to), r(x), r(do), s, w, a, None)
    case("vjp_par/satur=-1", True, lambda: vjpp(sat=-1))
    case("vjp_par/satur=-1+rpecons=0", True, lambda: vjpp(sat=-1, q=pe0))
    case("vjp_par/rpecons=0", True, lambda: vjpp(q=pe0))
    case("vjp_par/work_null", False, lambda: vjpp(w=None))
    case("vjp_par/par_adj_null", False, lambda: vjpp(a=None))
    case("vjp_par/satur=0_without_qsat", False, lambda: vjpp(i=ti_q0))
    case("vjp_par/satur=1_with_qsat", True, lambda: vjpp(sat=1, i=ti_q0))
    case("vjp_par/nproma=0", False, lambda: vjpp(g=G0))
    case("vjp_par/adj_in_stride", True, lambda: vjpp(x=W.ins("pert", l=2 * S)))
    case("vjp_par/no_checkpoint_plane", False, lambda: vjpp(q=pe, s=None))

    four = lambda **edit: (B.Outputs * 4)(*[W.outs(f"jac{k}", **(edit if k == 2 else {})) for k in range(4)])  # noqa: E731
    jac = lambda q=p, g=G, i=ti, y=None: L.cloudsc2_tl_launch_parjac(  # noqa: E731
        r(q) if q is not None else None, 3600.0, *g, r(i) if i else None, y if y is not None else four(), None)
    case("parjac/prm_null", False, lambda: jac(q=None))
    case("parjac/traj_in_null", False, lambda: jac(i=None))
    case("parjac/lphylin=0", True, lambda: jac(q=p0))
    case("parjac/rpecons=0", True, lambda: jac(q=pe0))
    case("parjac/lphylin=0+rpecons=0", True, lambda: jac(q=params(lphylin=0, levapls2=1, rpecons=0.0)))
    case("parjac/traj_in_null_field", False, lambda: jac(i=W.ins(q=None)))
    case("parjac/traj_in_stride", True, lambda: jac(i=W.ins(pap=2 * S)))
    case("parjac/block_null_field", False, lambda: jac(y=four(tenl=None)))
    case("parjac/block_stride", True, lambda: jac(y=four(tent=2 * S)))
    case("parjac/blocks_differ", True, lambda: jac(y=four(tent=2 * S, tenq=2 * S, tenl=2 * S, teni=2 * S)))
    case("parjac/fourth_block_with_evaporation", False, lambda: jac(q=pe, y=(B.Outputs * 4)(*[W.outs(f"jac{k}") for k in range(3)])))
    case("parjac/nproma=0", False, lambda: jac(g=G0))
    case("parjac/prm.nlev", False, lambda: jac(q=params(nlev=NLEV + 1)))
    case("parjac/lphylin=0+nproma=0", False, lambda: jac(q=p0, g=G0))

    res, wt, normal = W.outs("resid"), W.outs("weight"), W.dbl("normal", 14)
    pn = lambda q=p, g=G, i=ti, rs=res, w=wt, wk=work, nm=normal: L.cloudsc2_parnormal_launch(  # noqa: E731
        r(q) if q is not None else None, 3600.0, *g, r(i), r(rs) if rs else None, r(w) if w else None, wk, nm, None)
    case("parnormal/resid_null", False, lambda: pn(rs=None))
    case("parnormal/work_null", False, lambda: pn(wk=None))
    case("parnormal/lphylin=0+work_null", False, lambda: pn(q=p0, wk=None))
    case("parnormal/lphylin=0", True, lambda: pn(q=p0))
    case("parnormal/rpecons=0", True, lambda: pn(q=pe0))
    case("parnormal/traj_in_null_field", False, lambda: pn(i=W.ins(gtent=None)))
    case("parnormal/traj_in_stride", True, lambda: pn(i=W.ins(gtenl=2 * S)))
    case("parnormal/weight_without_residual", True, lambda: pn(rs=W.outs("resid", tenq=None)))
    case("parnormal/weight_without_residual+stride", True, lambda: pn(rs=W.outs("resid", tenq=None), w=W.outs("weight", teni=2 * S)))
    case("parnormal/nothing_observed", True, lambda: pn(rs=none_out, w=None))
    case("parnormal/resid_stride", True, lambda: pn(rs=W.outs("resid", fplsn=2 * SH), w=None))
    case("parnormal/weight_stride", True, lambda: pn(w=W.outs("weight", covptot=2 * S)))
    case("parnormal/resid_vs_weight_loc", True, lambda: pn(w=W.outs("weight", only=("tent", "tenq"), tent=2 * S, tenq=2 * S)))
    case("parnormal/resid_vs_weight_half", True, lambda: pn(w=W.outs("weight", only=("fhpsl",), fhpsl=2 * SH)))
    case("parnormal/nproma=0", False, lambda: pn(g=G0))
    case("parnormal/lphylin=0+nproma=0", False, lambda: pn(q=p0, g=G0))

    # ---- ensembles ----
    wsb = L.cloudsc2_ens_workspace_bytes
    for bad in ((0, *G), (65536, *G), (K, *G0), (K, NPROMA, 1, NGPTOT), (K, NPROMA, B.CLOUDSC2_MAX_NLEV + 1, NGPTOT), (K, NPROMA, NLEV, 0)):
        case("ens_workspace_bytes/" + "_".join(map(str, bad)), True, lambda bad=bad: wsb(*bad))
    ews = C.c_void_p(W.mem("ens_ws", max(int(wsb(K, *G)), 8) // 8, real=False))
    pdev, dpdev = W.dbl("params_dev", 4 * K), W.dbl("dparams_dev", 4 * K)
    own_in, own_out = (C.c_longlong * 16)(*[NB * SH] * 16), (C.c_longlong * 10)(*[NB * SH] * 10)
    nle = lambda q=p, g=G, m=K, pd=pdev, o=to, om=own_out, s=None, sm=0, ws=ews, i=ti: L.cloudsc2_nl_launch_ens(  # noqa: E731
        *h(q, g), m, pd, r(i) if i else None, None, r(o), om, s, sm, ws, None)
    tle = lambda q=p, g=G, sat=0, m=K, pd=pdev, dd=dpdev, i=ti, x=di, y=do, ym=own_out, ws=ews: L.cloudsc2_tl_launch_ens(  # noqa: E731
        *h(q, g), sat, m, pd, dd, r(i), None, r(x) if x else None, None, r(y), ym, ws, None)
    vje = lambda q=p, g=G, sat=0, m=K, pd=pdev, i=ti, x=di, xm=own_in, ws=ews, a=padj, s=scr: L.cloudsc2_vjp_launch_ens(  # noqa: E731
        *h(q, g), sat, m, pd, r(i), None, r(to), None, r(x) if x else None, xm, r(do), None, s, 0, ws, a, None)
    for name, call in (("nl_ens", nle), ("tl_ens", tle), ("vjp_ens", vje)):
        case(f"{name}/members=0", False, lambda call=call: call(m=0))
        case(f"{name}/members=65536", False, lambda call=call: call(m=65536))
        case(f"{name}/params_null", False, lambda call=call: call(pd=None))
        case(f"{name}/workspace_null", False, lambda call=call: call(ws=None))
        case(f"{name}/lphylin=0", True, lambda call=call: call(q=p0))
        case(f"{name}/nproma=0", False, lambda call=call: call(g=G0))
        case(f"{name}/grid_limit", False, lambda call=call: call(m=65535, g=(128, NLEV, 128 * 40000)))
        if name != "nl_ens":
            case(f"{name}/satur=2", True, lambda call=call: call(sat=2))
            case(f"{name}/satur=2+lphylin=0", True, lambda call=call: call(sat=2, q=p0))
            case(f"{name}/satur=0_without_qsat", False, lambda call=call: call(i=ti_q0))
            case(f"{name}/satur=1_with_qsat", True, lambda call=call: call(sat=1))
    case("nl_ens/shared_output", True, lambda: nle(om=None))
    case("nl_ens/shared_output_one_member", False, lambda: nle(om=None, m=1, i=None))
    case("nl_ens/shared_checkpoint", True, lambda: nle(s=scr, sm=0))
    case("nl_ens/shared_checkpoint+shared_output", True, lambda: nle(s=scr, sm=0, om=None))
    case("nl_ens/no_checkpoint_plane", False, lambda: nle(q=pe))
    case("nl_ens/output_null_field", False, lambda: nle(o=W.outs(clc=None)))
    case("tl_ens/shared_output", True, lambda: tle(ym=None))
    case("tl_ens/one_shared_output", True, lambda: tle(ym=(C.c_longlong * 10)(*([NB * SH] * 9 + [0]))))
    case("tl_ens/pert_in_null", False, lambda: tle(x=None))
    case("tl_ens/dparams_null", False, lambda: tle(dd=None))
    case("tl_ens/pert_out_stride", True, lambda: tle(y=W.outs("pert", tenq=2 * S)))
    case("vjp_ens/shared_adjoint", True, lambda: vje(xm=None))
    case("vjp_ens/par_adj_null", False, lambda: vje(a=None))
    case("vjp_ens/adj_in_null", False, lambda: vje(x=None))
    case("vjp_ens/adj_in_stride", True, lambda: vje(x=W.ins("pert", lu=2 * S)))

    # ---- batched sweeps ----
    two_in = lambda **edit: (B.Inputs * 2)(W.ins("pert"), W.ins("pert1", **edit))  # noqa: E731
    two_out = lambda **edit: (B.Outputs * 2)(W.outs("pert"), W.outs("pert1", **edit))  # noqa: E731
    tlb = lambda g=G, i=ti, n=2, x=None, y=None, null=False: L.cloudsc2_tl_launch_batch(  # noqa: E731
        *h(p, g), r(i), n, None if null else (x if x is not None else two_in()), y if y is not None else two_out(), None)
    vjb = lambda g=G, i=ti, o=to, n=2, x=None, y=None, null=False, q=p, s=scr: L.cloudsc2_vjp_launch_batch(  # noqa: E731
        *h(q, g), r(i), r(o), n, None if null else (x if x is not None else two_in()), y if y is not None else two_out(), s, None)
    for name, call in (("tl_batch", tlb), ("vjp_batch", vjb)):
        case(f"{name}/null_block", False, lambda call=call: call(null=True))
        case(f"{name}/nbatch=0", False, lambda call=call: call(n=0))
        case(f"{name}/null_block+nbatch=0", False, lambda call=call: call(null=True, n=0))
        case(f"{name}/nbatch=0+nproma=0", False, lambda call=call: call(n=0, g=G0))
        case(f"{name}/traj_qsat_null", False, lambda call=call: call(i=ti_q0))
        case(f"{name}/one_direction_traj_qsat_null", False, lambda call=call: call(i=ti_q0, n=1))
        case(f"{name}/second_direction_null_field", False, lambda call=call: call(x=two_in(mfu=None)))
        case(f"{name}/second_direction_qsat_null", False, lambda call=call: call(x=two_in(qsat=None)))
        case(f"{name}/second_direction_out_null_field", False, lambda call=call: call(y=two_out(teni=None)))
        case(f"{name}/stride_in_a_direction", True, lambda call=call: call(x=two_in(t=2 * S)))
        case(f"{name}/directions_differ", True, lambda call=call: call(x=two_in(gtent=2 * S, gtenq=2 * S, gtenl=2 * S, gteni=2 * S)))
        case(f"{name}/directions_differ_out", True, lambda call=call: call(y=two_out(tent=2 * S, tenq=2 * S, tenl=2 * S, teni=2 * S)))
        case(f"{name}/traj_in_stride", True, lambda call=call: call(i=W.ins(lude=2 * S)))
    case("vjp_batch/traj_out_no_flux", False, lambda: vjb(o=W.outs(fplsl=None)))
    case("vjp_batch/no_checkpoint_plane", False, lambda: vjb(q=pe, s=None))
    case("vjp_batch/one_direction_no_checkpoint_plane", False, lambda: vjb(q=pe, s=None, n=1))

    # ---- expansion and validation ----
    table = C.cast(W.real("table", 100 * (NLEV + 1)), RP)
    fld = W.field("expanded")
    ex = lambda tb=table, klon=100, period=100, start=0, nproma=NPROMA, f=fld: L.cloudsc2_expand_launch(  # noqa: E731
        tb, klon, period, start, NLEV, 1, nproma, NGPTOT, f, None)
    vws, vst = C.cast(W.dbl("validate_ws", 5 * 2048), DP), C.cast(W.dbl("validate_stats", 5), DP)
    va = lambda tb=table, klon=100, period=100, start=0, nproma=NPROMA, f=fld, ws=vws, st=vst: L.cloudsc2_validate_launch(  # noqa: E731
        tb, klon, period, start, NLEV, 1, nproma, NGPTOT, f, ws, st, None)
    for name, call in (("expand", ex), ("validate", va)):
        case(f"{name}/table_null", False, lambda call=call: call(tb=None))
        case(f"{name}/field_null", False, lambda call=call: call(f=no_field))
        case(f"{name}/period>klon", True, lambda call=call: call(period=101))
        case(f"{name}/start<0", False, lambda call=call: call(start=-1))  # (lost, it would read in front of the table)
        case(f"{name}/nproma=0", False, lambda call=call: call(nproma=0))
        case(f"{name}/block_stride_too_small", True, lambda call=call: call(f=W.field("expanded", stride=S - 1)))
        case(f"{name}/table_null+period>klon", False, lambda call=call: call(tb=None, period=101))
    case("validate/workspace_null", False, lambda: va(ws=None))
    case("validate/stats_null", False, lambda: va(st=None))

    # ---- the tests' statistics ----
    sums = W.dbl("sums", 2 * 10 * NCOLS * 10)
    tsum = lambda f=to, fp=do, t=res, s=sums: L.cloudsc2_taylor_sums_launch(NPROMA, NLEV, NGPTOT, r(f) if f else None, r(fp), r(t), 0.1, s, None)  # noqa: E731
    case("taylor_sums/null_block", False, lambda: tsum(f=None))
    case("taylor_sums/sums_null", False, lambda: tsum(s=None))
    case("taylor_sums/null_field", False, lambda: tsum(t=W.outs("resid", fhpsn=None)))
    tsw = lambda q=p, g=G, ns=NPROMA, i=ti, o=to, t=do, w=work, s=sums: L.cloudsc2_taylor_sweep_launch(  # noqa: E731
        *h(q, g), ns, r(i), r(o), r(t) if t else None, w, s, None)
    case("taylor_sweep/null_block", False, lambda: tsw(t=None))
    case("taylor_sweep/work_null", False, lambda: tsw(w=None))
    case("taylor_sweep/nproma=0", False, lambda: tsw(g=G0))
    case("taylor_sweep/nproma_stat=0", True, lambda: tsw(ns=0))
    case("taylor_sweep/lphylin=0", True, lambda: tsw(q=p0))
    case("taylor_sweep/nproma_stat=0+lphylin=0", True, lambda: tsw(ns=0, q=p0))
    case("taylor_sweep/in_stride", True, lambda: tsw(i=W.ins(mfu=2 * S)))
    case("taylor_sweep/out_null_field", False, lambda: tsw(o=W.outs(tenl=None)))
    case("taylor_sweep/tl_null_field", False, lambda: tsw(t=W.outs("pert", fplsn=None)))
    qf = W.field(("traj", "qsat"))
    an = lambda i=ti, q=qf, y=do, x=di, n=norms, m=gmax: L.cloudsc2_adjoint_norms_launch(  # noqa: E731
        NPROMA, NLEV, NGPTOT, r(i) if i else None, r(q) if q else None, r(y) if y else None, r(x) if x else None, n, m, None)
    case("adjoint_norms/norms_null", False, lambda: an(n=None))
    case("adjoint_norms/y_null_field", False, lambda: an(y=W.outs("pert", teni=None), x=None))
    case("adjoint_norms/y_stride", True, lambda: an(y=W.outs("pert", fhpsn=2 * SH), x=None))
    case("adjoint_norms/traj_in_null", False, lambda: an(y=None, i=None))
    case("adjoint_norms/qsat_null", False, lambda: an(y=None, q=None))
    case("adjoint_norms/blockmax_null", False, lambda: an(y=None, m=None))
    case("adjoint_norms/x_adj_qsat_null", False, lambda: an(y=None, x=di_q0))
    case("adjoint_norms/x_adj_stride", True, lambda: an(y=None, x=W.ins("pert", i=2 * S)))
    case("adjoint_norms/traj_in_stride", True, lambda: an(y=None, i=W.ins(q=2 * S)))
    return out


def run(W: World, column: str) -> dict:
    got = {}
    for name, gpu, fn in cases(W):
        if column == "gpu" and not gpu:
            continue
        rc = int(fn())
        got[name] = [rc, B.lib.cloudsc2_last_error().decode() if rc else ""]
    return got


def recorded() -> dict:
    with open(JSON) as f:
        return json.load(f)


def compare(got: dict, column: str) -> None:
    want = {k: v[column] for k, v in recorded().items() if v.get(column) is not None}
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong


def test_the_recorded_file_matches_the_cases():
    """every case is a refusal (no 0 was recorded), both columns belong to the cases, the device column to the admitted ones alone"""
    rec, cs = recorded(), cases(World(False))
    assert sorted(rec) == sorted(c[0] for c in cs)
    for name, gpu, _ in cs:
        assert rec[name]["cpu"][0] != 0 and rec[name]["cpu"][1], name
        assert (rec[name].get("gpu") is not None) == gpu, name
        if gpu:
            assert rec[name]["gpu"][0] == B.CLOUDSC2_EINVAL and rec[name]["gpu"][1], name


def test_refusals_without_a_device():
    if B.lib.cloudsc2_device_available():
        pytest.skip("a device is present: the dummy pointers of this column must not meet one (the gpu test compares the other column)")
    compare(run(World(False), "cpu"), "cpu")


@pytest.fixture(scope="module")
def device_world():
    return World(True)


@pytest.mark.gpu
def test_refusals_with_a_device(device_world):
    import torch

    compare(run(device_world, "gpu"), "gpu")
    torch.cuda.synchronize()


if __name__ == "__main__":
    column = sys.argv[1]
    assert column in ("cpu", "gpu") and bool(B.lib.cloudsc2_device_available()) == (column == "gpu")
    got = run(World(column == "gpu"), column)
    rec = recorded() if os.path.exists(JSON) else {}
    for name, gpu, _ in cases(World(False)):
        rec.setdefault(name, {"cpu": None, "gpu": None})
        if name in got:
            rec[name][column] = got[name]
            if got[name][0] == 0:
                print("NOT REFUSED:", name)
    rec = {k: rec[k] for k in (c[0] for c in cases(World(False)))}
    with open(os.environ.get("CLOUDSC2_REFUSALS_OUT", JSON), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rec.items()) + "\n}\n")  # one case per line
    print(f"{column}: {len(got)} cases recorded")
