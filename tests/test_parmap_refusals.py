"""What cloudsc2_nl_launch_parmap, cloudsc2_tl_launch_parmap and cloudsc2_vjp_launch_parmap refuse, with the geometry and the dummy
pointers of test_launcher_refusals.py (World in tests/gpu_util.py: NPROMA 8, NLEV 4, NGPTOT 12).  Every refusal is made before the
device is looked for, so every case is CLOUDSC2_EINVAL with or without a GPU and nothing launches; a well-formed call answers
CLOUDSC2_ENODEVICE where there is no device.  After every call the calling thread's launch log is empty: the parameter-map kernels are
no logged sweep family."""
from __future__ import annotations

import ctypes as C
import os

import pytest

from tests.gpu_util import R_NGPTOT as NGPTOT, R_NLEV as NLEV, R_NPROMA as NPROMA, S, World, refusal_params as params
from tests.util import B, ROOT

EINVAL = B.CLOUDSC2_EINVAL
NAMES = ("cloudsc2_nl_launch_parmap", "cloudsc2_tl_launch_parmap", "cloudsc2_vjp_launch_parmap")


def calls(W: World):
    L, r = B.lib, C.byref
    G = (NPROMA, NLEV, NGPTOT)
    tab = W.dbl("par")
    ref = lambda b: r(b) if b is not None else None  # noqa: E731

    def nl(q="p", g=G, par=tab, i="ins", o="outs", satur=0, scratch=None, **_):
        q = params() if q == "p" else q
        i = W.ins(qsat=None if satur else NPROMA * NLEV) if i == "ins" else i
        o = W.outs() if o == "outs" else o
        return L.cloudsc2_nl_launch_parmap(ref(q), 3600.0, *g, par, ref(i), ref(o), scratch, None)

    def tl(q="p", g=G, par=tab, dpar=tab, i="ins", d="ins", o="outs", satur=0, **_):
        q = params() if q == "p" else q
        i = W.ins(qsat=None if satur == 1 else NPROMA * NLEV) if i == "ins" else i
        d = W.ins("pert", qsat=None if satur == 1 else NPROMA * NLEV) if d == "ins" else d
        o = W.outs("pert") if o == "outs" else o
        return L.cloudsc2_tl_launch_parmap(ref(q), 3600.0, *g, satur, par, dpar, ref(i), ref(d), ref(o), None)

    def vjp(q="p", g=G, par=tab, dpar=tab, i="ins", d="ins", o="outs", satur=0, scratch=None, t="outs", **_):
        q = params() if q == "p" else q
        i = W.ins(qsat=None if satur == 1 else NPROMA * NLEV) if i == "ins" else i
        d = W.ins("adj", qsat=None if satur == 1 else NPROMA * NLEV) if d == "ins" else d
        o = W.outs("adj") if o == "outs" else o
        t = W.outs() if t == "outs" else t
        return L.cloudsc2_vjp_launch_parmap(ref(q), 3600.0, *g, satur, par, ref(i), ref(t), ref(d), ref(o), scratch, dpar, None)

    return nl, tl, vjp


def refused(fn, text=None, **kw):
    B.lib.cloudsc2_debug_launch_log_reset()
    rc = fn(**kw)
    msg = B.lib.cloudsc2_last_error().decode()
    assert rc == EINVAL and (text is None or text in msg), (fn.__name__, kw.keys(), rc, msg)
    assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0


def test_parmap_refusals_before_the_device_is_looked_for():
    W = World(False)
    nl, tl, vjp = calls(W)
    for fn in (nl, tl, vjp):
        refused(fn, "params is NULL", q=None)
        refused(fn, "table is NULL", par=None)                                  # the value table
        refused(fn, "lphylin", q=params(lphylin=0))
        refused(fn, "nproma >= 1", g=(0, NLEV, NGPTOT))
        refused(fn, "params.nlev", g=(NPROMA, NLEV + 1, NGPTOT))
        refused(fn, "math_mode", q=params(math_mode=3))
        refused(fn, "NULL argument block", i=None)
        refused(fn, "NULL argument block", o=None)
        refused(fn, "required input field", i=W.ins(mfu=None))                  # a NULL required field
        refused(fn, "share one block stride", i=W.ins(pap=2 * S))               # strides that differ within a layout group
        refused(fn, "required output field", o=W.outs("x", tenq=None))
        refused(fn, "share one block stride", o=W.outs("x", tenl=2 * S))
    for fn in (tl, vjp):
        refused(fn, "table is NULL", dpar=None)                                 # the tangent / the adjoint table
        refused(fn, "satur must be 0", satur=2)
        refused(fn, "satur must be 0", satur=-1)
        refused(fn, "NULL argument block", d=None)
        refused(fn, "qsat is required", i=W.ins(qsat=None))                     # satur = 0 without qsat
        refused(fn, "every qsat field must be NULL", satur=1, i=W.ins())        # satur = 1 with qsat
        refused(fn, "qsat field required", d=W.ins("x", qsat=None))
        refused(fn, "share one block stride", d=W.ins("x", gtenq=3 * S))
    refused(vjp, "PFPLSL5", t=W.outs("traj", only=("fplsn",)))
    refused(vjp, "NULL argument block", t=None)
    evap = params(levapls2=1)
    refused(nl, "scratch", q=evap)                                              # the cover checkpoint is kept exactly with the branch
    refused(vjp, "scratch", q=evap)


def test_a_well_formed_call_needs_a_device():
    if B.device_available():  # (the well-formed calls would launch on dummy pointers)
        return
    W = World(False)
    nl, tl, vjp = calls(W)
    dummy = C.c_void_p(256)
    for fn in (nl, tl, vjp):
        for kw in (dict(), dict(satur=1), dict(q=params(levapls2=1), scratch=dummy), dict(q=params(ldrain1d=1, lregcl=1), scratch=dummy, satur=1)):
            B.lib.cloudsc2_debug_launch_log_reset()
            assert fn(**kw) == B.CLOUDSC2_ENODEVICE, (fn.__name__, kw.keys(), B.lib.cloudsc2_last_error().decode())
            assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0


def test_header_binding_and_library_agree_on_the_new_symbols():
    with open(os.path.join(ROOT, "include", "cloudsc2_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert f"int {name}(" in header, name
        assert name in B.EXPORTED and hasattr(B.lib, name)
    assert len(B.FAMILIES) == 10 and not any("parmap" in f for f in B.FAMILIES)
    assert B.lib.cloudsc2_variant_built(10, 1) == EINVAL  # family 10 stays no family
