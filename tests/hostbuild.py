"""Host builds of the column functions (tests/hostcheck/hostcheck*.hip): the one build recipe, the one table of units and of their
prototypes, and the one switch of the arithmetic mode.  A unit-test vehicle, not a product path.

Every unit is a library of its own with its own copy of hostcheck.hip's globals, so the mode is kept here and given to every library
that is loaded and to every one loaded later: a test asks for it with the ``precise`` fixture and never names a library."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dwarf_p_cloudsc2_tl_ad_amd import binding as B  # noqa: E402

HIPCC = "/opt/rocm/bin/hipcc"
HOSTCHECK_DIR = os.path.join(ROOT, "tests", "hostcheck")
HOST_SO_FLAGS = ["--cuda-host-only", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17"]
# the stand-alone sanitizer programs (their own main, the runtimes linked in); -O0: the instrumented sweeps take minutes to optimise and
# a second to run as they are
SANITIZED_EXE_FLAGS = ["--cuda-host-only", "-x", "hip", "-O0", "-g", "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address,undefined",
                       "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-std=c++17"]
BUILT: list = []  # the outputs this process compiled, in order


def _stale(out: str, near: str) -> bool:
    """no output, no dependency file, or a file of the project named in it that is missing or newer than the output; the toolchain's
    headers (neither under the repository nor next to the source) are not looked at"""
    if not (os.path.exists(out) and os.path.exists(out + ".d")):
        return True
    with open(out + ".d") as f:
        deps = f.read().replace("\\\n", " ").split(": ", 1)[-1].split()
    built = os.path.getmtime(out)
    for d in (os.path.normpath(os.path.join(ROOT, d)) for d in deps):
        if d.startswith((ROOT + os.sep, near + os.sep)) and not (os.path.exists(d) and os.path.getmtime(d) <= built):
            return True
    return False


def build(src: str, out: str, flags=HOST_SO_FLAGS, single: bool = B.SINGLE) -> str:
    """``out`` from ``src`` by hipcc, run from the repository root, unless the compiler's own dependency file says it is up to date.
    Written under temporary names and renamed, the dependency file first: another process building the same file never sees half of it."""
    src, out = os.path.abspath(src), os.path.abspath(out)
    if _stale(out, os.path.dirname(src)):
        tmp = os.path.join(os.path.dirname(out), f"tmp{os.getpid()}_{os.path.basename(out)}")
        try:
            subprocess.check_call([HIPCC, *flags, *(["-DCLOUDSC2_SINGLE"] if single else []), "-MD", "-MF", tmp + ".d", "-o", tmp,
                                   os.path.relpath(src, ROOT)], cwd=ROOT)
            os.replace(tmp + ".d", out + ".d")
            os.replace(tmp, out)
        finally:
            for t in (tmp, tmp + ".d"):
                if os.path.exists(t):
                    os.remove(t)
        BUILT.append(out)
    return out


# unit -> its source under tests/hostcheck; the library is libhostcheck[_<unit>][_sp].so next to it
UNITS = {"": "hostcheck.hip", "vjp": "hostcheck_vjp.hip", "batch": "hostcheck_batch.hip", "satur_lin": "hostcheck_satur_lin.hip",
         "par": "hostcheck_par.hip", "parjac": "hostcheck_parjac.hip", "parnormal": "hostcheck_parnormal.hip",
         "parcolsum": "hostcheck_parcolsum.hip", "sparse": "hostcheck_sparse.hip", "colsum": "hostcheck_colsum.hip",
         "enscolsum": "hostcheck_enscolsum.hip", "ens": "hostcheck_ens.hip", "census": "hostcheck_census.hip"}

_I, _D, _V, _LL, _U = C.c_int, C.c_double, C.c_void_p, C.c_longlong, C.c_uint
_PP, _PI, _PO, _PD, _MS = C.POINTER(B.Params), C.POINTER(B.Inputs), C.POINTER(B.Outputs), C.POINTER(C.c_double), C.POINTER(C.c_longlong)
_G = [_PP, _D, _I, _I, _I]  # prm, ptsphy, nproma, nlev, ngptot: what every sweep begins with
# exported function -> (restype, argtypes), None: left as ctypes has it.  A unit that includes another exports its functions too, so the
# table is by function and a library takes every row it has.
PROTOTYPES = {
    "hostcheck_get_precise": (_I, []),
    "hostcheck_satur": (_I, [_PP, _I, _I, _I, B.Field, B.Field, B.Field]),
    "hostcheck_nl": (_I, _G + [_PI, _PO, B.Field, _D]),
    "hostcheck_tl": (_I, _G + [_PI, _PO, _PI, _PO]),
    "hostcheck_ad": (_I, _G + [_PI, _PO, _PI, _PO, _V]),
    "hostcheck_set_self_increment": (None, [_D]),
    "hostcheck_set_yy": (None, [_V]),
    "hostcheck_set_ad_norms": (None, [_V]),
    "hostcheck_get_norm3_max": (_D, None),
    "hostcheck_taylor_sweep": (_I, _G + [_PI, _PO, _PO, _V]),
    "hostcheck_vjp_sweep": (_I, _G + [_PI, _PO, _PI, _PO, _V, _I, _I]),
    "hostcheck_batch_max": (_I, None),
    "hostcheck_tl_batch": (_I, _G + [_PI, _I, _PI, _PO]),
    "hostcheck_vjp_batch": (_I, _G + [_PI, _PO, _I, _PI, _PO, _V]),
    "hostcheck_satur_lin": (_I, [_PP, _I, _I, _I] + [B.Field] * 5),
    "hostcheck_tl_satur": (_I, _G + [_PI, _PI, _PO]),
    "hostcheck_vjp_satur": (_I, _G + [_PI, _PO, _PI, _PO, _V]),
    "hostcheck_tl_par": (_I, _G + [_I, _PI, _PI, _PD, _PO]),
    "hostcheck_vjp_par": (_I, _G + [_I, _PI, _PO, _PI, _PO, _V, _V, _PD]),
    "hostcheck_tl_parjac": (_I, _G + [_PI, _PO]),
    "hostcheck_parnormal": (_I, _G + [_PI, _PO, _PO, _V]),
    "hostcheck_parjac_colsum": (_I, _G + [_PI, _V, _PO]),
    "hostcheck_parnormal_colsum": (_I, _G + [_PI, _V, _PO, _PO, _V]),
    "hostcheck_sparse_forward": (_I, _G + [_PI, _PO, _V]),
    "hostcheck_sparse_tl": (_I, _G + [_I, _I, _PI, _PI, _PO]),
    "hostcheck_sparse_vjp": (_I, _G + [_I, _I, _PI, _PO, _PI, _PO, _V]),
    "hostcheck_colsum_nl": (_I, _G + [_PI, _V, _PO, _PO, _V]),
    "hostcheck_colsum_tl": (_I, _G + [_I, _PI, _PI, _V, _PO]),
    "hostcheck_colsum_vjp": (_I, _G + [_I, _PI, _PO, _PI, _V, _PO, _V]),
    "hostcheck_enscolsum_nl": (_I, _G + [_I, _V, _PI, _MS, _V, _PO, _MS, _PO, _MS, _V, _LL]),
    "hostcheck_enscolsum_tl": (_I, _G + [_I, _I, _V, _V, _PI, _MS, _PI, _MS, _V, _PO, _MS]),
    "hostcheck_enscolsum_vjp": (_I, _G + [_I, _I, _V, _PI, _MS, _PO, _MS, _PI, _MS, _V, _PO, _MS, _V, _LL, _V, _V]),
    "hostcheck_enscolsum_locate": (None, [_U, _U, _U, _V, _V]),
    "hostcheck_ens_real_bytes": (_I, None),
    "hostcheck_ens_consts": (_I, [_PP, _D, _PD, _PD]),
    "hostcheck_ens_member_args": (_I, [_PP, _D, _PD, _PD, _I, _I]),
    "hostcheck_ens_locate": (None, [_U, _U, _U, _V, _V]),
    "hostcheck_census": (_LL, _G + [_PI, _PO, _V]),
}

_libs: dict = {}
_mode = 0


def host_lib(unit: str = "", single: bool = B.SINGLE) -> C.CDLL:
    """The library of a unit in the process's precision (`single` given: in that one), built when stale, its prototypes set, in the
    arithmetic mode last given to set_precise."""
    if (unit, single) not in _libs:
        if unit == "" and os.environ.get("CLOUDSC2_HOSTCHECK_LIB"):  # a differently built copy, e.g. the AddressSanitizer build of test_sanitize.py
            path = os.environ["CLOUDSC2_HOSTCHECK_LIB"]
        else:
            name = "libhostcheck" + ("_" + unit if unit else "") + ("_sp" if single else "") + ".so"
            path = build(os.path.join(HOSTCHECK_DIR, UNITS[unit]), os.path.join(HOSTCHECK_DIR, name), single=single)
        lib = C.CDLL(path)
        for fn, (restype, argtypes) in PROTOTYPES.items():
            if hasattr(lib, fn):
                getattr(lib, fn).restype = restype
                if argtypes is not None:
                    getattr(lib, fn).argtypes = argtypes
        if hasattr(lib, "hostcheck_set_precise"):  # (hostcheck_ens.hip does not include hostcheck.hip)
            lib.hostcheck_set_precise(_mode)
        _libs[unit, single] = lib
    return _libs[unit, single]


def set_precise(p: int) -> None:
    """the arithmetic of every host library that has the switch, loaded or yet to be: 0 shared-reciprocal fast math, 1 the reference's
    operation order with IEEE division and libm exp"""
    global _mode
    _mode = int(p)
    for lib in _libs.values():
        if hasattr(lib, "hostcheck_set_precise"):
            lib.hostcheck_set_precise(_mode)


@pytest.fixture(params=["fast", "precise"])
def precise(request):
    p = int(request.param == "precise")
    set_precise(p)
    yield p
    set_precise(0)
