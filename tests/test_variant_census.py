"""The census of kernel variants this build ships (cloudsc2_variant_built) and the semantics of the calling thread's launch log
(cloudsc2_debug_launch_log), as far as they show without a device.

The expected sets are restated here from the validity predicates of the variant tables (the `valid` column of the table in
csrc/cloudsc2_sweep_kernels.hpp: nl_variant_valid ... taylor_variant_valid, each next to its kernel there), not taken from the function under
test: a table that grows or loses a variant fails here until the census -- and tests/test_gpu_offset_variants.py, which must then
launch it -- is brought up to date."""
from __future__ import annotations

import ctypes as C
import threading

import pytest

from tests.util import (ADNORM, ASSIGN, CKPT, EVAP, NOLIN, OFF32, PARLIN, PERT, PRECISE, QSAT, SATLIN, SELFINC, TRAJ, VJP,  # noqa: F401
                        B, c2)

PEO = PRECISE | EVAP | OFF32
KMAX = B.lib.cloudsc2_batch_max()
WORDS = range(1024)


def _nl(f):  # nl_variant_valid, table of 128
    return f < 128 and (bool(f & EVAP) and not f & (PERT | NOLIN) if f & CKPT else not (f & NOLIN and f & PERT))


def _tl(f):  # tl_variant_valid, table of 256
    return f < 64 or (f < 256 and (f & ~PEO) == SATLIN)


def _ad(f):  # ad_variant_valid, table of 64
    return f < 64 and not f & ADNORM


def _ad_reverse(f):  # ad_reverse_variant_valid, table of 256
    if f >= 256:
        return False
    if f & SATLIN:
        return (f & ~PEO) == (SATLIN | ASSIGN | VJP)
    return (not f & ADNORM or (bool(f & ASSIGN) and not f & EVAP)) and (not f & VJP or (bool(f & ASSIGN) and not f & ADNORM))


def _batch(g):  # batch_kernel_valid: QSAT always, times PRECISE, EVAP, OFF32; the word is flags + 64 x directions
    f, k = g % 64, g // 64
    return bool(f & QSAT) and not f & ~(QSAT | PEO) and 2 <= k <= KMAX


def _parjac(f):  # parjac_variant_valid, table of 64
    return not f & ~(QSAT | PEO)


def _par(form):  # tl_par_variant_valid / vjp_par_variant_valid (par_variant_valid), tables of 512
    return lambda f: f < 512 and (f & ~PEO) in (PARLIN | form | QSAT, PARLIN | form | SATLIN)


def _taylor(f):  # taylor_variant_valid, table of 64
    return f < 64 and not f & (PERT | CKPT)


# family -> (name, validity, count).  The counts, by hand from the same expressions:
#   nl          CKPT: EVAP set, PERT and NOLIN clear, QSAT x PRECISE x OFF32 free = 8; no CKPT: 16 x the three of four PERT / NOLIN pairs = 48
#   tl          every word below 64, and SATLIN x PRECISE x EVAP x OFF32 = 8
#   ad          ADNORM clear: 32
#   ad_reverse  QSAT x PRECISE x OFF32 = 8 times { plain: EVAP x ASSIGN 4, ADNORM (ASSIGN, no EVAP) 1, VJP (ASSIGN, no ADNORM) x EVAP 2 },
#               and the SATLIN form x PRECISE x EVAP x OFF32 = 8
#   batched     8 flag words per direction count 2..KMAX
#   tl_parjac   QSAT x PRECISE x EVAP x OFF32 = 16;  tl_par, vjp_par  {QSAT, SATLIN} x PRECISE x EVAP x OFF32 = 16
#   taylor      QSAT x PRECISE x EVAP x OFF32 = 16
CENSUS = {
    0: ("nl", _nl, 8 + 48),
    1: ("tl", _tl, 64 + 8),
    2: ("ad", _ad, 32),
    3: ("ad_reverse", _ad_reverse, 8 * (4 + 1 + 2) + 8),
    4: ("tl_batch", _batch, 8 * (KMAX - 1)),
    5: ("vjp_batch", _batch, 8 * (KMAX - 1)),
    6: ("tl_parjac", _parjac, 16),
    7: ("tl_par", _par(0), 16),
    8: ("vjp_par", _par(ASSIGN | VJP), 16),
    9: ("taylor", _taylor, 16),
}


def expected_words(family: int) -> list:
    return [f for f in WORDS if CENSUS[family][1](f)]


def test_the_family_names_of_the_binding_are_the_census():
    assert B.FAMILIES == tuple(CENSUS[k][0] for k in sorted(CENSUS))


@pytest.mark.parametrize("family", sorted(CENSUS))
def test_census_of_built_variants(family):
    name, valid, count = CENSUS[family]
    built = [f for f in WORDS if B.lib.cloudsc2_variant_built(family, f) == 1]
    for f in WORDS:
        assert B.lib.cloudsc2_variant_built(family, f) in (0, 1), (name, f)
    assert len(expected_words(family)) == count, (name, "the restated expression and the count written next to it disagree")
    assert built == expected_words(family), (name, sorted(set(built) ^ set(expected_words(family))))
    assert len(built) == count, name
    # half of every family is the 64-bit form of the other half
    assert sorted(f | OFF32 for f in built if not f & OFF32) == [f for f in built if f & OFF32], name


def test_the_other_precision_ships_the_same_variants():
    """libcloudsc2_hip.so and libcloudsc2_hip_sp.so are the same tables over another cloudsc2_real: loaded side by side (the census
    needs no device), they answer alike for every family and word"""
    import os

    from tests.util import ROOT

    other = C.CDLL(os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "csrc", "libcloudsc2_hip.so" if B.SINGLE else "libcloudsc2_hip_sp.so"))
    other.cloudsc2_variant_built.argtypes = [C.c_int, C.c_uint]
    other.cloudsc2_variant_built.restype = C.c_int
    other.cloudsc2_real_bytes.restype = C.c_int
    assert other.cloudsc2_real_bytes() + B.lib.cloudsc2_real_bytes() == 12
    for family in CENSUS:
        assert [other.cloudsc2_variant_built(family, f) for f in WORDS] == [B.lib.cloudsc2_variant_built(family, f) for f in WORDS], family
    assert other.cloudsc2_variant_built(10, 1) == B.CLOUDSC2_EINVAL


def test_words_past_the_tables_and_unknown_families():
    for family in CENSUS:
        for f in (1024, 4096 + 1, 1 << 20, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFF):
            assert B.lib.cloudsc2_variant_built(family, f) == 0, (family, f)
    for family in (-1, 10, 11, 1 << 20, -(1 << 31)):
        assert B.lib.cloudsc2_variant_built(family, 1) == B.CLOUDSC2_EINVAL, family
        assert b"cloudsc2_variant_built" in B.lib.cloudsc2_last_error()
    # no direction count outside 2..KMAX, whatever the flag word
    for family in (4, 5):
        for k in (0, 1, KMAX + 1, 15):
            assert all(B.lib.cloudsc2_variant_built(family, f + 64 * k) == 0 for f in range(64)), (family, k)


def _log(n=B.LAUNCH_LOG_MAX):
    fam, word = (C.c_int * max(n, 1))(*([-7] * max(n, 1))), (C.c_uint * max(n, 1))(*([77] * max(n, 1)))
    return B.lib.cloudsc2_debug_launch_log(fam, word, n), list(fam), list(word)


def test_launch_log_argument_errors():
    B.launch_log_reset()
    fam, word = (C.c_int * 4)(), (C.c_uint * 4)()
    assert B.lib.cloudsc2_debug_launch_log(fam, word, -1) == B.CLOUDSC2_EINVAL
    assert b"cloudsc2_debug_launch_log" in B.lib.cloudsc2_last_error()
    assert B.lib.cloudsc2_debug_launch_log(None, word, 4) == B.CLOUDSC2_EINVAL
    assert B.lib.cloudsc2_debug_launch_log(fam, None, 4) == B.CLOUDSC2_EINVAL
    assert B.lib.cloudsc2_debug_launch_log(None, None, 0) == 0   # the count alone
    assert B.lib.cloudsc2_debug_launch_log(fam, word, 4) == 0
    assert B.launch_log() == []


def test_launch_log_stays_empty_when_a_launcher_refuses():
    """Only a kernel the runtime accepted is logged: a launcher that returns CLOUDSC2_EINVAL -- with or without a device -- or
    CLOUDSC2_ENODEVICE leaves the log as the reset left it, and the arrays of the caller untouched."""
    tab = c2.synthetic_table()
    prm = c2.default_params(c2.ceta_from_table(tab))
    i, o = B.Inputs(), B.Outputs()
    dummy = C.c_void_p(8)
    pp, nlev = C.byref(prm), prm.nlev
    K = (C.c_double * 4)(1.0, 0.0, 0.0, 0.0)
    arr_i, arr_o = (B.Inputs * 2)(), (B.Outputs * 2)()
    par_o = (B.Outputs * 4)()
    # every public sweep launcher with a wrong level count: CLOUDSC2_EINVAL before the device is looked for (check_geom), or -- the
    # parameter launchers, which look for the device first -- CLOUDSC2_ENODEVICE without one
    wrong = nlev - 1
    refused = {
        "nl": lambda n: B.lib.cloudsc2_nl_launch(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), B.Field(), 0.0, None),
        "tl": lambda n: B.lib.cloudsc2_tl_launch(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o), None),
        "tl_self": lambda n: B.lib.cloudsc2_tl_launch_self(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), 0.01, C.byref(o), None, None),
        "ad": lambda n: B.lib.cloudsc2_ad_launch(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o), dummy, None),
        "ad_assign": lambda n: B.lib.cloudsc2_ad_launch_assign(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o), dummy, None),
        "ad_forward": lambda n: B.lib.cloudsc2_ad_launch_forward(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), dummy, None),
        "ad_reverse": lambda n: B.lib.cloudsc2_ad_launch_reverse(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o), dummy, 1, None),
        "ad_reverse_norms": lambda n: B.lib.cloudsc2_ad_launch_reverse_norms(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o),
                                                                             dummy, dummy, None),
        "vjp": lambda n: B.lib.cloudsc2_vjp_launch(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o), dummy, None),
        "tl_satur": lambda n: B.lib.cloudsc2_tl_launch_satur(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(i), C.byref(o), None),
        "vjp_satur": lambda n: B.lib.cloudsc2_vjp_launch_satur(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), C.byref(i), C.byref(o), dummy, None),
        "tl_par": lambda n: B.lib.cloudsc2_tl_launch_par(pp, 3600.0, 32, n, 64, 1, C.byref(i), C.byref(i), K, C.byref(o), None),
        "vjp_par": lambda n: B.lib.cloudsc2_vjp_launch_par(pp, 3600.0, 32, n, 64, 1, C.byref(i), C.byref(o), C.byref(i), C.byref(o), dummy, dummy,
                                                           dummy, None),
        "tl_batch": lambda n: B.lib.cloudsc2_tl_launch_batch(pp, 3600.0, 32, n, 64, C.byref(i), 2, arr_i, arr_o, None),
        "vjp_batch": lambda n: B.lib.cloudsc2_vjp_launch_batch(pp, 3600.0, 32, n, 64, C.byref(i), C.byref(o), 2, arr_i, arr_o, dummy, None),
        "tl_parjac": lambda n: B.lib.cloudsc2_tl_launch_parjac(pp, 3600.0, 32, n, 64, C.byref(i), par_o, None),
        "taylor_sweep": lambda n: B.lib.cloudsc2_taylor_sweep_launch(pp, 3600.0, 32, n, 64, 32, C.byref(i), C.byref(o), C.byref(o), dummy, dummy, None),
    }
    have = c2.device_available()
    B.launch_log_reset()
    for name, call in refused.items():
        rc = call(wrong)
        if name in ("tl_par", "vjp_par") and not have:
            assert rc == B.CLOUDSC2_ENODEVICE, name
        else:
            assert rc == B.CLOUDSC2_EINVAL, (name, rc)
        assert _log() == (0, [-7] * B.LAUNCH_LOG_MAX, [77] * B.LAUNCH_LOG_MAX), name
    # a right level count and NULL fields: CLOUDSC2_ENODEVICE without a device, CLOUDSC2_EINVAL (a NULL field) with one
    for name, call in refused.items():
        rc = call(nlev)
        assert rc == (B.CLOUDSC2_EINVAL if have or name == "tl_parjac" else B.CLOUDSC2_ENODEVICE), (name, rc)
        assert B.launch_log() == [], name


def test_launch_log_is_per_thread():
    """a reset and a read on another thread are that thread's own (nothing can be launched here: what shows is that both calls work
    from a thread that never called the library before)"""
    seen = []

    def work():
        B.launch_log_reset()
        seen.append(_log(3))

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert seen == [(0, [-7] * 3, [77] * 3)]
