"""The C-ABI library loads, exports every symbol include/cloudsc2_hip.h declares, and its host-only entry points
behave like the reference (no compute calls here: there is no GPU in this container)."""
from __future__ import annotations

import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from tests.util import ROOT, B, c2


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "cloudsc2_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(cloudsc2_[a-z0-9_]+)\s*\(", hdr)))


def test_every_declared_symbol_is_exported():
    syms = declared_symbols()
    assert set(syms) == set(B.EXPORTED)
    for s in syms:
        assert hasattr(B.lib, s), s


def test_io_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "cloudsc2_io.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    syms = sorted(set(re.findall(r"\b(cloudsc2_[a-z0-9_]+)\s*\(", hdr)))
    assert "cloudsc2_file_open" in syms and "cloudsc2_file_read_params" in syms
    from dwarf_p_cloudsc2_tl_ad_amd import fileio

    lib = fileio._lib()
    for s in syms:
        assert hasattr(lib, s), s


def test_params_struct_layout_and_defaults():
    assert C.sizeof(B.Params) == 30 * 8 + 6 * 4 + 200 * 8
    p = c2.default_params()
    # the derived YOETHF constants
    assert p.r5les == p.r3les * (p.rtt - p.r4les) and p.r5alvcp == p.r5les * p.rlvtt / p.rcpd
    assert p.rlmlt == p.rlstt - p.rlvtt and p.rvtmp2 == 0.0 and p.lphylin == 1
    assert abs(p.rlptrc - 266.42345) < 1e-4
    assert p.rlstt == 2834500.0  # confirmed by config-files/reference.h5 (tests/test_oracle.py)


def test_verdicts_follow_the_reference_drivers():
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "drivers.json")))["drivers"]
    for key, want_pen in (("tl_nproma32_ngptot100", 0), ("tl_nproma1_ngptot100", 5)):
        ok, itest = c2.taylor_verdict(gold[key]["znormg"])
        assert ok and itest == want_pen
        assert gold[key]["verdict"].startswith("TEST PASSED") and gold[key]["verdict"].endswith(str(want_pen))
    # no lambda <= 1e-4 gets within 0.5: err 13 (cloudsc_driver_tl_mod.F90:285-286)
    assert c2.taylor_verdict([3.0] * 4 + [1.0] * 6) == (False, 13)
    # monotone convergence without the V turn: ITEST = 11 (:300)
    assert c2.taylor_verdict([1.0 + 10.0 ** (-k) for k in range(1, 11)])[1] in (11, 11 + 0)
    assert c2.adjoint_verdict(9999.0) and not c2.adjoint_verdict(10000.0)


def test_compute_entry_points_fail_loudly_without_a_gpu():
    if c2.device_available():
        pytest.skip("a GPU is present")
    tab = c2.synthetic_table()
    prm = c2.default_params(c2.ceta_from_table(tab))
    st = c2.state_from_table(tab, 32, 64)
    for which in ("nl", "tl", "ad"):
        with pytest.raises(c2.Cloudsc2Error) as e:
            c2.run_state(prm, st, which)
        assert e.value.code == B.CLOUDSC2_ENODEVICE
        assert "no CPU path" in str(e.value)
    # kernel-level entry points (host pointers are never dereferenced: the device check comes first)
    i, o = B.Inputs(), B.Outputs()
    dummy = C.c_void_p(8)
    launches = {
        "cloudsc2_nl_launch": lambda: B.lib.cloudsc2_nl_launch(C.byref(prm), 3600.0, 32, prm.nlev, 64, C.byref(i), C.byref(o), B.Field(), 0.0, None),
        "cloudsc2_tl_launch_self": lambda: B.lib.cloudsc2_tl_launch_self(C.byref(prm), 3600.0, 32, prm.nlev, 64, C.byref(i), C.byref(o), 0.01, C.byref(o), None, None),
        "cloudsc2_ad_launch_reverse_norms": lambda: B.lib.cloudsc2_ad_launch_reverse_norms(C.byref(prm), 3600.0, 32, prm.nlev, 64, C.byref(i), C.byref(o),
                                                                                          C.byref(i), C.byref(o), dummy, dummy, None),
        "cloudsc2_taylor_sweep_launch": lambda: B.lib.cloudsc2_taylor_sweep_launch(C.byref(prm), 3600.0, 32, prm.nlev, 64, 32, C.byref(i), C.byref(o),
                                                                                  C.byref(o), dummy, dummy, None),
    }
    for name, call in launches.items():
        assert call() == B.CLOUDSC2_ENODEVICE, name
        assert b"no CPU path" in B.lib.cloudsc2_last_error(), name


def test_state_layout_and_tiling():
    tab = c2.synthetic_table()
    st = c2.state_from_table(tab, 32, 250)
    assert st.nblocks == 8 and st.PT.shape == (8, 137, 32) and st.PAPH.shape == (8, 138, 32)
    cols = st.PT.transpose(0, 2, 1).reshape(-1, 137)
    assert np.array_equal(cols[:250], tab["PT"].T[np.arange(250) % 100])  # periodic tiling, expand_mod.F90:283-296
    assert not cols[250:].any()                                           # zero-padded tail (:299)
    assert np.array_equal(st.B_CML[:, 2].transpose(0, 2, 1).reshape(-1, 137)[:100], tab["TENDENCY_CML_Q"].T)
    # a rank's sub-range continues the same periodic sequence (dwarf_cloudsc.F90:66-69)
    a, b = c2.column_range(250, 1, 2)
    assert (a, b) == (125, 250)
    st1 = c2.state_from_table(tab, 32, b - a, col0=a)
    assert np.array_equal(st1.PT.transpose(0, 2, 1).reshape(-1, 137)[: b - a], cols[a:b])
    assert c2.bytes_per_column(137, "nl") == 27440 and c2.bytes_per_column(137, "tl") == 57072
    assert c2.bytes_per_column(137, "ad") == 85608


def test_bench_cpu_baseline_leg_runs():
    """bench.py's cpu_baseline leg (the reference, or the C port, timed on the host cores) on a small sample."""
    import bench

    from tests.util import c2

    tab = c2.synthetic_table()
    prm = c2.default_params(c2.ceta_from_table(tab))
    cb = bench.cpu_baseline(tab, prm, 32, 2000, budget_s=0.5)
    assert cb is not None and cb["unit"] == "columns/s" and cb["kind"] in ("reference", "port")
    assert cb["value"] > 0 and cb["numomp4_value"] > 0 and cb["cores"] >= 1


def test_device_state_layout_matches_state_take_in_cloudsc2_driver_hip():
    """DeviceState.ORDER is the order in which the arrays are carved out of the state's allocation; it has to be the library's own
    (csrc/cloudsc2_driver.hip: state_take), because cloudsc2_device_malloc_state judges its candidates by running the NL sweep on a
    state laid out that way: read-only arrays first, then everything the sweeps write."""
    import re

    from dwarf_p_cloudsc2_tl_ad_amd.driver import DeviceState

    names = set(DeviceState.FULL) | set(DeviceState.HALF) | {"B_CML", "B_LOC", "PCLV", "QSAT"}
    assert len(DeviceState.ORDER) == len(set(DeviceState.ORDER)) == len(names) and set(DeviceState.ORDER) == names
    written = [n for n in DeviceState.ORDER if n in DeviceState.WRITTEN or n == "QSAT"]
    assert DeviceState.ORDER[-len(written):] == tuple(written)  # what the sweeps write lies at the end of the allocation
    src = open(os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "csrc", "cloudsc2_driver.hip")).read()
    body = src[src.index("void state_take("):]
    body = body[:body.index("\n}\n")]
    lib_order = [m.upper() for m in re.findall(r"d\.(\w+) = a(?:in|out)\.take", body)]
    assert lib_order == [n.upper() for n in DeviceState.ORDER], (lib_order, DeviceState.ORDER)


def test_a_plain_c_caller_compiles_and_links_against_the_abi(tmp_path):
    """The boundary is a C ABI: every header under include/ must be valid C99 on its own (no C++-isms, no torch types), and a C
    program must link against the shared library and get the reference drivers' verdicts and the no-device error from it."""
    import glob
    import subprocess

    csrc = os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "csrc")
    libname = "cloudsc2_hip_sp" if B.SINGLE else "cloudsc2_hip"
    src = tmp_path / "caller.c"
    src.write_text("".join(f'#include "{os.path.basename(h)}"\n' for h in sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))) + r"""
#include <stdio.h>
int main(void) {
    cloudsc2_params p;
    double z[10];
    int itest = -1, k, ok;
    cloudsc2_params_default(&p);
    for (k = 0; k < 10; ++k) z[k] = 1.0 + 1e-7;           /* ratios this close to one at every lambda: PASSED, penalty 0 */
    ok = cloudsc2_taylor_verdict(z, &itest);
    printf("%d %d %d %d\n", ok, itest, cloudsc2_adjoint_verdict(100.0), cloudsc2_adjoint_verdict(1.0e6));
    return 0;
}
""")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror"] + (["-DCLOUDSC2_SINGLE"] if B.SINGLE else []) +
                   ["-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", csrc, f"-l{libname}", f"-Wl,-rpath,{csrc}"],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "1" and out[2] == "1" and out[3] == "0", out   # PASSED; 100 x eps is TEST OK, 1e6 x eps is not


def test_the_pacing_rule_of_partial_rounds():
    """cloudsc2_pace_plan (pure arithmetic behind the TL / AD launchers, include/cloudsc2_hip.h): paced = two to eight whole rounds of
    workgroups plus a partial one that fills at most half of the slots.  MI355X at one wave per SIMD has 512 slots of 128 threads."""
    import ctypes as C

    def plan(columns, slots=512):
        k, first, recip = C.c_int(), C.c_int(), C.c_int()
        on = B.lib.cloudsc2_pace_plan((columns + 127) // 128, slots, C.byref(k), C.byref(first), C.byref(recip))
        return on, k.value, first.value, recip.value

    assert plan(160000) == (1, 2, 226, 32768)         # BASELINE's size: 1250 workgroups = 2 rounds + 226; nap = 1/2 of a level
    assert plan(140000) == (1, 2, 70, 32768)
    assert plan(200000) == (1, 3, 27, 21845)
    assert plan(400000)[:3] == (1, 6, 53)
    assert plan(100000)[0] == 0 and plan(100000)[1] == 1   # one whole round: measured slower with the pacing
    assert plan(180000)[0] == 0                             # the partial round fills 75 % of the slots
    assert plan(131072)[0] == 0                             # exactly two rounds: nothing partial
    assert plan(1048576)[0] == 0                            # 16 rounds: nothing to gain
    assert plan(16384)[0] == 0 and plan(160000, 0)[0] == 0


def test_the_simd_population_rule_of_one_round_launches():
    """cloudsc2_simd_population (pure arithmetic behind the NL launcher's light-SIMD nap): 160 000 columns = 1250 blocks on 256 CUs: 226
    CUs carry five blocks = ten waves -- two SIMDs with three, two with two --, 30 carry four (two waves on every SIMD)."""
    import ctypes as C

    def pop(block, wave, wgs=1250, cus=256):
        a, b = C.c_int(), C.c_int()
        B.check(B.lib.cloudsc2_simd_population(wgs, cus, block, wave, C.byref(a), C.byref(b)))
        return a.value, b.value

    for c in (0, 100, 225):  # a five-block CU: blocks c, c+256, ... c+1024; the first block's two SIMDs end up with three waves
        got = [pop(c + 256 * j, w) for j in range(5) for w in (0, 1)]
        assert got == [(3, 3), (3, 3), (3, 3), (2, 3), (2, 3), (2, 3), (2, 3), (3, 3), (3, 3), (3, 3)], got
    for c in (226, 255):     # a four-block CU: all equal
        assert all(pop(c + 256 * j, w) == (2, 2) for j in range(4) for w in (0, 1))
    heavy = sum(pop(b, w)[0] == 3 for b in range(1250) for w in (0, 1))
    assert heavy == 1356  # = 452 SIMDs x 3 waves (profiles/r03_wave_times.txt)
    assert B.lib.cloudsc2_simd_population(1250, 256, 1250, 0, C.byref(C.c_int()), C.byref(C.c_int())) != 0


def test_the_synthetic_table_has_one_implementation():
    """cloudsc2_synthetic_table (host code in the library) is what every front end loads when input.h5 is absent: the Python side
    returns its arrays unchanged, the recipe's invariants hold, and the numpy-flavoured fixture (rounds 1-4's table, on which the
    reference's Taylor test fails at NPROMA 32: tests/golden/drivers.json) differs from it in the last place only."""
    import json

    tab = c2.synthetic_table()
    names = ("PT", "PQ", "PAP", "PAPH", "PLU", "PLUDE", "PMFU", "PMFD", "PCLV_QL", "PCLV_QI", "TENDENCY_CML_T", "TENDENCY_CML_Q")
    arr = {n: np.zeros((137 + (n == "PAPH"), 100)) for n in names}
    dp = C.POINTER(C.c_double)
    B.check(B.lib.cloudsc2_synthetic_table(100, 137, 287.0597, 461.5250, 273.16, *[arr[n].ctypes.data_as(dp) for n in names]))
    for n in names:
        assert np.array_equal(tab[n], arr[n]), n
    assert np.all(np.diff(tab["PAPH"], axis=0) > 0) and np.allclose(tab["PAP"], 0.5 * (tab["PAPH"][:-1] + tab["PAPH"][1:]), rtol=1e-15)
    assert tab["PT"].min() >= 205.0 and tab["PQ"].min() > 0 and np.all(tab["PCLV_QL"] > 0) and np.all(tab["PCLV_QI"] >= 0)
    assert np.any(tab["PLU"] > 0) and np.all(tab["PMFD"] <= 0) and not np.any(tab["PA"]) and not np.any(tab["PSUPSAT"])
    assert B.lib.cloudsc2_synthetic_table(0, 137, 287.0597, 461.5250, 273.16, *[arr[n].ctypes.data_as(dp) for n in names]) != 0
    z = np.load(os.path.join(ROOT, "tests", "golden", "table_numpy.npz"))
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "drivers.json")))["fixtures"]["table_numpy"]
    assert sorted(z.files) == sorted(meta["fields_that_differ_from_cloudsc2_synthetic_table"]) and "PQ" in z.files
    for n in z.files:
        rel = np.max(np.abs(z[n] - tab[n]) / np.abs(tab[n]))
        assert 0.0 < rel < 2e-14, (n, rel)
