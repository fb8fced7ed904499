"""Real-data readiness, pinned mechanically.

`config-files/input.h5` is not distributed with the reference checkout (`.MISSING_LARGE_BLOBS`), so the NL comparison with
`config-files/reference.h5` cannot run yet.  What CAN be pinned today is that the day the file appears nothing has to be
edited: the loaders of this build (csrc/cloudsc2_io.cpp `kScalars`, fileio.py, fortran/cloudsc2_hip_state_mod.F90) ask the file
for exactly the dataset names -- and shapes -- the reference's own loader asks for, restricted to what the hot path reads.

The expectation is EXTRACTED from the reference's sources as text (study, not execution; only dataset names and shapes are kept,
in tests/golden/reference_loaders.json, written by tests/golden/extract_reference_loaders.py):
  * every `LOAD_SCALAR('<dataset>', <variable>)` of yomcst.F90 / yoethf.F90 / yoecldp.F90 / yoephli.F90,
  * of those, the ones whose variable is READ by the hot path: the executable statements of satur / cuadjtqs / cloudsc2 /
    cuadjtqstl / cloudsc2tl / cuadjtqsad / cloudsc2ad plus the statement functions of fcttre*.func.h they reach (transitively),
  * every `LOAD_AND_EXPAND('<dataset>', ...)` of CLOUDSC2_ARRAY_STATE_LOAD (cloudsc2_array_state_mod.F90:164-199) and the four
    dataset suffixes of LOAD_AND_EXPAND_STATE (expand_mod.F90:151-154), with the level count each is read with.
CPU-only."""
from __future__ import annotations

import json
import os
import re

from tests.util import ROOT

LOADERS = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_loaders.json")))


def test_the_scalar_datasets_asked_for_are_exactly_what_the_hot_path_reads():
    loaded = LOADERS["loaded_scalars"]
    assert len(loaded) > 150 and loaded["RG"] == "RG" and loaded["YRECLDP_RCLCRIT"] == "YRECLDP%RCLCRIT"
    need = set(LOADERS["hot_path_scalars"])
    # YREPHLI%LPHYLIN is loaded and then overwritten by every main before the first kernel call (dwarf_cloudsc.F90:106-107 of
    # cloudsc2_nl / _tl / _ad: "overload LPHYLIN"): a flag of cloudsc2_params (lphylin, default 1), not a dataset this build reads
    assert LOADERS["lphylin_overloaded_by_every_main"]
    need.discard("YREPHLI_LPHYLIN")
    io = open(os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "csrc", "cloudsc2_io.cpp")).read()
    asked = re.findall(r'\{"(\w+)",\s*&cloudsc2_params::(\w+)\}', io)
    names = [a for a, _ in asked]
    assert len(names) == len(set(names))
    assert set(names) == need, (sorted(set(names) - need), sorted(need - set(names)))
    # and each lands in the parameter of the same name (RCLCRIT <- YRECLDP_RCLCRIT, RLPTRC <- YREPHLI_RLPTRC, RG <- RG ...)
    for ds, field in asked:
        assert ds.split("_", 1)[1].lower() == field if ds.startswith(("YRECLDP_", "YREPHLI_")) else ds.lower() == field, (ds, field)
    # the scalars of the state loader itself (cloudsc2_array_state_mod.F90:162-163,193)
    for ds in ("KLON", "KLEV", "PTSPHY"):
        assert f'"{ds}"' in io, ds


def test_the_field_datasets_asked_for_are_the_reference_loaders():
    want = {n: tuple(v) for n, v in LOADERS["field_datasets"].items()}
    assert set(want) == {"PT", "PQ", "PAP", "PAPH", "PLU", "PLUDE", "PMFU", "PMFD", "PA", "PCLV", "PSUPSAT", "TENDENCY_CML_T",
                         "TENDENCY_CML_A", "TENDENCY_CML_Q", "TENDENCY_CML_CLD"}, sorted(want)
    assert want["PAPH"] == ("KLEV+1", 1) and want["PCLV"] == ("KLEV", 5) and want["TENDENCY_CML_CLD"] == ("KLEV", 5)
    # the Python loader
    from dwarf_p_cloudsc2_tl_ad_amd import fileio

    py = open(fileio.__file__).read()
    asked_py = set(fileio.INPUT_FIELDS_2D) | set(re.findall(r'f\.read\("(\w+)"\)', py[py.index("def read_input_file"):py.index("def reference_table_from_state")]))
    assert asked_py == set(want), (sorted(asked_py ^ set(want)))
    # the Fortran loader of the mains (both the host-array and the device-resident path ask for every dataset)
    f90 = open(os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "fortran", "cloudsc2_hip_state_mod.F90")).read()
    tables = re.findall(r"READ_TABLE\(F,\s*'(\w+)',\s*(TABH?)\)", f90)
    bulk = re.findall(r"CLOUDSC2_FILE_READ_REAL\(F,\s*'(\w+)'//C_NULL_CHAR,\s*TAB3", f90)
    for path in (0, 1):  # the two LOAD variants list the datasets in the same order: first half, second half
        half = len(tables) // 2
        asked = {n for n, _ in tables[path * half:(path + 1) * half]} | set(bulk)
        assert asked == set(want), (path, sorted(asked ^ set(want)))
    for n, buf in tables:  # half-level datasets go through the (KLON, KLEV+1) buffer
        assert (buf == "TABH") == (want[n][0] == "KLEV+1"), n
    for n in bulk:
        assert want[n][1] == 5, n


def test_the_reference_file_datasets_compared_are_the_validators():
    """VALIDATE (cloudsc2_array_state_mod.F90:246-256) compares these ten datasets of reference.h5; WRITE_REFERENCE (:275-284)
    writes them.  The checkout's reference.h5 holds them with the shapes this build reads (tests/test_fileio.py reads the file)."""
    written = set(LOADERS["reference_file_datasets"])
    from dwarf_p_cloudsc2_tl_ad_amd import fileio

    assert written == set(fileio.REFERENCE_FIELDS), sorted(written ^ set(fileio.REFERENCE_FIELDS))
    f90 = open(os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "fortran", "cloudsc2_hip_state_mod.F90")).read()
    checked = set(re.findall(r"CALL CHECK2\('(\w+)'", f90)) | set(re.findall(r"CLOUDSC2_FILE_READ_REAL\(F,\s*'(TENDENCY_LOC_\w+)'", f90))
    assert checked == written, sorted(checked ^ written)
