"""csrc/cloudsc2_fields.hpp -- the one table of the 16 input and 10 output fields, resolve_in / resolve_out, writable, outputs_given and
ncols_pad -- has no device dependency, so it is checked directly: tests/hostcheck/fields_check.cpp is a program of its own (its own
main, its own fail()), built here for the host and run, in both precisions, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (the header walks the argument blocks as arrays of fields and of pointers: this is where that is exercised)."""
from __future__ import annotations

import os
import subprocess

import pytest

from tests.util import HIPCC, HOSTCHECK_DIR

SRC = os.path.join(HOSTCHECK_DIR, "fields_check.cpp")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("prec", ["dp", "sp"])
def test_the_field_table_by_its_own_program(tmp_path, prec, sanitize):
    exe = str(tmp_path / "fields_check")
    cmd = [HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function"]
    cmd += ["-DCLOUDSC2_SINGLE"] if prec == "sp" else []
    cmd += ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    r = subprocess.run(cmd + ["-o", exe, SRC], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (" ".join(cmd), r.stderr[-3000:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "0 failed" in r.stdout and not r.stderr, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
