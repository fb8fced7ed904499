"""The host build of the three parameter-map sweeps under the host sanitizers, as a stand-alone program (its own ``main``, no Python in
the process, nothing preloaded): tests/hostcheck/parmap_asan_main.cpp compiled with ``-fsanitize=address,undefined`` and run directly.
Every table (values, tangents, adjoints) and every plane is a ``malloc`` of exactly its extent and every absent one a NULL pointer, for
the four flag sets x qsat given / SATUR in the sweep x fast / precise at NPROMA 8, NLEV 137, NGPTOT 12.  Passes on exit 0 with no
sanitizer report."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np
import pytest

from tests.hostbuild import SANITIZED_EXE_FLAGS, build
from tests.util import B, HOSTCHECK_DIR, c2, host_qsat, increments_of, make_params, sanitizer_runtimes

FLAGSETS = (dict(), dict(levapls2=True, lregcl=True), dict(ldrain1d=True), dict(lregcl=True))


def test_parameter_map_sweeps_under_the_host_sanitizers(tmp_path):
    if not sanitizer_runtimes():
        pytest.skip("no AddressSanitizer / UndefinedBehaviorSanitizer runtime in this toolchain")
    exe = build(os.path.join(HOSTCHECK_DIR, "parmap_asan_main.cpp"), os.path.join(HOSTCHECK_DIR, "parmap_asan_main" + ("_sp" if B.SINGLE else "")),
                flags=SANITIZED_EXE_FLAGS)
    nproma, nlev, ngptot = 8, 137, 12
    tab = c2.random_table(nlev, 30, seed=11)
    st = c2.state_from_table(tab, nproma, ngptot)
    planes = {n: a * B.REAL(100.0) for n, a in increments_of(st, host_qsat(st)).items()}  # (the 16 inputs as flat planes)
    case_file = tmp_path / "cases.bin"
    with open(case_file, "wb") as f:
        f.write(struct.pack("4i", nproma, nlev, ngptot, len(FLAGSETS)))
        for flags in FLAGSETS:
            f.write(bytes(make_params(tab, **flags)))
            f.write(struct.pack("d", float(st.ptsphy)))
        for n in B.IN_NAMES:
            a = np.ascontiguousarray(planes[n], dtype=B.REAL)
            assert a.shape == (st.nblocks, nlev + (1 if n == "paph" else 0), nproma)
            f.write(a.tobytes())
    # (the sanitizer runtimes are linked into the executable: it runs in the environment as it is)
    r = subprocess.run([exe, str(case_file)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "16 runs of the three sweeps: every active element written, every padded tail untouched" in r.stdout
