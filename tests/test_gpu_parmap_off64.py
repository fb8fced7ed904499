"""The parameter-map sweeps with 64-bit offsets: tests/test_gpu_autograd_parmap.py once more in a process with CLOUDSC2_OFF32=0 (read
once per process), started the way tests/test_single_parcolsum.py starts its module: one child, one time limit, no retry.  The small
shapes of that module take the 32-bit byte offsets (C2F_OFF32) by default; here every launch of it runs the other addressing form of
the same kernels, held to the same bits."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

from tests.util import ROOT


@pytest.mark.gpu
def test_parameter_maps_with_64_bit_offsets_on_gpu():
    env = dict(os.environ, CLOUDSC2_OFF32="0")
    try:
        p = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_autograd_parmap.py"), "-q", "-s", "-p",
                            "no:cacheprovider", "-m", "gpu"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        rc, text, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:
        rc, text, err = 124, f"time limit: {e}", ""
    lines = text.splitlines()
    print("\n".join(ln for ln in lines if "elements differ" in ln))
    print("\n".join(lines[-10:]))
    assert rc == 0, (rc, text[-6000:], err[-2000:])
    last = lines[-1] if lines else ""
    assert " passed" in last and "failed" not in last and "error" not in last, last
