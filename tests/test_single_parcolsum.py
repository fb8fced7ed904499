"""The parameter column-sum sweep in the fp32 library: tests/test_gpu_autograd_parcolsum.py once more in a process with
CLOUDSC2_PRECISION=single, started the way tests/test_single.py starts its modules (one child, one time limit, no retry).  There the
sums launcher and ``param_jacobian_column_sums`` are held to the bits of the fold of the fp32 cloudsc2_tl_launch_parjac's planes, as in
fp64; the normal-equations comparisons are fp64 statements and are skipped in the child, which still runs the fp32 normal launcher
(finite sums, exact zeros, repeatable bits), the memory bound, graph capture and both addressing forms.
Measured on the MI355X: no element of any case differs from the fold in fp32 (worst case 0 units in the last place), so the fallback
bound of four times the parent route's error is not needed."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

from tests.util import ROOT


@pytest.mark.gpu
def test_single_parameter_column_sums_on_gpu():
    env = dict(os.environ, CLOUDSC2_PRECISION="single")
    try:
        p = subprocess.run([sys.executable, "-m", "pytest", os.path.join("tests", "test_gpu_autograd_parcolsum.py"), "-q", "-s", "-p",
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
    assert text.count("0 elements differ from the fold") >= 8 * 2 * 3, "the sums-form cases did not all run"
    assert "skipped" in last, "the normal-equations comparisons are fp64-only"
