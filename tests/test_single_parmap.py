"""``cloudsc2_param_maps`` in the fp32 library: tests/test_gpu_autograd_parmap.py once more in a process with
CLOUDSC2_PRECISION=single, started the way tests/test_single_parcolsum.py starts its module (one child, one time limit, no retry).
There outputs, field gradients, the group sums of the map gradients and the replay of a captured forward + ``autograd.grad`` are held
to the bits of the fp32 scalar-parameter op, as in fp64.  The output tangents under tangent maps miss those bits on the gfx950 build in
some planes; for them the child needs the fp64 library's scalar-route tangents on the same inputs, which this (fp64) process computes
first and hands over as a file: those planes are held to 4 x the error the fp32 scalar-parameter op itself has against the fp64 one --
the project's factor for the fp32 library, measured on the scalar route and never on the new code.
Measured on the MI355X, with every field and parameter tangent given, worst over the three cases, in units in the last place of the
field's maximum (largest difference / smallest bound): tent 0.41 / 203.6, tenq 0.10 / 201.4, tenl 0.27 / 1236.3, teni 2.90 / 586.3,
fplsl 0.67 / 68.6, fplsn 0.32 / 119.2, fhpsl 1.13 / 68.7, fhpsn 0.47 / 119.2; clc and covptot, and every plane of the six cases with one
parameter's tangent map alone, are the bits."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import B, ROOT


@pytest.mark.gpu
def test_single_parameter_maps_on_gpu(tmp_path):
    env = dict(os.environ, CLOUDSC2_PRECISION="single")
    if not B.SINGLE:  # the fp64 scalar route's tangents of every jvp case of the module
        import torch

        from tests import test_gpu_autograd_parmap as m

        ref = {}
        for case in m.CASES:
            for only in (None,) + (m.ONE_PARAMETER if case in m.CASES[:2] else ()):
                _, wants = m.scalar_route_tangents(case, only)
                for n, w in zip(B.OUT_NAMES, wants):
                    ref[m.reference_key(case, only, n)] = w.cpu().numpy()
        torch.cuda.synchronize()
        path = str(tmp_path / "fp64_tangents.npz")
        np.savez(path, **ref)
        env[m.REFERENCE_ENV] = path
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
    assert B.SINGLE or text.count("4 x the fp32 scalar route's error") >= 8 * 3, "the fp32 bound was not applied: no fp64 reference reached the child"
