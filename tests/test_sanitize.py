"""AddressSanitizer over the per-column sweeps, on the CPU build (GPU sanitizers are not available on the pool): the
device functions of csrc/cloudsc2_level.hpp + cloudsc2_column.hpp compiled for the host with -fsanitize=address and
driven by the same checks as tests/test_hostcheck.py (fp64) and tests/single_checks.py (fp32), in child processes that
preload the sanitizer runtime.  numpy's buffers come from the intercepted malloc, so any load or store of a sweep that
leaves its plane -- lane offsets, level offsets, the 32-bit byte-offset variants, the checkpoint plane -- aborts."""
from __future__ import annotations

import os
import subprocess
import sys

import pytest

from tests.util import HOSTCHECK_DIR, ROOT

HIPCC = "/opt/rocm/bin/hipcc"


def _asan_runtime():
    try:
        p = subprocess.run(["/opt/rocm/lib/llvm/bin/clang", "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True,
                           text=True, timeout=60).stdout.strip()
    except (OSError, subprocess.SubprocessError):
        return None
    return p if os.path.isabs(p) and os.path.exists(p) else None


def _build(single: bool) -> str:
    lib = os.path.join(HOSTCHECK_DIR, "libhostcheck_asan_sp.so" if single else "libhostcheck_asan.so")
    src = os.path.join(HOSTCHECK_DIR, "hostcheck.hip")
    deps = [src] + [os.path.join(ROOT, "dwarf_p_cloudsc2_tl_ad_amd", "csrc", f) for f in ("cloudsc2_level.hpp", "cloudsc2_column.hpp")]
    if (not os.path.exists(lib)) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        # host code only: --cuda-host-only builds no device code, and -fno-gpu-sanitize keeps the sanitizer off the device side
        subprocess.check_call([HIPCC, "--cuda-host-only", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address", "-fno-gpu-sanitize",
                               "-shared-libasan", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17"] +
                              (["-DCLOUDSC2_SINGLE"] if single else []) + ["-o", lib, src])
    return lib


@pytest.mark.parametrize("single", [False, True], ids=["fp64", "fp32"])
def test_column_sweeps_under_address_sanitizer(single):
    rt = _asan_runtime()
    if rt is None:
        pytest.skip("no AddressSanitizer runtime in this toolchain")
    if single and not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libcloudsc2_ref_sp.so")):
        pytest.skip("oracle/_ref/libcloudsc2_ref_sp.so not built")
    # the sanitizer runtime must come first; whatever the environment already preloads stays behind it
    preload = ":".join(p for p in (rt, os.environ.get("LD_PRELOAD", "")) if p)
    env = dict(os.environ, CLOUDSC2_HOSTCHECK_LIB=_build(single), LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               CLOUDSC2_PRECISION="single" if single else "double")
    cmd = ([sys.executable, os.path.join(ROOT, "tests", "single_checks.py"), "host"] if single else
           [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_hostcheck.py"), "-x", "-q", "-p", "no:cacheprovider"])
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    out = p.stdout + p.stderr
    assert "AddressSanitizer" not in out, out[-4000:]
    assert p.returncode == 0, out[-4000:]
