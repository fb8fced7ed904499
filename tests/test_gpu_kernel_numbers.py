"""The numbering of cloudsc2_kernel_occupancy, whole: the `kernel` column of the table of variant tables (csrc/cloudsc2_sweep_kernels.hpp)
as the registry of cloudsc2_policy.hip serves it.  Nothing is launched: the runtime is asked for the occupancy of one kernel per number."""
from __future__ import annotations

import ctypes as C

import pytest

from tests.util import ASSIGN, PARLIN, QSAT, VJP, B

pytestmark = pytest.mark.gpu


def test_kernel_occupancy_knows_kernels_0_to_6_and_10_to_14_and_no_other():
    per_cu = C.c_int(0)

    def ask(kernel, word):
        per_cu.value = -1
        return B.lib.cloudsc2_kernel_occupancy(kernel, word, C.byref(per_cu))

    two = 64 * 2  # the batched tables' word: flags + 64 x directions
    built = {0: 0, 1: QSAT, 2: QSAT, 3: QSAT, 4: QSAT + two, 5: QSAT + two, 6: QSAT,
             B.CLOUDSC2_KERNEL_TL_SPARSE: QSAT, B.CLOUDSC2_KERNEL_VJP_SPARSE: QSAT, B.CLOUDSC2_KERNEL_NL_COLSUM: 0,
             B.CLOUDSC2_KERNEL_TL_COLSUM: QSAT, B.CLOUDSC2_KERNEL_VJP_COLSUM: QSAT}
    assert sorted(built) == [0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14]
    for kernel, word in built.items():
        B.check(ask(kernel, word))
        assert 1 <= per_cu.value <= 8, (kernel, word, per_cu.value)
    # families 7, 8, 9 have a number in cloudsc2_variant_built and the launch log, none here: refused for a word they do build
    for family, word in ((7, PARLIN | QSAT), (8, PARLIN | ASSIGN | VJP | QSAT), (9, QSAT)):
        assert B.lib.cloudsc2_variant_built(family, word) == 1
        assert ask(family, word) == B.CLOUDSC2_EINVAL, family
        assert b"cloudsc2_kernel_occupancy" in B.lib.cloudsc2_last_error() and per_cu.value == -1
    for kernel in (15, 16, -1):
        assert ask(kernel, QSAT) == B.CLOUDSC2_EINVAL, kernel
    # the sparse and the TL / VJP column-sum tables hold QSAT or SATLIN forms only; the NL column-sum sweep evaluates SATUR itself
    for kernel in (B.CLOUDSC2_KERNEL_TL_SPARSE, B.CLOUDSC2_KERNEL_VJP_SPARSE, B.CLOUDSC2_KERNEL_TL_COLSUM, B.CLOUDSC2_KERNEL_VJP_COLSUM):
        assert ask(kernel, 0) == B.CLOUDSC2_EINVAL, kernel
    assert B.lib.cloudsc2_variant_built(10, QSAT) == B.CLOUDSC2_EINVAL  # family 10 stays no family
