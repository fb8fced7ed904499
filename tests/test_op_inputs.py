"""state.op_inputs / op_outputs: the one mapping from a state's arrays to the differentiable op's names.  The mapping is written out a
second time here, with literal plane numbers, which is where a second copy belongs."""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from tests.util import B, c2, refcall
from dwarf_p_cloudsc2_tl_ad_amd import autograd as ag

NPROMA, NGPTOT = 32, 250  # 8 blocks, the last with 26 active columns and a padded tail


def inputs_by_hand(st) -> dict:
    return {"paph": st.PAPH, "pap": st.PAP, "q": st.PQ, "t": st.PT, "l": st.PCLV[:, 0], "i": st.PCLV[:, 1], "lude": st.PLUDE,
            "lu": st.PLU, "mfu": st.PMFU, "mfd": st.PMFD, "gtent": st.B_CML[:, 0], "gtenq": st.B_CML[:, 2], "gtenl": st.B_CML[:, 3],
            "gteni": st.B_CML[:, 4], "supsat": st.PSUPSAT}


def outputs_by_hand(st) -> dict:
    return {"tent": st.B_LOC[:, 0], "tenq": st.B_LOC[:, 2], "tenl": st.B_LOC[:, 3], "teni": st.B_LOC[:, 4], "clc": st.PA,
            "fplsl": st.PFPLSL, "fplsn": st.PFPLSN, "fhpsl": st.PFHPSL, "fhpsn": st.PFHPSN, "covptot": st.PCOVPTOT}


@pytest.fixture(scope="module")
def st():
    st = c2.state_from_table(c2.synthetic_table(), NPROMA, NGPTOT)
    rng = np.random.default_rng(3)  # the outputs and the planes the table leaves zero: every plane its own values
    for a in (st.B_CML, st.B_LOC, st.PCLV, st.PA, st.PSUPSAT, st.PCOVPTOT, st.PFPLSL, st.PFPLSN, st.PFHPSL, st.PFHPSN):
        a[...] = rng.standard_normal(a.shape).astype(a.dtype)
    return st


def views_of(got: dict, want: dict):
    """every value is the hand-made slice of its state array: the same memory, not a copy"""
    for n, a in got.items():
        assert np.shares_memory(a, want[n]) and a.ctypes.data == want[n].ctypes.data and a.strides == want[n].strides, n
        assert np.array_equal(a, want[n]), n


def test_inputs_without_qsat_are_the_15_views(st):
    x = c2.op_inputs(st)
    assert list(x) == list(ag.SAT_NAMES)
    views_of(x, inputs_by_hand(st))
    qsat = np.zeros_like(st.PAP)
    x = c2.op_inputs(st, qsat)
    assert list(x) == list(B.IN_NAMES) and x["qsat"] is qsat
    views_of({n: a for n, a in x.items() if n != "qsat"}, inputs_by_hand(st))


def test_outputs_are_the_10_views(st):
    y = c2.op_outputs(st)
    assert list(y) == list(B.OUT_NAMES)
    views_of(y, outputs_by_hand(st))


def test_a_torch_state_with_qsat_gives_16_views(st):
    names = c2.Cloudsc2State.DRIVER_ORDER
    ts = types.SimpleNamespace(**{n: torch.from_numpy(getattr(st, n)) for n in names}, QSAT=torch.zeros(st.PAP.shape, dtype=B.torch_real()))
    x = c2.op_inputs(ts)
    want = dict(inputs_by_hand(ts), qsat=ts.QSAT)
    assert list(x) == list(B.IN_NAMES)
    for n in B.IN_NAMES:
        assert x[n].data_ptr() == want[n].data_ptr() and x[n].stride() == want[n].stride() and x[n].shape == want[n].shape, n
    given = torch.ones_like(ts.QSAT)
    assert c2.op_inputs(ts, given)["qsat"] is given


def test_refcall_blocks_of_the_tail_block(st):
    ibl = st.nblocks - 1
    assert ibl == 7 and NGPTOT - ibl * NPROMA < NPROMA
    x = refcall.block_inputs(st, ibl)
    assert list(x) == list(B.IN_NAMES)
    want = {n: a[ibl] for n, a in inputs_by_hand(st).items()}
    want["qsat"] = np.zeros_like(st.PAP[ibl])
    for n, a in x.items():
        assert a.flags["C_CONTIGUOUS"] and a.dtype == want[n].dtype and np.array_equal(a, want[n]), n
    qsat = np.full_like(st.PAP[ibl], 0.25)
    assert np.array_equal(refcall.block_inputs(st, ibl, qsat)["qsat"], qsat)
    y = refcall.state_outputs_block(st, ibl)
    assert list(y) == list(B.OUT_NAMES)
    for n, a in y.items():
        want = outputs_by_hand(st)[n][ibl]
        assert np.array_equal(a, want) and a.ctypes.data == want.ctypes.data, n  # views: ref_nl_state writes the state through them
