"""tools/timing_harness.py without a device: the alternation of fresh processes, the spread over them, the bandwidth row and the rotation
of forms.  The children are Python one-liners that print a JSON line; the timers themselves need a device and run with the tools."""
from __future__ import annotations

import importlib.util
import os
import sys

import pytest

from tests.hostbuild import ROOT


@pytest.fixture(scope="module")
def th():
    spec = importlib.util.spec_from_file_location("timing_harness", os.path.join(ROOT, "tools", "timing_harness.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def child(name: str, tmp_path, code: int = 0):
    """a process that leaves a marker file numbered by its place in the sequence, prints noise and then its JSON line"""
    src = ("import json, os, sys; d = sys.argv[1]; k = len(os.listdir(d)); open(os.path.join(d, '%03d_' % k + sys.argv[2]), 'w').close(); "
           "print('noise'); print(json.dumps({'who': sys.argv[2], 'place': k, 'cwd': os.getcwd()})); sys.exit(int(sys.argv[3]))")
    return [sys.executable, "-c", src, str(tmp_path), name, str(code)]


def test_children_alternate_in_both_orders(th, tmp_path):
    marks, cwd_b = tmp_path / "marks", tmp_path / "elsewhere"
    marks.mkdir(), cwd_b.mkdir()
    runs = th.children({"A": (child("A", marks), str(tmp_path)), "B": (child("B", marks), str(cwd_b))})
    want = list("ABABAB" + "BABABA")
    assert [r["which"] for r in runs] == want
    assert [r["result"]["who"] for r in runs] == want and [r["result"]["place"] for r in runs] == list(range(12))
    assert all(os.path.samefile(r["result"]["cwd"], cwd_b if r["which"] == "B" else tmp_path) for r in runs)
    assert [f[4:] for f in sorted(os.listdir(marks))] == want


def test_a_failed_child_ends_the_sequence(th, tmp_path, capsys):
    assert th.children({"A": (child("A", tmp_path), None), "B": (child("B", tmp_path, code=3), None)}) == 3
    assert sorted(os.listdir(tmp_path)) == ["000_A", "001_B"]  # nothing was started after the child that exited 3
    assert "noise" in capsys.readouterr().out  # its output tail was printed


def test_spread_is_max_minus_min_over_the_median(th):
    results = [{"forward": {"ms": v}, "n": 7} for v in (1.02, 0.98, 1.0, 1.07, 0.99, 1.01)]
    assert th.spread(results, ("forward", "ms")) == round((1.07 - 0.98) / 1.005, 4) == 0.0896
    assert th.spread([{"ms": 3.0}, {"ms": 4.0}, {"ms": 8.0}], ("ms",)) == 1.25 and th.spread(results, ("n",)) == 0.0


def test_row(th):
    r = th.row(2.0, 1000, 160000)
    assert list(r) == ["ms", "bytes_per_column", "frac_of_8TBps"]
    assert r["ms"] == 2.0 and r["bytes_per_column"] == 1000 and r["frac_of_8TBps"] == round(1000 * 160000 / 2e-3 / 8e12, 3) == 0.01
    assert th.row(0.123456, 46080, 160000)["ms"] == 0.1235 and th.PEAK == 8e12


@pytest.mark.parametrize("nforms,shift,reps", [(4, 4, 10), (3, 3, 7), (4, 1, 3), (4, 2, 5)])
def test_rotated_visits_every_form_once_per_repetition(th, nforms, shift, reps):
    calls = []
    forms = {f"f{k}": (lambda k=k: calls.append(k)) for k in range(nforms)}

    def timer(step):
        step()
        return float(len(calls))

    ms = th.rotated(forms, reps, timer, shift)
    assert list(ms) == list(forms) and all(len(v) == reps for v in ms.values())
    for r in range(reps):
        rep = calls[r * nforms:(r + 1) * nforms]
        assert sorted(rep) == list(range(nforms)) and rep[0] == r % shift
        assert rep == [(r % shift + j) % nforms for j in range(nforms)]  # the order is kept, only its start moves
    assert all(ms[f"f{calls[k]}"].count(float(k + 1)) == 1 for k in range(len(calls)))  # every time under its form's name
