"""The yardstick of the parameter column-sum tests (host build and MI355X), from the PARENT's code alone: the planes of the parameter
Jacobian (hostcheck_tl_parjac / cloudsc2_tl_launch_parjac) folded sequentially over the levels the way the column-sum tests fold output
planes (``acc = +0; acc = fl(acc + fl(w[k] * J[k]))`` in the library's real type), and, for the normal equations, contracted in float64
in the style of tests/parnormal_yardstick.py: contract.

Bound of the normal equations: ``|got - want| <= 1e-12 * S`` entry by entry, ``S`` the sum of the absolute products -- the bound
tests/parnormal_yardstick.py derives.  The chains here are shorter: the sensitivities of the sums are the same bits on both sides
(asserted by the sums-form tests), so a column's chain is at most 8 observed sums, plus ngptot / 1024 + 10 additions in the fold over
the columns.

Works on numpy arrays and torch tensors alike (``*``, ``+``, ``abs`` only)."""
from __future__ import annotations

from tests.parnormal_yardstick import BOUND, RPECONS_ROWS, row_g, row_h  # noqa: F401
from tests.util import B

HALF = ("fplsl", "fplsn", "fhpsl", "fhpsn")
PAR_SUMS = tuple(n for n in B.OUT_NAMES if n not in ("clc", "covptot"))  # the outputs that depend on a parameter


def fold_levels(w, plane, zeros):
    """w: (nlevx,), plane: (..., nlevx, ncols-like) indexed [.., k, ..] on axis -2, zeros: the accumulator's start.  Sequential."""
    acc = zeros
    for k in range(len(w)):
        p = w[k] * plane[..., k, :]
        acc = acc + p
    return acc


def contract_sums(s: list, r: dict, w: dict) -> dict:
    """s[k][name], r[name], w[name] (a name missing from w: weight 1): float64, one value per column.  The observed sums are r's names;
    k runs over the directions that were run.  -> {row: (want, S)}, each per column: the sum over the observed sums and the sum of the
    absolute products."""
    out = {}
    for a in range(len(s)):
        for b in list(range(a, len(s))) + [None]:
            want = S = 0.0
            for n in B.OUT_NAMES:
                if n not in r:
                    continue
                wj = s[a][n] * w[n] if n in w else s[a][n]
                p = wj * (s[b][n] if b is not None else r[n])
                want = want + p
                S = S + abs(p)
            out[row_h(a, b) if b is not None else row_g(a)] = (want, S)
    return out
