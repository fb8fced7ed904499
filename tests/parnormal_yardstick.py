"""The yardstick of the normal-equations tests (host build and MI355X): J^T W J and J^T W r contracted in float64 from the PARENT's
parameter Jacobian (hostcheck_tl_parjac / cloudsc2_tl_launch_parjac), never from the code under test, with the absolute sums the bound
is stated in.

Bound: ``|got - want| <= 1e-12 * S`` entry by entry, ``S`` the sum of the absolute products.  Both sides add the same products in a
different order, so each side's error is at most (chain length) * 2^-53 * S; the sweep's longest chain is 10 outputs x 138 levels plus
ngptot / 1024 + 10 in the fold, under 1500 at every shape tested; two sides and the products' own roundings give about 3.5e-13 * S.

Works on numpy arrays and torch tensors alike (only ``*``, ``abs`` and ``.sum(0)`` are used): the planes are ``(nlevx, ncols)`` float64,
active columns only."""
from __future__ import annotations

from tests.util import B, refcall

NPAR = len(B.PARAM_NAMES)
BOUND = 1e-12


def row_h(a: int, b: int) -> int:
    """row of (J^T W J)[a][b], a <= b: the upper triangle row by row in PARAM_NAMES order"""
    return a * NPAR - a * (a - 1) // 2 + (b - a)


def row_g(a: int) -> int:
    return NPAR * (NPAR + 1) // 2 + a


RPECONS_ROWS = tuple(sorted({row_h(a, NPAR - 1) for a in range(NPAR)} | {row_g(NPAR - 1)}))


def contract(J: list, r: dict, w: dict) -> dict:
    """J[k][name], r[name], w[name] (a name missing from w: weight 1): float64 planes (nlevx, ncols).  The observed outputs are r's
    names; k runs over the directions that were run.  Half level 0 of the fluxes (the zero flux at the model top) takes no part.
    -> {row: (want, S)}, each (ncols,): every column's sum over levels and outputs, and the sum of the absolute products."""
    out = {}
    for a in range(len(J)):
        for b in list(range(a, len(J))) + [None]:
            want = S = 0.0
            for n in B.OUT_NAMES:
                if n not in r:
                    continue
                lo = 1 if n in refcall.HALF else 0
                wj = J[a][n][lo:] * w[n][lo:] if n in w else J[a][n][lo:]
                p = wj * (J[b][n][lo:] if b is not None else r[n][lo:])
                want = want + p.sum(0)
                S = S + abs(p).sum(0)
            out[row_h(a, b) if b is not None else row_g(a)] = (want, S)
    return out
