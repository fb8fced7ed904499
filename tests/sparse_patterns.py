"""The mask patterns the sparse sweeps are tested on, shared by the CPU and the GPU tests (no test of its own).

A pattern is ``(name, ins, outs)``: the fields present on the input side and on the output side of the derivative blocks.
  reverse sweep: ``ins`` = the gradients wanted (adj_in, written), ``outs`` = the cotangents given (adj_out, read);
  TL sweep:      ``ins`` = the tangents given (pert_in, read),     ``outs`` = the output tangents stored (pert_out, written).
Every other field of the two blocks is a NULL pointer.
"""
from __future__ import annotations

import numpy as np

from dwarf_p_cloudsc2_tl_ad_amd import binding as B

NARROW = (("q", "t"), ("fplsl", "fplsn"))  # surface precipitation differentiated with respect to t and q


def in_names(satur: bool) -> tuple:
    return tuple(n for n in B.IN_NAMES if not (satur and n == "qsat"))


def patterns(satur: bool, tl: bool = False, nrandom: int = 8) -> list:
    ins, outs = in_names(satur), tuple(B.OUT_NAMES)
    pats = [("all", ins, outs)]
    pats += [(f"out:{o}", ins, (o,)) for o in outs]  # one cotangent (TL: one output tangent stored) with everything on the other side
    # one gradient (TL: one tangent) with everything on the other side; in:paph and in:lu are the planes with accesses outside the level loop
    pats += [(f"in:{i}", (i,), outs) for i in ins]
    pats.append(("narrow",) + NARROW)
    rng = np.random.default_rng(20261019 + (1 if satur else 0))
    for k in range(nrandom):
        while True:
            pi = tuple(n for n in ins if rng.random() < 0.4)
            po = tuple(n for n in outs if rng.random() < 0.4)
            if pi and po:
                break
        pats.append((f"random{k}", pi, po))
    if tl:
        pats.append(("tangents:q,t", NARROW[0], outs))  # what the op's jvp launches for a loss differentiated with respect to t and q
        pats.append(("no_tangent", (), outs))           # allowed: the zero tangent
    return pats
