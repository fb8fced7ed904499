"""The kernel-family units are written down twice: as the rows C2_ROWS_<unit> of the table in csrc/cloudsc2_sweep_kernels.hpp, from
which the accessors, the units' variant tables, the single-unit build and the host's registry are generated, and as FAMILIES in
csrc/Makefile, because the build needs the object names.  The two lists are held together here, from the text alone (no library is
loaded): a unit on one side only is otherwise caught late -- a name the table does not know does not compile, one the Makefile does
not know leaves an accessor undefined and the library does not load."""
from __future__ import annotations

import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dwarf_p_cloudsc2_tl_ad_amd", "csrc")


def _text(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read().replace("\\\n", " ")  # (continuation lines joined)


def _makefile_families() -> list:
    (line,) = re.findall(r"^FAMILIES\s*:=\s*(.*)$", _text("Makefile"), flags=re.M)
    return line.split()


def _table():
    """(units that have rows, units C2_KERNEL_TABLES expands, accessor names of the rows per unit)"""
    hdr = _text("cloudsc2_sweep_kernels.hpp")
    rows = {unit: re.findall(r"\bX\(\s*(\w+)\s*,", body) for unit, body in re.findall(r"^#define C2_ROWS_(\w+)\(X\)(.*)$", hdr, flags=re.M)}
    (all_rows,) = re.findall(r"^#define C2_KERNEL_TABLES\(X\)(.*)$", hdr, flags=re.M)
    return list(rows), re.findall(r"C2_ROWS_(\w+)\(X\)", all_rows), rows


def test_the_makefile_builds_exactly_the_units_of_the_table():
    defined, expanded, _ = _table()
    families = _makefile_families()
    assert len(set(families)) == len(families) and len(set(defined)) == len(defined) and len(set(expanded)) == len(expanded)
    assert set(defined) == set(expanded), sorted(set(defined) ^ set(expanded))  # every unit's rows are part of the whole table
    assert set(families) == set(defined), sorted(set(families) ^ set(defined))
    assert len(families) == 22


def test_every_table_is_one_row_of_one_unit():
    _, _, rows = _table()
    names = [n for unit in rows.values() for n in unit]
    assert len(names) == 24 and len(set(names)) == 24, names
    assert all(unit in rows[unit] for unit in rows), "a unit is named after a table it holds"
    assert rows["ad"] == ["ad_reverse", "ad"] and rows["vjp_ens_colsum"] == ["vjp_ens_colsum", "vjp_ens_colsum_fields"]
    assert [unit for unit in rows if len(rows[unit]) != 1] == ["ad", "vjp_ens_colsum"]


def test_the_units_have_one_source():
    assert [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "cloudsc2_kern*.hip"))] == ["cloudsc2_kern.hip"]
    mk = _text("Makefile")
    # both precisions compile it once per unit, the unit's name in C2_FAMILY
    assert len(re.findall(r"^obj_[ds]p/cloudsc2_kern_%\.o: cloudsc2_kern\.hip .*\n\t.*-DC2_FAMILY=\$\* ", mk, flags=re.M)) == 2
    assert "C2_ROWS_OF(C2_FAMILY)(C2_DEFINE_VARIANT)" in _text("cloudsc2_kern.hip")
    assert "C2_KERNEL_TABLES(C2_DEFINE_VARIANT)" in _text("cloudsc2_launch.hip")  # the single-unit build: every row
