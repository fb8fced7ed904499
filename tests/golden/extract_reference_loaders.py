"""Extract what the reference's loaders ask an input / reference file for into tests/golden/reference_loaders.json, the
expectation of tests/test_real_data_readiness.py.  Study of the reference's sources as text, not execution; only the dataset
names and shapes are kept:
  * every `LOAD_SCALAR('<dataset>', <variable>)` of yomcst.F90 / yoethf.F90 / yoecldp.F90 / yoephli.F90,
  * of those, the ones whose variable is READ by the hot path: the executable statements of satur / cuadjtqs / cloudsc2 /
    cuadjtqstl / cloudsc2tl / cuadjtqsad / cloudsc2ad plus the statement functions of fcttre*.func.h they reach (transitively),
  * whether every main overwrites YREPHLI%LPHYLIN before the first kernel call (dwarf_cloudsc.F90 of cloudsc2_nl / _tl / _ad),
  * every `LOAD_AND_EXPAND('<dataset>', ...)` of CLOUDSC2_ARRAY_STATE_LOAD (cloudsc2_array_state_mod.F90:164-199) and the four
    dataset suffixes of LOAD_AND_EXPAND_STATE (expand_mod.F90:151-154), with the level count each is read with,
  * the datasets WRITE_REFERENCE writes (cloudsc2_array_state_mod.F90:275-284).

    python tests/golden/extract_reference_loaders.py <reference checkout>
"""
from __future__ import annotations

import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_loaders.json")
REF = None  # <reference checkout>/src, set by main()

KERNELS = (("cloudsc2_nl", ("satur", "cuadjtqs", "cloudsc2")), ("cloudsc2_tl", ("cuadjtqstl", "cloudsc2tl", "cloudsc2")),
           ("cloudsc2_ad", ("cuadjtqsad", "cloudsc2ad")))


def _code(text: str) -> str:
    """Executable text: comments, preprocessor lines and USE statements dropped, continuation lines joined, upper case."""
    lines = []
    for ln in text.splitlines():
        if ln.lstrip().startswith(("!", "#")):
            continue
        lines.append(ln.split("!")[0])
    joined = re.sub(r"&\s*\n\s*&?", " ", "\n".join(lines)).upper()
    return "\n".join(ln for ln in joined.splitlines() if not re.match(r"\s*USE\b", ln))


def _loaded_scalars() -> dict:
    """dataset name -> Fortran variable, for the four *_LOAD_PARAMETERS routines."""
    out = {}
    for mod in ("yomcst", "yoethf", "yoecldp", "yoephli"):
        for ln in open(f"{REF}/common/module/{mod}.F90"):
            m = re.search(r"LOAD_SCALAR\('(\w+)',\s*([\w%]+)\)", ln)
            if m:
                out[m.group(1)] = m.group(2).upper()
    return out


def _hot_path_text() -> str:
    body = "\n".join(_code(open(f"{REF}/{d}/{f}.F90").read()) for d, fs in KERNELS for f in fs)
    funcs = {}  # statement functions of the include files: name -> right-hand side
    for h in ("fcttre", "fcttretl", "fcttread", "fccld"):
        for ln in _code(open(f"{REF}/common/include/{h}.func.h").read()).splitlines():
            m = re.match(r"\s*(\w+)\s*\(([^)]*)\)\s*=\s*(.*)$", ln)
            if m and not re.match(r"\s*REAL", ln):
                funcs[m.group(1)] = m.group(3)
    used, todo = set(), [f for f in funcs if re.search(rf"\b{f}\s*\(", body)]
    while todo:
        f = todo.pop()
        if f in used:
            continue
        used.add(f)
        todo += [g for g in funcs if g not in used and re.search(rf"\b{g}\s*\(", funcs[f])]
    assert {"FOEALFA", "FOEEWM"} <= used  # the saturation formulas (fcttre.func.h:74,...)
    return body + "\n" + "\n".join(funcs[f] for f in used)


def _reference_fields() -> dict:
    """dataset name -> ('KLEV' | 'KLEV+1', ndim) as CLOUDSC2_ARRAY_STATE_LOAD reads them."""
    src = open(f"{REF}/common/module/cloudsc2_array_state_mod.F90").read()
    out = {}
    for m in re.finditer(r"CALL LOAD_AND_EXPAND\('(\w+)',\s*SELF%\w+,\s*KLON,\s*SELF%(KLEV(?:\+1)?),\s*(NCLV,)?", src):
        out[m.group(1)] = (m.group(2), 5 if m.group(3) else 1)
    m = re.search(r"CALL LOAD_AND_EXPAND_STATE\('(\w+)'", src)
    ex = open(f"{REF}/common/module/expand_mod.F90").read()
    for sfx, nd in re.findall(r"load_array\(name//'(_\w+)',\s*start,\s*end,\s*size,\s*nlon,\s*nlev,\s*(ndim,)?", ex):
        out[m.group(1) + sfx] = ("KLEV", 5 if nd else 1)
    return out


def main():
    global REF
    REF = os.path.join(sys.argv[1], "src")
    loaded = _loaded_scalars()
    text = _hot_path_text()
    need = sorted(n for n, v in loaded.items() if re.search(r"(?<![\w%])" + re.escape(v) + r"\b", text))
    lphylin = all(re.search(r"^\s*YREPHLI%LPHYLIN\s*=\s*\.true\.", open(f"{REF}/{d}/dwarf_cloudsc.F90").read(), flags=re.M | re.I)
                  for d in ("cloudsc2_nl", "cloudsc2_tl", "cloudsc2_ad"))
    written = sorted(set(re.findall(r"CALL WRITE_ARRAY\('(\w+)'", open(f"{REF}/common/module/cloudsc2_array_state_mod.F90").read())))
    out = {"loaded_scalars": loaded, "hot_path_scalars": need, "lphylin_overloaded_by_every_main": lphylin,
           "field_datasets": {n: list(v) for n, v in sorted(_reference_fields().items())}, "reference_file_datasets": written}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
