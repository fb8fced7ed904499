#!/usr/bin/env python3
"""Compare two `make asm` outputs function by function: asm_compare.py OLD.s NEW.s [--allow REGEX]

For every function present in either file, one line with one of
  identical        the same instructions once comments are removed and the block labels are renumbered in order of appearance
  same arithmetic  not identical, but the count of every vector floating-point mnemonic and of every vector memory mnemonic is
                   equal: the arithmetic and the traffic are those of the old file, registers and scheduling may differ
  differs          anything else, a function missing on one side included
and for kernels the registers, AGPR offset, scratch and LDS bytes of both files' .amdhsa_ blocks.

Mnemonics are classified by prefix class only: `v_` with a floating-point type suffix is vector floating point (arithmetic,
conversions and compares alike), the prefixes of MEMORY are vector memory.  An encoding suffix (_e32, _e64, ...) is not part of the
mnemonic.

Exit status 1 when a function whose name does not match --allow is not identical, or when one that matches it differs.
"""
import argparse
import collections
import re
import sys

MEMORY = ("global_", "flat_", "ds_", "buffer_", "scratch_")
FLOAT = re.compile(r"_(f16|bf16|f32|f64)(_|$)")
ENCODING = re.compile(r"_(e32|e64|sdwa|dpp|e64_dpp)$")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")
RESOURCES = collections.OrderedDict([
    ("regs", ".amdhsa_next_free_vgpr"), ("agpr_offset", ".amdhsa_accum_offset"),
    ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size")])


def parse(text):
    """{function: list of instruction lines with labels renumbered}, {kernel: {resource: value}}"""
    funcs, kernels = collections.OrderedDict(), {}
    name, body, labels, kernel = None, None, None, None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if kernel is not None:  # inside an .amdhsa_kernel block
            if line.startswith(".end_amdhsa_kernel"):
                kernel = None
            else:
                for key, directive in RESOURCES.items():
                    if line.startswith(directive + " "):
                        kernels[kernel][key] = int(line.split()[1], 0)
            continue
        if line.startswith(".amdhsa_kernel "):
            kernel = line.split()[1]
            kernels[kernel] = {}
            continue
        m = re.match(r"\.type\s+([^,\s]+),@function", line)
        if m:
            name, body, labels = m.group(1), [], {}
            continue
        if name is None or not line:
            continue
        if line.startswith(".Lfunc_end") or line.startswith(".size"):
            if body is not None:
                funcs[name] = body
            name, body = None, None
            continue
        if line == name + ":" or (line.startswith(".") and not LABEL.match(line)):
            continue  # the function's own label, directives
        body.append(LABEL.sub(lambda x: labels.setdefault(x.group(0), ".L%d" % len(labels)), " ".join(line.split())))
    return funcs, kernels


def arithmetic(body):
    """counts of the vector floating-point and the vector memory mnemonics"""
    counts = collections.Counter()
    for line in body:
        if line.endswith(":"):
            continue
        mnemonic = ENCODING.sub("", line.split()[0])
        if mnemonic.startswith(MEMORY) or (mnemonic.startswith("v_") and FLOAT.search(mnemonic)):
            counts[mnemonic] += 1
    return counts


def classify(old, new):
    if old is None or new is None:
        return "differs"
    if old == new:
        return "identical"
    return "same arithmetic" if arithmetic(old) == arithmetic(new) else "differs"


def compare(old_text, new_text, allow=None):
    """[(function, status, note)] in the old file's order, then the functions only the new one has; and whether all is allowed"""
    (fo, ko), (fn, kn) = parse(old_text), parse(new_text)
    allowed = re.compile(allow) if allow else None
    rows, ok = [], True
    for f in list(fo) + [f for f in fn if f not in fo]:
        status = classify(fo.get(f), fn.get(f))
        note = "" if f in fo and f in fn else "(only in %s)" % ("OLD" if f in fo else "NEW")
        if f in ko or f in kn:
            a, b = ko.get(f, {}), kn.get(f, {})
            note += " " + " ".join("%s %s->%s" % (k, a.get(k, "-"), b.get(k, "-")) for k in RESOURCES)
        inside = allowed is not None and allowed.search(f) is not None
        if status == "differs" or (status != "identical" and not inside):
            ok = False
        rows.append((f, status, note.strip()))
    return rows, ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", metavar="REGEX", help="functions that may be `same arithmetic` instead of identical")
    args = ap.parse_args(argv)
    with open(args.old) as f, open(args.new) as g:
        rows, ok = compare(f.read(), g.read(), args.allow)
    for f, status, note in rows:
        print("%-15s %s %s" % (status, f, note))
    tally = collections.Counter(status for _, status, _ in rows)
    print("%d functions: " % len(rows) + ", ".join("%d %s" % (tally[s], s) for s in ("identical", "same arithmetic", "differs")))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
