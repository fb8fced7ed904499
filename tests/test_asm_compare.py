"""tools/asm_compare.py on tiny synthetic assembly texts: what counts as identical, as the same arithmetic, and as different."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "asm_compare", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "asm_compare.py"))
asm_compare = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(asm_compare)


def _func(name, index, body, regs=12, kernel=True):
    text = """
	.globl	{n} ; -- Begin function {n}
	.type	{n},@function
{n}: ; @{n}
; %bb.0:
{b}
	s_endpgm
.Lfunc_end{i}:
	.size	{n}, .Lfunc_end{i}-{n}
""".format(n=name, i=index, b=body)
    if kernel:
        text += """	.amdhsa_kernel {n}
		.amdhsa_group_segment_fixed_size 512
		.amdhsa_private_segment_fixed_size 0
		.amdhsa_next_free_vgpr {r}
		.amdhsa_accum_offset 12
	.end_amdhsa_kernel
""".format(n=name, r=regs)
    return text


BODY = """	global_load_dwordx2 v[2:3], v[0:1], off
.LBB{i}_1: ; =>This Inner Loop Header: Depth=1
	s_waitcnt vmcnt(0)
	v_mul_f64 v[4:5], v[2:3], v[2:3] ; a comment
	v_add_f64_e32 v[2:3], v[4:5], v[2:3]
	s_cbranch_scc1 .LBB{i}_1
	global_store_dwordx2 v[0:1], v[2:3], off"""

OLD = _func("sweep_a", 0, BODY.format(i=0)) + _func("sweep_b", 1, BODY.format(i=1)) + _func("helper", 2, BODY.format(i=2), kernel=False)


def _status(rows):
    return {f: s for f, s, _ in rows}


def test_renumbered_label_is_identical_and_renamed_register_is_same_arithmetic():
    moved = BODY.format(i=7).replace("; a comment", "; another").replace(".LBB7_1", ".LBB7_5")
    renamed = BODY.format(i=1).replace("v[4:5]", "v[6:7]").replace("v_add_f64_e32", "v_add_f64_e64")
    new = _func("sweep_a", 7, moved) + _func("sweep_b", 1, renamed, regs=14) + _func("helper", 2, BODY.format(i=2), kernel=False)
    rows, ok = asm_compare.compare(OLD, new)
    assert _status(rows) == {"sweep_a": "identical", "sweep_b": "same arithmetic", "helper": "identical"}
    assert not ok  # nothing was allowed to be anything but identical
    rows, ok = asm_compare.compare(OLD, new, allow="sweep_[bc]")
    assert ok
    note = {f: n for f, _, n in rows}
    assert "regs 12->14" in note["sweep_b"] and "scratch 0->0" in note["sweep_b"] and "lds 512->512" in note["sweep_b"]
    assert "agpr_offset 12->12" in note["sweep_a"] and note["helper"] == ""


def test_one_more_multiply_differs_even_where_allowed():
    more = BODY.format(i=1).replace("\ts_cbranch", "\tv_mul_f64 v[2:3], v[2:3], v[2:3]\n\ts_cbranch")
    new = _func("sweep_a", 0, BODY.format(i=0)) + _func("sweep_b", 1, more) + _func("helper", 2, BODY.format(i=2), kernel=False)
    rows, ok = asm_compare.compare(OLD, new, allow="sweep_b")
    assert _status(rows) == {"sweep_a": "identical", "sweep_b": "differs", "helper": "identical"}
    assert not ok
    # one store fewer is a different traffic, not the same arithmetic
    fewer = BODY.format(i=1).replace("\tglobal_store_dwordx2 v[0:1], v[2:3], off", "\ts_nop 0")
    rows, ok = asm_compare.compare(OLD, _func("sweep_a", 0, BODY.format(i=0)) + _func("sweep_b", 1, fewer), allow="sweep_b|helper")
    assert _status(rows)["sweep_b"] == "differs" and not ok


def test_function_missing_on_one_side(tmp_path, capsys):
    new = _func("sweep_a", 0, BODY.format(i=0)) + _func("sweep_c", 1, BODY.format(i=1)) + _func("helper", 2, BODY.format(i=2), kernel=False)
    rows, ok = asm_compare.compare(OLD, new, allow="sweep_[bc]")
    assert [(f, s) for f, s, _ in rows] == [("sweep_a", "identical"), ("sweep_b", "differs"), ("helper", "identical"), ("sweep_c", "differs")]
    note = {f: n for f, _, n in rows}
    assert note["sweep_b"].startswith("(only in OLD)") and note["sweep_c"].startswith("(only in NEW)")
    assert not ok
    # the command line: one line per function, a tally, and the exit status
    old_s, new_s = tmp_path / "old.s", tmp_path / "new.s"
    old_s.write_text(OLD)
    new_s.write_text(new)
    assert asm_compare.main([str(old_s), str(new_s), "--allow", "sweep_[bc]"]) == 1
    out = capsys.readouterr().out.splitlines()
    assert len(out) == 5 and out[-1] == "4 functions: 2 identical, 0 same arithmetic, 2 differs"
    assert asm_compare.main([str(old_s), str(old_s)]) == 0
