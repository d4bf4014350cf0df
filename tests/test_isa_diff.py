"""tools/isa_diff.py on three small synthetic assembly files (CPU, no compiler): the comparison that shows a refactor left the device code
alone must call a kernel equal when only the function-index part of its local labels moved, different when one operand changed, and
must name a kernel that is gone."""
import importlib.util
import io
import os

_spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(os.path.dirname(__file__), "..", "tools", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def _kernel(name, index, operand="v1", first_label=2):
    """One kernel as the compiler prints it: function number `index` of its file, local labels numbered from `first_label`."""
    a, b = first_label, first_label + 3
    return f"""	.globl	{name}
	.p2align	8
	.type	{name},@function
{name}:                                 ; @{name}
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	s_cbranch_scc1 .LBB{index}_{b}
.LBB{index}_{a}:                                ; =>This Inner Loop Header: Depth=1
	v_add_f64 v[2:3], v[2:3], {operand}
	s_cbranch_vccnz .LBB{index}_{a}
.LBB{index}_{b}:                                ;   in Loop: Header=BB{index}_{a} Depth=1
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {name}
		.amdhsa_group_segment_fixed_size 0
		.amdhsa_next_free_vgpr 4
	.end_amdhsa_kernel
	.text
.Lfunc_end{index}:
	.size	{name}, .Lfunc_end{index}-{name}
                                        ; -- End function
"""


TAIL = """	.type	__hip_cuid_0123456789abcdef,@object
	.globl	__hip_cuid_0123456789abcdef
__hip_cuid_0123456789abcdef:
	.byte	0
"""
PARENT = "\t.text\n" + _kernel("_Z5k_onePd", 0) + _kernel("_Z6k_gonePd", 1) + _kernel("_Z5k_twoPd", 2) + TAIL
# k_gone removed: k_two becomes function 1 of its file, and its basic blocks are numbered from another start
SHIFTED = "\t.text\n" + _kernel("_Z5k_onePd", 0) + _kernel("_Z5k_twoPd", 1, first_label=5) + TAIL.replace("0123456789abcdef", "fedcba9876543210")
CHANGED = "\t.text\n" + _kernel("_Z5k_onePd", 0) + _kernel("_Z5k_twoPd", 1, operand="v[4:5]") + TAIL


def test_functions_hold_body_and_descriptor_and_skip_the_cuid():
    f = isa_diff.functions(PARENT)
    assert sorted(f) == ["_Z5k_onePd", "_Z5k_twoPd", "_Z6k_gonePd"]
    text = "\n".join(f["_Z5k_twoPd"])
    assert "v_add_f64" in text and ".amdhsa_next_free_vgpr 4" in text and text.count(".end_amdhsa_kernel") == 1
    assert "BB2_" not in text and ".Lfunc_end2" not in text


def test_shifted_label_indices_compare_equal_and_the_removed_kernel_is_only_in_a():
    equal, differ, only_a, only_b = isa_diff.compare(isa_diff.functions(PARENT), isa_diff.functions(SHIFTED))
    assert equal == ["_Z5k_onePd", "_Z5k_twoPd"] and differ == [] and only_a == ["_Z6k_gonePd"] and only_b == []
    out = io.StringIO()
    assert isa_diff.report(isa_diff.functions(PARENT), isa_diff.functions(SHIFTED), out=out) == 0
    assert "ONLY IN A _Z6k_gonePd" in out.getvalue()


def test_one_changed_operand_is_reported_as_different():
    a, b = isa_diff.functions(SHIFTED), isa_diff.functions(CHANGED)
    equal, differ, only_a, only_b = isa_diff.compare(a, b)
    assert equal == ["_Z5k_onePd"] and differ == ["_Z5k_twoPd"] and only_a == [] and only_b == []
    out = io.StringIO()
    assert isa_diff.report(a, b, out=out) == 1
    text = out.getvalue()
    assert "DIFFERENT _Z5k_twoPd" in text and "-\tv_add_f64 v[2:3], v[2:3], v1" in text and "+\tv_add_f64 v[2:3], v[2:3], v[4:5]" in text


def test_rename_makes_a_kernel_that_lost_a_template_argument_compare_equal(tmp_path):
    """k_two<29, true> of A is k_two<true> of B: the same text under another mangled name.  Without --rename it is gone from A and new in B
    (exit status 1); with A's name rewritten it is equal, a changed operand still shows, and only the variant that was really removed
    (k_two<13, true>) is left in A.  k_two is function 12 of A's file and function 1 of B's: the compiler pads the comment behind a label
    to a column, so its labels are followed by one blank less."""
    a = "\t.text\n" + _kernel("_Z5k_oneILi29ELb1EEvPd", 0) + _kernel("_Z5k_oneILi13ELb1EEvPd", 1) + _kernel("_Z5k_twoPd", 12).replace("_2: ", "_2:") + TAIL
    b = "\t.text\n" + _kernel("_Z5k_oneILb1EEvPd", 0) + _kernel("_Z5k_twoPd", 1, first_label=5) + TAIL
    for d, text in (("a", a), ("b", b), ("c", b.replace("v1", "v[4:5]", 1))):
        (tmp_path / d).mkdir()
        (tmp_path / d / "unit.s").write_text(text)
    equal, differ, only_a, only_b = isa_diff.compare(isa_diff.load(tmp_path / "a"), isa_diff.load(tmp_path / "b"))
    assert equal == ["unit.s: _Z5k_twoPd"] and only_b == ["unit.s: _Z5k_oneILb1EEvPd"] and len(only_a) == 2
    renames = [(r"_Z5k_oneILi29E", "_Z5k_oneI")]
    ra = isa_diff.load(tmp_path / "a", renames)
    out = io.StringIO()
    assert isa_diff.report(ra, isa_diff.load(tmp_path / "b"), out=out) == 0
    assert out.getvalue().splitlines() == ["equal: 2  different: 0  only in A: 1  only in B: 0", "ONLY IN A unit.s: _Z5k_oneILi13ELb1EEvPd"]
    equal, differ, only_a, only_b = isa_diff.compare(ra, isa_diff.load(tmp_path / "c"))
    assert differ == ["unit.s: _Z5k_oneILb1EEvPd"] and equal == ["unit.s: _Z5k_twoPd"] and only_b == []
