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
