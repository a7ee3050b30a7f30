"""tools/kernel_isa_diff.py -- the per-kernel text comparison of two builds' device assembly that a refactor of csrc/ is
checked with: bodies that differ only in .LBB numbering and comments are identical, a changed operand is not, a kernel on
one side only is reported as such, and the register / LDS / scratch figures of both sides come out beside the verdict."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_isa_diff as K  # noqa: E402


def module(fn_no, body, sym="_Z3fooPf", vgpr=24, lds=512):
    return f"""
	.text
	.globl	{sym}
	.type	{sym},@function
{sym}:                               ; @{sym}
; %bb.0:
{body}
.Lfunc_end{fn_no}:
	.size	{sym}, .Lfunc_end{fn_no}-{sym}
	.section	.rodata,"a",@progbits
	.amdhsa_kernel {sym}
		.amdhsa_group_segment_fixed_size {lds}
		.amdhsa_private_segment_fixed_size 0
		.amdhsa_next_free_vgpr {vgpr}
		.amdhsa_next_free_sgpr 18
	.end_amdhsa_kernel
"""


BODY = """	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_lshlrev_b32_e32 v1, 2, v0            ; a comment
.LBB{n}_1:                                ; =>This Inner Loop Header: Depth=1
	v_add_f32_e32 v2, v2, v1
	s_cbranch_scc1 .LBB{n}_1
; %bb.2:
	global_store_dword v1, v2, s[0:1]
	s_endpgm"""


def rows(a, b):
    return {r[0]: r for r in K.compare(K.kernels(a), K.kernels(b))}


def test_label_numbering_and_comments_do_not_count():
    a = module(3, BODY.format(n=3))
    b = module(17, BODY.format(n=17).replace("; a comment", "; another comment").replace("; %bb.2:", "; %bb.2:   ; preds"))
    r = rows(a, b)["_Z3fooPf"]
    assert r[1] == "identical" and r[2] == r[3] == 6
    assert r[4] == r[5] == {"next_free_vgpr": "24", "next_free_sgpr": "18", "group_segment_fixed_size": "512",
                            "private_segment_fixed_size": "0"}


def test_changed_operand_is_different():
    a = module(3, BODY.format(n=3))
    b = module(3, BODY.format(n=3).replace("v_add_f32_e32 v2, v2, v1", "v_add_f32_e32 v2, v2, v3"), vgpr=25)
    r = rows(a, b)["_Z3fooPf"]
    assert r[1] == "DIFFERENT" and r[2] == r[3] == 6
    assert r[4]["next_free_vgpr"] == "24" and r[5]["next_free_vgpr"] == "25"


def test_kernel_on_one_side_only():
    a = module(0, BODY.format(n=0)) + module(1, BODY.format(n=1), sym="_Z3barPf")
    b = module(0, BODY.format(n=0)) + module(1, BODY.format(n=1), sym="_Z3bazPf")
    r = rows(a, b)
    assert r["_Z3fooPf"][1] == "identical"
    assert r["_Z3barPf"][1] == "only in A" and r["_Z3barPf"][3] is None
    assert r["_Z3bazPf"][1] == "only in B" and r["_Z3bazPf"][2] is None
