"""tools/device_asm_diff.py --by-kernel pairs kernels by name wherever they sit, after replacing the compiler's per-unit
function ordinal in local labels (normalize_ordinals).  Three short synthetic assembly texts, no compiler: the normalisation
hides the ordinal and nothing else -- a changed instruction and a changed basic-block number are both reported, for the
kernel they are in and for no other."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import device_asm_diff as dad  # noqa: E402


def _kernel(name, ordinal, instruction="v_add_f64 v[0:1], v[0:1], v[2:3]", block=1):
    return f"""\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\ts_cbranch_scc1 .LBB{ordinal}_{block}
\t{instruction}
.LBB{ordinal}_{block}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 4
\t.end_amdhsa_kernel
\t.section\t.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{ordinal}:
\t.size\t{name}, .Lfunc_end{ordinal}-{name}
"""


def _unit(*kernels):
    return "\t.text\n" + "".join(kernels) + "\t.amdgpu_metadata\n---\namdhsa.kernels: []\n...\n\t.end_amdgpu_metadata\n"


def _pooled(**units):
    return dad.pool({u: dad.symbols(dad.normalize_ordinals(t))[0] for u, t in units.items()})


ONE_UNIT = _unit(_kernel("k_a", 0), _kernel("k_b", 1))


def test_texts_that_differ_only_in_the_function_ordinal_compare_equal():
    # the same two kernels in the other order, and spread over two units (k_b is then function 0 of its own unit)
    swapped = _unit(_kernel("k_b", 0), _kernel("k_a", 1))
    syms, kernels = dad.symbols(dad.normalize_ordinals(ONE_UNIT))
    assert kernels == {"k_a", "k_b"}
    assert dad.symbols(ONE_UNIT)[0]["k_b"] != dad.symbols(swapped)[0]["k_b"]  # the default mode sees the ordinal
    assert syms["k_a"] == dad.symbols(dad.normalize_ordinals(swapped))[0]["k_a"]
    a = _pooled(one=ONE_UNIT)
    assert dad.compare_pools(a, _pooled(one=swapped)) == ([], [])
    assert dad.compare_pools(a, _pooled(first=_unit(_kernel("k_a", 0)), second=_unit(_kernel("k_b", 0)))) == ([], [])
    # a kernel that two units hold: equal copies pass, and a kernel on one side only is named
    assert dad.compare_pools(a, _pooled(first=ONE_UNIT, second=_unit(_kernel("k_b", 0)))) == ([], [])
    assert dad.compare_pools(a, _pooled(first=_unit(_kernel("k_a", 0)))) == (["k_b"], [])


def test_a_changed_instruction_is_reported_for_its_kernel_alone():
    edited = _unit(_kernel("k_a", 0), _kernel("k_b", 1, instruction="v_add_f64 v[0:1], v[0:1], v[4:5]"))
    assert dad.compare_pools(_pooled(one=ONE_UNIT), _pooled(one=edited)) == ([], ["k_b"])
    # ... also when only ONE of two copies on a side has changed
    assert dad.compare_pools(_pooled(one=ONE_UNIT), _pooled(first=ONE_UNIT, second=_unit(_kernel("k_b", 0, instruction="s_nop 0")))) == ([], ["k_b"])


def test_a_changed_basic_block_ordinal_is_reported():
    edited = _unit(_kernel("k_a", 0, block=2), _kernel("k_b", 1))
    assert dad.normalize_ordinals(".LBB7_12 .Lfunc_begin7 .Lfunc_end7 .LJTI7_0") == ".LBB#_12 .Lfunc_begin# .Lfunc_end# .LJTI#_0"
    # the label's comment: the block it names, and its padding to a column that depends on the digits of the ordinal
    assert dad.normalize_ordinals(".LBB123_4:      ; in Loop: Header=BB123_2 Depth=1\n") == \
        dad.normalize_ordinals(".LBB7_4:        ; in Loop: Header=BB7_2 Depth=1\n") == ".LBB#_4: ; in Loop: Header=BB#_2 Depth=1\n"
    assert dad.normalize_ordinals(".LBB7_4: ; Header=BB7_3\n") != dad.normalize_ordinals(".LBB7_4: ; Header=BB7_2\n")
    assert dad.compare_pools(_pooled(one=ONE_UNIT), _pooled(one=edited)) == ([], ["k_a"])
