"""CPU: tools/device_code_diff.py on synthetic gfx950 listings (no compiler): what depends only on
emission order compares equal, and every kind of real change is reported under its symbol."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dcd():
    spec = importlib.util.spec_from_file_location("device_code_diff", os.path.join(ROOT, "tools", "device_code_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel(name, idx, op="v_add_f32_e32 v1, v0, v0", vgpr=8, tmp=0):
    lbb = f".LBB{idx}_1:".ljust(40)   # the compiler pads a label's comment to column 40
    return f"""\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                  ; @{name}
.Lfunc_begin{idx}:
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
{lbb}; =>This Inner Loop Header: Depth=1
\t{op}
.Ltmp{tmp}:
\ts_cbranch_scc1 .LBB{idx}_1
; %bb.2:                                ;   in Loop: Header=BB{idx}_1 Depth=1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 12
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{idx}:
\t.size\t{name}, .Lfunc_end{idx}-{name}
                                        ; -- End function
"""


def metadata(name, vgpr=8):
    return f"""  - .agpr_count:     0
    .args:
      - .address_space:  global
        .name:           x
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .name:           {name}
    .vgpr_count:     {vgpr}
    .wavefront_size: 64
"""


def listing(kernels, cuid="0123456789abcdef", table=64, md=None):
    """kernels: (name, function index, keyword arguments of kernel()) in emission order"""
    body = "".join(kernel(n, i, **kw) for n, i, kw in kernels)
    mds = "".join(metadata(n, kw.get("vgpr", 8)) for n, _, kw in (md if md is not None else kernels))
    return f"""\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.file\t"unit-{cuid}.hip"
\t.text
{body}\t.type\tg_table,@object
\t.section\t.rodata,"a",@progbits
g_table:
\t.quad\t0x3ff0000000000000
\t.size\tg_table, {table}

\t.type\t__hip_cuid_{cuid},@object
\t.section\t.bss,"aw",@nobits
\t.globl\t__hip_cuid_{cuid}
__hip_cuid_{cuid}:
\t.byte\t0
\t.size\t__hip_cuid_{cuid}, 1

\t.ident\t"clang built in {cuid}"
\t.amdgpu_metadata
---
amdhsa.kernels:
{mds}amdhsa.target:   amdgcn-amd-amdhsa--gfx950
amdhsa.version:
  - 1
  - 2
...

\t.end_amdgpu_metadata
"""


A = listing([("_Z2k1Pf", 0, {}), ("_Z2k2Pf", 1, {"tmp": 1})])


def test_split_finds_every_kind(dcd):
    assert sorted(dcd.split(A)) == ["fn:_Z2k1Pf", "fn:_Z2k2Pf", "kd:_Z2k1Pf", "kd:_Z2k2Pf", "md:_Z2k1Pf", "md:_Z2k2Pf",
                                    "obj:__hip_cuid_", "obj:g_table"]
    assert any("v_add_f32" in ln for ln in dcd.split(A)["fn:_Z2k1Pf"])


def test_swapped_order_and_renumbered_labels_compare_equal(dcd):
    b = listing([("_Z2k2Pf", 0, {"tmp": 5}), ("_Z2k1Pf", 1, {"tmp": 9})], cuid="fedcba9876543210")
    assert dcd.compare_text(A, b) == ([], [], [])


def test_label_padding_of_a_narrower_function_index_compares_equal(dcd):
    # a file that loses a kernel ahead of its tenth: index 10 becomes 9, and the padding behind the
    # label grows by a blank
    a = listing([("_Z2k1Pf", 10, {})])
    b = listing([("_Z2k1Pf", 9, {})])
    assert ".LBB10_1:" + 31 * " " + ";" in a and ".LBB9_1:" + 32 * " " + ";" in b
    assert dcd.compare_text(a, b) == ([], [], [])


def test_changed_instruction_is_reported_under_its_symbol(dcd):
    b = listing([("_Z2k1Pf", 0, {}), ("_Z2k2Pf", 1, {"tmp": 1, "op": "v_mul_f32_e32 v1, v0, v0"})])
    assert dcd.compare_text(A, b) == ([], [], ["fn:_Z2k2Pf"])


def test_missing_kernel_is_reported(dcd):
    b = listing([("_Z2k1Pf", 0, {})])
    assert dcd.compare_text(A, b) == (["fn:_Z2k2Pf", "kd:_Z2k2Pf", "md:_Z2k2Pf"], [], [])
    assert dcd.compare_text(b, A) == ([], ["fn:_Z2k2Pf", "kd:_Z2k2Pf", "md:_Z2k2Pf"], [])


def test_changed_next_free_vgpr_is_reported(dcd):
    b = listing([("_Z2k1Pf", 0, {"vgpr": 9}), ("_Z2k2Pf", 1, {"tmp": 1})])
    assert dcd.compare_text(A, b) == ([], [], ["kd:_Z2k1Pf", "md:_Z2k1Pf"])
    # the descriptor alone
    b = listing([("_Z2k1Pf", 0, {"vgpr": 9}), ("_Z2k2Pf", 1, {"tmp": 1})], md=[("_Z2k1Pf", 0, {}), ("_Z2k2Pf", 1, {})])
    assert dcd.compare_text(A, b) == ([], [], ["kd:_Z2k1Pf"])


def test_changed_object_size_is_reported(dcd):
    assert dcd.compare_text(A, listing([("_Z2k1Pf", 0, {}), ("_Z2k2Pf", 1, {"tmp": 1})], table=72)) == ([], [], ["obj:g_table"])


def test_compare_directories_exit_status(dcd, tmp_path, capsys):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    (a / "u.s").write_text(A)
    (b / "u.s").write_text(listing([("_Z2k2Pf", 0, {"tmp": 1}), ("_Z2k1Pf", 1, {})], cuid="aaaaaaaaaaaaaaaa"))
    assert dcd.compare(str(a), str(b)) == 0
    assert "u.s: 2 kernels, 2 functions, 2 objects compared, 0 differences" in capsys.readouterr().out
    (b / "u.s").write_text(listing([("_Z2k1Pf", 0, {"op": "v_sub_f32_e32 v1, v0, v0"}), ("_Z2k2Pf", 1, {"tmp": 1})]))
    assert dcd.compare(str(a), str(b)) == 1
    assert "u.s: differs: fn:_Z2k1Pf" in capsys.readouterr().out
