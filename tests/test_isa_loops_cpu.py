"""CPU: the listing parser of tools/isa_loops.py (`edge` mode) on a short synthetic listing: a
kernel whose loop holds an unrolled block of 16 steps, each ending in `v_readlane_b32 ..., 63`,
a rolled path for partial blocks beside it, and a loop header.  Checked: the loop and its run of
reduction ends are found (the rolled path's single one is not taken for the block), s_nop N counts
N + 1 issue slots, and the edge path is the shortest one from the block's last reduction end round
the back edge to its first, by instruction category."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import isa_loops as I  # noqa: E402


def listing(head_salu, tail_salu):
    out = ["kern:                                   ; @kern", "; %bb.0:", "\ts_mov_b32 s0, 4"]
    out += [".LBB0_1:                                ; =>This Loop Header"]
    out += ["\ts_add_i32 s1, s1, 0x800"] * head_salu
    out += ["\ts_cmp_lg_u32 s2, 0", "\ts_cbranch_scc1 .LBB0_3"]
    # the rolled path: a loop of its own with one reduction end, far longer than the branch over it
    out += [".LBB0_2:", "\tv_add_f32_e32 v1, v2, v3"] + ["\tv_mov_b32_e32 v9, v9"] * 40
    out += ["\tv_readlane_b32 s3, v20, 63", "\ts_cbranch_scc0 .LBB0_2", "\ts_branch .LBB0_4"]
    out += [".LBB0_3:                                ; the unrolled block"]
    for jj in range(16):
        out += ["\tv_add_f32_e32 v1, v2, v3", "\tds_read_b64 v[2:3], v20 offset:2048",
                "\tv_max_f32_dpp v23, v22, v22 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1",
                "\ts_nop 1", "\tv_readlane_b32 s3, v20, 63  ; step %d" % jj]
    out += ["\tv_add_f32_e32 v1, v2, v3", "\tds_write_b32 v20, v18 offset:59392"]
    out += [".LBB0_4:", "\ts_waitcnt lgkmcnt(0)", "\ts_barrier"]
    out += ["\ts_add_i32 s0, s0, -1"] * tail_salu
    out += ["\ts_cmp_lg_u32 s0, 0", "\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm", ".Lfunc_end0:"]
    return "\n".join(out)


def test_parse_skips_labels_comments_and_directives():
    ins, labels = I.parse(I.function_lines(listing(2, 3), "kern"))
    assert ins[0] == ("s_mov_b32", "s0, 4")
    assert labels[".LBB0_1"] == 1
    assert all(not op.startswith((".", ";")) for op, _ in ins)
    assert I.slots(("s_nop", "1")) == 2 and I.slots(("v_add_f32_e32", "v1, v2, v3")) == 1
    assert I.is_red_end(("v_readlane_b32", "s3, v20, 63")) and not I.is_red_end(("v_readlane_b32", "s3, v20, 15"))


def test_edge_report_counts_steps_and_edge_path():
    head, tail = 2, 3
    rep = I.edge_report(I.function_lines(listing(head, tail), "kern"))
    assert len(rep) == 1
    h, t, n, steps, edge = rep[0]
    assert n == 16
    # a step: add, read, dpp, s_nop 1 (two slots), readlane -> 5 instructions, 6 slots, from one end to the next
    assert steps == [(5, 6)] * 15
    ni, ns, c = edge
    # the edge path: readlane | add, ds_write | waitcnt, barrier, tail salu, cmp, branch | head salu, cmp,
    # branch (taken to the block) | add, read, dpp, s_nop 1 of step 0
    assert c["salu"] == tail + head + 2 and c["branch"] == 2
    assert c["waitcnt"] == 1 and c["barrier"] == 1 and c["lds"] == 2
    assert c["valu"] == 1 + 1 + 2 and c["nop"] == 1
    assert ni == 1 + 2 + 2 + tail + 2 + head + 2 + 4
    assert ns == ni + 1
