"""tools/check_dpp_hazards.py: its parser and rules on short hand-written listings (no GPU)."""
import importlib.util
import os

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_dpp_hazards.py")
_spec = importlib.util.spec_from_file_location("check_dpp_hazards", _PATH)
haz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(haz)

DPP = " row_mask:0xf bank_mask:0xf bound_ctrl:1"


def listing(*instrs):
    return ["\t.text\n", "kernel:                                 ; @kernel\n", "; %bb.0:\n"] + ["\t" + i + "\n" for i in instrs]


def test_parse_skips_what_is_no_instruction():
    assert haz.parse("\t.p2align 8\n") is None
    assert haz.parse(".LBB0_3:\n") is None
    assert haz.parse("\t;;#ASMSTART\n") is None
    assert haz.parse("\t; sched_barrier mask(0x00000000)\n") is None
    assert haz.parse("\tv_max_f32_dpp v2, v4, v2 row_shr:2" + DPP + " ; note\n") == (
        "v_max_f32_dpp", ["v2", "v4", "v2 row_shr:2" + DPP])
    assert haz.regs("v[14:15]", "v") == {14, 15} and haz.regs("s[2:3]", "s") == {2, 3} and haz.regs("v7", "s") == set()


def test_dpp_read_right_behind_the_write_is_reported():
    got = haz.check(listing("v_max_f32_e32 v25, v14, v15", "v_max_f32_dpp v25, v25, v25 quad_perm:[1,0,3,2]" + DPP))
    assert len(got) == 1 and "v25 through DPP" in got[0] and ":5:" in got[0]
    # one instruction between is one slot: still short
    got = haz.check(listing("v_max_f32_e32 v25, v14, v15", "v_add_f32_e32 v1, v2, v3", "v_max_f32_dpp v25, v25, v25 row_ror:4" + DPP))
    assert len(got) == 1


def test_s_nop_1_cures_it_and_s_nop_0_does_not():
    write, read = "v_max_f32_e32 v25, v14, v15", "v_max_f32_dpp v25, v25, v25 row_ror:8" + DPP
    assert haz.check(listing(write, "s_nop 1", read)) == []
    assert len(haz.check(listing(write, "s_nop 0", read))) == 1
    assert haz.check(listing(write, "s_nop 0", "ds_write_b64 v23, v[18:19] offset:27136", read)) == []
    assert haz.check(listing(write, "v_add_f32_e32 v1, v2, v3", "s_waitcnt lgkmcnt(2)", read)) == []


def test_only_the_register_read_through_dpp_counts():
    # the accumulator (src1) was just written, the shifted register (src0) is settled
    assert haz.check(listing("v_add_f32_e32 v4, v1, v1", "s_nop 1", "v_max_f32_dpp v2, v4, v4 row_shr:1" + DPP,
                             "v_max_f32_dpp v2, v4, v2 row_shr:2" + DPP, "v_max_f32_dpp v2, v4, v2 row_shr:3" + DPP)) == []
    # a write of a 64-bit pair covers both registers
    assert len(haz.check(listing("v_lshlrev_b64 v[4:5], 5, v[2:3]", "v_mov_b32_dpp v1, v5 row_shr:1" + DPP))) == 1


def test_asm_written_source():
    # the instructions of an asm statement count as any other: the markers are comments
    asm = [";;#ASMSTART", "v_max_f32_dpp v2, v4, v2 row_shr:2" + DPP, "v_max_f32_dpp v2, v4, v2 row_shr:3" + DPP, ";;#ASMEND"]
    nxt = "v_max_f32_dpp v3, v2, v2 row_shr:4" + DPP
    got = haz.check(listing("v_max_f32_dpp v2, v4, v4 row_shr:1" + DPP, *asm, nxt))
    assert len(got) == 1 and "v2 through DPP" in got[0]
    assert len(haz.check(listing("v_max_f32_dpp v2, v4, v4 row_shr:1" + DPP, *asm, "ds_read_b64 v[14:15], v24 offset:4096", nxt))) == 1
    assert haz.check(listing("v_max_f32_dpp v2, v4, v4 row_shr:1" + DPP, *asm, "s_nop 1", nxt)) == []
    assert haz.check(listing("v_max_f32_dpp v2, v4, v4 row_shr:1" + DPP, *asm, "ds_read_b64 v[14:15], v24 offset:4096",
                             "v_add_f32_e32 v26, v6, v18", nxt)) == []


def test_v_readlane_ahead_and_behind():
    lvl = "v_max_f32_dpp v25, v25, v25 row_bcast:31" + DPP
    rl = "v_readlane_b32 s2, v25, 63"
    pre = ["v_mov_b32_e32 v25, v1", "s_nop 1"]
    assert len(haz.check(listing(*pre, lvl, rl))) == 1                      # no slot ahead
    assert haz.check(listing(*pre, lvl, "s_nop 0", rl)) == []
    use = "v_max_f32_e32 v26, s2, v27"
    assert len(haz.check(listing(*pre, lvl, "s_nop 0", rl, use))) == 1       # read right behind
    assert len(haz.check(listing(*pre, lvl, "s_nop 0", rl, "v_add_f32_e32 v14, v14, v4", use))) == 1
    assert haz.check(listing(*pre, lvl, "s_nop 0", rl, "v_add_f32_e32 v14, v14, v4", "v_add_f32_e32 v15, v15, v8", use)) == []
    assert haz.check(listing(*pre, lvl, "s_nop 0", rl, "s_nop 1", use)) == []
    # an asm v_writelane reads the SGPR as a VALU instruction does; another SGPR is no matter
    assert len(haz.check(listing(*pre, lvl, "s_nop 0", rl, ";;#ASMSTART", "v_writelane_b32 v22, s2, 1", ";;#ASMEND"))) == 1
    assert haz.check(listing(*pre, lvl, "s_nop 0", rl, "v_max_f32_e32 v26, s3, v27", "s_nop 0", use)) == []
    # the carry-out pair of v_mad_u64_u32 is written, not read
    assert haz.check(listing(*pre, lvl, "s_nop 0", rl, "v_mad_u64_u32 v[0:1], s[2:3], s4, v2, v[4:5]")) == []
    assert len(haz.check(listing(*pre, lvl, "s_nop 0", rl, "v_mad_u64_u32 v[0:1], s[4:5], s2, v2, v[4:5]"))) == 1


def test_stream_restarts_behind_a_branch():
    assert haz.check(listing("v_max_f32_e32 v25, v14, v15", "s_branch .LBB0_2", "v_max_f32_dpp v25, v25, v25 row_ror:4" + DPP)) == []
