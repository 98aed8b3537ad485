"""Checks the DPP and v_readlane wait states in gfx950 listings of the six banded chain units.

    python tools/check_dpp_hazards.py                 compiles fb_np64/128/256 and vit_np64/128/256
                                                      with build_native's flags and checks them
    python tools/check_dpp_hazards.py a.s b.s ...     checks the given listings
    [HAZ_DEFINES="A=1 B=2"] further defines for the compile

The rules, on the instruction stream as it is listed (an `s_nop n` counts as n + 1 instructions,
every other instruction as one; labels, directives and comments as none, so the instructions of an
asm statement count like the compiler's own; the stream restarts behind an unconditional branch
or the end of a program):
  * a DPP instruction: neither of the two instructions before it is a VALU instruction that wrote
    the register it reads through DPP (its first source operand);
  * v_readlane: the instruction before it is no VALU write of the VGPR it reads, and neither of the
    two instructions behind it is a VALU instruction that reads the SGPR it wrote.
A listing the compiler padded itself reports nothing; the rules are there for the instructions it
does not pad, those of asm statements.  Exit status 1 if anything is reported."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
UNITS = ["fb_np64", "fb_np128", "fb_np256", "vit_np64", "vit_np128", "vit_np256"]
_REG = re.compile(r"\b([vs])(?:(\d+)|\[(\d+):(\d+)\])")
_CARRY_OUT = ("v_mad_u64_u32", "v_mad_i64_i32", "v_add_co_", "v_sub_co_", "v_subrev_co_", "v_addc_co_", "v_subb_co_",
              "v_subbrev_co_", "v_div_scale_")
_RESTART = ("s_branch", "s_endpgm", "s_setpc_b64")


def regs(text, kind):
    """the registers of one kind ('v' or 's') named in an operand: a set of numbers"""
    out = set()
    for k, one, lo, hi in _REG.findall(text):
        if k == kind:
            out.update([int(one)] if one else range(int(lo), int(hi) + 1))
    return out


def parse(line):
    """(mnemonic, operands) of an instruction line, None for anything else"""
    t = line.split(";", 1)[0].strip()
    if not t or t.startswith(".") or t.endswith(":") or t.startswith("//"):
        return None
    m = re.match(r"([a-z_][a-z0-9_]*)\s*(.*)$", t)
    if not m:
        return None
    ops = [o.strip() for o in m.group(2).split(",")] if m.group(2) else []
    return m.group(1), ops


def valu_writes(mn, ops):
    """the VGPRs a VALU instruction writes"""
    if not mn.startswith("v_") or not ops:
        return set()
    if mn.startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
        return set()
    w = regs(ops[0], "v")
    if "permlane" in mn and "swap" in mn and len(ops) > 1:
        w |= regs(ops[1], "v")
    return w


def check(lines, name="<listing>"):
    """the violations in a listing: a list of strings"""
    found = []
    hist = []          # the slots before the current instruction, latest last: (lineno, mnemonic, operands) or None for a pad
    pending = []       # [slots left, sgpr set, lineno] of the v_readlane instructions still to be watched
    for no, line in enumerate(lines, 1):
        p = parse(line)
        if p is None:
            continue
        mn, ops = p
        if mn == "s_nop":
            n = int(ops[0], 0) + 1 if ops else 1
            hist.extend([None] * n)
            for q in pending:
                q[0] -= n
            pending = [q for q in pending if q[0] > 0]
            continue
        if mn.startswith("v_"):
            for q in pending:
                # (the second operand of the carry-out forms is an SGPR pair they write)
                first = 2 if mn.startswith(_CARRY_OUT) else 1
                read = set().union(*[regs(o, "s") for o in ops[first:]]) if len(ops) > first else set()
                if read & q[1]:
                    found.append(f"{name}:{no}: {mn} reads s{sorted(read & q[1])[0]} {3 - q[0]} slot(s) behind the "
                                 f"v_readlane of line {q[2]} (2 needed)")
        for q in pending:
            q[0] -= 1
        pending = [q for q in pending if q[0] > 0]
        if mn.endswith("_dpp") and len(ops) >= 2:
            src = regs(ops[1], "v")
            for back, h in enumerate(reversed(hist[-2:]), 1):
                if h and valu_writes(h[1], h[2]) & src:
                    found.append(f"{name}:{no}: {mn} reads v{sorted(src)[0]} through DPP {back - 1} slot(s) behind its "
                                 f"write by {h[1]} in line {h[0]} (2 needed)")
                    break  # (the nearest write: one report an instruction)
        if mn == "v_readlane_b32" and len(ops) >= 2:
            src = regs(ops[1], "v")
            h = hist[-1] if hist else None
            if h and valu_writes(h[1], h[2]) & src:
                found.append(f"{name}:{no}: v_readlane_b32 reads v{sorted(src)[0]} right behind its write by {h[1]} in "
                             f"line {h[0]} (1 slot needed)")
            pending.append([2, regs(ops[0], "s"), no])
        if mn in _RESTART:
            hist, pending = [], []
        else:
            hist.append((no, mn, ops))
            del hist[:-4]
    return found


def compile_units(outdir):
    sys.path.insert(0, os.path.dirname(HERE))
    from pytorch_hmm_amd import build_native as bn
    paths = []
    for u in UNITS:
        out = os.path.join(outdir, u + ".s")
        cmd = [bn._hipcc(), *bn.FLAGS, *["-D" + d for d in os.environ.get("HAZ_DEFINES", "").split()],
               "--cuda-device-only", "-S", os.path.join(bn.CSRC, u + ".hip"), "-o", out]
        subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
        paths.append(out)
    return paths


def main(argv):
    with tempfile.TemporaryDirectory() as tmp:
        paths = argv or compile_units(tmp)
        total = 0
        for p in paths:
            with open(p) as f:
                lines = f.readlines()
            found = check(lines, os.path.basename(p))
            ndpp = sum(1 for ln in lines if (q := parse(ln)) and q[0].endswith("_dpp"))
            nrl = sum(1 for ln in lines if (q := parse(ln)) and q[0] == "v_readlane_b32")
            for v in found:
                print(v)
            print(f"{os.path.basename(p)}: {ndpp} DPP instructions, {nrl} v_readlane, {len(found)} reported", flush=True)
            total += len(found)
    print("nothing reported" if total == 0 else f"{total} reported")
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
