"""Diagnostic: cycles and shader clock of the banded chain waves (HMM355_STAMP=1 build,
recur.h band_chain), each op alone and both ops side by side on two streams.
Build here:  [STAMP_LIB=path] [STAMP_DEFINES="A=1 B=2"] python tools/band_stamps.py build [items]     Run on the GPU box: [STAMP_LIB=path] python tools/band_stamps.py [f]
(f: the work beside the chains on; items: also the staging helpers' work by item and the psi waves).  Per chain: cycles per step, cycles per step at the block
barriers (waiting for the helpers), and the clock (s_memtime cycles / s_memrealtime at 100 MHz); the chain's whole blocks by
part (steps 1 .. 15 | step 0 and the block edge: `edges`); the forward-backward launch's staging waves by chain.
STAMP_DEFINES="HMM355_STAMP_BAR=0" leaves out the stamps round the chain's block barrier."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("STAMP_LIB", os.path.join(HERE, "ablate_libs", "libhmm355_stamp.so"))
if sys.argv[1:2] == ["build"]:
    # `build items`: HMM355_STAMP=2, which also stamps the staging helpers' block work by item and
    # the psi waves; those stamps slow the helpers, so the chains' figures come from a plain build
    sys.path.insert(0, os.path.dirname(HERE))
    from pytorch_hmm_amd import build_native as bn
    level = 2 if sys.argv[2:] == ["items"] else 1
    # STAMP_DEFINES: further defines, e.g. "HMM355_EMIS_AHEAD_BETA=2" or "HMM355_ABL=134217728" (wrong results)
    extra = os.environ.get("STAMP_DEFINES", "").split()
    print(bn.build(force=True, defines=[f"HMM355_STAMP={level}", *extra], out=LIB, sources=bn.RECURSION_SOURCES))
    sys.exit(0)
import numpy as np
import torch

FOLLOW = len(sys.argv) > 1 and "f" in sys.argv[1]
sys.argv = [sys.argv[0]] + [LIB + ":" + (sys.argv[1] if len(sys.argv) > 1 else "")]
sys.path.insert(0, HERE)
import time_follow as tf  # noqa: E402  (builds the inputs and the two op closures)

L = ctypes.CDLL(LIB)
fb, vit = tf.make(sys.argv[1])
NW = 16  # stamp slots per workgroup (recur.h band_chain / rec_band, follow.h)


def raw(tag, nblk):
    sym = getattr(L, f"hmm355_debug_stamps_{tag}")
    sym.argtypes = [ctypes.c_void_p, ctypes.c_int]
    n = 512 * 16 * 8
    buf = (ctypes.c_ulonglong * n)()
    assert sym(buf, n) == 0
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, NW, 8)[:nblk, 0].astype(np.float64)


def timeline(name, chains, fol, nstamp):
    """real-time (us) of each chain's end, its final publish, and its follower's stamps,
    from the earliest chain start; medians over the sequences"""
    t0 = chains[:, 0].min()
    med = lambda x: float(np.median(x))
    msg = (f"  {name:10s} chain start {med(chains[:, 0] - t0) / 100:6.1f} end {med(chains[:, 1] - t0) / 100:6.1f}"
           f" (max {(chains[:, 1] - t0).max() / 100:6.1f}) publish {med(chains[:, 2] - t0) / 100:6.1f}")
    if fol is not None:
        msg += "  follower " + " ".join(f"{med(fol[:, k] - t0) / 100:6.1f}" for k in range(nstamp))
        msg += f" (last exit {(fol[:, nstamp - 1] - t0).max() / 100:6.1f})"
    print(msg, flush=True)


def chain_exit(name, tag, nblk, t0):
    """real-time (us) of the chain workgroups' exit (helper 0, wave 1, its stores retired): median
    and last; a build without that stamp leaves the entry 0"""
    sym = getattr(L, f"hmm355_debug_stamps_{tag}")
    sym.argtypes = [ctypes.c_void_p, ctypes.c_int]
    n = 512 * 16 * 8
    buf = (ctypes.c_ulonglong * n)()
    assert sym(buf, n) == 0
    x = np.frombuffer(buf, dtype=np.uint64).reshape(-1, NW, 8)[:nblk, 1, 2].astype(np.float64)
    if x.min() <= 0:
        print(f"  {name:10s} chain workgroups' exit: not stamped by this build")
    else:
        print(f"  {name:10s} chain workgroups' exit {float(np.median(x - t0)) / 100:6.1f} (last {(x - t0).max() / 100:6.1f})", flush=True)


def helpers(name, tag, nblk, waves, psi=(), blocks=None):
    """cycles per block of the staging helpers' work, whole and by item, and their wait at the
    block barrier; the same two for the psi waves of the fused Viterbi chain (blocks: the
    workgroups to average over, e.g. one chain's of the forward-backward launch)"""
    sym = getattr(L, f"hmm355_debug_stamps_{tag}")
    sym.argtypes = [ctypes.c_void_p, ctypes.c_int]
    n = 512 * 16 * 8
    buf = (ctypes.c_ulonglong * n)()
    assert sym(buf, n) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(-1, NW, 8)[:nblk].astype(np.float64)
    if blocks is not None:
        a = a[blocks]
    for w in waves:
        nb = np.maximum(a[:, w, 4], 1)
        item = [np.mean(a[:, w, k] / nb) for k in (3, 5, 6, 7)]  # (0 unless the build stamps them: `build items`)
        print(f"  {name:10s} helper wave {w:2d}: work/block {np.mean(a[:, w, 0] / nb):7.0f}  wait/block {np.mean(a[:, w, 1] / nb):7.0f}"
              + (f"  stage+load {item[0]:6.0f}  flush {item[1]:6.0f}  psi copy {item[2]:6.0f}  poll+publish {item[3]:6.0f}"
                 if max(item) > 0 else ""))
    for w in psi:
        if a[:, w, 4].max() <= 0:
            continue  # (not stamped by this build)
        nb = np.maximum(a[:, w, 4], 1)
        print(f"  {name:10s} psi wave    {w:2d}: work/block {np.mean(a[:, w, 0] / nb):7.0f}  wait/block {np.mean(a[:, w, 1] / nb):7.0f}")


def edges(name, tag, blocks):
    """the chain wave's whole blocks by part (recur.h band_chain, the record of wave 4): cycles per
    steady step (top of step 1 to behind step 15, / 15; the block barrier's wait where it stands
    inside those steps taken out), cycles per edge (the rest of a block: step 0 and what stands
    between two blocks, the barrier's wait where it stands there taken out) and the edge's excess
    over a steady step as cycles a step (/ 16)"""
    sym = getattr(L, f"hmm355_debug_stamps_{tag}")
    sym.argtypes = [ctypes.c_void_p, ctypes.c_int]
    n = 512 * 16 * 8
    buf = (ctypes.c_ulonglong * n)()
    assert sym(buf, n) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(-1, NW, 8).astype(np.float64)
    e, c = a[blocks, 4], a[blocks, 0]
    if e[:, 1].min() <= 0 or e[:, 3].min() <= 0:
        print(f"  {name:10s} block parts: not stamped by this build")
        return
    bar_in = e[:, 4] / e[:, 1]                        # barrier wait inside steps 1 .. 15, per block
    bar_out = (c[:, 3] - e[:, 4]) / (c[:, 4] / 16.0)  # the other barriers' wait, per block (all blocks)
    steady = (e[:, 0] / e[:, 1] - bar_in) / 15.0
    edge = e[:, 2] / e[:, 3] - (bar_out if bar_in.mean() < 1 else 0.0)
    print(f"  {name:10s} steady step {steady.mean():6.1f} (min {steady.min():6.1f} max {steady.max():6.1f})  "
          f"edge (step 0 + block edge) {edge.mean():6.1f} (min {edge.min():6.1f} max {edge.max():6.1f})  "
          f"edge over a steady step, per step {((edge - steady) / 16.0).mean():5.1f}  "
          f"barrier wait/block {(bar_in + bar_out).mean():5.0f}", flush=True)


def read(tag, nblk):
    sym = getattr(L, f"hmm355_debug_stamps_{tag}")
    sym.argtypes = [ctypes.c_void_p, ctypes.c_int]
    n = 512 * 16 * 8
    buf = (ctypes.c_ulonglong * n)()
    assert sym(buf, n) == 0
    a = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8)[: nblk * NW].reshape(nblk, NW, 8)[:, 0].astype(np.float64)
    return a


def show(name, a):
    steps = np.maximum(a[:, 4], 1)
    tot = a[:, 5] / steps
    bar = a[:, 3] / steps
    clk = a[:, 6] / np.maximum(a[:, 7], 1) * 100.0
    print(f"  {name:10s} cycles/step {tot.mean():7.1f} (max {tot.max():7.1f})  barrier/step {bar.mean():6.1f}"
          f"  clock MHz {np.median(clk):6.0f} (min {clk.min():6.0f})  chain us {np.median(a[:, 7]) / 100:7.1f}", flush=True)


B = tf.B
cur = torch.cuda.current_stream(tf.dev)
for mode in ("fb", "vit", "both"):
    for _ in range(3):
        if mode == "fb":
            fb(cur)
        elif mode == "vit":
            vit(cur)
        else:
            tf.both(fb, vit)
    torch.cuda.synchronize()
    print(mode, flush=True)
    fl = FOLLOW
    if mode in ("fb", "both"):
        a = read("fb", 2 * B)
        show("alpha", a[0::2])
        show("beta", a[1::2])
        edges("alpha", "fb", np.arange(0, 2 * B, 2))
        edges("beta", "fb", np.arange(1, 2 * B, 2))
        helpers("fb", "fb", 2 * B, (1, 2, 3))
        if mode == "fb":  # every staging wave of the launch, by chain
            helpers("fb alpha", "fb", 2 * B, (1, 2, 3, 5, 6, 7, 9, 10, 11), blocks=np.arange(0, 2 * B, 2))
            helpers("fb beta", "fb", 2 * B, (1, 2, 3, 5, 6, 7, 9, 10, 11), blocks=np.arange(1, 2 * B, 2))
        r = raw("fb", 4 * B)
        ch = r[:2 * B].reshape(B, 2, 8)
        late = np.where(ch[:, 0, 1:2] >= ch[:, 1, 1:2], ch[:, 0], ch[:, 1])  # the later chain of each pair
        timeline("fb", late, r[2 * B:3 * B] if fl else None, 3)
        if fl:
            timeline("fb f1", late, r[3 * B:], 3)
        chain_exit("fb", "fb", 2 * B, late[:, 0].min())
    if mode in ("vit", "both"):
        show("viterbi", read("vit", B))
        edges("viterbi", "vit", np.arange(B))
        helpers("vit", "vit", B, (1, 2, 3, 9, 10, 11), (5, 6, 7, 13, 14, 15))
        r = raw("vit", 2 * B)
        timeline("vit", r[:B], r[B:] if fl else None, 4)
        chain_exit("vit", "vit", B, r[:B, 0].min())
