"""Time the duration-penalty Viterbi (csrc/dchmm.hip) on an MI355X.

    python tools/time_dchmm.py [--runs 20] [--warmup 3] [--out profiles/dchmm_timing.json]

Shapes: B = 16, T = 1000, S = 64 with the batch coupled (one workgroup) and per_sequence (16
workgroups), and B = 32, T = 2000, S = 128 coupled, which is the B * S limit.  min_duration 3,
max_duration 30.  Two yardsticks on the same device and inputs:
  1. torch_per_step: the same recursion written with torch ops, one (B,S,S) broadcast maximum per
     step and a gather per step for the backtrace: several launches per step.
  2. ops.viterbi with a dense plan at the same B, T, S: the same S * S candidates per cell and
     step without the counters and penalties (log_delta included, which that op always writes).
HIP events around each call, warm-up first, the median of the timed runs (the torch restatement
is slow: --yard-runs, default 3, after one warm-up).  Prints one JSON object and writes it to
--out.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_per_step(e, lT, mn, mx, w=0.1, per_sequence=False):
    """The recursion of include/hmm355.h in torch ops.  torch.max on the GPU does not promise the
    first index among equal maxima, so on exact ties its states may differ from the kernel's."""
    B, T, S = e.shape
    dev = e.device
    negw = torch.tensor(-w, dtype=torch.float32, device=dev)
    none = torch.tensor(-0.0, dtype=torch.float32, device=dev)
    eye = torch.eye(S, dtype=torch.bool, device=dev)[None]
    ar = torch.arange(S, device=dev)[None]
    delta = e[:, 0] - math.log(S)
    dur = torch.ones((B, S), dtype=torch.int32, device=dev)
    psi = torch.zeros((B, T, S), dtype=torch.int64, device=dev)
    for t in range(1, T):
        if per_sequence:
            dmax1, dmin = dur + 1, dur
        else:
            dmax1, dmin = dur.amax(0, keepdim=True) + 1, dur.amin(0, keepdim=True)
        pen_self = torch.where(dmax1 > mx, negw * (dmax1 - mx).float(), none)
        pen_from = torch.where(dmin < mn, negw * (mn - dmin).float(), none)
        et = e[:, t]
        cand = ((delta[:, :, None] + lT[None]) + et[:, None, :]) + pen_from[:, :, None]
        own = (delta + et) + pen_self
        cand = torch.where(eye, own[:, None, :], cand)
        delta, arg = cand.max(dim=1)
        dead = delta == float("-inf")
        arg = torch.where(dead, 0, arg)
        dur = torch.where(dead, 0, torch.where(arg == ar, dur + 1, 1)).to(torch.int32)
        psi[:, t] = arg
    states = torch.empty((B, T), dtype=torch.int64, device=dev)
    states[:, T - 1] = delta.argmax(dim=1)
    for t in range(T - 2, -1, -1):
        states[:, t] = psi[:, t + 1].gather(1, states[:, t + 1, None])[:, 0]
    return states


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yard-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dchmm_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    mn, mx = 3, 30
    out = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup, "yardstick_runs": a.yard_runs,
           "timer": "HIP events around one call (argument checks, allocation of outputs and workspace included)",
           "min_duration": mn, "max_duration": mx, "cases": {}}
    for name, B, T, S, alone in (("B16_T1000_S64_coupled", 16, 1000, 64, False),
                                 ("B16_T1000_S64_per_sequence", 16, 1000, 64, True),
                                 ("B32_T2000_S128_coupled", 32, 2000, 128, False)):
        rng = np.random.default_rng(S)
        e = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, S)).astype(np.float32)), 2).to(dev)
        lT = torch.log(torch.softmax(torch.from_numpy(rng.standard_normal((S, S)).astype(np.float32)), 1) + 1e-8).to(dev)
        init = torch.full((S,), -math.log(S), device=dev)
        plan = ops.make_plan(lT, dense=True)
        fns = {
            "dchmm": (lambda: ops.duration_constrained_viterbi(e, lT, mn, mx, 0.1, alone), a.warmup, a.runs),
            "dchmm_with_trellis": (lambda: ops.duration_constrained_viterbi(e, lT, mn, mx, 0.1, alone, True), a.warmup, a.runs),
            "ops_viterbi_dense": (lambda: ops.viterbi(e, lT, init, ops.OBS_LOG, plan), a.warmup, a.runs),
            "torch_per_step": (lambda: torch_per_step(e, lT, mn, mx, 0.1, alone), 1, a.yard_runs),
        }
        c = {"B": B, "T": T, "S": S, "per_sequence": alone}
        for key, (fn, warm, runs) in fns.items():
            for _ in range(warm):
                fn()
            torch.cuda.synchronize()
            ms = [timed(fn) for _ in range(runs)]
            c[key] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                      "ms_max": round(max(ms), 4)}
        mine = ops.duration_constrained_viterbi(e, lT, mn, mx, 0.1, alone)[0]
        c["frames_where_torch_per_step_decodes_other_states"] = int((mine != torch_per_step(e, lT, mn, mx, 0.1, alone)).sum())
        c["ratio_to_torch_per_step"] = round(c["dchmm"]["ms_per_call"] / c["torch_per_step"]["ms_per_call"], 5)
        c["ratio_to_ops_viterbi_dense"] = round(c["dchmm"]["ms_per_call"] / c["ops_viterbi_dense"]["ms_per_call"], 3)
        c["us_per_step"] = round(1000 * c["dchmm"]["ms_per_call"] / T, 3)
        out["cases"][name] = c
        print(name, json.dumps(c), flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
