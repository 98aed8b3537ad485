"""Time the batch-tiled (wide) Viterbi and forward-backward ops (csrc/wide.hip) on an MI355X.

    python tools/time_wide.py [--B 32] [--T 2000] [--runs 20] [--warmup 3] [--out profiles/wide_timing.json]

For each op the wide form at N in {256, 512, 1024} and, as the yardstick, the dense narrow chain
at N = 256 (make_plan(dense=True); its code does not depend on the wide form).  HIP events around
each call, warm-up first, the median of the timed runs; the narrow and wide forms alternate run by
run.  Reports ms per call, us per time step and the step kernel's grid, prints one JSON object and
writes it to --out.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import ops  # noqa: E402

COL_TILE = 64
BT = int(re.search(r"constexpr int kBT = (\d+);",
                   open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "wide.hip")).read()).group(1))


def inputs(B, T, N, dev):
    rng = np.random.default_rng(N)
    obs = torch.from_numpy(rng.random((B, T, N), dtype=np.float32)).to(dev)
    P = torch.from_numpy(rng.random((N, N), dtype=np.float32))
    P = P / P.sum(1, keepdim=True)
    log_P = torch.log(P + 1e-8).to(dev)
    log_p0 = torch.log(torch.full((N,), 1.0 / N) + 1e-8).to(dev)
    return obs, log_P, log_p0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_wide.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    B, T = args.B, args.T

    cases = {}   # name -> (callable, grid description)
    for N in args.sizes:
        obs, log_P, log_p0 = inputs(B, T, N, dev)
        tiles = ((N + COL_TILE - 1) // COL_TILE, (B + BT - 1) // BT)
        cases[f"viterbi_wide_N{N}"] = (
            lambda o=obs, p=log_P, i=log_p0: ops.viterbi(o, p, i, ops.OBS_PROB, wide=True),
            {"N": N, "form": "wide", "op": "viterbi", "grid_per_step": [tiles[0], tiles[1], 1]})
        cases[f"fb_wide_N{N}"] = (
            lambda o=obs, p=log_P, i=log_p0: ops.forward_backward(o, p, i, ops.OBS_PROB, ops.FB_POSTERIOR, wide=True),
            {"N": N, "form": "wide", "op": "forward_backward", "grid_per_step": [tiles[0], tiles[1], 2]})
        if N == 256:
            plan = ops.make_plan(log_P, dense=True)
            cases["viterbi_narrow_dense_N256"] = (
                lambda o=obs, p=log_P, i=log_p0, pl=plan: ops.viterbi(o, p, i, ops.OBS_PROB, pl),
                {"N": N, "form": "narrow dense chain", "op": "viterbi", "grid_per_step": None})
            cases["fb_narrow_dense_N256"] = (
                lambda o=obs, p=log_P, i=log_p0, pl=plan: ops.forward_backward(o, p, i, ops.OBS_PROB,
                                                                                ops.FB_POSTERIOR, pl),
                {"N": N, "form": "narrow dense chain", "op": "forward_backward", "grid_per_step": None})

    for _ in range(args.warmup):
        for fn, _d in cases.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.runs):          # the forms alternate run by run
        for k, (fn, _d) in cases.items():
            samples[k].append(timed(fn))
    result = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "runs": args.runs, "warmup": args.warmup,
              "timer": "HIP events around one op call (allocation of outputs and workspace included)",
              "batch_tile": BT, "column_tile": COL_TILE, "cases": {}}
    for k, (fn, desc) in cases.items():
        ms = statistics.median(samples[k])
        result["cases"][k] = dict(desc, ms_per_call=round(ms, 4), us_per_step=round(1e3 * ms / T, 4),
                                  ms_min=round(min(samples[k]), 4), ms_max=round(max(samples[k]), 4))
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
