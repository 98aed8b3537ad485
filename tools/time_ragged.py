"""Time forward-backward and Viterbi over a padded batch with per-sequence lengths
(csrc/ragged.hip) on an MI355X.

    python tools/time_ragged.py [--runs 20] [--warmup 3] [--out profiles/ragged_timing.json]

B = 32, Tmax = 2000, N = 128, left-to-right 0.7; lengths uniform in [200, 2000], fixed seed.
Three forms of each of forward-backward (posterior only, mask 1) and Viterbi, alternating in one
run:
  (a) ragged     ops.forward_backward_ragged / ops.viterbi_ragged on the padded batch;
  (b) loop       the only correct alternative without lengths: the tuned ops (with the model's
                 plan) called once per sequence on obs[b:b+1, :len_b];
  (c) padded     the tuned ops on the whole padded batch.  Their result is WRONG for the shorter
                 sequences: the cost yardstick only.
HIP events around each form, warm-up first, the median of the timed runs and their spread.  Prints
one JSON object and writes it to --out.  Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import ops  # noqa: E402
from pytorch_hmm_amd.utils import create_left_to_right_matrix  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, N = 32, 2000, 128
    rng = np.random.default_rng(0)
    lengths = torch.from_numpy(rng.integers(200, T + 1, B))
    obs = torch.from_numpy(rng.random((B, T, N), dtype=np.float32)).to(dev)
    P = create_left_to_right_matrix(N, 0.7)
    P = P / P.sum(1, keepdim=True)
    log_P = torch.log(P + 1e-8).to(dev)
    log_p0 = torch.log(torch.ones(N) / N + 1e-8).to(dev)
    plan = ops.make_plan(log_P)
    slices = [obs[b:b + 1, :int(n)].contiguous() for b, n in enumerate(lengths)]

    def fb_loop():
        for x in slices:
            ops.forward_backward(x, log_P, log_p0, ops.OBS_PROB, ops.FB_POSTERIOR, plan)

    def vit_loop():
        for x in slices:
            ops.viterbi(x, log_P, log_p0, ops.OBS_PROB, plan)

    cases = {
        "fb_ragged": lambda: ops.forward_backward_ragged(obs, log_P, log_p0, ops.OBS_PROB, lengths, ops.FB_POSTERIOR),
        "fb_loop_per_sequence": fb_loop,
        "fb_padded_tuned": lambda: ops.forward_backward(obs, log_P, log_p0, ops.OBS_PROB, ops.FB_POSTERIOR, plan),
        "viterbi_ragged": lambda: ops.viterbi_ragged(obs, log_P, log_p0, ops.OBS_PROB, lengths),
        "viterbi_loop_per_sequence": vit_loop,
        "viterbi_padded_tuned": lambda: ops.viterbi(obs, log_P, log_p0, ops.OBS_PROB, plan),
    }
    for _ in range(a.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.runs):   # the forms alternate within one run
        for k, fn in cases.items():
            ms[k].append(timed(fn))
    steps = int(lengths.max())
    out = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup,
           "timer": "HIP events around one form (argument checks, the host read of the lengths, allocation of "
                    "outputs and workspace included); the forms alternate within a run",
           "shape": {"B": B, "Tmax": T, "N": N, "matrix": "left-to-right 0.7", "obs_mode": "OBS_PROB",
                     "lengths": "uniform in [200, 2000], seed 0", "longest": steps,
                     "frames_valid": int(lengths.sum()), "frames_padded": B * T},
           "note": "*_padded_tuned computes a wrong result for the shorter sequences: the cost yardstick only",
           "cases": {k: {"ms_per_call": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                         "ms_max": round(max(v), 4)} for k, v in ms.items()}}
    c = {k: v["ms_per_call"] for k, v in out["cases"].items()}
    out["us_per_step_of_the_longest_sequence"] = {"fb_ragged": round(1e3 * c["fb_ragged"] / steps, 4),
                                                  "viterbi_ragged": round(1e3 * c["viterbi_ragged"] / steps, 4)}
    out["ratio_loop_to_ragged"] = {"fb": round(c["fb_loop_per_sequence"] / c["fb_ragged"], 2),
                                   "viterbi": round(c["viterbi_loop_per_sequence"] / c["viterbi_ragged"], 2)}
    out["ratio_ragged_to_padded_tuned"] = {"fb": round(c["fb_ragged"] / c["fb_padded_tuned"], 2),
                                           "viterbi": round(c["viterbi_ragged"] / c["viterbi_padded_tuned"], 2)}
    out["condition_ragged_not_slower_than_loop"] = {"fb": c["fb_ragged"] <= c["fb_loop_per_sequence"],
                                                    "viterbi": c["viterbi_ragged"] <= c["viterbi_loop_per_sequence"]}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
