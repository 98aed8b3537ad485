"""Time the CTC lattice ops (csrc/ctc.hip) on an MI355X.

    python tools/time_ctc.py [--runs 20] [--warmup 3] [--out profiles/ctc_timing.json]

Cases at T = 1000, B = 32, C = 80, L = 100 (input lengths 700..1000, target lengths 60..100):
ctc_forward_algorithm (the value-only call), ops.ctc with alpha and beta, with the Viterbi path,
ops.ctc_grad on the stored tables, and CTCLogLik forward + backward.  The yardstick is torch's own
F.ctc_loss forward and forward + backward on the same device and inputs.  HIP events around each
call, warm-up first, the median of the timed runs.  Prints one JSON object and writes it to --out.
Needs a GPU: there is no fall-back.
"""
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import ops  # noqa: E402
from pytorch_hmm_amd.alignment import ctc_forward_algorithm  # noqa: E402
from pytorch_hmm_amd.autograd import CTCLogLik  # noqa: E402

_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "ctc.hip")).read()


def const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    T, B, C, L = 1000, 32, 80, 100
    rng = np.random.default_rng(0)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, C)).astype(np.float32)), 2).to(dev)
    tg = torch.from_numpy(rng.integers(1, C, (B, L))).to(dev)
    il = torch.from_numpy(rng.integers(700, T + 1, B))
    tl = torch.from_numpy(rng.integers(60, L + 1, B))
    il[0], tl[0] = T, L
    loglik, alpha, beta, _, _ = ops.ctc(lp, tg, il, tl, 0, alpha=True, beta=True)
    leaf = lp.clone().requires_grad_()

    def ours_fwd_bwd():
        leaf.grad = None
        (-CTCLogLik.apply(leaf, tg, il, tl, 0).sum()).backward()

    def torch_fwd_bwd():
        leaf.grad = None
        F.ctc_loss(leaf, tg, il, tl, blank=0, reduction="sum").backward()

    cases = {
        "ctc_value_only": lambda: ctc_forward_algorithm(lp, tg, il, tl, 0),
        "ctc_alpha_beta": lambda: ops.ctc(lp, tg, il, tl, 0, alpha=True, beta=True),
        "ctc_viterbi": lambda: ops.ctc(lp, tg, il, tl, 0, viterbi=True),
        "ctc_grad": lambda: ops.ctc_grad(alpha, beta, loglik, tg, il, tl, C, 0),
        "ctc_loglik_forward_backward": ours_fwd_bwd,
        "torch_ctc_loss_forward": lambda: F.ctc_loss(lp, tg, il, tl, blank=0, reduction="sum"),
        "torch_ctc_loss_forward_backward": torch_fwd_bwd,
    }
    out = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup,
           "timer": "HIP events around one call (argument checks, allocation of outputs and workspace included)",
           "shape": {"T": T, "B": B, "C": C, "L": L, "input_lengths": "700..1000", "target_lengths": "60..100"},
           "threads": const("kCtcThreads"), "positions_per_thread": const("kCtcPos"), "ahead": const("kCtcAhead"),
           "cases": {}}
    for name, fn in cases.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(a.runs)]
        out["cases"][name] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                              "ms_max": round(max(ms), 4)}
    # the same value from both: torch's loss is -loglik
    ref = F.ctc_loss(lp, tg, il, tl, blank=0, reduction="none")
    mine = ctc_forward_algorithm(lp, tg, il, tl, 0)
    out["loglik_of_sequence_0"] = {"hmm355": float(mine[0]), "torch": -float(ref[0])}
    out["max_abs_loglik_difference_from_torch"] = float((ref.double() + mine.double()).abs().max())
    c = out["cases"]
    out["ratio_to_torch"] = {
        "forward": round(c["ctc_value_only"]["ms_per_call"] / c["torch_ctc_loss_forward"]["ms_per_call"], 3),
        "forward_backward": round(c["ctc_loglik_forward_backward"]["ms_per_call"] /
                                  c["torch_ctc_loss_forward_backward"]["ms_per_call"], 3)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
