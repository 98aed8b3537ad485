"""Time the HSMM forward-backward (csrc/hsmm_fb.hip) on an MI355X.

    python tools/time_hsmm_fb.py [--runs 20] [--warmup 3] [--out profiles/hsmm_fb_timing.json]

Shape B = 16, T = 2000, S = 64, Dmax = 40 (BASELINE config 5's states and durations).  Cases: the
likelihood alone (the forward sum), the full forward-backward with all four posterior / count
outputs, and HSMMLayer.log_likelihood + backward (80 features: the Gaussian scorer, the tables
and their autograd included).  For scale, ops.hsmm_viterbi on the same tables in the same run.
HIP events around each call, warm-up first, the median of the timed runs.  Prints one JSON line
and writes it to --out.  Needs a GPU: there is no fall-back.
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

import pytorch_hmm_amd as ph  # noqa: E402
from pytorch_hmm_amd import ops  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hsmm_fb_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, S, Dm, D = 16, 2000, 64, 40, 80
    torch.manual_seed(0)
    layer = ph.HSMMLayer(S, D, max_duration=Dm).to(dev)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32)).to(dev)
    with torch.no_grad():
        lp, dur_lp, log_T = layer._segment_tables(x)
        lp, dur_lp, log_T = lp.contiguous(), dur_lp.contiguous(), log_T.contiguous()

    def layer_step():
        layer.zero_grad(set_to_none=True)
        layer.compute_loss(x).backward()

    cases = {
        "hsmm_fb_loglik_only": lambda: ops.hsmm_forward_backward(lp, dur_lp, log_T),
        "hsmm_fb_all_outputs": lambda: ops.hsmm_forward_backward(lp, dur_lp, log_T, want_gamma=True, want_dur=True,
                                                                 want_trans=True, want_init=True),
        "hsmm_fb_gamma_only": lambda: ops.hsmm_forward_backward(lp, dur_lp, log_T, want_gamma=True),
        "layer_log_likelihood_backward": layer_step,
        "hsmm_viterbi": lambda: ops.hsmm_viterbi(lp, dur_lp, log_T),
    }
    out = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup,
           "timer": "HIP events around one call (argument checks, allocation of outputs and workspace included)",
           "shape": {"B": B, "T": T, "S": S, "Dmax": Dm, "features": D}, "cases": {}}
    for name, fn in cases.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(a.runs)]
        out["cases"][name] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                              "ms_max": round(max(ms), 4)}
    ll = ops.hsmm_forward_backward(lp, dur_lp, log_T)[0]
    best = ops.hsmm_viterbi(lp, dur_lp, log_T)[1]
    out["loglik_of_sequence_0"] = float(ll[0])
    out["viterbi_score_of_sequence_0"] = float(best[0])
    text = json.dumps(out)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
