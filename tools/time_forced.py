"""Time the transcript forced-alignment ops (csrc/forced.hip) on an MI355X.

    python tools/time_forced.py [--runs 20] [--warmup 3] [--out profiles/forced_timing.json]

Cases at T = 1000, B = 32, C = 80, Smax = 201 (input lengths 700..1000, chain lengths 121..201),
ids with repeats and all three weight tensors: the value-only call, ops.forced with alpha and beta,
with the Viterbi path, ops.forced_grad on the stored tables (log_probs and the three transition
gradients) and ForcedLogLik forward + backward.  The same shape in the monotonic-alignment-search
form (no ids, no weights, value (B,T,Smax)).  Yardsticks: ops.ctc at the equal lattice width
(2 L + 1 = Smax, L = 100, the same T, B, C), and the same recursion as a plain per-frame torch loop
on the GPU (forward, and forward + backward through autograd).  HIP events around each call,
warm-up first, the median of the timed runs.  Prints one JSON object and writes it to --out.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import ops  # noqa: E402
from pytorch_hmm_amd.alignment import forced_alignment_loglik, monotonic_alignment_search  # noqa: E402
from pytorch_hmm_amd.autograd import ForcedLogLik  # noqa: E402

_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "forced.hip")).read()
BIGNEG = -1e30  # -inf of the torch loop: exp(BIGNEG - m) is exactly 0 and autograd sees no NaN


def const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_loop(lp, ids, il, sl, ws, wn, wk):
    """loglik (B) by one torch step per frame on lp's device (il, sl on that device too)."""
    B, T, C = lp.shape
    S = ids.shape[1]
    live = torch.arange(S, device=lp.device)[None, :] < sl[:, None]
    E = torch.where(live[:, None, :], lp.gather(2, ids.long()[:, None, :].expand(B, T, S)), lp.new_tensor(BIGNEG))
    pad1, pad2 = lp.new_full((B, 1), BIGNEG), lp.new_full((B, 2), BIGNEG)
    a = torch.cat([E[:, 0, :1], lp.new_full((B, S - 1), BIGNEG)], 1)
    for t in range(1, T):
        c = torch.stack([a + ws, torch.cat([pad1, (a + wn)[:, :-1]], 1), torch.cat([pad2, (a + wk)[:, :-2]], 1)])
        new = (torch.logsumexp(c.clamp(min=BIGNEG), 0) + E[:, t]).clamp(min=BIGNEG)
        a = torch.where((t < il)[:, None], new, a)
    return a.gather(1, (sl.long() - 1)[:, None])[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-runs", type=int, default=3, help="timed runs of the per-frame torch loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    T, B, C, L = 1000, 32, 80, 100
    S = 2 * L + 1
    rng = np.random.default_rng(0)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)), 2).to(dev)
    ids_np = rng.integers(0, C, (B, S))
    rep = rng.random((B, S)) < 0.2
    for i in range(1, S):
        ids_np[:, i] = np.where(rep[:, i], ids_np[:, i - 1], ids_np[:, i])
    ids = torch.from_numpy(ids_np).to(dev, torch.int32)
    il = torch.from_numpy(rng.integers(700, T + 1, B))
    sl = torch.from_numpy(rng.integers(121, S + 1, B))
    il[0], sl[0] = T, S
    w = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, S, 3)).astype(np.float32)), 2).to(dev)
    ws, wn, wk = (w[..., i].contiguous() for i in range(3))
    value = torch.from_numpy(rng.standard_normal((B, T, S)).astype(np.float32)).to(dev)
    # the CTC yardstick: the same T, B, C, a lattice of 2 L + 1 = Smax positions
    lp_tbc = lp.transpose(0, 1).contiguous()
    tg = torch.from_numpy(rng.integers(1, C, (B, L))).to(dev)
    tl = (sl - 1) // 2

    args = (lp, ids, il, sl, ws, wn, wk)
    loglik, alpha, beta = ops.forced(*args, alpha=True, beta=True)[:3]
    leaves = [t.clone().requires_grad_() for t in (lp, ws, wn, wk)]

    def ours_fwd_bwd():
        for t in leaves:
            t.grad = None
        (-ForcedLogLik.apply(leaves[0], ids, il, sl, *leaves[1:]).sum()).backward()

    ild, sld = il.to(dev), sl.to(dev)

    def loop_fwd_bwd():
        for t in leaves:
            t.grad = None
        (-torch_loop(leaves[0], ids, ild, sld, *leaves[1:]).sum()).backward()

    cases = {
        "forced_value_only": lambda: forced_alignment_loglik(*args),
        "forced_alpha_beta": lambda: ops.forced(*args, alpha=True, beta=True),
        "forced_viterbi": lambda: ops.forced(*args, viterbi=True),
        "forced_grad": lambda: ops.forced_grad(alpha, beta, loglik, *args, want_grad=True, want_stay=True,
                                               want_next=True, want_skip=True),
        "forced_loglik_forward_backward": ours_fwd_bwd,
        "mas_value_only": lambda: ops.forced(value, None, il, sl),
        "mas_alpha_beta": lambda: ops.forced(value, None, il, sl, alpha=True, beta=True),
        "mas_viterbi": lambda: monotonic_alignment_search(value, il, sl),
        "ctc_value_only": lambda: ops.ctc(lp_tbc, tg, il, tl, 0),
        "ctc_alpha_beta": lambda: ops.ctc(lp_tbc, tg, il, tl, 0, alpha=True, beta=True),
        "ctc_viterbi": lambda: ops.ctc(lp_tbc, tg, il, tl, 0, viterbi=True),
    }
    loops = {
        "torch_loop_forward": lambda: torch_loop(lp, ids, ild, sld, ws, wn, wk),
        "torch_loop_forward_backward": loop_fwd_bwd,
    }
    out = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup, "loop_runs": a.loop_runs,
           "timer": "HIP events around one call (argument checks, allocation of outputs and workspace included)",
           "shape": {"T": T, "B": B, "C": C, "Smax": S, "input_lengths": "700..1000", "state_lengths": "121..201",
                     "ctc_target_lengths": "60..100 (2 L + 1 = the chain's length)"},
           "threads": const("kForcedThreads"), "positions_per_thread": 1, "ahead": const("kForcedAhead"),
           "cases": {}}
    for name, fn in list(cases.items()) + list(loops.items()):
        runs, warm = (a.loop_runs, 1) if name in loops else (a.runs, a.warmup)
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(runs)]
        out["cases"][name] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                              "ms_max": round(max(ms), 4)}
    # the same value from the kernel and the loop
    ref = torch_loop(lp.double(), ids, ild, sld, ws.double(), wn.double(), wk.double())
    out["loglik_of_sequence_0"] = {"hmm355": float(loglik[0]), "torch_loop_fp64": float(ref[0])}
    out["max_abs_loglik_difference_from_torch_loop_fp64"] = float((ref - loglik.double()).abs().max())
    c = {k: v["ms_per_call"] for k, v in out["cases"].items()}
    out["ratio_to_ctc_at_equal_width"] = {k: round(c["forced_" + k] / c["ctc_" + k], 3)
                                          for k in ("value_only", "alpha_beta", "viterbi")}
    out["ratio_mas_to_forced"] = {k: round(c["mas_" + k] / c["forced_" + k], 3)
                                  for k in ("value_only", "alpha_beta", "viterbi")}
    out["ratio_torch_loop_to_forced"] = {
        "forward": round(c["torch_loop_forward"] / c["forced_value_only"], 1),
        "forward_backward": round(c["torch_loop_forward_backward"] / c["forced_loglik_forward_backward"], 1)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
