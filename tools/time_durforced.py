"""Time explicit-duration forced alignment (csrc/durforced.hip) on an MI355X.

    python tools/time_durforced.py [--runs 20] [--warmup 3] [--out profiles/durforced_timing.json]

B = 32, T = 800, L = 128 positions, Dmax = 64 (input lengths 600..800, chain lengths 96..128, 60
classes with repeats): duration_forced_loglik forward + backward (log_probs and dur_lp both
require grad), duration_forced_align, and the pieces (value-only call, tables, gradient call).
Beside them two comparators:
  - the same recursion as a plain per-frame torch loop on the GPU, forward + backward through
    autograd (in this tool only; the product has no such path);
  - autograd.HsmmLogLik forward + backward (ops.hsmm_forward_backward) with S = 128 states and the
    same Dmax on emissions of the same size.  It is the closest existing kernel and NOT the same
    model: its states are ergodic (an S x S predecessor reduction per step, one dur_lp for the
    batch, no order and no end constraint), so the ratio says what the chain structure saves, not
    that the two compute the same thing.
HIP events around each call, warm-up first, the median of the timed runs.  Prints one JSON object
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

from pytorch_hmm_amd import ops  # noqa: E402
from pytorch_hmm_amd.alignment import duration_forced_align, duration_forced_loglik  # noqa: E402
from pytorch_hmm_amd.autograd import HsmmLogLik  # noqa: E402

BIGNEG = -1e30  # -inf of the torch loop: exp(BIGNEG - m) is exactly 0 and autograd sees no NaN


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_loop(lp, ids, il, sl, du):
    """loglik (B) by one torch step per frame on lp's device (il, sl on that device too): the open
    segments of every position as a (B,L,Dmax) tensor, shifted by one duration per frame."""
    B, T, C = lp.shape
    L, D = du.shape[1], du.shape[2]
    live = torch.arange(L, device=lp.device)[None, :] < sl[:, None]
    E = torch.where(live[:, None, :], lp.gather(2, ids.long()[:, None, :].expand(B, T, L)), lp.new_tensor(BIGNEG))
    du = du.clamp(min=BIGNEG)
    seg = lp.new_full((B, L, D), BIGNEG)
    beg = torch.cat([lp.new_zeros(B, 1), lp.new_full((B, L - 1), BIGNEG)], 1)
    pad = lp.new_full((B, 1), BIGNEG)
    out = lp.new_full((B,), BIGNEG)
    last = (sl.long() - 1)[:, None]
    for t in range(T):
        seg = (torch.cat([beg[:, :, None], seg[:, :, :-1]], 2) + E[:, t, :, None]).clamp(min=BIGNEG)
        F = torch.logsumexp((seg + du).clamp(min=BIGNEG), 2)
        beg = torch.cat([pad, F[:, :-1]], 1)
        out = torch.where(il == t + 1, F.gather(1, last)[:, 0], out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-runs", type=int, default=3, help="timed runs of the per-frame torch loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "durforced_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, L, D, C = 32, 800, 128, 64, 60
    rng = np.random.default_rng(0)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)), 2).to(dev)
    ids = torch.from_numpy(rng.integers(0, C, (B, L))).to(dev, torch.int32)
    il = torch.from_numpy(rng.integers(600, T + 1, B))
    sl = torch.from_numpy(rng.integers(96, L + 1, B))
    il[0], sl[0] = T, L
    du = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, L, D)).astype(np.float32)), 2).to(dev)
    # the HSMM comparator: S = L ergodic states, one duration table, emissions of the same size
    lp_s = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, L)).astype(np.float32)), 2).to(dev)
    du_s = du[0].contiguous()
    log_T = torch.log_softmax(torch.from_numpy(rng.standard_normal((L, L)).astype(np.float32)), 1).to(dev)

    args = (lp, ids, il, sl, du)
    tabs = ops.durforced(*args, tables=True)
    leaves = [lp.clone().requires_grad_(), du.clone().requires_grad_()]
    hleaves = [lp_s.clone().requires_grad_(), du_s.clone().requires_grad_()]
    ild, sld = il.to(dev), sl.to(dev)

    def ours_fwd_bwd():
        for t in leaves:
            t.grad = None
        (-duration_forced_loglik(leaves[0], ids, il, sl, leaves[1]).sum()).backward()

    def loop_fwd_bwd():
        for t in leaves:
            t.grad = None
        (-torch_loop(leaves[0], ids, ild, sld, leaves[1]).sum()).backward()

    def hsmm_fwd_bwd():
        for t in hleaves:
            t.grad = None
        (-HsmmLogLik.apply(hleaves[0], hleaves[1], log_T, None).sum()).backward()

    cases = {
        "durforced_loglik_forward_backward": ours_fwd_bwd,
        "durforced_align": lambda: duration_forced_align(*args),
        "durforced_value_only": lambda: duration_forced_loglik(*args),
        "durforced_tables": lambda: ops.durforced(*args, tables=True),
        "durforced_grad": lambda: ops.durforced_grad(*tabs[1:7], *args, want_grad=True, want_dur=True),
        "hsmm_fb_S128_forward_backward": hsmm_fwd_bwd,
    }
    loops = {"torch_loop_forward_backward": loop_fwd_bwd}
    out = {"device": torch.cuda.get_device_name(dev), "runs": a.runs, "warmup": a.warmup, "loop_runs": a.loop_runs,
           "timer": "HIP events around one call (argument checks, allocation of outputs and workspace included)",
           "shape": {"B": B, "T": T, "Lmax": L, "Dmax": D, "C": C, "input_lengths": "600..800",
                     "state_lengths": "96..128"},
           "note": "hsmm_fb_S128 is an ergodic 128-state HSMM on emissions of the same size: not the same model",
           "cases": {}}
    for name, fn in list(cases.items()) + list(loops.items()):
        runs, warm = (a.loop_runs, 1) if name in loops else (a.runs, a.warmup)
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = [timed(fn) for _ in range(runs)]
        out["cases"][name] = {"ms_per_call": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                              "ms_max": round(max(ms), 4)}
    with torch.no_grad():
        ref = torch_loop(lp.double(), ids, ild, sld, du.double())
    out["max_abs_loglik_difference_from_torch_loop_fp64"] = float((ref - tabs[0].double()).abs().max())
    c = {k: v["ms_per_call"] for k, v in out["cases"].items()}
    out["ratio_torch_loop_to_durforced"] = round(c["torch_loop_forward_backward"] / c["durforced_loglik_forward_backward"], 1)
    out["ratio_hsmm_fb_to_durforced"] = round(c["hsmm_fb_S128_forward_backward"] / c["durforced_loglik_forward_backward"], 2)
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
