"""Time N-best Viterbi (csrc/nbest.hip) on an MI355X.

    python tools/time_nbest.py [--B 32] [--T 2000] [--runs 20] [--warmup 3] [--out profiles/nbest_timing.json]

For N in {64, 128, 256} and K in {1, 4, 16} paths per sequence, in one run:
  nbest        hmm355_viterbi_nbest_f32 (one launch: chain, final selection, K backtraces) on
               inputs, outputs and workspace allocated beforehand
  ragged       hmm355_viterbi_ragged_f32 on the same inputs with every length T: the single-path
               chain of the same one-workgroup-per-sequence form, the yardstick for K = 1
  torch_loop   the same recursion written with torch ops on the GPU, a topk over the (B, N*K, N)
               candidates per step and a gather per step of the backtrace: what a user writes
               without the kernel
HIP events around each call, warm-up first, the median of the timed runs; the forms alternate run
by run.  Prints one JSON object and the DESIGN.md table, writes the JSON to --out.  Needs a GPU:
there is no fall-back.
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

from pytorch_hmm_amd import _native as nat  # noqa: E402
from pytorch_hmm_amd import ops  # noqa: E402


def inputs(B, T, N, dev):
    rng = np.random.default_rng(N)
    lo = torch.log(torch.from_numpy(rng.random((B, T, N), dtype=np.float32)) + 1e-8).to(dev)
    P = torch.from_numpy(rng.random((N, N), dtype=np.float32))
    P = P / P.sum(1, keepdim=True)
    log_P = torch.log(P + 1e-8).to(dev)
    init = torch.log(torch.full((N,), 1.0 / N) + 1e-8).to(dev)
    return lo, log_P, init


def torch_loop(lo, log_P, init, K):
    """List Viterbi with torch ops: lo (B,T,N) -> (paths (B,K,T), scores (B,K))."""
    B, T, N = lo.shape
    d = torch.full((B, N, K), float("-inf"), device=lo.device)
    d[:, :, 0] = init + lo[:, 0]
    ptr = torch.empty((B, T, K, N), dtype=torch.int64, device=lo.device)
    for t in range(1, T):
        cand = (d[:, :, :, None] + log_P[None, :, None, :]).reshape(B, N * K, N)   # row i*K + r
        v, idx = cand.topk(K, dim=1)                                               # (B,K,N)
        d = (v + lo[:, t, None, :]).transpose(1, 2)
        ptr[:, t] = idx
    scores, cur = d.reshape(B, N * K).topk(K, dim=1)                               # j*K + k
    paths = torch.empty((B, K, T), dtype=torch.int64, device=lo.device)
    for t in range(T - 1, 0, -1):
        j, k = cur // K, cur % K
        paths[:, :, t] = j
        cur = ptr[:, t].reshape(B, K * N).gather(1, k * N + j)
    paths[:, :, 0] = cur // K
    return paths, scores


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--paths", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbest_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_nbest.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    B, T = args.B, args.T
    L = nat.lib()

    cases = {}
    keep = []   # buffers the raw calls point into
    for N in args.sizes:
        lo, log_P, init = inputs(B, T, N, dev)
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        states = torch.empty((B, T), dtype=torch.int64, device=dev)
        delta = torch.empty((B, T, N), device=dev)
        final = torch.empty(B, device=dev)
        rws = torch.empty(L.hmm355_viterbi_ragged_workspace_bytes(B, T, N, ops.OBS_LOG), dtype=torch.uint8, device=dev)
        keep += [lo, log_P, init, lens, states, delta, final, rws]

        def ragged(lo=lo, p=log_P, i=init, n=lens, s=states, d=delta, f=final, w=rws, N=N):
            nat.check(L.hmm355_viterbi_ragged_f32(nat.ptr(lo), ops.OBS_LOG, nat.ptr(p), nat.ptr(i), nat.ptr(n), B, T, N,
                                                  nat.ptr(s), nat.ptr(d), nat.ptr(f), nat.ptr(w), w.numel(),
                                                  nat.stream_of(dev)))
        cases[f"ragged_N{N}"] = (ragged, {"N": N, "K": 1, "what": "ragged"})
        for K in args.paths:
            paths = torch.empty((B, K, T), dtype=torch.int64, device=dev)
            scores = torch.empty((B, K), device=dev)
            count = torch.empty(B, dtype=torch.int32, device=dev)
            ws = torch.empty(L.hmm355_viterbi_nbest_workspace_bytes(B, T, N, K, ops.OBS_LOG), dtype=torch.uint8,
                             device=dev)
            keep += [paths, scores, count, ws]

            def raw(lo=lo, p=log_P, i=init, pa=paths, s=scores, c=count, w=ws, N=N, K=K):
                nat.check(L.hmm355_viterbi_nbest_f32(nat.ptr(lo), ops.OBS_LOG, nat.ptr(p), nat.ptr(i), None, B, T, N, K,
                                                     nat.ptr(pa), nat.ptr(s), nat.ptr(c), nat.ptr(w), w.numel(),
                                                     nat.stream_of(dev)))
            cases[f"nbest_N{N}_K{K}"] = (raw, {"N": N, "K": K, "what": "nbest", "workspace_bytes": ws.numel()})
            cases[f"torch_loop_N{N}_K{K}"] = (lambda lo=lo, p=log_P, i=init, K=K: torch_loop(lo, p, i, K),
                                              {"N": N, "K": K, "what": "torch_loop"})

    for _ in range(args.warmup):
        for fn, _d in cases.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.runs):          # the forms alternate run by run
        for k, (fn, _d) in cases.items():
            samples[k].append(timed(fn))
    result = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "runs": args.runs, "warmup": args.warmup,
              "timer": "HIP events around one call; nbest / ragged: the C entry point on preallocated buffers, "
                       "torch_loop includes its allocations", "cases": {}}
    for k, (fn, desc) in cases.items():
        ms = statistics.median(samples[k])
        result["cases"][k] = dict(desc, ms_per_call=round(ms, 4), us_per_step=round(1e3 * ms / T, 4),
                                  ms_min=round(min(samples[k]), 4), ms_max=round(max(samples[k]), 4))
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")

    # the DESIGN.md table (section 13J)
    c = result["cases"]
    print("\n| N | K | nbest (ms) | us / step | single-path ragged chain (ms) | torch-op loop (ms) | loop / nbest |")
    print("|---|---|---|---|---|---|---|")
    for N in args.sizes:
        for K in args.paths:
            nb, tl = c[f"nbest_N{N}_K{K}"], c[f"torch_loop_N{N}_K{K}"]
            rg = f"{c[f'ragged_N{N}']['ms_per_call']:.3f}" if K == 1 else "-"
            print(f"| {N} | {K} | {nb['ms_per_call']:.3f} | {nb['us_per_step']:.2f} | {rg} | "
                  f"{tl['ms_per_call']:.1f} | {tl['ms_per_call'] / nb['ms_per_call']:.0f}x |")


if __name__ == "__main__":
    main()
