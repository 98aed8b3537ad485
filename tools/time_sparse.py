"""Time the sparse-transition Viterbi and forward-backward (csrc/sparse.hip) on an MI355X against
the dense ops on the same model.

    python tools/time_sparse.py [--B 32] [--T 2000] [--runs 20] [--warmup 3] [--out profiles/sparse_timing.json]

The model is left-to-right with a skip (i -> i, i + 1, i + 2: 3 N - 3 arcs) at N in {256, 1024,
4096, 8192}.  Per size:
  sparse_viterbi_*        ops.sparse_viterbi, the arcs in registers (at most 3 per state)
  sparse_fb_counts_*      ops.sparse_forward_backward with the posterior, then ops.sparse_arc_counts
  *_streamed_*            the same model plus the arcs 0..4 -> 5 and 5 -> 6..9: one state with more
                          in-arcs and one with more out-arcs than the register budget, so the same
                          kernels read every arc through L2 each step (the register-versus-streamed
                          comparison: 10 arcs more work)
  dense_viterbi_*, dense_fb_*   ops.viterbi / ops.forward_backward (OBS_LOG) on the densified matrix,
                          N <= 4096: the narrow chain at 256, the batch-tiled form above
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

from pytorch_hmm_amd import ops, sparse  # noqa: E402


def lr_skip(N, extra):
    i = np.arange(N)
    src = np.concatenate([i, i[:-1], i[:-2]])
    dst = np.concatenate([i, i[1:], i[2:]])
    if extra:   # a state with 5 + in-arcs and one with 5 + out-arcs: beyond the register budget
        have = set(zip(src.tolist(), dst.tolist()))
        more = [(s, 5) for s in range(5)] + [(5, d) for d in range(6, 10)]
        more = [a for a in more if a not in have]
        src = np.concatenate([src, [a[0] for a in more]])
        dst = np.concatenate([dst, [a[1] for a in more]])
    rng = np.random.default_rng(N)
    w = rng.uniform(0.1, 1.0, src.size)
    w = np.log(w / np.bincount(src, weights=w, minlength=N)[src]).astype(np.float32)
    return src, dst, w


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(cases, warmup, runs):
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(runs):          # the forms alternate run by run
        for k, fn in cases.items():
            samples[k].append(timed(fn))
    return samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 4096, 8192])
    ap.add_argument("--dense-max", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sparse.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    B, T = args.B, args.T
    result = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "runs": args.runs, "warmup": args.warmup,
              "timer": "HIP events around one op call (allocation of outputs and workspace included)",
              "model": "left-to-right with a skip, 3 N - 3 arcs", "cases": {}}
    for N in args.sizes:
        g = torch.Generator(device=dev).manual_seed(N)
        obs = torch.randn(B, T, N, device=dev, generator=g) * 1.5 - 1.0
        p0 = torch.full((N,), -float(np.log(N)), device=dev)
        cases, desc = {}, {}
        for extra in (False, True):
            src, dst, w = lr_skip(N, extra)
            tr = sparse.SparseTransitions(src, dst, torch.from_numpy(w).to(dev), N)
            tag = "_streamed" if extra else ""
            form = "arcs streamed through L2" if extra else "arcs in registers"
            w_in, w_out = tr.log_w[tr.perm_in].contiguous(), tr.log_w[tr.perm_out].contiguous()

            def vit(tr=tr, w_in=w_in):
                return ops.sparse_viterbi(obs, tr.in_ptr_host, tr.in_ptr, tr.in_src, w_in, p0)

            def fbc(tr=tr, w_in=w_in, w_out=w_out):
                _, _, ws = ops.sparse_forward_backward(obs, tr.in_ptr_host, tr.in_ptr, tr.in_src, w_in, tr.out_ptr_host,
                                                       tr.out_ptr, tr.out_dst, w_out, p0, True)
                return ops.sparse_arc_counts(obs, tr.in_src, tr.in_dst, w_in, ws)
            cases[f"sparse_viterbi{tag}_N{N}"] = vit
            cases[f"sparse_fb_counts{tag}_N{N}"] = fbc
            desc[f"sparse_viterbi{tag}_N{N}"] = {"N": N, "arcs": tr.num_arcs, "op": "viterbi", "form": form}
            desc[f"sparse_fb_counts{tag}_N{N}"] = {"N": N, "arcs": tr.num_arcs, "op": "forward_backward + arc counts",
                                                   "form": form}
            if not extra and N <= args.dense_max:
                P = tr.to_dense()
                cases[f"dense_viterbi_N{N}"] = lambda P=P: ops.viterbi(obs, P, p0, ops.OBS_LOG)
                cases[f"dense_fb_N{N}"] = lambda P=P: ops.forward_backward(obs, P, p0, ops.OBS_LOG, ops.FB_POSTERIOR)
                dform = "narrow chain" if N <= ops.NARROW_MAX_STATES else "batch-tiled (wide)"
                desc[f"dense_viterbi_N{N}"] = {"N": N, "op": "viterbi", "form": "dense, " + dform}
                desc[f"dense_fb_N{N}"] = {"N": N, "op": "forward_backward (posterior, no counts)",
                                          "form": "dense, " + dform}
        samples = measure(cases, args.warmup, args.runs)
        for k in cases:
            ms = statistics.median(samples[k])
            result["cases"][k] = dict(desc[k], ms_per_call=round(ms, 4), us_per_step=round(1e3 * ms / T, 4),
                                      ms_min=round(min(samples[k]), 4), ms_max=round(max(samples[k]), 4))
            print(k, result["cases"][k]["ms_per_call"], "ms", flush=True)
        del obs, cases
        torch.cuda.empty_cache()
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
