"""Time posterior path sampling (csrc/ffbs.hip) on an MI355X.

    python tools/time_ffbs.py [--B 32] [--T 2000] [--runs 20] [--warmup 3] [--out profiles/ffbs_timing.json]

For N in {64, 128, 256} and K in {1, 16} samples per sequence, three things:
  ffbs            hmm355_ffbs_f32 alone (the A^T kernel and the sampling kernel) on rows, uniforms,
                  states and workspace allocated beforehand; once with the product library (A^T
                  staged in LDS up to HMM355_FFBS_LDS_MAX_NP) and once with a diagnostic build that
                  reads the A^T row from global memory at every N (-DHMM355_FFBS_LDS_MAX_NP=0, built
                  into tools/ablate_libs/ when it is missing)
  posterior_sample  the whole ops.posterior_sample call: forward-backward that keeps U, then ffbs
  torch_loop      the same backward sampling written with torch ops on the GPU, one step at a
                  time from the same U rows and uniforms (the yardstick: several launches per step)
HIP events around each call, warm-up first, the median of the timed runs; the forms alternate run
by run.  Prints one JSON object and the DESIGN.md table, writes the JSON to --out.  Needs a GPU:
there is no fall-back.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import _native as nat  # noqa: E402
from pytorch_hmm_amd import autograd, build_native, ops  # noqa: E402

GLOBAL_LIB = os.path.join(ROOT, "tools", "ablate_libs", "libhmm355_ffbs_global.so")


def global_lib():
    """The diagnostic build whose sampling kernel reads A^T from global memory at every N."""
    if not os.path.exists(GLOBAL_LIB):
        build_native.build(force=True, defines=["HMM355_FFBS_LDS_MAX_NP=0"], out=GLOBAL_LIB, sources=["ffbs.hip"])
    L = ctypes.CDLL(GLOBAL_LIB)
    L.hmm355_ffbs_f32.argtypes = nat.lib().hmm355_ffbs_f32.argtypes
    L.hmm355_ffbs_f32.restype = ctypes.c_int
    return L


def inputs(B, T, N, dev):
    rng = np.random.default_rng(N)
    obs = torch.from_numpy(rng.random((B, T, N), dtype=np.float32)).to(dev)
    P = torch.from_numpy(rng.random((N, N), dtype=np.float32))
    P = P / P.sum(1, keepdim=True)
    log_P = torch.log(P + 1e-8).to(dev)
    log_p0 = torch.log(torch.full((N,), 1.0 / N) + 1e-8).to(dev)
    return obs, log_P, log_p0


def torch_loop(U, log_P, u):
    """Backward sampling with torch ops: per step a gather of A^T rows, a product, a cumsum, a
    compare-and-count.  U (B,T,N), u (B,K,T) -> states (B,K,T)."""
    B, T, N = U.shape
    K = u.shape[1]
    AT = torch.exp(log_P).t().contiguous()
    states = torch.empty((B, K, T), dtype=torch.int64, device=U.device)
    z = None
    for t in range(T - 1, -1, -1):
        w = U[:, None, t, :].expand(B, K, N)
        if z is not None:
            w = w * AT[z]
        c = torch.cumsum(w, -1)
        r = u[:, :, t, None] * c[..., -1:]
        z = (c <= r).sum(-1).clamp_(max=N - 1)
        states[:, :, t] = z
    return states


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
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ffbs_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ffbs.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    B, T = args.B, args.T
    libs = {"lds": nat.lib(), "global": global_lib()}
    lds_max = 128   # HMM355_FFBS_LDS_MAX_NP of the product build (csrc/ffbs.hip)

    cases = {}
    keep = []   # buffers the raw calls point into
    for N in args.sizes:
        obs, log_P, log_p0 = inputs(B, T, N, dev)
        plan = ops.make_plan(log_P)
        _, _, _, U, *_ = autograd._run_fb(obs, log_P, log_p0, ops.OBS_PROB, plan=plan)
        U = U.clone()   # (B,T,N) contiguous: ld = N
        NP = 64 if N <= 64 else (128 if N <= 128 else 256)
        for K in args.samples:
            u = torch.rand((B, K, T), device=dev, generator=torch.Generator(device=dev).manual_seed(N + K))
            states = torch.empty((B, K, T), dtype=torch.int64, device=dev)
            ws = torch.empty(nat.lib().hmm355_ffbs_workspace_bytes(N), dtype=torch.uint8, device=dev)
            keep += [U, u, states, ws, log_P]
            for form, L in libs.items():
                if form == "lds" and NP > lds_max:
                    continue   # the product build reads from global there: the "global" row is it

                def raw(L=L, U=U, p=log_P, u=u, s=states, w=ws, N=N, K=K):
                    nat.check(L.hmm355_ffbs_f32(nat.ptr(U), N, nat.ptr(p), None, nat.ptr(u), B, T, N, K, nat.ptr(s),
                                                nat.ptr(w), w.numel(), nat.stream_of(dev)))
                cases[f"ffbs_{form}_N{N}_K{K}"] = (raw, {"N": N, "K": K, "what": "ffbs", "A^T": form})
            cases[f"posterior_sample_N{N}_K{K}"] = (
                lambda o=obs, p=log_P, i=log_p0, u=u, K=K, pl=plan: ops.posterior_sample(o, p, i, ops.OBS_PROB, K,
                                                                                         uniforms=u, plan=pl),
                {"N": N, "K": K, "what": "posterior_sample", "A^T": "lds" if NP <= lds_max else "global"})
            cases[f"torch_loop_N{N}_K{K}"] = (lambda U=U, p=log_P, u=u: torch_loop(U, p, u),
                                              {"N": N, "K": K, "what": "torch_loop", "A^T": None})

    for _ in range(args.warmup):
        for fn, _d in cases.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.runs):          # the forms alternate run by run
        for k, (fn, _d) in cases.items():
            samples[k].append(timed(fn))
    result = {"device": torch.cuda.get_device_name(0), "B": B, "T": T, "runs": args.runs, "warmup": args.warmup,
              "timer": "HIP events around one call; ffbs_*: the C entry point on preallocated buffers, the others "
                       "include their allocations", "lds_max_np": lds_max, "cases": {}}
    for k, (fn, desc) in cases.items():
        ms = statistics.median(samples[k])
        result["cases"][k] = dict(desc, ms_per_call=round(ms, 4), us_per_step=round(1e3 * ms / T, 4),
                                  ms_min=round(min(samples[k]), 4), ms_max=round(max(samples[k]), 4))
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")

    # the DESIGN.md table (section 13H)
    c = result["cases"]
    ms = lambda key: f"{c[key]['ms_per_call']:.3f}" if key in c else "-"
    print("\n| N | K | ffbs, A^T in LDS (ms) | ffbs, A^T from global (ms) | posterior_sample (ms) | torch-op loop (ms) |")
    print("|---|---|---|---|---|---|")
    for N in args.sizes:
        for K in args.samples:
            print(f"| {N} | {K} | {ms(f'ffbs_lds_N{N}_K{K}')} | {ms(f'ffbs_global_N{N}_K{K}')} | "
                  f"{ms(f'posterior_sample_N{N}_K{K}')} | {ms(f'torch_loop_N{N}_K{K}')} |")


if __name__ == "__main__":
    main()
