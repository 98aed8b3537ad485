"""Time the dynamic-time-warping ops (csrc/dtw.hip) on an MI355X.

    python tools/time_dtw.py [--runs 20] [--warmup 3] [--out profiles/dtw_timing.json]

Cases: ops.dtw (symmetric) with cost matrix and path, and value-only, at B in {1, 32}, N = M = 2000;
one ragged phoneme-like batch (N = 200, M = 2000, per-pair lengths); ops.soft_dtw and
ops.soft_dtw_grad at B = 32, N = M = 1000.  The yardstick is a batched torch-op wavefront written
here, independent of the kernel: the distance matrices are skewed once so that an anti-diagonal
is a contiguous row, then one group of torch ops per anti-diagonal advances all B pairs (the obvious
way to run this recursion without hand-written HIP); it returns the skewed cost table and the totals
(no backtrace).  HIP events around each call, warm-up first, the median of the timed runs.  Prints
one JSON object and writes it to --out.  Needs a GPU: there is no fall-back.
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

_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "dtw.hip")).read()
ROWS = int(re.search(r"constexpr int kDtwRows = (\d+);", _SRC).group(1))
THREADS = int(re.search(r"constexpr int kDtwThreads = (\d+);", _SRC).group(1))
STEP_US = 4.71   # profiles/wide_timing.json, fb_wide_N256: one launched step on this hardware


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_wavefront(dist):
    """Symmetric hard DTW of (B,N,M) by anti-diagonals, torch ops only: (skewed costs (B,N+M-1,N),
    totals (B)).  Row s of the skewed table holds C[i, s-i] at index i, +inf where s-i is outside
    [0, M)."""
    B, N, M = dist.shape
    S = N + M - 1
    dev = dist.device
    j = torch.arange(S, device=dev)[None, :] - torch.arange(N, device=dev)[:, None]   # (N,S)
    bad = (j < 0) | (j >= M)
    sk = dist.gather(2, j.clamp(0, M - 1)[None].expand(B, N, S)).masked_fill(bad[None], float("inf"))
    sk = sk.transpose(1, 2).contiguous()                                                 # (B,S,N)
    C = torch.empty_like(sk)
    C[:, 0] = sk[:, 0]
    for s in range(1, S):
        p1 = C[:, s - 1]
        best = p1[:, :-1]                                   # up: C[i-1, j]
        if s > 1:
            best = torch.minimum(best, C[:, s - 2, :-1])    # diagonal: C[i-1, j-1]
        best = torch.minimum(best, p1[:, 1:])               # left: C[i, j-1]
        torch.add(sk[:, s, 1:], best, out=C[:, s, 1:])
        torch.add(sk[:, s, 0], p1[:, 0], out=C[:, s, 0])
    return C, C[:, S - 1, N - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yardstick-runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dtw.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.from_numpy(rng.random(shape, dtype=np.float32)).to(dev)

    cases, yard = {}, {}
    for B in (1, 32):
        d = rand(B, 2000, 2000)
        cases[f"dtw_cost_path_B{B}_2000x2000"] = (
            lambda d=d: ops.dtw(d, ops.DTW_SYMMETRIC), {"op": "dtw", "B": B, "N": 2000, "M": 2000, "outputs": "cost, path"})
        cases[f"dtw_value_only_B{B}_2000x2000"] = (
            lambda d=d: ops.dtw(d, ops.DTW_SYMMETRIC, None, None, False, False),
            {"op": "dtw", "B": B, "N": 2000, "M": 2000, "outputs": "total"})
        # the two outputs apart: which of them the difference to the value-only call belongs to
        cases[f"dtw_cost_only_B{B}_2000x2000"] = (
            lambda d=d: ops.dtw(d, ops.DTW_SYMMETRIC, None, None, True, False),
            {"op": "dtw", "B": B, "N": 2000, "M": 2000, "outputs": "cost"})
        cases[f"dtw_path_only_B{B}_2000x2000"] = (
            lambda d=d: ops.dtw(d, ops.DTW_SYMMETRIC, None, None, False, True),
            {"op": "dtw", "B": B, "N": 2000, "M": 2000, "outputs": "path"})
        yard[f"torch_wavefront_B{B}_2000x2000"] = (
            lambda d=d: torch_wavefront(d), {"op": "torch anti-diagonal wavefront", "B": B, "N": 2000, "M": 2000,
                                             "outputs": "skewed cost, total", "launch_groups": 3998})
        # the yardstick computes what the kernel computes
        assert torch.equal(torch_wavefront(d)[1], ops.dtw(d, ops.DTW_SYMMETRIC)[1])
    d = rand(32, 200, 2000)
    n_len = torch.from_numpy(rng.integers(100, 201, 32).astype(np.int32)).to(dev)
    m_len = torch.from_numpy(rng.integers(1000, 2001, 32).astype(np.int32)).to(dev)
    cases["dtw_cost_path_ragged_B32_200x2000"] = (
        lambda d=d: ops.dtw(d, ops.DTW_ASYMMETRIC, n_len, m_len),
        {"op": "dtw", "B": 32, "N": 200, "M": 2000, "outputs": "cost, path", "lengths": "n 100..200, m 1000..2000"})
    d = rand(32, 1000, 1000)
    R, _ = ops.soft_dtw(d, 0.1)
    cases["soft_dtw_forward_B32_1000x1000"] = (
        lambda d=d: ops.soft_dtw(d, 0.1), {"op": "soft_dtw", "B": 32, "N": 1000, "M": 1000, "gamma": 0.1})
    cases["soft_dtw_grad_B32_1000x1000"] = (
        lambda d=d, R=R: ops.soft_dtw_grad(d, R, 0.1), {"op": "soft_dtw_grad", "B": 32, "N": 1000, "M": 1000, "gamma": 0.1})

    for _ in range(args.warmup):
        for fn, _d in cases.values():
            fn()
    for fn, _d in yard.values():
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in list(cases) + list(yard)}
    for _ in range(args.runs):
        for k, (fn, _d) in cases.items():
            samples[k].append(timed(fn))
    for _ in range(args.yardstick_runs):
        for k, (fn, _d) in yard.items():
            samples[k].append(timed(fn))

    result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "yardstick_runs": args.yardstick_runs,
              "warmup": args.warmup,
              "timer": "HIP events around one op call (allocation of outputs and workspace included)",
              "rows_per_thread": ROWS, "threads": THREADS, "rows_per_pass": ROWS * THREADS, "cases": {}}
    for k, (fn, desc) in list(cases.items()) + list(yard.items()):
        ms = statistics.median(samples[k])
        cells = desc["B"] * desc["N"] * desc["M"]
        result["cases"][k] = dict(desc, ms_per_call=round(ms, 4), ms_min=round(min(samples[k]), 4),
                                  ms_max=round(max(samples[k]), 4), gcells_per_s=round(cells / ms / 1e6, 3),
                                  us_per_antidiagonal=round(1e3 * ms / (desc["N"] + desc["M"] - 1), 4))
    flag = result["cases"]["dtw_cost_path_B32_2000x2000"]["ms_per_call"]
    floor = 3999 * STEP_US / 1e3
    result["bar"] = {"case": "dtw_cost_path_B32_2000x2000", "ms_per_call": flag,
                     "one_launch_per_antidiagonal_floor_ms": round(floor, 2), "below_floor": flag < floor,
                     "yardstick_ms": result["cases"]["torch_wavefront_B32_2000x2000"]["ms_per_call"],
                     "below_yardstick": flag < result["cases"]["torch_wavefront_B32_2000x2000"]["ms_per_call"]}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
