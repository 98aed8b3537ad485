"""Time the Baum-Welch emission statistics (csrc/emstats.hip) and one EM iteration on an MI355X.

    python tools/time_emstats.py [--runs 20] [--warmup 3] [--out profiles/emstats_timing.json]

Shapes: BASELINE config 3 (B=32, T=2000, S=128, C=4, D=80), the single-Gaussian S=128, C=1, D=80 at
the same frames, and a small one.  Per shape:
  kernel      hmm355_gmm_stats_f32 alone (its three launches) on inputs, outputs and workspace
              allocated beforehand
  op          ops.gmm_stats: the same call with its allocations
  torch       the torch restatement: the T-chunked GEMM expressions of autograd.GmmLogProb.backward
              with g = gamma (component scores through two GEMMs, a (frames, S*C) softmax, the sums
              through two more GEMMs), centred at the end to the same three outputs
  em_step     one full em_step of the layer the shape belongs to (MixtureGaussianHMMLayer for C > 1,
              GaussianHMMLayer for C == 1): scorer, forward-backward, xi, statistics, M-step
HIP events around each call, warm-up first, the median of the timed runs; the forms alternate run
by run.  Prints one JSON object and the DESIGN.md table, writes the JSON to --out.  Needs a GPU:
there is no fall-back.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pytorch_hmm_amd import GaussianHMMLayer, MixtureGaussianHMMLayer  # noqa: E402
from pytorch_hmm_amd import _native as nat  # noqa: E402
from pytorch_hmm_amd import ops  # noqa: E402

SHAPES = {"config3": (32, 2000, 128, 4, 80), "gaussian": (32, 2000, 128, 1, 80), "small": (4, 200, 16, 4, 24)}


def inputs(B, T, S, C, D, dev):
    rng = np.random.default_rng(S * C + D)
    means = rng.normal(size=(S, C, D)).astype(np.float32) * 2.0 / math.sqrt(D)
    log_vars = (rng.normal(size=(S, C, D)) * 0.3).astype(np.float32)
    log_w = np.log(rng.dirichlet(np.ones(C) * 2, S)).astype(np.float32)
    pick = rng.integers(0, S * C, size=(B, T))
    x = (means.reshape(-1, D)[pick] + rng.normal(size=(B, T, D))).astype(np.float32)
    gamma = rng.dirichlet(np.ones(S) * 0.1, (B, T)).astype(np.float32)
    return [torch.from_numpy(a).to(dev) for a in (x, gamma, means, log_vars, log_w)]


def torch_stats(x, g, means, log_vars, log_w, mix_lse):
    """GmmLogProb.backward's chunked expressions with g = gamma, to (occ, sx, sxx)."""
    B, T, D = x.shape
    S, C, _ = means.shape
    mu = means.reshape(S * C, D)
    lv = log_vars.reshape(S * C, D)
    iv = torch.exp(-lv)
    cst = lv.sum(-1) + D * math.log(2 * math.pi)
    lw = log_w.reshape(S * C)
    q2 = (mu * mu * iv).sum(-1)
    gx2 = torch.zeros_like(mu)
    gx1 = torch.zeros_like(mu)
    gsum = torch.zeros(S * C, device=x.device)
    step = max(1, (1 << 22) // max(1, B * S * C))
    for t0 in range(0, T, step):
        xc = x[:, t0:t0 + step].reshape(-1, D)
        gl = g[:, t0:t0 + step].reshape(-1, S)
        if mix_lse:
            maha = (xc * xc) @ iv.t() - 2.0 * (xc @ (mu * iv).t()) + q2
            comp3 = (-0.5 * (maha + cst) + lw).view(-1, S, C)
            m = comp3.max(-1, keepdim=True)[0]
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            ex = torch.exp(comp3 - m)
            se = ex.sum(-1, keepdim=True)
            r = torch.where(se > 1e-8, ex / se, torch.zeros_like(ex))
            gc = (r * gl.unsqueeze(-1)).reshape(-1, S * C)
        else:
            gc = gl.reshape(-1, S * C)
        gsum += gc.sum(0)
        gx1 += gc.t() @ xc
        gx2 += gc.t() @ (xc * xc)
    sx = gx1 - mu * gsum[:, None]
    sxx = gx2 - 2 * mu * gx1 + mu * mu * gsum[:, None]
    return gsum.view(S, C), sx.view(S, C, D), sxx.view(S, C, D)


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
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emstats_timing.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_emstats.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    L = nat.lib()
    cases, keep, agree = {}, [], {}
    for name in args.shapes:
        B, T, S, C, D = SHAPES[name]
        x, gamma, means, log_vars, log_w = t = inputs(B, T, S, C, D, dev)
        mix = int(C > 1)
        outs = [torch.empty(S, C, device=dev), torch.empty(S, C, D, device=dev), torch.empty(S, C, D, device=dev)]
        need = L.hmm355_gmm_stats_workspace_bytes(B, T, D, S, C)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        keep += t + outs + [ws]
        desc = {"shape": name, "B": B, "T": T, "S": S, "C": C, "D": D}

        def raw(t=t, outs=outs, ws=ws, B=B, T=T, S=S, C=C, D=D, mix=mix):
            nat.check(L.hmm355_gmm_stats_f32(*[nat.ptr(a) for a in t], None, B, T, D, S, C, mix,
                                             *[nat.ptr(o) for o in outs], nat.ptr(ws), ws.numel(), nat.stream_of(dev)))
        cases[f"kernel_{name}"] = (raw, dict(desc, what="kernel", workspace_bytes=int(need)))
        cases[f"op_{name}"] = (lambda t=t, mix=mix: ops.gmm_stats(*t, mix), dict(desc, what="op"))
        cases[f"torch_{name}"] = (lambda t=t, mix=mix: torch_stats(*t, mix), dict(desc, what="torch"))
        if C > 1:
            layer = MixtureGaussianHMMLayer(S, D, C).to(dev)
        else:
            layer = GaussianHMMLayer(S, D, transition_type="ergodic").to(dev)
        with torch.no_grad():
            layer.means.copy_(means if C > 1 else means[:, 0])
        keep.append(layer)
        cases[f"em_step_{name}"] = (lambda layer=layer, x=x: layer.em_step(x), dict(desc, what="em_step"))
        # the two forms compute the same sums: the largest difference relative to the largest entry
        raw()
        ref = torch_stats(*t, mix)
        agree[name] = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(outs, ref)]

    for _ in range(args.warmup):
        for fn, _d in cases.values():
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.runs):          # the forms alternate run by run
        for k, (fn, _d) in cases.items():
            samples[k].append(timed(fn))
    result = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
              "timer": "HIP events around one call; kernel_*: the C entry point on preallocated buffers, the others "
                       "include their allocations; em_step_* changes the layer's parameters from run to run",
              "kernel_vs_torch_max_rel_diff": agree, "cases": {}}
    for k, (fn, desc) in cases.items():
        ms = statistics.median(samples[k])
        result["cases"][k] = dict(desc, ms_per_call=round(ms, 4), ms_min=round(min(samples[k]), 4),
                                  ms_max=round(max(samples[k]), 4))
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")

    # the DESIGN.md table (section 13I)
    c = result["cases"]
    print("\n| shape | B x T | S | C | D | kernel (ms) | ops.gmm_stats (ms) | torch restatement (ms) | em_step (ms) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for name in args.shapes:
        B, T, S, C, D = SHAPES[name]
        ms = lambda what: f"{c[f'{what}_{name}']['ms_per_call']:.3f}"
        print(f"| {name} | {B} x {T} | {S} | {C} | {D} | {ms('kernel')} | {ms('op')} | {ms('torch')} | {ms('em_step')} |")


if __name__ == "__main__":
    main()
