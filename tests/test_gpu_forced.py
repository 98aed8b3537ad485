"""GPU parity of transcript forced alignment (csrc/forced.hip; ops.forced / ops.forced_grad /
autograd.ForcedLogLik; pytorch_hmm_amd.alignment.forced).

Contracts:
  * Viterbi path, score and durations: bit-identical to the fp32 restatement (tests/forced_numpy.py:
    one add per candidate, an exact max in the order stay, s-1, s-2 with strict >, one add of the
    emission), planted exact ties included (integer-valued and all-zero inputs).
  * alpha, beta, loglik: the -inf pattern equals the restatement's; finite entries obey
        |x_gpu - x_fp64| <= 5 n 2^-24 max(1, |x_fp64|),
    n the recursion steps behind the entry: t + 1 for alpha[t], T_b - t for beta[t], T_b for
    loglik.  This is the CTC tables' 4 n bound plus one rounding per step for the added weight.
    Measured on MI355X over every case here: the largest error is 0.14 of the bound for alpha,
    0.15 for beta and 0.12 for loglik (STEP_BOUND_USE below); none exceeds 0.5.
  * gamma: |gamma_gpu - gamma_64| <= gamma_64 (exp(b_alpha + b_beta + b_loglik) - 1) + 2^-23 with
    the three bounds above at the entry.
  * Gradients through ForcedLogLik (log_probs and every weight tensor given, each on its own):
    with g_64 / g_cpu32 the fp64 / fp32 torch-CPU autograd gradients of a plain torch loop of the
    recursion (reference_loglik below),
        max |g_gpu - g_64| <= 8 x max |g_cpu32 - g_64|
    (the margin test_gpu_ctc.py and test_gpu_dtw.py grant).  Measured ratios on MI355X: see
    GRADIENT_RATIOS below.  Padding and pairs with no path get exact zeros; two calls are
    torch.equal.

The shapes sit on the kernel's own boundaries, read from forced.hip: Smax around the single-wave
limit and around threads x positions-per-thread of every tier up to the ABI maximum, T around the
prefetch ring's depth and one long run, ragged batches of 5 (a full-size pair, S_b = T_b + 1 --
no path without skips, one with --, S_b = 1, T_b = 1, S_b = T_b), repeated ids, an id outside
[0, C), -inf emissions and weights, and the forms without ids and without weights.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forced_numpy as fz  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "forced.hip")).read()


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


THREADS, POS_LOW, POS, POS_MID, POS_WIDE, AHEAD = (_const(n) for n in (
    "kForcedThreads", "kForcedPosLow", "kForcedPos", "kForcedPosMid", "kForcedPosWide", "kForcedAhead"))
MAX_S = 4096
# measured on MI355X: the largest |x_gpu - x_64| / bound over the 73 boundary cases of this file
# (must be <= 1; none exceeds 0.5)
STEP_BOUND_USE = {"alpha": 0.141, "beta": 0.150, "loglik": 0.116}
# measured on MI355X: max |g_gpu - g_64| / max |g_cpu32 - g_64| per gradient case, for log_probs,
# log_stay, log_next, log_skip in that order (bound: 8).  The errors themselves run from 2e-7
# (T = 12) to 2.2e-3 in log_probs and 0.23 in log_stay (T = 600, C = 50, |loglik| ~ 2500, a stay
# count of 596), torch's fp32 alike.
GRADIENT_RATIOS = {
    "(12, 5, 5, 7, 1, 'general')": (0.34, 1.17, 0.33, 0.29),
    "(40, 30, 5, 9, 2, 'general')": (0.25, 0.05, 0.26, 0.29),
    "(600, 40, 5, 50, 3, 'general')": (0.82, 0.49, 1.53, 0.57),
    "(90, 64, 5, 7, 5, 'noskip')": (0.84, 0.40, 0.66, None),
    "(600, 200, 5, 7, 7, 'general')": (0.35, 0.06, 0.22, 0.24),
    "(300, 260, 5, 30, 8, 'general')": (0.60, 0.76, 1.12, 0.99),
    "(60, 20, 5, 7, 9, 'nullw')": (0.30, None, None, None),
    "(80, 30, 5, 7, 10, 'plain')": (0.22, None, None, None),
    "(60, 20, 5, 7, 4, 'neginf')": (0.69, 0.46, 1.18, 0.26),
}


@pytest.fixture(scope="module", autouse=True)
def _native():
    import pytorch_hmm_amd._native as nat
    nat.lib()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()


def ops():
    from pytorch_hmm_amd import ops as o
    return o


def al():
    import pytorch_hmm_amd.alignment as a
    return a


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def gpu_args(case):
    lp, ids, il, sl, ws, wn, wk = case
    return (dev(lp, torch.float32), dev(ids), torch.as_tensor(np.asarray(il)), torch.as_tensor(np.asarray(sl)),
            dev(ws, torch.float32), dev(wn, torch.float32), dev(wk, torch.float32))


MODES = ("general", "noskip", "nullw", "plain", "neginf")


@functools.lru_cache(maxsize=None)
def generated(T, Smax, B, C, seed, mode="general", integer=0):
    """A ragged case and its oracles.
      general  ids with repeats (one outside [0, C) in the full-size chain), all three weights
      noskip   ids, log_stay and log_next only
      nullw    ids, no weights
      plain    no ids (C = Smax), no weights
      neginf   general with -inf sprinkled over the emissions and every weight tensor
    integer=1: small negative integers everywhere (exact ties), integer=2: all zero."""
    assert mode in MODES
    rng = np.random.default_rng(seed)
    if mode == "plain":
        C = Smax
    if integer == 2:
        lp = np.zeros((B, T, C), dtype=np.float32)
    elif integer == 1:
        lp = -rng.integers(0, 3, (B, T, C)).astype(np.float32)
    else:
        x = rng.standard_normal((B, T, C))
        lp = (x - np.log(np.exp(x).sum(2, keepdims=True))).astype(np.float32) if C <= 64 else (x - 3).astype(np.float32)
    ids = None
    if mode != "plain":
        ids = rng.integers(0, C, (B, Smax)).astype(np.int32)
        rep = rng.random((B, Smax)) < 0.2
        for i in range(1, Smax):
            ids[:, i] = np.where(rep[:, i], ids[:, i - 1], ids[:, i])
        if mode in ("general", "neginf") and Smax >= 3:
            ids[0, Smax // 2] = C + 3          # never an index; the chain has to skip it
    w = [None, None, None]
    if mode in ("general", "noskip", "neginf"):
        for i in range(3):
            if integer == 2:
                w[i] = np.zeros((B, Smax), dtype=np.float32)
            elif integer == 1:
                w[i] = -rng.integers(0, 2, (B, Smax)).astype(np.float32)
            else:
                w[i] = (0.5 * rng.standard_normal((B, Smax)) - 0.7).astype(np.float32)
        if mode == "noskip":
            w[2] = None
    if mode == "neginf":
        lp[rng.random(lp.shape) < 0.03] = -np.inf
        for i in range(3):
            w[i][rng.random(w[i].shape) < 0.05] = -np.inf
    # (T_b, S_b): full size; one more position than frames; one position; one frame; S_b = T_b
    t1 = max(1, min(T, Smax - 1))
    t4 = min(T, Smax)
    pairs = [(T, Smax), (t1, min(Smax, t1 + 1)), (max(1, T - 3), 1), (1, 1), (t4, t4)][:B]
    il = np.array([p[0] for p in pairs])
    sl = np.array([p[1] for p in pairs])
    case = (lp, ids, il, sl, w[0], w[1], w[2])
    A64, ll64 = fz.alpha(*case, dtype=np.float64)
    B64 = fz.beta(*case, dtype=np.float64)
    return case, dict(alpha64=A64, beta64=B64, loglik64=ll64, viterbi=fz.viterbi(*case))


def check_tables(case, want):
    lp, ids, il, sl = case[:4]
    B, T, _ = lp.shape
    a = gpu_args(case)
    loglik, A, Bt, path, score, dur = ops().forced(*a, alpha=True, beta=True)
    assert path.numel() == 0 and score.numel() == 0 and dur.numel() == 0
    value_only = ops().forced(*a)
    assert all(t.numel() == 0 for t in value_only[1:])
    assert torch.equal(value_only[0], loglik)            # the value-only call runs the same chain
    A, Bt, loglik = A.cpu().numpy(), Bt.cpu().numpy(), loglik.cpu().numpy()
    assert A.shape == want["alpha64"].shape and A.dtype == np.float32
    ex = (fz.step_bound_excess(A, want["alpha64"], fz.alpha_steps(T, B)),
          fz.step_bound_excess(Bt, want["beta64"], fz.beta_steps(T, il)),
          fz.step_bound_excess(loglik, want["loglik64"], np.asarray(il)))
    print("step-bound use (alpha, beta, loglik): %.3f %.3f %.3f" % ex)
    assert max(ex) <= 1.0, ex
    return A, Bt, loglik


def check_viterbi(case, want):
    _, A, Bt, path, score, dur = ops().forced(*gpu_args(case), viterbi=True)
    wpath, wscore, wdur = want
    assert A.numel() == 0 and Bt.numel() == 0
    assert path.dtype == torch.int32 and dur.dtype == torch.int32
    assert np.array_equal(path.cpu().numpy(), wpath)
    assert np.array_equal(bits(score.cpu().numpy()), bits(wscore))
    assert np.array_equal(dur.cpu().numpy(), wdur)
    il = case[2]
    feasible = np.isfinite(wscore)
    assert np.array_equal(dur.cpu().numpy().sum(1), np.where(feasible, il, 0))


def check_occupancy(case, want, A, Bt, loglik):
    """gamma against the fp64 restatement within the bound the three tables' bounds give; the
    gradients' invariants and exact zeros; run-to-run bits."""
    lp, ids, il, sl, ws, wn, wk = case
    B, T, C = lp.shape
    g64, grad64, gs64, gn64, gk64 = fz.occupancy(*case, tables=(want["alpha64"], want["beta64"], want["loglik64"]))
    a = gpu_args(case)
    call = lambda: ops().forced_grad(dev(A), dev(Bt), dev(loglik), *a, want_gamma=True, want_grad=True,  # noqa: E731
                                     want_stay=True, want_next=True, want_skip=True)
    out, out2 = call(), call()
    assert all(torch.equal(x, y) for x, y in zip(out, out2))
    gamma, grad, gs, gn, gk = (t.cpu().numpy() for t in out)
    b_alpha = fz.step_bound(want["alpha64"], fz.alpha_steps(T, B))
    b_beta = fz.step_bound(want["beta64"], fz.beta_steps(T, il))
    b_ll = fz.step_bound(want["loglik64"], np.asarray(il))[:, None, None]
    tol = g64 * np.expm1(b_alpha + b_beta + b_ll) + 2.0 ** -23
    assert (np.abs(gamma - g64) <= tol).all()
    for b in range(B):
        Tb, Sb = int(il[b]), int(sl[b])
        assert (gamma[b, Tb:] == 0).all() and (gamma[b, :, Sb:] == 0).all() and (grad[b, Tb:] == 0).all()
        for g in (gs, gn, gk):
            assert (g[b, Sb:] == 0).all()
        if not np.isfinite(loglik[b]):
            assert (gamma[b] == 0).all() and (grad[b] == 0).all()
            assert (gs[b] == 0).all() and (gn[b] == 0).all() and (gk[b] == 0).all()
            continue
        # Sums of occupancies.  F bounds the relative error of any exp(alpha + .. + beta - loglik) of
        # the sequence; every term adds its expf / rounding slack of 2^-23, and a sum of n terms in
        # fp32 (the class sums) n roundings of a partial sum that stays below 1 + F.
        F = float(np.expm1(b_alpha[b, :Tb].max() + b_beta[b, :Tb].max() + b_ll[b].max()))
        c = np.arange(Sb) if ids is None else ids[b, :Sb]
        n_c = np.bincount(c[(c >= 0) & (c < C)], minlength=C)
        tol_grad = grad64[b, :Tb] * F + n_c[None, :] * (2.0 ** -23 + 2.0 ** -24 * (1 + F))
        assert (np.abs(grad[b, :Tb] - grad64[b, :Tb]) <= tol_grad).all()
        assert (np.abs(grad[b, :Tb].astype(np.float64).sum(1) - 1) <= tol_grad.sum(1) + 1e-12).all()
        # the transition sums: T_b - 1 terms each, added in fp64 and rounded once
        total, total_tol = 0.0, 0.0
        for g, g_64 in ((gs, gs64), (gn, gn64), (gk, gk64)):
            tol_w = g_64[b] * (F + 2.0 ** -24) + (Tb - 1) * 2.0 ** -23
            assert (np.abs(g[b] - g_64[b]) <= tol_w).all()
            total, total_tol = total + g[b].astype(np.float64).sum(), total_tol + tol_w[:Sb].sum()
        assert abs(total - (Tb - 1)) <= total_tol + 1e-9


# --------------------------------------------------------- the kernel's own boundaries
def _T_for(Smax, mode):
    """Frames that let the full-size chain through: every position without skips, half with."""
    return Smax + 8 if mode in ("noskip", "nullw", "plain") else Smax // 2 + Smax // 8 + 8


BOUNDARY = []
# Smax = 63, 64, 65: the single-wave limit; every form
BOUNDARY += [(_T_for(S, m), S, 5, 7, m) for S in (63, 64, 65) for m in ("general", "noskip", "nullw", "plain")]
# the prefetch ring: T around its depth in the single-wave and in two LDS forms; long runs
BOUNDARY += [(T, S, 5, 7, m) for T in (1, 2, AHEAD - 1, AHEAD, AHEAD + 1) for S in (5, 100, 300)
             for m in ("general", "plain")]
BOUNDARY += [(600, 5, 5, 3, "general"), (600, 40, 5, 7, "general"), (600, 300, 5, 7, "general"),
             (600, 40, 5, 7, "plain"), (600, 300, 5, 7, "noskip")]
# chains of one and two positions
BOUNDARY += [(9, 1, 3, 4, m) for m in ("general", "plain")] + [(9, 2, 5, 4, "general")]
# -inf emissions and weights
BOUNDARY += [(60, 20, 5, 7, "neginf"), (200, 70, 5, 7, "neginf"), (300, 260, 5, 7, "neginf")]
# Smax around threads x positions-per-thread of each tier, up to the ABI maximum
TIERS = [THREADS, THREADS * POS_LOW, THREADS * POS, THREADS * POS_MID]
TIER_S = sorted({S + d for S in TIERS for d in (-1, 0, 1)} | {MAX_S - 1, MAX_S})
BOUNDARY += [(_T_for(S, "general"), S, 2, 7, "general") for S in TIER_S]
BOUNDARY += [(_T_for(S, "plain"), S, 1, S, "plain") for S in TIER_S if S - 1 not in TIER_S or S == MAX_S]


@pytest.mark.parametrize("T,Smax,B,C,mode", BOUNDARY)
def test_across_kernel_boundaries(T, Smax, B, C, mode):
    assert THREADS * POS_WIDE >= MAX_S and 64 < THREADS
    case, want = generated(T, Smax, B, C, T * 7919 + Smax * 31 + C, mode)
    A, Bt, loglik = check_tables(case, want)
    check_viterbi(case, want["viterbi"])
    if Smax <= 300 or Smax in (THREADS * POS, MAX_S):
        check_occupancy(case, want, A, Bt, loglik)
    if mode != "neginf" and (T >= Smax or (mode == "general" and T >= Smax // 2 + 2)):
        assert np.isfinite(loglik[0])      # the full-size pair has a path: the case says something
    if B == 5 and mode in ("noskip", "nullw", "plain") and Smax >= 2:
        assert np.isneginf(loglik[1])      # one more position than frames and no skips
    if B == 5 and mode == "general" and min(T, Smax - 1) >= 2:
        assert np.isfinite(loglik[1])      # ... and a path with them


@pytest.mark.parametrize("T,Smax,mode,integer", [(20, 5, "general", 1), (100, 40, "general", 1), (30, 5, "plain", 1),
                                                 (20, 5, "general", 2), (100, 40, "plain", 2), (100, 70, "noskip", 1),
                                                 (400, 300, "general", 1), (700, 600, "general", 2),
                                                 (700, 600, "plain", 1), (1400, 1100, "general", 1)])
def test_viterbi_exact_ties(T, Smax, mode, integer):
    case, want = generated(T, Smax, 5, 7, 11 + T, mode, integer)
    assert np.array_equal(case[0], np.round(case[0]))
    assert np.isfinite(want["viterbi"][1][0])
    check_viterbi(case, want["viterbi"])


# ------------------------------------------------------------------------------ gradient
BIGNEG = -1e30   # stands for -inf in the torch loop: exp(BIGNEG - m) is exactly 0 and no gradient is NaN


def reference_loglik(lp, ids, il, sl, ws, wn, wk):
    """(loglik (B), feasible (B)) by a plain per-frame torch loop of the recursion, in lp's dtype,
    differentiable by torch autograd.  All tensors on the CPU; absent weights are None."""
    B, T, C = lp.shape
    dt = lp.dtype
    S = ids.shape[1] if ids is not None else (ws.shape[1] if ws is not None else C)
    idx = torch.arange(S).expand(B, S) if ids is None else ids.long()
    ok = (idx >= 0) & (idx < C) & (torch.arange(S)[None, :] < sl[:, None])
    neg = torch.full((), BIGNEG, dtype=dt)
    E = torch.where(ok[:, None, :], lp.clamp(min=BIGNEG).gather(2, idx.clamp(0, C - 1)[:, None, :].expand(B, T, S)), neg)
    zero = torch.zeros(B, S, dtype=dt)
    ws = zero if ws is None else ws.clamp(min=BIGNEG)
    wn = zero if wn is None else wn.clamp(min=BIGNEG)
    wk = zero + neg if wk is None else wk.clamp(min=BIGNEG)
    pad1, pad2 = torch.full((B, 1), BIGNEG, dtype=dt), torch.full((B, 2), BIGNEG, dtype=dt)
    a = torch.cat([E[:, 0, :1], torch.full((B, S - 1), BIGNEG, dtype=dt)], 1)
    for t in range(1, T):
        c = torch.stack([a + ws, torch.cat([pad1, (a + wn)[:, :-1]], 1), torch.cat([pad2, (a + wk)[:, :-2]], 1)[:, :S]])
        new = torch.logsumexp(c.clamp(min=BIGNEG), 0) + E[:, t]
        a = torch.where((t < il)[:, None], new.clamp(min=BIGNEG), a)
    ll = a.gather(1, (sl.long() - 1)[:, None])[:, 0]
    return ll, ll > BIGNEG / 1e3


@functools.lru_cache(maxsize=None)
def torch_cpu_gradient(key):
    """(case, [g_64 per differentiable input], [g_cpu32 ...], feasible)"""
    case, _ = generated(*key)
    lp, ids, il, sl, ws, wn, wk = case
    out = []
    for dtype in (torch.float64, torch.float32):
        leaves = [None if x is None else torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_()
                  for x in (lp, ws, wn, wk)]
        ll, ok = reference_loglik(leaves[0], None if ids is None else torch.from_numpy(ids), torch.from_numpy(il),
                                  torch.from_numpy(sl), *leaves[1:])
        ll[ok].sum().backward()
        out.append([None if x is None else x.grad.numpy().astype(np.float64) for x in leaves])
        feasible = ok.numpy()
    return case, out[0], out[1], feasible


GRADIENT_CASES = [(12, 5, 5, 7, 1, "general"), (40, 30, 5, 9, 2, "general"), (600, 40, 5, 50, 3, "general"),
                  (90, 64, 5, 7, 5, "noskip"), (600, 200, 5, 7, 7, "general"), (300, 260, 5, 30, 8, "general"),
                  (60, 20, 5, 7, 9, "nullw"), (80, 30, 5, 7, 10, "plain"), (60, 20, 5, 7, 4, "neginf")]


@pytest.mark.parametrize("key", GRADIENT_CASES, ids=str)
def test_gradients_against_torch_autograd(key):
    from pytorch_hmm_amd.autograd import ForcedLogLik
    case, g64, g32, feasible = torch_cpu_gradient(key)
    lp, ids, il, sl, ws, wn, wk = gpu_args(case)
    assert feasible.any()

    def run(entry):
        leaves = [None if x is None else x.clone().requires_grad_() for x in (lp, ws, wn, wk)]
        ll = entry(leaves[0], ids, il, sl, *leaves[1:])
        assert ll.requires_grad and np.array_equal(torch.isfinite(ll).cpu().numpy(), feasible)
        ll[torch.isfinite(ll)].sum().backward()
        return [None if x is None else x.grad for x in leaves]
    g1 = run(ForcedLogLik.apply)
    g2 = run(al().forced_alignment_loglik)     # goes through ForcedLogLik when an input requires grad
    names = ("log_probs", "log_stay", "log_next", "log_skip")
    for name, a, b, w64, w32 in zip(names, g1, g2, g64, g32):
        if a is None:
            assert w64 is None
            continue
        assert torch.equal(a, b)                # two calls, the same bits
        got = a.cpu().numpy().astype(np.float64)
        err_gpu, err_cpu = np.abs(got - w64).max(), np.abs(w32 - w64).max()
        print("gradient %s %s: gpu %.3e, torch cpu fp32 %.3e, ratio %.2f" % (key, name, err_gpu, err_cpu,
                                                                            err_gpu / max(err_cpu, 1e-300)))
        assert err_gpu <= 8 * err_cpu
        for i in range(len(case[2])):
            Tb, Sb = int(case[2][i]), int(case[3][i])
            pad = got[i, Tb:] if name == "log_probs" else got[i, Sb:]
            assert (pad == 0).all()
            if not feasible[i]:
                assert (got[i] == 0).all()


def test_gradient_only_in_what_requires_it():
    from pytorch_hmm_amd.autograd import ForcedLogLik
    case, _ = generated(40, 30, 5, 9, 2, "general")
    lp, ids, il, sl, ws, wn, wk = gpu_args(case)
    wn = wn.clone().requires_grad_()
    ll = ForcedLogLik.apply(lp, ids, il, sl, ws, wn, wk)
    ll[torch.isfinite(ll)].sum().backward()
    assert wn.grad is not None and torch.isfinite(wn.grad).all() and float(wn.grad.abs().sum()) > 0
    assert not al().forced_alignment_loglik(lp, ids, il, sl, ws, wn.detach(), wk).requires_grad


# ------------------------------------------------------------------------------ the module
def test_forced_aligner_end_to_end():
    torch.manual_seed(0)
    B, T, D, Lmax, K, V = 4, 50, 6, 7, 3, 11
    aligner = al().ForcedAligner(V, states_per_token=K, allow_skip=True).to(DEV)
    means = torch.nn.Parameter(torch.randn(V * K, D, device=DEV))
    log_var = torch.nn.Parameter(torch.zeros(V * K, D, device=DEV))
    x = torch.randn(B, T, D, device=DEV)

    def scorer(x):   # diagonal Gaussians per class, as GaussianHMMLayer scores its states
        d = x[:, :, None, :] - means[None, None]
        return -0.5 * ((d * d) * torch.exp(-log_var) + log_var + np.log(2 * np.pi)).sum(-1)
    tokens = torch.randint(0, V, (B, Lmax), device=DEV)
    il, tl = torch.tensor([50, 41, 30, 10]), torch.tensor([7, 5, 1, 6])    # the last: 18 states in 10 frames
    loss = aligner(scorer(x), tokens, il, tl)
    assert loss.shape == (B,) and torch.isfinite(loss).all()
    loss.sum().backward()
    for p in (aligner.transition_logits, means, log_var):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0
    used = torch.zeros(V * K, dtype=torch.bool)
    ids, sl = aligner.expand(tokens, tl)
    for b in range(B):
        used[ids[b, :int(sl[b])].long().cpu()] = True
    assert (aligner.transition_logits.grad[~used.to(DEV)] == 0).all()

    with torch.no_grad():
        lp = scorer(x)
    out = aligner.align(lp, tokens, il, tl)
    assert out["path"].shape == (B, T) and out["token_durations"].shape == (B, Lmax)
    assert out["token_durations"].dtype == torch.int32
    assert out["token_durations"].sum(1).cpu().tolist() == il.tolist()
    for b in range(B):
        assert (out["token_durations"][b, int(tl[b]):] == 0).all()
        p = out["path"][b, :int(il[b])].cpu().numpy()
        assert p[0] == 0 and p[-1] == int(sl[b]) - 1 and (np.diff(p) >= 0).all() and (np.diff(p) <= 2).all()
    assert (-loss.detach() >= out["score"] - 1e-3).all()                   # the sum holds the best path
    post = aligner.posteriors(lp, tokens, il, tl)
    assert post.shape == (B, T, Lmax * K)
    for b in range(B):
        assert torch.allclose(post[b, :int(il[b])].sum(1), torch.ones(int(il[b]), device=DEV), atol=1e-4)
        assert (post[b, int(il[b]):] == 0).all()
    # without skips the last pair has more states than frames: +inf loss, zero gradient, no NaN
    strict = al().ForcedAligner(V, states_per_token=K).to(DEV)
    loss = strict(scorer(x), tokens, il, tl)
    assert torch.isposinf(loss[3]) and torch.isfinite(loss[:3]).all()
    means.grad = None
    loss[:3].sum().backward()
    assert torch.isfinite(means.grad).all() and torch.isfinite(strict.transition_logits.grad).all()
    out = strict.align(lp, tokens, il, tl)
    assert (out["path"][3] == -1).all() and (out["token_durations"][3] == 0).all() and torch.isneginf(out["score"][3])


def test_monotonic_alignment_search_is_the_identity_chain():
    case, want = generated(70, 40, 5, 40, 21, "plain")
    value, _, il, sl = gpu_args(case)[:4]
    path, dur, score = al().monotonic_alignment_search(value, il, sl)
    ids = torch.arange(40, device=DEV, dtype=torch.int32).expand(5, 40).contiguous()
    path2, dur2, score2 = al().forced_align(value, ids, il, sl)
    assert torch.equal(path, path2) and torch.equal(dur, dur2) and torch.equal(score, score2)
    assert np.array_equal(path.cpu().numpy(), want["viterbi"][0])
    # ... and the sums: the form without ids and weights against the general kernel with explicit defaults
    zeros = torch.zeros(5, 40, device=DEV)
    ll, A, Bt = ops().forced(value, None, il, sl, alpha=True, beta=True)[:3]
    ll2, A2, Bt2 = ops().forced(value, ids, il, sl, zeros, zeros, None, alpha=True, beta=True)[:3]
    assert torch.equal(torch.isinf(A), torch.isinf(A2)) and torch.equal(torch.isinf(Bt), torch.isinf(Bt2))
    fin = torch.isfinite(ll)
    assert torch.equal(fin, torch.isfinite(ll2)) and fin.any()
    assert torch.allclose(ll[fin], ll2[fin], rtol=1e-5, atol=1e-4)
    gamma = al().forced_alignment_posteriors(value, None, il, sl)
    assert np.abs(gamma.cpu().numpy() - fz.occupancy(*case)[0]).max() <= 1e-4


def test_side_stream_matches_the_default_stream():
    case, _ = generated(200, 70, 5, 7, 33, "general")
    a = gpu_args(case)
    base = ops().forced(*a, alpha=True, beta=True, viterbi=True)
    gbase = ops().forced_grad(base[1], base[2], base[0], *a, want_gamma=True, want_stay=True, want_next=True,
                              want_skip=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = ops().forced(*a, alpha=True, beta=True, viterbi=True)
        gside = ops().forced_grad(side[1], side[2], side[0], *a, want_gamma=True, want_stay=True, want_next=True,
                                  want_skip=True)
    s.synchronize()
    for x, y in zip(base + gbase, side + gside):
        assert torch.equal(x, y)


def test_argument_errors_on_the_device():
    lp = torch.zeros(2, 6, 4, device=DEV)
    ids = torch.tensor([[1, 3, 0], [0, 1, 2]], device=DEV)
    ok = dict(ids=ids, il=torch.tensor([6, 4]), sl=torch.tensor([3, 1]), ws=None)
    for bad in (dict(il=torch.tensor([7, 4])), dict(il=torch.tensor([0, 4])), dict(sl=torch.tensor([4, 1])),
                dict(sl=torch.tensor([3, 0])), dict(ws=torch.zeros(2, 4, device=DEV)), dict(ids=ids.float()),
                dict(ids=None, sl=torch.tensor([5, 1]))):
        a = dict(ok)
        a.update(bad)
        with pytest.raises(ValueError):
            ops().forced(lp, a["ids"], a["il"], a["sl"], a["ws"])
        with pytest.raises(ValueError):
            al().forced_align(lp, a["ids"], a["il"], a["sl"], a["ws"])
    with pytest.raises(ValueError):
        ops().forced(lp[0], ids, ok["il"], ok["sl"])
    # lengths on the device are accepted too
    ll = ops().forced(lp, ids, ok["il"].to(DEV), ok["sl"].to(DEV))[0]
    assert torch.equal(ll, ops().forced(lp, ids, ok["il"], ok["sl"])[0])
