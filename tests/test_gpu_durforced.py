"""GPU: ops.durforced / ops.durforced_grad (csrc/durforced.hip), autograd.DurForcedLogLik and the
alignment functions built on them, every output against the fp64 numpy model
(tests/durforced_numpy.py).

Allowances.  The model was run in float32 against float64 over exactly the cases of this file
(tools/measure_durforced_tolerance.py; CPU only) and the largest error per quantity taken; the GPU
is allowed 8x that, for its different summation order and the 1-2 ulp of the hardware exp / log
against numpy's.  Both the absolute and the relative bound of a quantity must hold.  Relative
errors of counts are taken over counts >= COUNT_FLOOR: below it a count is a rounding-sized share
of a segment and only its absolute error says anything.

    quantity, T <= 300: 213 calls                    fp32 model, largest                    allowance (8x)
    loglik       absolute                            1.457e-03  (L256-D2-T256)              1.17e-02
    loglik       relative to max(|.|, 1)             9.885e-07  (L256-D2-T256)              7.91e-06
    gamma        absolute                            1.833e-03  (L256-D2-T258)              1.47e-02
    gamma        |row sum - 1|                       1.833e-03  (L256-D2-T258)              1.47e-02
    grad_lp      absolute                            1.833e-03  (L256-D2-T258)              1.47e-02
    dur_post     absolute                            1.635e-03  (L256-D2-T256)              1.31e-02
    dur_post     relative (>= floor)                 1.790e-03  (L256-D2-T258)              1.43e-02
    dur_post     |row sum - 1|                       1.757e-03  (L256-D2-T258)              1.41e-02
    aligner logit gradient, relative to its max-norm 2.969e-06  (aligner)                   2.38e-05
    quantity, T > 300: 5 calls                       fp32 model, largest                    allowance (8x)
    loglik       absolute                            6.409e-03  (L1024-D2-T1024)            5.13e-02
    loglik       relative to max(|.|, 1)             1.377e-06  (L1024-D16-T1024)           1.10e-05
    gamma        absolute                            7.983e-03  (L1024-D1-T1024)            6.39e-02
    gamma        |row sum - 1|                       7.782e-03  (L1024-D1-T1024)            6.23e-02
    grad_lp      absolute                            7.983e-03  (L1024-D1-T1024)            6.39e-02
    dur_post     absolute                            7.981e-03  (L1024-D1-T1024)            6.39e-02
    dur_post     relative (>= floor)                 7.981e-03  (L1024-D1-T1024)            6.39e-02
    dur_post     |row sum - 1|                       7.981e-03  (L1024-D1-T1024)            6.39e-02

The two blocks: an fp32 table's rounding grows with the size of its values, which grow with the
number of frames, and a chain of more than T_CAP positions needs more than T_CAP frames; the calls
above T_CAP frames (Lmax = 1024) have allowances of their own, so that they do not widen those of
all the others.  The largest figures come from chains that fill every frame with Dmax <= 2: a few
segmentations, tables in the thousands, and posteriors that are sums of a few exponentials of
differences of such numbers.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import durforced_numpy as M  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 8.0
MEASURED = dict(loglik_abs=1.457e-03, loglik_rel=9.885e-07, gamma_abs=1.833e-03, gamma_row=1.833e-03,
                grad_lp_abs=1.833e-03, dur_abs=1.635e-03, dur_rel=1.790e-03, dur_row=1.757e-03,
                layer_grad_rel=2.969e-06)
MEASURED_LONG = dict(loglik_abs=6.409e-03, loglik_rel=1.377e-06, gamma_abs=7.983e-03, gamma_row=7.782e-03,
                     grad_lp_abs=7.983e-03, dur_abs=7.981e-03, dur_rel=7.981e-03, dur_row=7.981e-03)
ALLOW = {k: FACTOR * v for k, v in MEASURED.items()}
ALLOW_LONG = {k: FACTOR * v for k, v in MEASURED_LONG.items()}
COUNT_FLOOR = 1e-3

POSITIONS = (1, 2, 63, 64, 65, 256, 257, 1024)
DURATIONS = (1, 2, 16, 64, 65, 128)
MAX_CELLS = 16384
T_CAP = 300


def allowance(T):
    """The allowances of a call over T frames: those of the long calls above T_CAP"""
    return ALLOW_LONG if T > T_CAP else ALLOW


def lanes(L, D):
    """Lanes per position as hmm355_durforced_f32 chooses them: a power of two, as many as 1024
    threads hold and the position's Dmax slots have work for."""
    sub = 64
    while sub > 1 and L * sub > 1024:
        sub >>= 1
    while sub > 1 and (sub >> 1) >= D:
        sub >>= 1
    return sub


def one_wave(L, D):
    """The chain sits in one wave: the hand-off is lane shuffles, there is no barrier."""
    return (L * lanes(L, D) + 63) // 64 == 1


# The chain kernel has one body and two switches, both chosen by size (csrc/durforced.hip): the
# lanes per position, 64 .. 1, halved while Lmax * lanes > 1024 (Lmax 16|17, 32|33, 64|65, 128|129,
# 256|257, 512|513) and while half of them still cover Dmax (Dmax 1|2|3, 4|5, 8|9, 16|17, 32|33);
# and the hand-off, lane shuffles when Lmax * lanes <= 64, else LDS and a barrier ((2,32)|(2,33),
# (4,16)|(4,17), (8,8)|(8,9), (32,2)|(33,2), (64,1)|(65,1)).  Both sides of each:
SWITCH_PAIRS = [(16, 40), (17, 40), (32, 40), (33, 40), (128, 40), (129, 40), (512, 32), (513, 31),
                (5, 3), (5, 4), (5, 5), (5, 8), (5, 9), (5, 17), (5, 32), (5, 33),
                (2, 32), (2, 33), (4, 16), (4, 17), (8, 8), (8, 9), (32, 2), (33, 2)]
PAIRS = [(L, D) for L in POSITIONS for D in DURATIONS if L * D <= MAX_CELLS] + SWITCH_PAIRS


def test_switch_pairs_cross_every_switch():
    subs = {lanes(L, D) for L, D in PAIRS}
    assert subs == {1, 2, 4, 8, 16, 32, 64}
    for a, b in ((16, 17), (32, 33), (128, 129)):
        assert lanes(a, 40) == 2 * lanes(b, 40)
    assert lanes(512, 32) == 2 * lanes(513, 31) == 2 and lanes(64, 128) == 2 * lanes(65, 128)
    assert [lanes(5, D) for D in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33)] == [1, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64]
    for wave, lds in (((2, 32), (2, 33)), ((4, 16), (4, 17)), ((8, 8), (8, 9)), ((32, 2), (33, 2)), ((64, 1), (65, 1))):
        assert one_wave(*wave) and not one_wave(*lds)


# ------------------------------------------------------------------------------------ cases
# (everything below this line down to "the GPU side" runs without a GPU: the tolerance tool
# imports it).  A case is (name, lp (B,T,C), ids (B,Lmax) or None, il (B), sl (B), dur (B,Lmax,Dmax)).
def lengths(L, D):
    """T in {L, L+1, L+Dmax, min(L Dmax, 3 L)}, capped at T_CAP but never below L, without the
    lengths the full chain cannot fill (T > L Dmax)"""
    return sorted({max(L, min(t, T_CAP)) for t in (L, L + 1, L + D, min(L * D, 3 * L)) if t <= L * D})


def ragged(L, D, T):
    """Three feasible (T_b, L_b): the full pair, two thirds of the chain, half of it"""
    sl = [L, max(1, (2 * L + 2) // 3), max(1, L // 2)]
    il = [T, min(T, max(sl[1], min(sl[1] * D, T - 1))), min(T, max(sl[2], min(sl[2] * D, (T + 1) // 2)))]
    return np.array(il, np.int32), np.array(sl, np.int32)


def random_case(L, D, T, seed, classes=None, B=3, mean=-5.0, std=3.0):
    rng = np.random.default_rng(seed)
    C = classes or (min(L, 23) + 2)   # chains longer than that repeat classes
    lp = rng.normal(mean, std, (B, T, C)).astype(np.float32)
    ids = rng.integers(0, C, (B, L)).astype(np.int32)
    du = np.log(rng.random((B, L, D)) + 1e-3).astype(np.float32)
    il, sl = ragged(L, D, T)
    return lp, ids, il[:B], sl[:B], du


def pair_cases(L, D):
    return [(f"L{L}-D{D}-T{T}", *random_case(L, D, T, 100000 * L + 100 * D + T)) for T in lengths(L, D)]


def case_infeasible():
    """Four pairs: feasible, T_b < L_b, T_b > L_b Dmax, and -inf durations that leave no
    segmentation (every position needs three frames, there are not enough)."""
    rng = np.random.default_rng(21)
    L, D, T = 6, 4, 20
    lp = rng.normal(-5, 3, (4, T, 5)).astype(np.float32)
    ids = rng.integers(0, 5, (4, L)).astype(np.int32)
    du = np.log(rng.random((4, L, D)) + 1e-3).astype(np.float32)
    du[3, :, :2] = -np.inf
    return ("infeasible", lp, ids, np.array([12, 3, 20, 14], np.int32), np.array([6, 5, 4, 5], np.int32), du)


def case_min_duration():
    lp, ids, il, sl, du = random_case(7, 8, 40, 22)
    du[:, :, :2] = -np.inf   # no segment shorter than 3 frames
    return ("min-duration", lp, ids, il, sl, du)


def case_large_emissions():
    """Emissions around -300 per frame: unshifted tables would reach 1e4 and lose the posteriors"""
    lp, ids, il, sl, du = random_case(12, 10, 64, 23, mean=-300.0, std=30.0)
    return ("large-emissions", lp, ids, il, sl, du)


def case_inf_emissions():
    """Scattered -inf emissions and two class ids outside [0, C): one past the end of the third
    chain (never read), one inside the second chain, which then has no segmentation left"""
    lp, ids, il, sl, du = random_case(6, 6, 24, 24, classes=6)
    hole = np.random.default_rng(30).random(lp.shape) < 0.15
    lp[hole] = -np.inf
    ids[2, 5] = 99
    ids[1, 3] = -4   # inside the second chain: it has no segmentation left
    return ("inf-emissions", lp, ids, il, sl, du)


def case_identity_chain():
    """state_ids None: position l emits column l of log_probs (B,T,Lmax)"""
    lp, _, il, sl, du = random_case(9, 5, 21, 26, classes=9)
    return ("identity-chain", lp, None, il, sl, du)


def case_integer_ties():
    """Integer-valued scores from a small set: every fp32 sum is exact and many segmentations tie"""
    rng = np.random.default_rng(27)
    B, L, D, T = 3, 7, 5, 19
    lp = rng.integers(-3, 1, (B, T, 4)).astype(np.float32)
    ids = rng.integers(0, 4, (B, L)).astype(np.int32)
    du = rng.integers(-2, 1, (B, L, D)).astype(np.float32)
    il, sl = ragged(L, D, T)
    return ("integer-ties", lp, ids, il, sl, du)


def case_integer_ties_wide():
    """The same over several waves and lanes per position, flat scores: everything ties"""
    B, L, D, T = 3, 70, 9, 150
    lp = np.zeros((B, T, 3), np.float32)
    ids = (np.arange(B * L).reshape(B, L) % 3).astype(np.int32)
    du = np.zeros((B, L, D), np.float32)
    du[:, ::2, 0] = -1.0
    il, sl = ragged(L, D, T)
    return ("integer-ties-wide", lp, ids, il, sl, du)


SPECIAL = (case_infeasible, case_min_duration, case_large_emissions, case_inf_emissions, case_identity_chain,
           case_integer_ties, case_integer_ties_wide)


def aligner_case():
    """tokens, lengths and emissions of the DurationForcedAligner tests"""
    rng = np.random.default_rng(28)
    B, T, K, L, D = 3, 30, 6, 8, 7
    lp = rng.normal(-4, 2, (B, T, K)).astype(np.float32)
    tokens = rng.integers(0, K, (B, L)).astype(np.int64)
    logits = rng.normal(0, 1, (K, D)).astype(np.float32)
    return lp, tokens, np.array([30, 22, 9], np.int64), np.array([8, 6, 3], np.int64), logits


def aligner_logit_grad(dur_post, tokens, tl, logits):
    """d sum_b loglik / d logits (K,D) from the duration posteriors: the log-softmax's chain rule"""
    z = logits.astype(np.float64)
    sm = np.exp(z - z.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    g = np.zeros_like(z)
    for b in range(tokens.shape[0]):
        for q in range(int(tl[b])):
            row = dur_post[b, q].astype(np.float64)
            g[tokens[b, q]] += row - sm[tokens[b, q]] * row.sum()
    return g


def aligner_dur_lp(tokens, logits):
    z = logits.astype(np.float64)
    lsm = z - z.max(1, keepdims=True)
    lsm = lsm - np.log(np.exp(lsm).sum(1, keepdims=True))
    return lsm[tokens].astype(np.float32)


def all_cases():
    for L, D in PAIRS:
        yield from pair_cases(L, D)
    for make in SPECIAL:
        yield make()


def errors(got, ref, il, sl):
    """The figures the allowances bound, of one call: got and ref are dicts of loglik, gamma,
    dur_post, grad_lp as model() returns them"""
    out = {}
    fin = np.isfinite(ref["loglik"])
    d = np.abs(got["loglik"][fin] - ref["loglik"][fin])
    out["loglik_abs"] = float(d.max()) if fin.any() else 0.0
    out["loglik_rel"] = float((d / np.maximum(np.abs(ref["loglik"][fin]), 1.0)).max()) if fin.any() else 0.0
    out["gamma_abs"] = float(np.abs(got["gamma"] - ref["gamma"]).max())
    out["grad_lp_abs"] = float(np.abs(got["grad_lp"] - ref["grad_lp"]).max())
    dd = np.abs(got["dur_post"] - ref["dur_post"])
    out["dur_abs"] = float(dd.max())
    big = ref["dur_post"] >= COUNT_FLOOR
    out["dur_rel"] = float((dd[big] / ref["dur_post"][big]).max()) if big.any() else 0.0
    rows_g, rows_d = [0.0], [0.0]
    for b in np.nonzero(fin)[0]:
        rows_g.append(float(np.abs(got["gamma"][b, :il[b], :sl[b]].sum(1) - 1.0).max()))
        rows_d.append(float(np.abs(got["dur_post"][b, :sl[b]].sum(1) - 1.0).max()))
    out["gamma_row"] = max(rows_g)
    out["dur_row"] = max(rows_d)
    return out


# ------------------------------------------------------------------------------------ the GPU side
DEV = "cuda"


def dev(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(DEV)


def run_gpu(lp, ids, il, sl, du, viterbi=True):
    from pytorch_hmm_amd import ops
    args = (dev(lp), dev(ids), torch.as_tensor(il), torch.as_tensor(sl), dev(du))
    out = ops.durforced(*args, tables=True, viterbi=viterbi)
    gamma, grad, dur_post = ops.durforced_grad(*out[1:7], *args, want_gamma=True, want_grad=True, want_dur=True)
    got = dict(loglik=out[0], gamma=gamma, grad_lp=grad, dur_post=dur_post)
    if viterbi:
        got.update(path=out[7], score=out[8], durations=out[9])
    return {k: v.cpu().numpy().astype(np.float64 if v.dtype.is_floating_point else np.int64) for k, v in got.items()}


def check(name, case, got, ref):
    lp, ids, il, sl, du = case
    for k, v in got.items():
        assert not np.isnan(v).any(), (name, k, "NaN")
    fin = np.isfinite(ref["loglik"])
    assert np.array_equal(np.isfinite(got["loglik"]), fin), (name, got["loglik"], ref["loglik"])
    assert np.all(got["loglik"][~fin] == -np.inf)
    e = errors(got, ref, il, sl)
    print(name, " ".join(f"{k}={v:.3e}" for k, v in e.items()))
    allow = allowance(lp.shape[1])
    for k, v in e.items():
        assert v <= allow[k], (name, k, v, allow[k])
    for b in range(len(il)):
        # past either length, and an infeasible pair, everything is exactly zero
        assert not got["gamma"][b, il[b]:].any() and not got["gamma"][b, :, sl[b]:].any(), name
        assert not got["grad_lp"][b, il[b]:].any() and not got["dur_post"][b, sl[b]:].any(), name
        if not fin[b]:
            assert not got["gamma"][b].any() and not got["grad_lp"][b].any() and not got["dur_post"][b].any(), name
    if "path" in got:
        check_viterbi(name, case, got, ref)


def check_viterbi(name, case, got, ref):
    """A valid segmentation whose fp64 score is the fp64 optimum within the loglik allowance"""
    lp, ids, il, sl, du = case
    for b in range(len(il)):
        Tb, Lb = int(il[b]), int(sl[b])
        path, d = got["path"][b], got["durations"][b]
        if not np.isfinite(ref["score"][b]):
            assert got["score"][b] == -np.inf and np.all(path == -1) and not d.any(), (name, b)
            continue
        assert np.all(path[Tb:] == -1) and not d[Lb:].any(), (name, b)
        assert d[:Lb].min() >= 1 and d[:Lb].max() <= du.shape[2] and d[:Lb].sum() == Tb, (name, b, d[:Lb])
        assert np.array_equal(path[:Tb], np.repeat(np.arange(Lb), d[:Lb])), (name, b)
        opt = float(ref["score"][b])
        scale = max(abs(opt), 1.0)
        allow = allowance(lp.shape[1])
        for value in (M.rescore(lp[b], None if ids is None else ids[b], du[b], d, Tb, Lb), float(got["score"][b])):
            err = abs(value - opt)
            assert err <= allow["loglik_abs"] and err / scale <= allow["loglik_rel"], (name, b, value, opt)


LENGTHS = [(L, D, T) for L, D in PAIRS for T in lengths(L, D)]


@pytest.mark.parametrize("L,D,T", LENGTHS, ids=[f"L{L}-D{D}-T{T}" for L, D, T in LENGTHS])
def test_against_model(L, D, T):
    """One (Lmax, Dmax, T): a ragged batch of three, then its first sequence alone."""
    (name, *case), = [c for c in pair_cases(L, D) if c[1].shape[1] == T]
    ref = M.model(*case)
    check(name + "-B3", case, run_gpu(*case), ref)
    one = tuple(None if a is None else a[:1] for a in case)
    check(name + "-B1", one, run_gpu(*one), {k: v[:1] for k, v in ref.items()})


@pytest.mark.parametrize("make", SPECIAL, ids=[m.__name__[5:] for m in SPECIAL])
def test_special_case_against_model(make):
    name, *case = make()
    ref = M.model(*case)
    got = run_gpu(*case)
    check(name, case, got, ref)
    if name == "infeasible":
        assert np.isfinite(ref["loglik"]).tolist() == [True, False, False, False]
    if name == "inf-emissions":
        assert np.isfinite(ref["loglik"]).tolist() == [True, False, True]
    if name.startswith("integer-ties"):
        # exact: every sum is an integer below 2^24, so the tie rule decides
        assert np.array_equal(got["durations"], ref["durations"]), (got["durations"], ref["durations"])
        assert np.array_equal(got["path"], ref["path"]) and np.array_equal(got["score"], ref["score"])


def test_value_only_and_viterbi_only_calls_agree():
    """Without tables no table comes back, and loglik / the segmentation have the bits of the full call"""
    from pytorch_hmm_amd import ops
    name, *case = case_min_duration()
    args = (dev(case[0]), dev(case[1]), torch.as_tensor(case[2]), torch.as_tensor(case[3]), dev(case[4]))
    full = ops.durforced(*args, tables=True, viterbi=True)
    plain = ops.durforced(*args)
    vit = ops.durforced(*args, viterbi=True)
    assert all(t.numel() == 0 for t in plain[1:]) and all(t.numel() == 0 for t in vit[1:7])
    assert torch.equal(plain[0], full[0]) and torch.equal(vit[0], full[0])
    for k in (7, 8, 9):
        assert torch.equal(vit[k], full[k])


def test_matches_forced_alignment_with_geometric_durations():
    """Dmax >= T and dur_lp[b,l,d-1] = (d-1) log_stay[b,l] + (l < L_b-1 ? log_next[b,l] : 0) is the
    stay / next chain of ops.forced without skips: loglik and the Viterbi score agree."""
    from pytorch_hmm_amd import ops
    rng = np.random.default_rng(31)
    B, T, L, C = 3, 40, 9, 7
    lp = rng.normal(-5, 3, (B, T, C)).astype(np.float32)
    ids = rng.integers(0, C, (B, L)).astype(np.int32)
    il, sl = np.array([40, 33, 17], np.int32), np.array([9, 6, 4], np.int32)
    stay = np.log(rng.uniform(0.3, 0.9, (B, L))).astype(np.float32)
    nxt = np.log1p(-np.exp(stay.astype(np.float64))).astype(np.float32)
    d1 = np.arange(T, dtype=np.float64)[None, None, :]
    last = np.arange(L)[None, :] >= (sl[:, None] - 1)
    du = (d1 * stay[:, :, None] + np.where(last, 0.0, nxt)[:, :, None]).astype(np.float32)
    a = ops.forced(dev(lp), dev(ids), torch.as_tensor(il), torch.as_tensor(sl), dev(stay), dev(nxt), None,
                   viterbi=True)
    d = ops.durforced(dev(lp), dev(ids), torch.as_tensor(il), torch.as_tensor(sl), dev(du), viterbi=True)
    for mine, theirs in ((d[0], a[0]), (d[8], a[4])):
        mine, theirs = mine.double().cpu().numpy(), theirs.double().cpu().numpy()
        err = np.abs(mine - theirs)
        print("forced cross-check", err.max())
        assert err.max() <= ALLOW["loglik_abs"] and (err / np.maximum(np.abs(theirs), 1)).max() <= ALLOW["loglik_rel"]


def torch_loglik(lp, ids, il, sl, du):
    """The forward recursion in plain torch (fp64, autograd): loglik (B).  -1e30 stands for -inf:
    exp(-1e30 - m) is exactly 0 and autograd's logsumexp sees no NaN."""
    out = []
    for b in range(lp.shape[0]):
        Tb, Lb = int(il[b]), int(sl[b])
        e = lp[b, :Tb][:, ids[b, :Lb].long()]
        Dm = du.shape[2]
        ninf = lp.new_full((), -1e30)
        begin = [torch.stack([lp.new_zeros(()) if q == 0 else ninf for q in range(Lb)])]
        cs = torch.cat([e.new_zeros(1, Lb), e.cumsum(0)])
        for t in range(Tb):
            cand = [begin[t - d] + (cs[t + 1] - cs[t - d]) + du[b, :Lb, d] for d in range(min(Dm, t + 1))]
            Ft = torch.logsumexp(torch.stack(cand), 0)
            begin.append(torch.cat([ninf.reshape(1), Ft[:-1]]))
        out.append(Ft[Lb - 1])
    return torch.stack(out)


def test_autograd_matches_torch_fp64():
    """DurForcedLogLik against torch autograd through the plain-torch recursion; gradients come
    only in what requires them"""
    from pytorch_hmm_amd.alignment import duration_forced_loglik
    from pytorch_hmm_amd.autograd import DurForcedLogLik
    lp, ids, il, sl, du = random_case(6, 5, 17, 41, classes=4)
    w = torch.tensor([0.7, -1.3, 2.0], dtype=torch.float64)
    lp64 = torch.tensor(lp, dtype=torch.float64, requires_grad=True)
    du64 = torch.tensor(du, dtype=torch.float64, requires_grad=True)
    ref = torch_loglik(lp64, torch.tensor(ids), il, sl, du64)
    (ref * w).sum().backward(retain_graph=True)
    g_lp, g_du = dev(lp).requires_grad_(), dev(du).requires_grad_()
    ll = DurForcedLogLik.apply(g_lp, dev(ids), torch.as_tensor(il), torch.as_tensor(sl), g_du)
    (ll.double() * w.to(DEV)).sum().backward()
    err = (ll.detach().double().cpu() - ref.detach()).abs().max().item()
    assert err <= ALLOW["loglik_abs"], err
    wmax = float(w.abs().max())
    for mine, theirs, key in ((g_lp.grad, lp64.grad, "grad_lp_abs"), (g_du.grad, du64.grad, "dur_abs")):
        err = (mine.double().cpu() - theirs).abs().max().item()
        print("autograd", key, err)
        assert err <= wmax * ALLOW[key], (key, err)
    # only what requires grad
    a, b = dev(lp).requires_grad_(), dev(du)
    duration_forced_loglik(a, dev(ids), torch.as_tensor(il), torch.as_tensor(sl), b).sum().backward()
    assert a.grad is not None and b.grad is None
    assert (a.grad.double().cpu() - torch.autograd.grad(ref.sum(), lp64, retain_graph=True)[0]).abs().max().item() <= ALLOW["grad_lp_abs"]
    a, b = dev(lp), dev(du).requires_grad_()
    duration_forced_loglik(a, dev(ids), torch.as_tensor(il), torch.as_tensor(sl), b).sum().backward()
    assert a.grad is None and (b.grad.double().cpu() - torch.autograd.grad(ref.sum(), du64)[0]).abs().max().item() \
        <= ALLOW["dur_abs"]
    assert not duration_forced_loglik(dev(lp), dev(ids), torch.as_tensor(il), torch.as_tensor(sl), dev(du)).requires_grad


def test_infeasible_pairs_give_zero_gradient():
    from pytorch_hmm_amd.alignment import duration_forced_loglik
    name, lp, ids, il, sl, du = case_infeasible()
    a, b = dev(lp).requires_grad_(), dev(du).requires_grad_()
    ll = duration_forced_loglik(a, dev(ids), torch.as_tensor(il), torch.as_tensor(sl), b)
    assert torch.isinf(ll[1:]).all() and torch.isfinite(ll[0])
    (-ll).sum().backward()
    for g in (a.grad, b.grad):
        assert not torch.isnan(g).any() and not g[1:].any() and g[0].any()


def test_aligner_end_to_end():
    """DurationForcedAligner: forward's gradients against torch fp64, align and posteriors against
    the model, and a predictor's dur_lp in the place of the module's table"""
    import pytorch_hmm_amd as ph
    lp, tokens, il, tl, logits = aligner_case()
    K, D = logits.shape
    m = ph.DurationForcedAligner(K, D).to(DEV)
    assert torch.allclose(torch.softmax(m.duration_logits, 1), torch.full((K, D), 1.0 / D, device=DEV))
    with torch.no_grad():
        m.duration_logits.copy_(dev(logits))
    lpg = dev(lp).requires_grad_()
    loss = m(lpg, dev(tokens), torch.as_tensor(il), torch.as_tensor(tl))
    assert loss.shape == (3,)
    loss.sum().backward()
    du = aligner_dur_lp(tokens, logits)
    case = (lp, tokens.astype(np.int32), il.astype(np.int32), tl.astype(np.int32), du)
    ref = M.model(*case)
    assert np.abs(-loss.detach().double().cpu().numpy() - ref["loglik"]).max() <= ALLOW["loglik_abs"]
    assert np.abs(-lpg.grad.double().cpu().numpy() - ref["grad_lp"]).max() <= ALLOW["grad_lp_abs"]
    want = -aligner_logit_grad(ref["dur_post"], tokens, tl, logits)
    err = np.abs(m.duration_logits.grad.double().cpu().numpy() - want).max() / np.abs(want).max()
    print("aligner logit gradient, relative to its max-norm", err)
    assert err <= ALLOW["layer_grad_rel"], err
    out = m.align(dev(lp), dev(tokens), torch.as_tensor(il), torch.as_tensor(tl))
    got = dict(path=out["path"].cpu().numpy(), durations=out["token_durations"].cpu().numpy(),
               score=out["score"].double().cpu().numpy())
    assert out["token_durations"].dtype == torch.int32 and out["path"].dtype == torch.int32
    check_viterbi("aligner", case, got, ref)
    gamma, dur_post = m.posteriors(dev(lp), dev(tokens), torch.as_tensor(il), torch.as_tensor(tl))
    assert np.abs(gamma.double().cpu().numpy() - ref["gamma"]).max() <= ALLOW["gamma_abs"]
    assert np.abs(dur_post.double().cpu().numpy() - ref["dur_post"]).max() <= ALLOW["dur_abs"]
    # the duration-predictor use: dur_lp given, differentiable, the module's logits untouched
    m.zero_grad()
    pred = dev(du[:, :, :5] + 0.25).requires_grad_()
    loss2 = m(dev(lp), dev(tokens), torch.as_tensor(il), torch.as_tensor(tl), dur_lp=pred)
    loss2.sum().backward()
    ref2 = M.model(lp, case[1], case[2], case[3], du[:, :, :5] + 0.25)
    assert np.abs(-loss2.detach().double().cpu().numpy() - ref2["loglik"]).max() <= ALLOW["loglik_abs"]
    assert np.abs(-pred.grad.double().cpu().numpy() - ref2["dur_post"]).max() <= ALLOW["dur_abs"]
    assert m.duration_logits.grad is None


def test_side_stream_and_repeat_give_the_same_bits():
    name, *case = pair_cases(65, 16)[-1]
    first = run_gpu(*case)
    again = run_gpu(*case)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = run_gpu(*case)
    torch.cuda.current_stream().wait_stream(s)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
        assert np.array_equal(first[k], side[k]), k
