"""GPU parity of the CTC lattice (csrc/ctc.hip; ops.ctc / ops.ctc_grad / autograd.CTCLogLik;
pytorch_hmm_amd.alignment.ctc).

Contracts:
  * alpha, beta: the -inf pattern equals the fixture's (the reference's beta, the fp64 tables) and
    the numpy restatement's exactly; finite entries and loglik obey
        |x_gpu - x_fp64| <= 4 n 2^-24 max(1, |x_fp64|),
    n the recursion steps behind the entry: t + 1 for alpha[t], T_b - t for beta[t] (beta runs down
    from frame T_b - 1), T_b for loglik.  Each step is an exact max, a few fp32 roundings at the
    magnitude of the value and an expf / logf on O(1) arguments (soft-DTW's 4 (N+M) 2^-24 has the
    same form).  Measured on MI355X over every case here: the largest error is 0.15 of the bound
    for alpha, 0.22 for beta and 0.09 for loglik.
  * Viterbi positions and score: bit-identical to the fp32 restatement (an exact max and one add
    per cell), planted exact ties included (integer-valued and all-equal log-probs).
  * Gradient: with g_64 / g_cpu32 the fp64 / fp32 gradients of torch's CPU nn.CTCLoss at the
    logits (through log_softmax), CTCLogLik back-propagated through log_softmax on the GPU has
        max |g_gpu - g_64| <= 8 x max |g_cpu32 - g_64|
    (the margin test_gpu_dtw.py grants the soft-DTW gradient).  Measured ratios on MI355X:
    see GRADIENT_RATIOS below.  Frames >= input_lengths[b] and pairs with no alignment get
    exact zeros, and two successive calls are torch.equal.
  * ctc_alignment_path: method="reference" equals the fixture (all blank); "viterbi" equals the
    restatement; "posterior" equals the fp64 restatement's argmax wherever that argmax leads the
    runner-up by more than the two tables' error bounds (below that fp32 cannot tell them apart,
    and the kernel's choice must then be one of the near-maximal positions).

Beyond the fixtures the cases sit on the kernel's own boundaries, read from ctc.hip: S' around the
single-wave limit and a wave multiple, L around threads x positions-per-thread (and the tier
limits), T around the prefetch ring's depth and one long run, ragged batches of 5, C in {2, 7}.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_numpy as cn  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "ctc.hip")).read()


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


THREADS, POS_LOW, POS, POS_MID, POS_WIDE, AHEAD = (_const(n) for n in (
    "kCtcThreads", "kCtcPosLow", "kCtcPos", "kCtcPosMid", "kCtcPosWide", "kCtcAhead"))
MAX_L = 2048
# measured on MI355X: max |g_gpu - g_64| / max |g_cpu32 - g_64| per gradient case (bound: 8);
# the errors themselves run from 5e-7 (T = 12) to 1.9e-3 (T = 600, |loglik| ~ 1000), torch's alike
GRADIENT_RATIOS = {"basic": 0.97, "empty": 0.52, "blank3": 1.89, "long": 0.85, "T600_L40": 0.97, "T90_L64": 0.97,
                   "T600_L200": 1.01}


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
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def gpu_args(case):
    lp, tg, il, tl, blank = case
    return dev(lp, torch.float32), dev(tg), torch.as_tensor(np.asarray(il)), torch.as_tensor(np.asarray(tl)), blank


def fixture_case(g):
    return g["lp"], g["targets"], g["input_lengths"], g["target_lengths"], int(g["blank"])


@functools.lru_cache(maxsize=None)
def generated(T, Lmax, B, C, seed, integer=0):
    """A ragged case and its oracles.  The first sequence uses all of T and Lmax; labels repeat now
    and then; with C == 2 every label is the one non-blank class.  integer=1: log-probs are small
    negative integers (exact ties), integer=2: all zero (every comparison ties)."""
    rng = np.random.default_rng(seed)
    if integer == 2:
        lp = np.zeros((T, B, C), dtype=np.float32)
    elif integer == 1:
        lp = -rng.integers(0, 3, (T, B, C)).astype(np.float32)
    else:
        x = rng.standard_normal((T, B, C))
        lp = (x - np.log(np.exp(x).sum(2, keepdims=True))).astype(np.float32)
    blank = 0 if C == 2 else 1
    labels = [c for c in range(C) if c != blank]
    tg = rng.choice(labels, size=(B, Lmax))
    rep = rng.random((B, Lmax)) < 0.15
    for i in range(1, Lmax):
        tg[:, i] = np.where(rep[:, i], tg[:, i - 1], tg[:, i])
    tl = np.array([Lmax, Lmax // 2, 0, 1, (3 * Lmax) // 4][:B])
    il = np.array([T, max(1, T - 3), max(1, T // 2), T, max(1, T - 1)][:B])
    case = (lp, tg, il, tl, blank)
    A64, ll64 = cn.alpha(*case, dtype=np.float64)
    B64 = cn.beta(*case, dtype=np.float64)
    return case, dict(alpha64=A64, beta64=B64, loglik64=ll64, viterbi=cn.viterbi(*case))


def check_tables(case, want):
    lp, tg, il, tl, blank = case
    T, B, _ = lp.shape
    loglik, A, Bt, _, _ = ops().ctc(*gpu_args(case)[:4], blank, alpha=True, beta=True)
    value_only = ops().ctc(*gpu_args(case)[:4], blank)
    assert value_only[1].numel() == 0 and value_only[2].numel() == 0
    assert torch.equal(value_only[0], loglik)            # the value-only call runs the same chain
    A, Bt, loglik = A.cpu().numpy(), Bt.cpu().numpy(), loglik.cpu().numpy()
    assert A.shape == want["alpha64"].shape and A.dtype == np.float32
    ex = (cn.step_bound_excess(A, want["alpha64"], cn.alpha_steps(T, B)),
          cn.step_bound_excess(Bt, want["beta64"], cn.beta_steps(T, il)),
          cn.step_bound_excess(loglik, want["loglik64"], np.asarray(il)))
    print("step-bound use (alpha, beta, loglik): %.3f %.3f %.3f" % ex)
    assert max(ex) <= 1.0, ex
    return A, Bt, loglik


def check_viterbi(case, want):
    _, _, _, path, score = ops().ctc(*gpu_args(case)[:4], case[4], viterbi=True)
    wpos, wscore = want
    assert path.dtype == torch.int32
    assert np.array_equal(path.cpu().numpy(), wpos)
    assert np.array_equal(bits(score.cpu().numpy()), bits(wscore))


def check_gradient(case, A, Bt, loglik):
    """gamma and the class gradient against the fp64 restatement; exact zeros; run-to-run bits."""
    lp, tg, il, tl, blank = case
    T, B, C = lp.shape
    g64, grad64 = cn.occupancy(*case)
    a = gpu_args(case)
    call = lambda: ops().ctc_grad(dev(A), dev(Bt), dev(loglik), a[1], a[2], a[3], C, blank, want_gamma=True)  # noqa: E731
    grad, gamma = call()
    grad2, gamma2 = call()
    assert torch.equal(grad, grad2) and torch.equal(gamma, gamma2)
    grad, gamma = grad.cpu().numpy(), gamma.cpu().numpy()
    for b in range(B):
        assert (grad[il[b]:, b] == 0).all() and (gamma[b, il[b]:] == 0).all()
        if not np.isfinite(loglik[b]):
            assert (grad[:, b] == 0).all() and (gamma[b] == 0).all()
            continue
        # exp(alpha + beta - loglik): the exponent carries the three step bounds
        mag = max(1.0, np.abs(A[b][np.isfinite(A[b])]).max(), np.abs(Bt[b][np.isfinite(Bt[b])]).max(initial=0.0))
        e = 4 * (2 * int(il[b]) + 1 + int(il[b])) * cn.EPS24 * mag
        tol = np.expm1(e) + 4 * cn.EPS24
        assert np.abs(gamma[b] - g64[b]).max() <= tol
        assert np.abs(grad[:, b] - grad64[:, b]).max() <= tol * (1 + 2 * cn.EPS24 * (2 * int(tl[b]) + 1))


# ------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", cn.FIXTURES)
def test_fixture_tables_viterbi_and_gradient(gold, name):
    g = gold("ctc_" + name)
    case = fixture_case(g)
    A, Bt, loglik = check_tables(case, g)
    assert np.array_equal(np.isneginf(Bt), np.isneginf(g["ref_beta"]))
    assert np.array_equal(np.isneginf(loglik), np.isneginf(g["ref_loglik"]))
    A32, _ = cn.alpha(*case)
    assert np.array_equal(np.isneginf(A), np.isneginf(A32))
    check_viterbi(case, cn.viterbi(*case))
    check_gradient(case, A, Bt, loglik)


@pytest.mark.parametrize("name", cn.FIXTURES)
def test_alignment_module_on_fixture(gold, name):
    g = gold("ctc_" + name)
    case = fixture_case(g)
    lp, tg, il, tl, blank = gpu_args(case)
    T, B, C = case[0].shape
    ll = al().ctc_forward_algorithm(lp, tg, il, tl, blank)
    bt = al().ctc_backward_algorithm(lp, tg, il, tl, blank)
    assert ll.shape == (B,) and ll.dtype == torch.float32 and bt.shape == g["ref_beta"].shape and bt.dtype == torch.float32
    loglik, _, beta, _, _ = ops().ctc(lp, tg, il, tl, blank, beta=True)
    assert torch.equal(ll, loglik) and torch.equal(bt, beta)
    # lengths on the device are accepted too
    assert torch.equal(al().ctc_forward_algorithm(lp, tg, il.to(DEV), tl.to(DEV), blank), ll)

    aligner = al().CTCAligner(C, blank_id=blank)
    for paths in (al().ctc_alignment_path(lp, tg, il, tl, blank), aligner.align(lp, tg, il, tl)):
        for b, p in enumerate(paths):
            assert p.is_cuda and p.dtype == torch.int64
            assert np.array_equal(p.cpu().numpy(), g["ref_align"][b, :case[2][b]])

    wpos, wscore = cn.viterbi(*case)
    pos, toks, score = al().ctc_forced_align(lp, tg, il, tl, blank)
    assert pos.dtype == torch.int64 and np.array_equal(pos.cpu().numpy(), wpos)
    assert np.array_equal(bits(score.cpu().numpy()), bits(wscore))
    want_tokens = cn.tokens(wpos, case[1], case[2], blank)
    for got in (toks, al().ctc_alignment_path(lp, tg, il, tl, blank, method="viterbi"),
                aligner.align(lp, tg, il, tl, method="viterbi")):
        for b in range(B):
            assert got[b].dtype == torch.int64 and np.array_equal(got[b].cpu().numpy(), want_tokens[b])

    # posterior: the fp64 argmax wherever it is decided by more than the tables' error bounds
    with np.errstate(all="ignore"):
        tot = g["alpha64"] + g["beta64"]
    want = cn.posterior_positions(g["alpha64"], g["beta64"], case[2])
    pos, toks, score = al().ctc_forced_align(lp, tg, il, tl, blank, method="posterior")
    pos = pos.cpu().numpy()
    assert torch.equal(score, ll)
    decided = 0
    for b in range(B):
        Tb = int(case[2][b])
        assert (pos[b, Tb:] == -1).all()
        for t in range(Tb):
            row = tot[b, t]
            if not np.isfinite(row.max()):
                assert pos[b, t] == 0       # nothing reachable: the lowest index
                continue
            slack = 2 * 4 * (Tb + 1) * cn.EPS24 * max(1.0, abs(row.max()))   # two entries, each alpha + beta
            assert row[pos[b, t]] >= row.max() - slack
            if np.sort(row)[-2] < row.max() - slack:
                decided += 1
                assert pos[b, t] == want[b, t]
    assert decided >= 0.5 * sum(int(case[2][b]) for b in range(B) if np.isfinite(g["loglik64"][b]))
    ptoks = al().ctc_alignment_path(lp, tg, il, tl, blank, method="posterior")
    ext = cn.expand(case[1], blank)
    for b in range(B):
        assert np.array_equal(ptoks[b].cpu().numpy(), ext[b, np.maximum(pos[b, :case[2][b]], 0)])
        assert np.array_equal(toks[b].cpu().numpy(), ptoks[b].cpu().numpy())


# --------------------------------------------------------- the kernel's own boundaries
FULL = THREADS * POS           # positions of the first LDS form
BOUNDARY = []
# S' = 63, 65, 127, 129: the single-wave limit and the next wave multiple
BOUNDARY += [(2 * L + 40, L, 5, 7) for L in (31, 32, 63, 64)]
# the prefetch ring: T around its depth, in the single-wave and in two LDS forms; long runs
BOUNDARY += [(T, Lmax, 5, 7) for T in (1, AHEAD - 1, AHEAD, AHEAD + 1) for Lmax in (3, 40, 200)]
BOUNDARY += [(600, 3, 5, 2), (600, 40, 5, 7), (600, 200, 5, 7)]
# C = 2: every label is the same class, every skip is forbidden
BOUNDARY += [(30, 5, 5, 2), (AHEAD + 1, 2, 5, 2)]
# S' around the tier limits (threads x positions-per-thread of each form) and L around that product
TIER_L = sorted({THREADS // 2 - 1, THREADS // 2, THREADS * POS_LOW // 2 - 1, THREADS * POS_LOW // 2,
                 FULL // 2 - 1, FULL // 2, THREADS * POS_MID // 2 - 1, THREADS * POS_MID // 2,
                 FULL - 1, FULL, FULL + 1, MAX_L})
BOUNDARY += [(L + L // 4 + 8, L, 2, 7) for L in TIER_L]


@pytest.mark.parametrize("T,Lmax,B,C", BOUNDARY)
def test_across_kernel_boundaries(T, Lmax, B, C):
    case, want = generated(T, Lmax, B, C, seed=T * 7919 + Lmax * 31 + C)
    assert THREADS * POS_WIDE >= 2 * MAX_L + 1 and FULL + 1 <= MAX_L
    A, Bt, loglik = check_tables(case, want)
    check_viterbi(case, want["viterbi"])
    if Lmax <= 64 or Lmax in (THREADS // 2, 200, FULL // 2, FULL, MAX_L):
        check_gradient(case, A, Bt, loglik)
    if T >= 2 * Lmax + 30:
        assert np.isfinite(loglik[0])      # the full-width sequence is feasible: the case says something


@pytest.mark.parametrize("T,Lmax,C,integer", [(20, 5, 7, 1), (100, 40, 7, 1), (30, 5, 2, 1), (20, 5, 7, 2),
                                              (100, 40, 7, 2), (400, 150, 7, 1), (500, 200, 7, 1), (1400, 600, 7, 1)])
def test_viterbi_exact_ties(T, Lmax, C, integer):
    case, want = generated(T, Lmax, 5, C, seed=11 + T, integer=integer)
    assert np.array_equal(case[0], np.round(case[0]))
    assert np.isfinite(want["viterbi"][1][0])
    check_viterbi(case, want["viterbi"])


def test_empty_targets_matrix_and_argument_errors():
    rng = np.random.default_rng(3)
    lp = np.log(rng.dirichlet(np.ones(4), (6, 2))).astype(np.float32)
    il = torch.tensor([6, 4])
    loglik, A, Bt, path, score = ops().ctc(dev(lp), torch.zeros((2, 0), dtype=torch.long, device=DEV), il,
                                           torch.tensor([0, 0]), 2, alpha=True, beta=True, viterbi=True)
    want = np.array([lp[:6, 0, 2].astype(np.float64).sum(), lp[:4, 1, 2].astype(np.float64).sum()])
    assert A.shape == (2, 6, 1) and Bt.shape == (2, 6, 1)
    assert np.abs(loglik.cpu().numpy() - want).max() <= 4 * 6 * cn.EPS24 * np.abs(want).max()
    assert path.cpu().numpy().tolist() == [[0] * 6, [0] * 4 + [-1] * 2]
    tg = torch.tensor([[1, 3], [0, 1]], device=DEV)
    for bad in (dict(il=torch.tensor([7, 4])), dict(il=torch.tensor([0, 4])), dict(tl=torch.tensor([3, 1])),
                dict(tl=torch.tensor([2, -1])), dict(blank=4), dict(tg=torch.tensor([[1, 4], [0, 1]], device=DEV))):
        a = dict(tg=tg, il=il, tl=torch.tensor([2, 1]), blank=0)
        a.update(bad)
        with pytest.raises(ValueError):
            ops().ctc(dev(lp), a["tg"], a["il"], a["tl"], a["blank"])
        with pytest.raises(ValueError):
            al().ctc_forward_algorithm(dev(lp), a["tg"], a["il"], a["tl"], a["blank"])


# ------------------------------------------------------------------------------ gradient
@functools.lru_cache(maxsize=None)
def torch_cpu_gradient(key):
    """(logits fp32, targets, il, tl, blank, g_64, g_cpu32): d(sum of nn.CTCLoss) / d logits on the CPU."""
    if isinstance(key, str):
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "ctc_%s.npz" % key)))
        logits, tg, il, tl, blank = fixture_case(g)
    else:
        (logits, tg, il, tl, blank), _ = generated(*key)
    out = []
    for dtype in (torch.float64, torch.float32):
        x = torch.from_numpy(logits).to(dtype).requires_grad_()
        loss = torch.nn.functional.ctc_loss(torch.log_softmax(x, dim=2), torch.from_numpy(np.asarray(tg)),
                                            torch.from_numpy(np.asarray(il)), torch.from_numpy(np.asarray(tl)),
                                            blank=blank, reduction="sum")
        loss.backward()
        out.append(x.grad.numpy().astype(np.float64))
    return (logits, tg, il, tl, blank), out[0], out[1]


# feasible pairs only: torch's loss is +inf otherwise
GRADIENT_CASES = ["basic", "empty", "blank3", "long", (600, 40, 5, 7, 600 * 7919 + 40 * 31 + 7), (90, 64, 5, 7, 5),
                  (600, 200, 5, 7, 600 * 7919 + 200 * 31 + 7)]


@pytest.mark.parametrize("key", GRADIENT_CASES, ids=str)
def test_gradient_at_the_logits_against_torch(key):
    from pytorch_hmm_amd.autograd import CTCLogLik
    case, g64, g32 = torch_cpu_gradient(key)
    logits, tg, il, tl, blank = gpu_args(case)

    def run(entry):
        x = logits.clone().requires_grad_()
        ll = entry(torch.log_softmax(x, dim=2), tg, il, tl, blank)
        assert ll.requires_grad and torch.isfinite(ll).all()
        (-ll.sum()).backward()
        return x.grad
    g1 = run(CTCLogLik.apply)
    g2 = run(al().ctc_forward_algorithm)       # goes through CTCLogLik when log_probs requires grad
    assert torch.equal(g1, g2)
    err_gpu = np.abs(g1.cpu().numpy().astype(np.float64) - g64).max()
    err_cpu = np.abs(g32 - g64).max()
    print("gradient %s: gpu %.3e, torch cpu fp32 %.3e, ratio %.2f" % (key, err_gpu, err_cpu, err_gpu / err_cpu))
    assert err_gpu <= 8 * err_cpu
    for b, n in enumerate(case[2]):
        assert (g1[n:, b] == 0).all()


def test_gradient_true_convention_and_zeros(gold):
    """CTCLogLik returns +sum gamma at log_probs (rows of a live frame sum to 1), not torch's
    exp(lp) - sum gamma; infeasible pairs and frames past input_lengths get exact zeros."""
    from pytorch_hmm_amd.autograd import CTCLogLik
    for name in ("infeasible", "neginf", "one_frame", "basic"):
        g = gold("ctc_" + name)
        case = fixture_case(g)
        lp, tg, il, tl, blank = gpu_args(case)
        x = lp.clone().requires_grad_()
        ll = CTCLogLik.apply(x, tg, il, tl, blank)
        ll[torch.isfinite(ll)].sum().backward()
        grad = x.grad.cpu().numpy()
        assert np.abs(grad - g["grad64"]).max() <= 1e-5
        for b in range(len(case[2])):
            live = np.isfinite(g["loglik64"][b])
            assert (grad[case[2][b]:, b] == 0).all()
            if not live:
                assert (grad[:, b] == 0).all()
            else:
                assert np.abs(grad[:case[2][b], b].sum(1) - 1).max() <= 1e-5
