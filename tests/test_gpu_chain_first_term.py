"""GPU: the banded forward-backward chain step (recur.h band_chain) with the first window term
written as a product -- a lane shift in it folds into one v_mul_f32_dpp -- and beta's unfoldable
lane shift issued as a filler of its own inside the wave reduction.  Every form the change
reaches, at the smallest shapes that reach it: B = 2; N = 100 (padded to 128) and 128; T = 1, 2,
15 (rolled partial blocks only), 16 (one unrolled block, its step 0), 17, 33 and 48 (whole
blocks plus a partial one, three whole blocks); and the matrices
  l2r      left-to-right 0.7: alpha window -1..0 (the shift is the FIRST term of state j = 0),
           beta window 0..+1 (the shift is the LAST term of state j = 1);
  l2r_T    its transpose, renormalised: the mirrored windows, so each chain takes the other's;
  tri      offsets -1..+1: a three-term Toeplitz window, shifts in its first and last terms;
  per_row  the same with a floor per row: alpha keeps its second, weighted reduction and its
           window sum starts from it, so the product form must not apply there;
  lds      offsets -1..+2: too wide for the register windows, the LDS-window chain (w4).
Emissions are 60 * softmax(randn): no row underflows at these lengths, so every forward and
backward value is compared.

Contracts (tests/test_gpu_band.py, tests/test_gpu_chain_fill.py): Viterbi states, trellis and
final score bit-identical to the C oracle; forward-backward against the fp64 oracle with
posterior atol 2e-5, log-likelihood rtol 2e-6, forward / backward rtol 1e-4 where the oracle's
value exceeds 1e-30.

The zero case pins the sign argument of the product form: fma(v, w, +0) and v * w are the same
bits only while no product is -0, i.e. while chain values and window weights are non-negative.
Log-emissions with -inf entries (exact-zero emissions) on the left-to-right table (whose edge
states have zero window weights: the shifted-in 0 of the wave edge times a weight 0): every
output the oracle has as an exact zero must be a zero here, and no output may carry a sign
bit."""
import functools

import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 2
TS = (1, 2, 15, 16, 17, 33, 48)
NS = (100, 128)
KINDS = ("l2r", "l2r_T", "tri", "per_row", "lds")
# (Viterbi and alpha, beta) chains each kind is built to select at NP = 128
CHAINS = {"l2r": ("tw2 d0=-1", "tw2 d0=0"), "l2r_T": ("tw2 d0=0", "tw2 d0=-1"),
          "tri": ("tw3 d0=-1", "tw3 d0=-1"), "per_row": ("tw3 d0=-1", "tw3 d0=-1"), "lds": ("w4", "w4")}


def t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def ops():
    from pytorch_hmm_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def model(kind, N):
    rng = np.random.default_rng([KINDS.index(kind), N])
    if kind in ("l2r", "l2r_T"):
        P = O.left_to_right_matrix(N, 0.7)
        lP, lp0 = (x.numpy() for x in O.hmm_params(P.T.contiguous() if kind == "l2r_T" else P))
    else:
        name = "gen{-1..2}" if kind == "lds" else M.TRI
        lP = M.band_case(name, N, "per_row" if kind == "per_row" else "uniform", rng)
        p = rng.random(N) + 0.1
        lp0 = np.log(p / p.sum()).astype(np.float32)
    c = M.classify(lP)
    assert (c["col_chain"], c["row_chain"]) == CHAINS[kind], (kind, N, c)
    assert c["banded"] and c["uniform_floor"] == int(kind != "per_row"), (kind, N, c)
    return np.ascontiguousarray(lP, np.float32), np.ascontiguousarray(lp0, np.float32)


@functools.lru_cache(maxsize=None)
def emissions(kind, N, T):
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + 10 * T + N)
    return (60.0 * torch.softmax(torch.randn(B, T, N, generator=g), -1)).numpy()  # (shared: never written)


@functools.lru_cache(maxsize=None)
def fb_reference(kind, N, T):
    lP, lp0 = model(kind, N)
    return O.c_fb64(np.log(emissions(kind, N, T) + np.float32(1e-8)), lP, lp0)


def check_fb(out, ref, label):
    la, lb, post64, ll64 = ref
    post, fwd, bwd, loglik = (x.cpu().numpy() for x in out[:4])
    np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0, err_msg=label + " posterior")
    np.testing.assert_allclose(loglik, ll64, rtol=2e-6, err_msg=label + " loglik")
    for got, lg, what in ((fwd, la, " forward"), (bwd, lb, " backward")):
        with np.errstate(under="ignore"):
            want = np.exp(lg)
        big = want > 1e-30
        np.testing.assert_allclose(got[big], want[big], rtol=1e-4, err_msg=label + what)
    return post, fwd, bwd


def fb_runs(o, plan):
    return (("no plan", None, None), ("plan + followers", plan, False), ("pair", plan, True))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_first_term_fb_vs_fp64(kind, N, T):
    o = ops()
    lP, lp0 = model(kind, N)
    obs = emissions(kind, N, T)
    ref = fb_reference(kind, N, T)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for label, p, pair in fb_runs(o, plan):
        check_fb(o.forward_backward(t(obs), t(lP), t(lp0), o.OBS_PROB, 7, p, pair=pair), ref, label)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_first_term_viterbi_bitexact(kind, N, T):
    o = ops()
    lP, lp0 = model(kind, N)
    lo = np.log(emissions(kind, N, T) + np.float32(1e-8)).astype(np.float32)
    cs, cd, _ = O.c_viterbi(lo, lP, lp0)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for label, p, follow in (("no plan", None, None), ("plan", plan, None), ("plan, follow=False", plan, False)):
        states, delta, final = o.viterbi(t(lo), t(lP), t(lp0), o.OBS_LOG, p, follow)
        assert np.array_equal(delta.cpu().numpy(), cd), label
        assert np.array_equal(states.cpu().numpy(), cs), label
        assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), label


@pytest.mark.parametrize("N", NS)
def test_viterbi_with_log_leaders_bitexact(N):
    """OBS_PROB with a plan: the log leaders run, and the staging helpers poll their count every
    block and read it three blocks on (rec_band: the poll is decoded where it is read).  T = 160
    is ten blocks, so blocks 4 .. 9 may come from the leaders' rows or from the raw emissions,
    whichever the poll says: the same bits either way."""
    o = ops()
    lP, lp0 = model("l2r", N)
    g = torch.Generator().manual_seed(N)
    x = torch.softmax(torch.randn(B, 160, N, generator=g), -1).numpy()
    lo = np.log((x + np.float32(1e-8)).astype(np.float64)).astype(np.float32)  # correctly rounded, as logcr.h
    cs, cd, _ = O.c_viterbi(lo, lP, lp0)
    plan = o.make_plan(t(lP))
    for follow in (None, False):
        states, delta, final = o.viterbi(t(x), t(lP), t(lp0), o.OBS_PROB, plan, follow)
        assert np.array_equal(delta.cpu().numpy(), cd), follow
        assert np.array_equal(states.cpu().numpy(), cs), follow
        assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), follow


@pytest.mark.parametrize("T", (17, 48))
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ("l2r", "l2r_T", "tri"))
def test_first_term_exact_zeros(kind, N, T):
    """exact-zero emissions (log-emissions of -inf in about a third of the entries, never a whole
    row) and the zero window weights of the tables' edge states"""
    o = ops()
    lP, lp0 = model(kind, N)
    rng = np.random.default_rng([7, KINDS.index(kind), N, T])
    lo = np.log(emissions(kind, N, T)).astype(np.float32)
    dead = rng.random((B, T, N)) < 0.35
    dead[..., N // 2] = False
    lo[dead] = -np.inf
    ref = O.c_fb64(lo, lP, lp0)
    assert np.isfinite(ref[3]).all() and (ref[2][dead] == 0).all()
    plan = o.make_plan(t(lP))
    for label, p, pair in fb_runs(o, plan):
        post, fwd, bwd = check_fb(o.forward_backward(t(lo), t(lP), t(lp0), o.OBS_LOG, 7, p, pair=pair), ref, label)
        for got, lg, what in ((post, None, "posterior"), (fwd, ref[0], "forward"), (bwd, ref[1], "backward")):
            assert np.isfinite(got).all(), (label, what)
            assert not np.signbit(got).any(), (label, what)
            zero = ref[2] == 0 if lg is None else np.isneginf(lg)
            assert (got[zero] == 0).all(), (label, what)
    # the Viterbi chain reads the same table and emissions: bit-exact with -inf scores
    cs, cd, _ = O.c_viterbi(lo, lP, lp0)
    states, delta, final = o.viterbi(t(lo), t(lP), t(lp0), o.OBS_LOG, plan, None)
    assert np.array_equal(delta.cpu().numpy(), cd)
    assert np.array_equal(states.cpu().numpy(), cs)
    assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1))
