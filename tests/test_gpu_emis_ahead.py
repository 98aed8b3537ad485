"""GPU: the banded chain wave's emission read (recur.h band_chain, `emis_ahead`).  Inside an
unrolled 16-step block the wave reads a step's staged emission row EA steps ahead into a
rotation of EA register sets; the rolled partial blocks read one step ahead.  A row taken one
step off, a slot of the rotation consumed out of turn, or a read across a block's edge gives a
wrong emission in some step.

Shapes: B = 2; N = 128 and 100 (padded states); T = 1, 2, 3 (rolled only), 15, 16, 17, 18 (the
first whole block's edge: block 0 is rolled because step 0 is row 0, T = 17 ends on the first
step of block 1), 31 .. 34 (block 1 is the first unrolled block; 33 and 34 leave one and two
rolled steps behind it), 47 .. 50 (two unrolled blocks and the same tails), 65 (the 64-row ring
wraps).  These put every slot of the rotation against the block edge and the partial blocks.
Matrices (the chain each selects at NP = 128 is asserted):
  l2r      left-to-right 0.7 (alpha -1..0, beta 0..+1), l2r_T its transpose (the mirrored ones),
  tri      offsets -1..+1, per_row the same with a floor per row (alpha's second reduction),
  ergodic  the factory's ergodic matrix: a width-1 window,
  lds      offsets -1..+2: the LDS-window chain (w4).
Emissions are 60 * softmax(randn), drawn independently for every step, so the row of a
neighbouring step cannot pass: forward-backward runs with them as probabilities, Viterbi with
their logs.

Contracts, as tests/test_gpu_chain_first_term.py states them: forward-backward against the fp64
oracle with posterior atol 2e-5, log-likelihood rtol 2e-6, forward / backward rtol 1e-4 where
the oracle's value exceeds 1e-30 (no row underflows at these lengths); Viterbi states, trellis
and final score bit-identical to the C oracle.  Paths: with the followers, without them
(follow=False) and through the pair kernel.

What the three paths share is the chain wave, so what it produces -- the forward and backward
outputs, and with them the log-likelihood of the two-kernel paths -- is the same bits on all
three: a wrong emission in any step of either chain shows there.  The values each path forms
from the rows in its own way are held to the contracts the existing tests state for them:
with and without followers (tests/test_gpu_follow.py) the posterior is identical at N = 128
and within atol 1e-6 at the padded N = 100; the reference's compute_likelihood value is a
logsumexp the two paths reduce in different orders, rtol 2e-6; the pair kernel
(tests/test_gpu_fbpair.py) forms the posterior as x*y / sum(x*y) where the others max-normalise
first and accumulates the log-scales in its own scan: rtol 2e-6 (posterior atol 1e-12) for
posterior, log-likelihood and compute_likelihood value."""
import functools

import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 2
TS = (1, 2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 47, 48, 49, 50, 65)
NS = (128, 100)
KINDS = ("l2r", "l2r_T", "tri", "ergodic", "per_row", "lds")
# (Viterbi and alpha, beta) chains each kind is built to select at NP = 128
CHAINS = {"l2r": ("tw2 d0=-1", "tw2 d0=0"), "l2r_T": ("tw2 d0=0", "tw2 d0=-1"), "tri": ("tw3 d0=-1", "tw3 d0=-1"),
          "ergodic": ("tw1 d0=0", "tw1 d0=0"), "per_row": ("tw3 d0=-1", "tw3 d0=-1"), "lds": ("w4", "w4")}


def t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def ops():
    from pytorch_hmm_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def model(kind, N):
    rng = np.random.default_rng([11, KINDS.index(kind), N])
    if kind in ("l2r", "l2r_T"):
        P = O.left_to_right_matrix(N, 0.7)
        lP, lp0 = (x.numpy() for x in O.hmm_params(P.T.contiguous() if kind == "l2r_T" else P))
    elif kind == "ergodic":
        lP, lp0 = (x.numpy() for x in O.hmm_params(O.transition_matrix(N, "ergodic")))
    else:
        name = "gen{-1..2}" if kind == "lds" else M.TRI
        lP = M.band_case(name, N, "per_row" if kind == "per_row" else "uniform", rng)
        p = rng.random(N) + 0.1
        lp0 = np.log(p / p.sum()).astype(np.float32)
    c = M.classify(lP)
    assert c["banded"] and (c["col_chain"], c["row_chain"]) == CHAINS[kind], (kind, N, c)
    if kind != "ergodic":  # (its rows are renormalised by fp32 sums that may differ in the last bit)
        assert c["uniform_floor"] == int(kind != "per_row"), (kind, N, c)
    return np.ascontiguousarray(lP, np.float32), np.ascontiguousarray(lp0, np.float32)


@functools.lru_cache(maxsize=None)
def emissions(kind, N, T):
    g = torch.Generator().manual_seed(77000 + 1000 * KINDS.index(kind) + 10 * T + N)
    return (60.0 * torch.softmax(torch.randn(B, T, N, generator=g), -1)).numpy()  # (shared: never written)


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


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_emis_ahead_fb_vs_fp64(kind, N, T):
    o = ops()
    lP, lp0 = model(kind, N)
    obs = emissions(kind, N, T)
    ref = O.c_fb64(np.log(obs + np.float32(1e-8)), lP, lp0)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    args = (t(obs), t(lP), t(lp0), o.OBS_PROB, 7, plan)
    on = o.forward_backward(*args, pair=False)
    off = o.forward_backward(*args, pair=False, follow=False)
    pair = o.forward_backward(*args, pair=True)
    for label, out in (("followers", on), ("no followers", off), ("pair", pair)):
        check_fb(out, ref, label)
    npy = lambda x: x.cpu().numpy()
    for k, name in ((1, "forward"), (2, "backward")):
        assert torch.equal(on[k], off[k]), name
        assert torch.equal(pair[k], on[k]), "pair " + name
    assert torch.equal(on[3], off[3]), "loglik"
    if N == 128:
        assert torch.equal(on[0], off[0]), "posterior"
    else:
        np.testing.assert_allclose(npy(on[0]), npy(off[0]), atol=1e-6, rtol=0, err_msg="posterior")
    np.testing.assert_allclose(npy(on[4]), npy(off[4]), rtol=2e-6, err_msg="lik_ref")
    np.testing.assert_allclose(npy(pair[0]), npy(on[0]), rtol=2e-6, atol=1e-12, err_msg="pair posterior")
    for k, name in ((3, "loglik"), (4, "lik_ref")):
        np.testing.assert_allclose(npy(pair[k]), npy(on[k]), rtol=2e-6, err_msg="pair " + name)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_emis_ahead_viterbi_bitexact(kind, N, T):
    o = ops()
    lP, lp0 = model(kind, N)
    lo = np.log(emissions(kind, N, T) + np.float32(1e-8)).astype(np.float32)
    cs, cd, _ = O.c_viterbi(lo, lP, lp0)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for label, p, follow in (("followers", plan, None), ("no followers", plan, False), ("no plan", None, None)):
        states, delta, final = o.viterbi(t(lo), t(lP), t(lp0), o.OBS_LOG, p, follow)
        assert np.array_equal(delta.cpu().numpy(), cd), label
        assert np.array_equal(states.cpu().numpy(), cs), label
        assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), label
