"""GPU: the banded chain wave across the edges of its 16-step blocks (recur.h band_chain).  The
wave runs block 0 (which has no step 0) and a partial last block rolled, and every whole block in
between in one unrolled loop that holds nothing else: the loop's bases (emission slot of the 3-slot
staging ring, row / normaliser slot of the 64-row rings) advance by increments with a wrap, the
wave meets its helpers' barrier EA steps before the block's end, and behind it reads the first
emission rows of the NEXT block, so that no block starts with an exposed read.  A base that wraps a
block early or late, a row taken from the slot the helpers are staging, a barrier on the wrong side
of a read, or a normaliser stored to another block's slot gives a wrong row in some step, and every
later row with it.  The file tests the contract, not the form: it passes on the loop it replaced.

Matrices (tests/test_gpu_emis_ahead.py's, through tests/test_gpu_chain_reduce.py's `model`, which
builds them at any N): left-to-right 0.7, its transpose, tri-band, ergodic, per-row floors (alpha's
second reduction), an LDS-window chain.  N = 128 and 100 (NP = 128, padded states at 100) with every
matrix; N = 64, 40 (NP = 64: one state a lane) and 200 (NP = 256: four, LDS windows throughout) with
the left-to-right, the per-row-floor and the LDS-window one.  B = 2.

T, every place the loop can go wrong:
  1, 2, 14 .. 18           the first block alone and the first edge, at each read-ahead position
  31 .. 34, 47 .. 50,      two to four blocks: the helper loop's three phases, the first whole block
  63 .. 66                 with and without a whole block behind it, the first wrap of the 3-slot ring
  79 .. 82, 97, 113, 129   the wrap of the 64-row row / normaliser / psi rings; the barrier in
                           every phase of the rings
  209, 225, 241, 257       the every-fourth-block publish, the late-block publishes and the end-row
                           switch at T = 256, each with a partial last block

Emissions: logs uniform in (-60, 0), drawn independently for every step and state, so a row of
another step or slot cannot pass.

Viterbi: states, trellis and final score bit-identical to the C oracle; with log leaders and
followers, without followers, without a plan; log input (OBS_LOG) and probability input (OBS_PROB:
exp of the logs, the oracle fed log(x + 1e-8) formed as the kernel forms it).
Forward-backward (log input): against the fp64 oracle O.c_fb64 at tests/test_gpu_band.py's
tolerances, posterior atol 2e-5 and log-likelihood rtol 2e-6, on the plain, the no-follower and the
pair-kernel path; forward, backward and log-likelihood the same bits on the two-kernel paths and
forward and backward on the pair kernel, as tests/test_gpu_emis_ahead.py asserts them (the three
paths share the chain wave)."""
import functools

import numpy as np
import pytest
import torch

from oracle import hmm_oracle as O
from test_gpu_chain_reduce import model
from test_gpu_emis_ahead import KINDS, ops, t

pytestmark = pytest.mark.gpu

B = 2
TS_FIRST = (1, 2, 14, 15, 16, 17, 18)
TS = TS_FIRST + (31, 32, 33, 34, 47, 48, 49, 50, 63, 64, 65, 66,
                 79, 80, 81, 82, 97, 113, 129,
                 209, 225, 241, 257)
SUBSET = ("l2r", "per_row", "lds")
CASES = [(k, n) for n in (128, 100) for k in KINDS] + [(k, n) for n in (64, 40, 200) for k in SUBSET]


@functools.lru_cache(maxsize=None)
def log_emissions(kind, N, T):
    rng = np.random.default_rng([31, KINDS.index(kind), N, T])
    return (-60.0 * rng.random((B, T, N))).astype(np.float32)  # (shared: never written)


def _ts(first):
    return TS_FIRST if first else tuple(T for T in TS if T not in TS_FIRST)


@pytest.mark.parametrize("first", (True, False), ids=("first_block", "later_blocks"))
@pytest.mark.parametrize("kind,N", CASES)
def test_block_edge_viterbi_bitexact(kind, N, first):
    o = ops()
    lP, lp0 = model(kind, N)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for T in _ts(first):
        lo = log_emissions(kind, N, T)
        x = np.exp(lo)  # float32: the probability input
        lo_x = np.log((x + np.float32(1e-8)).astype(np.float64)).astype(np.float32)
        for mode, inp, lo_ref in ((o.OBS_LOG, lo, lo), (o.OBS_PROB, x, lo_x)):
            cs, cd, _ = O.c_viterbi(lo_ref, lP, lp0)
            for label, p, follow in (("followers", plan, None), ("no followers", plan, False), ("no plan", None, None)):
                states, delta, final = o.viterbi(t(inp), t(lP), t(lp0), mode, p, follow)
                where = (T, "OBS_LOG" if mode == o.OBS_LOG else "OBS_PROB", label)
                assert np.array_equal(delta.cpu().numpy(), cd), where
                assert np.array_equal(states.cpu().numpy(), cs), where
                assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), where


@pytest.mark.parametrize("first", (True, False), ids=("first_block", "later_blocks"))
@pytest.mark.parametrize("kind,N", CASES)
def test_block_edge_fb_vs_fp64(kind, N, first):
    o = ops()
    lP, lp0 = model(kind, N)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for T in _ts(first):
        lo = log_emissions(kind, N, T)
        _, _, post64, ll64 = O.c_fb64(lo, lP, lp0)
        args = (t(lo), t(lP), t(lp0), o.OBS_LOG, 7, plan)
        on = o.forward_backward(*args, pair=False)
        off = o.forward_backward(*args, pair=False, follow=False)
        pair = o.forward_backward(*args, pair=True)
        for label, out in (("followers", on), ("no followers", off), ("pair", pair)):
            post, loglik = out[0].cpu().numpy(), out[3].cpu().numpy()
            np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0, err_msg=f"T={T} {label} posterior")
            np.testing.assert_allclose(loglik, ll64, rtol=2e-6, err_msg=f"T={T} {label} loglik")
        for k, name in ((1, "forward"), (2, "backward")):
            assert torch.equal(on[k], off[k]), (T, name)
            assert torch.equal(pair[k], on[k]), (T, "pair " + name)
        assert torch.equal(on[3], off[3]), (T, "loglik")
