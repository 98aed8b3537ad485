"""GPU: the forward-backward end rows (recur.h rec_band, post.h kEndBlocks = 2).  With a banded
plan and posterior followers, each chain's own workgroup forms the posterior of the rows of its
last two 16-step blocks once it has ended, from its LDS ring and the partner chain's published
rows; the followers keep the interior and whatever the chains' left-over words name.  The
arithmetic is the followers' own function, so the contract is bits: end rows on == end rows off
== every odd block left over, for the posterior, forward and backward alike.

Shapes: the host switches the end rows on at T >= 256 (255, 256, 257: sixteen whole blocks, and a
seventeenth of one row, so the end rows are 32 and 17); 575 / 576 / 577, 592, 609 and 700 mix
whole and partial last blocks with even and odd block counts (which of the two end blocks the
odd-blocks mode leaves over); 17 and 33 show the short form unchanged.  N = 64, 100, 128, 200: one,
two (padded and full) and four (padded) states per lane, and 4, 9, 9 and 12 helpers sharing the
rows.  Against the fp64 oracle the bounds are those of tests/test_gpu_chain_fill.py: posterior
atol 2e-5, log-likelihood rtol 2e-6."""
import functools

import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
KINDS = ("l2r", "tri", "ragged", "per_row")  # (the indices seed the tables, as in test_gpu_chain_fill)


def t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def ops():
    from pytorch_hmm_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def model(kind, N):
    """(log_P, log_p0) float32 arrays: tests/test_gpu_chain_fill.py's tables"""
    rng = np.random.default_rng([KINDS.index(kind), N])
    if kind == "l2r":
        lP, lp0 = (x.numpy() for x in O.hmm_params(O.left_to_right_matrix(N, 0.7)))
    else:
        lP = M.band_case(M.TRI, N, "per_row" if kind == "per_row" else "uniform", rng)
        p = rng.random(N) + 0.1
        lp0 = np.log(p / p.sum()).astype(np.float32)
    assert M.classify(lP)["banded"], (kind, N)
    return np.ascontiguousarray(lP, np.float32), np.ascontiguousarray(lp0, np.float32)


TS = (17, 33, 255, 256, 257, 575, 576, 577, 592, 609, 700)
NS = (64, 100, 128, 200)
ENDS_KINDS = ("l2r", "per_row")


def inputs(kind, N, T, salt=0):
    rng = np.random.default_rng([KINDS.index(kind), N, T, 9, salt])
    return rng.random((B, T, N), dtype=np.float32)


@functools.lru_cache(maxsize=None)
def fp64(kind, N, T):
    lP, lp0 = model(kind, N)
    _, _, post64, ll64 = O.c_fb64(np.log(inputs(kind, N, T) + np.float32(1e-8)), lP, lp0)
    return post64, ll64


def run(o, obs, lP, lp0, plan, extra):
    return o.forward_backward(obs, lP, lp0, o.OBS_PROB, 7 | extra, plan, pair=False)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ENDS_KINDS)
def test_end_rows_same_bits(kind, N, T):
    o = ops()
    lP, lp0 = (t(x) for x in model(kind, N))
    obs = t(inputs(kind, N, T))
    plan = o.make_plan(lP)
    assert plan._hmm355_banded
    on = run(o, obs, lP, lp0, plan, 0)
    off = run(o, obs, lP, lp0, plan, o.FB_NO_END_ROWS)
    odd = run(o, obs, lP, lp0, plan, o.FB_END_ROWS_ODD_LEFT)
    assert torch.equal(on[0], off[0]), "posterior, end rows on vs off"
    assert torch.equal(odd[0], off[0]), "posterior, odd blocks left over vs off"
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2]), "forward / backward on vs off"
    assert torch.equal(on[3], off[3]) and torch.equal(on[4], off[4]), "likelihoods on vs off"
    post64, ll64 = fp64(kind, N, T)
    for label, out in (("on", on), ("odd left", odd)):
        np.testing.assert_allclose(out[0].cpu().numpy(), post64, atol=2e-5, rtol=0, err_msg=label + " posterior")
        np.testing.assert_allclose(out[3].cpu().numpy(), ll64, rtol=2e-6, err_msg=label + " loglik")


@pytest.mark.parametrize("N", (100, 128))
def test_three_calls_in_a_row(N):
    """three calls back to back on one stream, no synchronisation between them: a count, token
    or left-over word of the call before would show in the next one's posterior"""
    o = ops()
    kind, T = "l2r", 609
    lP, lp0 = (t(x) for x in model(kind, N))
    plan = o.make_plan(lP)
    obs = [t(inputs(kind, N, T, salt)) for salt in (1, 2, 3)]
    want = [run(o, x, lP, lp0, plan, o.FB_NO_END_ROWS)[0].clone() for x in obs]
    torch.cuda.synchronize()
    got = [run(o, x, lP, lp0, plan, extra)[0] for x, extra in zip(obs, (o.FB_END_ROWS_ODD_LEFT, 0, o.FB_END_ROWS_ODD_LEFT))]
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(got[k], want[k]), f"call {k}"
