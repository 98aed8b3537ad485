"""GPU: the banded chain step (recur.h band_chain) as it stands since its wave reductions became
plain DPP levels: beta and Viterbi with their independent work pinned inside the reduction
(wave_red_fill), alpha with the plain reduction, the forward-backward step sums in their pinned
fused form (prod_sum) -- on every form of the step: the Toeplitz-register and the LDS-window
mode, NB = 1, 2, 4 states per lane (NP = 64, 128, 256), one floor for all rows and a floor per
row (alpha: a second, weighted reduction), and every block shape of the time loop --
partial-only blocks (T = 1, 2), one whole unrolled block (16), whole plus partial (17, 33), two
whole blocks (32), and the row ring's wrap slot (81: rows 63 / 64).

Contracts (tests/test_gpu_band.py): Viterbi states and trellis bit-identical to the C oracle;
forward-backward against the fp64 oracle with posterior atol 2e-5, log-likelihood rtol 2e-6,
forward / backward rtol 1e-4 where the oracle's value exceeds 1e-30.  The reference's own fp32
recursion (oracle.forward_backward) holds the same bounds against the fp64 oracle on these
inputs (checked on the CPU: worst posterior error 4.8e-6 of 2e-5, forward / backward 6.4e-5 of
1e-4, the log-sum-exp of its last log-alpha row 7.8e-7 of 2e-6)."""
import functools

import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

B = 3
TS = (1, 2, 16, 17, 32, 33, 81)
NS = (64, 100, 128, 200)            # NB = 1, 2 with padding, 2, 4 with padding
KINDS = ("l2r", "tri", "ragged", "per_row")
# the chain each kind selects for (Viterbi and alpha, beta) at NP <= 128 / NP = 256
CHAINS = {"l2r": (("tw2 d0=-1", "tw2 d0=0"), ("w2", "w2")),
          "tri": (("tw3 d0=-1", "tw3 d0=-1"), ("w4", "w4")),
          "ragged": (("w8", "w8"), ("w8", "w8")),
          "per_row": (("tw3 d0=-1", "tw3 d0=-1"), ("w4", "w4"))}


def t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def ops():
    from pytorch_hmm_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def model(kind, N):
    """(log_P, log_p0) float32 arrays of the kind's table at N states, after the guard that it
    selects the chains the case is meant for"""
    rng = np.random.default_rng([KINDS.index(kind), N])
    if kind == "l2r":
        lP, lp0 = (x.numpy() for x in O.hmm_params(O.left_to_right_matrix(N, 0.7)))
    else:
        name = "ragged" if kind == "ragged" else M.TRI
        lP = M.band_case(name, N, "per_row" if kind == "per_row" else "uniform", rng)
        p = rng.random(N) + 0.1
        lp0 = np.log(p / p.sum()).astype(np.float32)
    c = M.classify(lP)
    assert (c["col_chain"], c["row_chain"]) == CHAINS[kind][N > 128], (kind, N, c)
    assert c["banded"] and c["uniform_floor"] == int(kind != "per_row"), (kind, N, c)
    return np.ascontiguousarray(lP, np.float32), np.ascontiguousarray(lp0, np.float32)


def inputs(kind, N, T):
    rng = np.random.default_rng([KINDS.index(kind), N, T])
    return rng.random((B, T, N), dtype=np.float32)


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_filled_viterbi_bitexact(kind, N, T):
    o = ops()
    lP, lp0 = model(kind, N)
    lo = np.log(inputs(kind, N, T) + np.float32(1e-8)).astype(np.float32)
    cs, cd, _ = O.c_viterbi(lo, lP, lp0)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for label, p, follow in (("no plan", None, None), ("plan", plan, None), ("plan, follow=False", plan, False)):
        states, delta, final = o.viterbi(t(lo), t(lP), t(lp0), o.OBS_LOG, p, follow)
        assert np.array_equal(delta.cpu().numpy(), cd), label
        assert np.array_equal(states.cpu().numpy(), cs), label
        assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), label


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_filled_fb_vs_fp64(kind, N, T):
    o = ops()
    lP, lp0 = model(kind, N)
    obs = inputs(kind, N, T)
    la, lb, post64, ll64 = O.c_fb64(np.log(obs + np.float32(1e-8)), lP, lp0)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    runs = [("no plan", None, None), ("plan + followers", plan, False)] + ([("pair", plan, True)] if N <= 128 else [])
    for label, p, pair in runs:
        out = o.forward_backward(t(obs), t(lP), t(lp0), o.OBS_PROB, 7, p, pair=pair)
        post, fwd, bwd, loglik, _ = (x.cpu().numpy() for x in out)
        np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0, err_msg=label + " posterior")
        np.testing.assert_allclose(loglik, ll64, rtol=2e-6, err_msg=label + " loglik")
        for got, lg, what in ((fwd, la, " forward"), (bwd, lb, " backward")):
            want = np.exp(lg)
            big = want > 1e-30
            np.testing.assert_allclose(got[big], want[big], rtol=1e-4, err_msg=label + what)
