"""GPU: the banded chain step's wave reduction (recur.h wave_red_level / wave_red_fill, every form
of HMM355_RED_FORM).  The step reduces one value a lane -- the maximum or the sum of the lane's
states -- over the 64 lanes of the chain wave: in-row levels (quad_perm and row_ror pairs, or
triples of row_shr of one register), then row_bcast:15, row_bcast:31 and v_readlane 63.  A level
that misses a lane, reads one twice, or reads a register before it is settled changes the floor
term of the next row, and with it every later row.  The file tests the contract, not the form.

Matrices (tests/test_gpu_emis_ahead.py's, whose helpers are imported): left-to-right 0.7, its
transpose, tri-band, ergodic, per-row floors (alpha's second reduction), an LDS-window chain.
N = 128 and 100 (NP = 128: two states a lane), 64 and 40 (NP = 64: one), 200 (NP = 256: four,
LDS windows throughout).  T = 1, 2 (the rolled first block), 17 (ends on the first step of the
second block), 33 (one whole unrolled block and a rolled step behind it).  B = N.

Emissions, as logs:
  extreme  in row t of sequence b: 0 at state (b + 7t) mod N and -50 + log1p(noise), noise up to
           1e-3, elsewhere.  Over the B = N sequences every state -- both states of every lane,
           every lane of every row of 16 -- holds the row's maximum, or all but e^-50 of its sum,
           in every row t;
  random   uniform in (-60, 0).

Viterbi: states, trellis and final score bit-identical to the C oracle; with log leaders and
followers, without followers, without a plan; log input (OBS_LOG) and probability input
(OBS_PROB: exp of the logs, the oracle fed log(x + 1e-8) formed as the kernel forms it, the sum in
fp32 and the log in fp64 rounded once).
Forward-backward (log input, so that e^-50 stays e^-50): against the fp64 oracle O.c_fb64 at
tests/test_gpu_band.py's tolerances, posterior atol 2e-5 and log-likelihood rtol 2e-6, on the
plain, the no-follower and the pair-kernel path; forward, backward and log-likelihood the same
bits on the two-kernel paths and forward and backward on the pair kernel, as
tests/test_gpu_emis_ahead.py asserts them (the three paths share the chain wave).

The oracles run once per case, the sequences split over a few threads (they are independent)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O
from test_gpu_emis_ahead import CHAINS, KINDS, ops, t

pytestmark = pytest.mark.gpu

NS = (128, 100, 64, 40, 200)
TS = (1, 2, 17, 33)
EMIS = ("extreme", "random")
_POOL = ThreadPoolExecutor(max_workers=8)


def model(kind, N):
    """tests/test_gpu_emis_ahead.py's matrices at any N (at NP = 256 every chain is an LDS-window one)"""
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
    assert c["banded"], (kind, N, c)
    if M.pad_states(N) <= 128:
        assert (c["col_chain"], c["row_chain"]) == CHAINS[kind], (kind, N, c)
    else:
        assert c["col_chain"][0] == "w" and c["row_chain"][0] == "w", (kind, N, c)
    if kind != "ergodic":
        assert c["uniform_floor"] == int(kind != "per_row"), (kind, N, c)
    return np.ascontiguousarray(lP, np.float32), np.ascontiguousarray(lp0, np.float32)


def log_emissions(emis, kind, N, T):
    rng = np.random.default_rng([29, EMIS.index(emis), KINDS.index(kind), N, T])
    if emis == "random":
        return (-60.0 * rng.random((N, T, N))).astype(np.float32)
    lo = (-50.0 + np.log1p(1e-3 * rng.random((N, T, N)))).astype(np.float32)
    b, q = np.meshgrid(np.arange(N), np.arange(T), indexing="ij")
    lo[b, q, (b + 7 * q) % N] = 0.0
    return lo


def by_sequences(fn, lo, *rest):
    """fn(lo, *rest) with the batch split over the pool: the tuple of its outputs, joined"""
    O.c_oracle()  # (built once, outside the threads)
    parts = [p for p in np.array_split(lo, 8) if len(p)]
    outs = list(_POOL.map(lambda p: fn(np.ascontiguousarray(p), *rest), parts))
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(len(outs[0])))


@pytest.mark.parametrize("emis", EMIS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_reduce_viterbi_bitexact(kind, N, emis):
    o = ops()
    lP, lp0 = model(kind, N)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for T in TS:
        lo = log_emissions(emis, kind, N, T)
        x = np.exp(lo)  # float32: the probability input
        lo_x = np.log((x + np.float32(1e-8)).astype(np.float64)).astype(np.float32)
        for mode, inp, lo_ref in ((o.OBS_LOG, lo, lo), (o.OBS_PROB, x, lo_x)):
            cs, cd, _ = by_sequences(O.c_viterbi, lo_ref, lP, lp0)
            for label, p, follow in (("followers", plan, None), ("no followers", plan, False), ("no plan", None, None)):
                states, delta, final = o.viterbi(t(inp), t(lP), t(lp0), mode, p, follow)
                where = (T, "OBS_LOG" if mode == o.OBS_LOG else "OBS_PROB", label)
                assert np.array_equal(delta.cpu().numpy(), cd), where
                assert np.array_equal(states.cpu().numpy(), cs), where
                assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), where


@pytest.mark.parametrize("emis", EMIS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_chain_reduce_fb_vs_fp64(kind, N, emis):
    o = ops()
    lP, lp0 = model(kind, N)
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    for T in TS:
        lo = log_emissions(emis, kind, N, T)
        _, _, post64, ll64 = by_sequences(O.c_fb64, lo, lP, lp0)
        args = (t(lo), t(lP), t(lp0), o.OBS_LOG, 7, plan)
        on = o.forward_backward(*args, pair=False)
        off = o.forward_backward(*args, pair=False, follow=False)
        pair = o.forward_backward(*args, pair=True)
        for label, out in (("followers", on), ("no followers", off), ("pair", pair)):
            post, loglik = out[0].cpu().numpy(), out[3].cpu().numpy()
            print(f"{kind} N={N} {emis} T={T} {label}: posterior max|d| {np.abs(post - post64).max():.3e} "
                  f"loglik max rel {np.abs(loglik / ll64 - 1).max():.3e}")
            np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0, err_msg=f"T={T} {label} posterior")
            np.testing.assert_allclose(loglik, ll64, rtol=2e-6, err_msg=f"T={T} {label} loglik")
        for k, name in ((1, "forward"), (2, "backward")):
            assert torch.equal(on[k], off[k]), (T, name)
            assert torch.equal(pair[k], on[k]), (T, "pair " + name)
        assert torch.equal(on[3], off[3]), (T, "loglik")
