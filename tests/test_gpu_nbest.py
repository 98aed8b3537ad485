"""GPU: N-best Viterbi (csrc/nbest.hip, hmm355_viterbi_nbest_f32; ops.viterbi_nbest;
HMMPyTorch.viterbi_nbest; the layers' nbest_alignment).

The contract is exact (include/hmm355.h), so every comparison here is bit for bit:
  * paths, scores and count equal tests/nbest_numpy.py's (the recursion in numpy fp32 with a stable
    descending sort), on random inputs, with structural -inf and with integer inputs (exact ties);
  * rank 0 equals states / final_score of ops.viterbi and ops.viterbi_ragged in both obs modes;
  * at N = 3, T = 7 the 16 scores are the 16 largest of the 2187 enumerated path scores.
The one tolerance, 1e-4 on path_log_posterior being non-increasing in the rank, is that function's
fp64 summation order against the kernel's fp32 left fold.
Shapes: every padding of the state count and both sides of it (1, 3, 64 | 65 | 129, 256), every K
bucket (1 | 2 | 5 | 16), T = 1, 2, 17 and 70 (more than one 64-row pointer chunk; at NP = 256 and
K = 16 a chunk holds 7 rows), three workgroups with lengths (T, 1, T // 2) and NaN in the padded
frames.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nbest_numpy as nm  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG = -np.inf


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


@pytest.fixture(scope="module", autouse=True)
def _native():
    import pytorch_hmm_amd._native as nat
    nat.lib()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()


def ops():
    from pytorch_hmm_amd import ops as o
    return o


def run(obs, lP, init, mode, K, lengths=None):
    lens = None if lengths is None else torch.as_tensor(lengths)
    paths, scores, count = ops().viterbi_nbest(t(obs), t(lP), t(init), mode, K, lens)
    assert paths.dtype == torch.int64 and scores.dtype == torch.float32 and count.dtype == torch.int32
    return paths.cpu().numpy(), scores.cpu().numpy(), count.cpu().numpy()


def random_model(rng, B, T, N):
    lo = np.log(rng.random((B, T, N)) + 1e-3).astype(np.float32)
    lP = np.log(rng.random((N, N)) ** 3 + 1e-4).astype(np.float32)
    init = np.log(rng.random(N) + 1e-3).astype(np.float32)
    return lo, lP, init


def check_against_model(got, lo, lP, init, K, lengths=None):
    paths, scores, count = nm.nbest(lo, lP, init, K, lengths)
    assert np.array_equal(got[2], count), (got[2], count)
    assert np.array_equal(got[1], scores), np.argwhere(got[1] != scores)[:5]
    assert np.array_equal(got[0], paths), np.argwhere(got[0] != paths)[:5]


# ------------------------------------------------------------ bit-exact against the model
SHAPES = [(N, K, T) for N in (1, 3, 64, 65, 129, 256) for K in (1, 2, 5, 16) for T in (1, 2, 17, 70)
          if not (N == 256 and T > 20)]


@pytest.mark.parametrize("N,K,T", SHAPES)
def test_obs_log_matches_model(N, K, T):
    rng = np.random.default_rng(N * 1000 + K * 100 + T)
    lo, lP, init = random_model(rng, 3, T, N)
    check_against_model(run(lo, lP, init, ops().OBS_LOG, K), lo, lP, init, K)
    lengths = [T, 1, max(T // 2, 1)]
    padded = lo.copy()
    for b, L in enumerate(lengths):
        padded[b, L:] = np.nan
    check_against_model(run(padded, lP, init, ops().OBS_LOG, K, lengths), lo, lP, init, K, lengths)


# --------------------------------------------------------------------- structural zeros
@pytest.mark.parametrize("N,K", [(5, 4), (70, 16), (130, 8)])
def test_left_to_right_and_dead_columns(N, K):
    rng = np.random.default_rng(N + K)
    B, T = 3, 19
    lo, _, _ = random_model(rng, B, T, N)
    lP = np.full((N, N), NEG, np.float32)
    for i in range(N):
        for j, p in ((i, 0.6), (i + 1, 0.3), (i + 2, 0.1)):
            if j < N:
                lP[i, j] = np.log(p)
    init = np.full(N, NEG, np.float32)
    init[0] = 0.0
    lo[0, 7, :] = NEG          # sequence 0: an emission row that is all -inf -> every path is -inf
    lo[1, :, 1] = NEG          # sequence 1: a dead state
    got = run(lo, lP, init, ops().OBS_LOG, K)
    check_against_model(got, lo, lP, init, K)
    assert got[2][0] == 0 and np.all(got[0][0, 0] == 0) and got[1][0, 0] == NEG
    assert np.all(got[0][0, 1:] == -1) and np.all(got[1][0, 1:] == NEG)
    # a left-to-right path never steps back
    for b in (1, 2):
        for k in range(int(got[2][b])):
            assert np.all(np.diff(got[0][b, k]) >= 0)


# --------------------------------------------------------------------------- exact ties
@pytest.mark.parametrize("N,K,T", [(3, 5, 9), (64, 16, 12), (100, 8, 70), (200, 4, 9)])
def test_exact_ties(N, K, T):
    rng = np.random.default_rng(N + K + T)
    B = 2
    lo = -rng.integers(0, 3, (B, T, N)).astype(np.float32)
    lP = -rng.integers(0, 3, (N, N)).astype(np.float32)
    init = -rng.integers(0, 2, N).astype(np.float32)
    got = run(lo, lP, init, ops().OBS_LOG, K)
    check_against_model(got, lo, lP, init, K)
    states, _, final = ops().viterbi(t(lo), t(lP), t(init), ops().OBS_LOG)
    assert np.array_equal(got[0][:, 0], states.cpu().numpy())
    assert np.array_equal(got[1][:, 0], final.cpu().numpy())


# ------------------------------------------------------- rank 0 against the existing decoders
@pytest.mark.parametrize("N", [5, 64, 200])
@pytest.mark.parametrize("mode", ["prob", "log"])
def test_rank0_is_the_viterbi_path(N, mode):
    o = ops()
    rng = np.random.default_rng(N)
    B, T, K = 3, 41, 4
    if mode == "prob":
        obs = rng.random((B, T, N)).astype(np.float32)
        obs[0, 3, :] = 0.0                                   # log(0 + 1e-8) in a whole row
        m = o.OBS_PROB
    else:
        obs = np.log(rng.random((B, T, N)) + 1e-3).astype(np.float32)
        obs[0, 3, 1] = NEG
        m = o.OBS_LOG
    _, lP, init = random_model(rng, 1, 1, N)
    lP[rng.random((N, N)) < 0.3] = NEG
    paths, scores, count = o.viterbi_nbest(t(obs), t(lP), t(init), m, K)
    states, _, final = o.viterbi(t(obs), t(lP), t(init), m)
    assert torch.equal(paths[:, 0], states) and torch.equal(scores[:, 0], final)
    lengths = torch.tensor([T, 1, 17])
    padded = t(obs).clone()
    padded[1, 1:] = float("nan")
    padded[2, 17:] = float("nan")
    paths, scores, count = o.viterbi_nbest(padded, t(lP), t(init), m, K, lengths)
    states, _, final = o.viterbi_ragged(padded, t(lP), t(init), m, lengths)
    assert torch.equal(paths[:, 0], states) and torch.equal(scores[:, 0], final)
    assert bool((paths[1, :, 1:] == -1).all()) and bool((paths[2, :, 17:] == -1).all())


# ------------------------------------------------------------ OBS_PROB, all ranks, bit-exact
@pytest.mark.parametrize("N,K", [(4, 3), (70, 16), (129, 5)])
def test_obs_prob_matches_model_on_the_library_log(N, K):
    o = ops()
    rng = np.random.default_rng(N * 7 + K)
    B, T = 3, 23
    obs = rng.random((B, T, N)).astype(np.float32)
    obs[1, 5, :2] = 0.0
    _, lP, init = random_model(rng, 1, 1, N)
    # the library's own log-emissions: a one-frame Viterbi with init = 0 returns log_delta = lo
    _, lo, _ = o.viterbi(t(obs).reshape(B * T, 1, N), t(lP), torch.zeros(N, device=DEV), o.OBS_PROB)
    lo = lo.reshape(B, T, N).cpu().numpy()
    assert np.allclose(lo, np.log(obs + np.float32(1e-8)), atol=1e-5)
    check_against_model(run(obs, lP, init, o.OBS_PROB, K), lo, lP, init, K)
    lengths = [T, 1, 11]
    check_against_model(run(obs, lP, init, o.OBS_PROB, K, lengths), lo, lP, init, K, lengths)


# ------------------------------------------------------------- enumeration on the device
def test_scores_are_the_largest_enumerated():
    rng = np.random.default_rng(3)
    N, T, K = 3, 7, 16
    lo, lP, init = random_model(rng, 2, T, N)
    paths, scores, count = run(lo, lP, init, ops().OBS_LOG, K)
    for b in range(2):
        assert np.array_equal(scores[b], nm.top_scores(lo[b], lP, init, K))
        assert count[b] == K and len({tuple(p) for p in paths[b]}) == K
        for k in range(K):
            assert nm.fold(paths[b, k], lo[b], lP, init) == scores[b, k]


# ------------------------------------------------- reproducibility and degenerate calls
def test_reproducible_and_degenerate_calls():
    o = ops()
    rng = np.random.default_rng(9)
    B, T, N, K = 4, 33, 70, 8
    lo, lP, init = random_model(rng, B, T, N)
    a = o.viterbi_nbest(t(lo), t(lP), t(init), o.OBS_LOG, K)
    b = o.viterbi_nbest(t(lo), t(lP), t(init), o.OBS_LOG, K)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # float64 and non-contiguous inputs are converted, as by ops.viterbi
    wide = torch.zeros(B, T, 2 * N, device=DEV, dtype=torch.float64)
    wide[..., ::2] = t(lo).double()
    c = o.viterbi_nbest(wide[..., ::2], t(lP).double().t().contiguous().t(), t(init).double(), o.OBS_LOG, K)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # lengths equal to T are the plain call
    e = o.viterbi_nbest(t(lo), t(lP), t(init), o.OBS_LOG, K, torch.full((B,), T))
    assert all(torch.equal(x, y) for x, y in zip(a, e))
    paths, scores, count = o.viterbi_nbest(torch.zeros(0, T, N, device=DEV), t(lP), t(init), o.OBS_LOG, K)
    assert paths.shape == (0, K, T) and scores.shape == (0, K) and count.shape == (0,)


def test_captured_into_a_graph():
    """One launch, no host synchronisation without lengths: a captured call replays on new inputs."""
    o = ops()
    rng = np.random.default_rng(21)
    B, T, N, K = 2, 19, 70, 4
    lo, lP, init = random_model(rng, B, T, N)
    x, lPd, initd = t(lo).clone(), t(lP), t(init)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        o.viterbi_nbest(x, lPd, initd, o.OBS_LOG, K)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=s):
        out = o.viterbi_nbest(x, lPd, initd, o.OBS_LOG, K)
    torch.cuda.synchronize()
    for k in range(2):
        x.copy_(t(np.roll(lo, k + 1, axis=2)))
        gr.replay()
        torch.cuda.synchronize()
        ref = o.viterbi_nbest(x.clone(), lPd, initd, o.OBS_LOG, K)
        assert all(torch.equal(a, b) for a, b in zip(out, ref))


# ------------------------------------------------------------------------- public layer
def test_hmm_viterbi_nbest():
    import pytorch_hmm_amd as ph
    rng = np.random.default_rng(11)
    N, B, T, K = 6, 3, 25, 5
    P = rng.random((N, N)).astype(np.float32) + 0.05
    P /= P.sum(1, keepdims=True)
    hmm = ph.HMMPyTorch(P)
    obs = t(rng.random((B, T, N)).astype(np.float32))
    paths, scores = hmm.viterbi_nbest(obs, K)
    assert paths.shape == (B, K, T) and scores.shape == (B, K)
    states, _ = hmm.viterbi_decode(obs)
    assert torch.equal(paths[:, 0], states)
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())
    assert len({tuple(p) for p in paths[0].cpu().numpy()}) == K
    # the normalised scores keep the order: path_log_posterior sums the same fp32 terms in fp64
    lp = hmm.path_log_posterior(obs, paths)
    assert lp.shape == (B, K) and bool((lp[:, :-1] - lp[:, 1:] >= -1e-4).all())
    assert bool((lp <= 1e-4).all())
    # 2-D input is squeezed
    p2, s2 = hmm.viterbi_nbest(obs[1], K)
    assert p2.shape == (K, T) and s2.shape == (K,)
    assert torch.equal(p2, paths[1]) and torch.equal(s2, scores[1])
    # lengths
    lengths = [T, 4, 13]
    pl, sl = hmm.viterbi_nbest(obs, K, lengths)
    sr, _ = hmm.viterbi_decode(obs, lengths)
    assert torch.equal(pl[:, 0], sr) and bool((pl[1, :, 4:] == -1).all())
    p4, s4 = hmm.viterbi_nbest(obs[1, :4], K)
    assert torch.equal(pl[1, :, :4], p4) and torch.equal(sl[1], s4)


def test_layers_nbest_alignment():
    import pytorch_hmm_amd as ph
    torch.manual_seed(0)
    B, T, S, D, K = 2, 21, 5, 4, 3
    lengths = [T, 9]
    layer = ph.HMMLayer(S).to(DEV)
    x = torch.randn(B, T, S, device=DEV)
    for lens in (None, lengths):
        paths, scores = layer.nbest_alignment(x, K, lens)
        assert paths.shape == (B, K, T) and scores.shape == (B, K)
        assert torch.equal(paths[:, 0], layer.align(x, lens)[0])
    g = ph.GaussianHMMLayer(S, D).to(DEV)
    xf = torch.randn(B, T, D, device=DEV)
    for lens in (None, lengths):
        paths, scores = g.nbest_alignment(xf, K, lens)
        with torch.no_grad():
            ref = g.hmm_layer.align(g._observation_probs(xf, lens), lens)[0]
        assert paths.shape == (B, K, T) and torch.equal(paths[:, 0], ref)
    m = ph.MixtureGaussianHMMLayer(S, D).to(DEV).eval()
    for lens in (None, lengths):
        paths, scores = m.nbest_alignment(xf, K, lens)
        with torch.no_grad():
            states, best = m(xf, return_log_probs=True, lengths=lens)
        assert torch.equal(paths[:, 0], states) and torch.equal(scores[:, 0], best)
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())
