"""GPU: posterior path sampling (csrc/ffbs.hip, hmm355_ffbs_f32; ops.ffbs / ops.posterior_sample;
HMMPyTorch.sample_posterior / path_log_posterior; the layers' sample_alignment).

Contracts (the model is tests/ffbs_numpy.py, fp64):
  * Kernel given rows: every draw passes the teacher-forced interval check -- with the kernel's own
    z_{t+1}, w formed in fp64 from the same fp32 inputs and F = cumsum(w) / sum(w), the drawn state
    has w > 0 and F[z-1] - eps <= u <= F[z] + eps, eps = (N + 16) 2^-23 (the fp32 prefix sum of N
    non-negative terms, the product, expf and u * total, doubled for numerator and denominator).
    Padded frames are -1 and never read (NaN there), columns N .. ld-1 are never read (7.0 there).
  * Exact cases with dyadic weights and A = 1; exact zeros keep a left-to-right path monotone.
  * The same uniforms give the same states: twice, on a side stream, and through posterior_sample.
  * End to end, 2048 samples: per-cell state frequencies and the (z_2, z_3) pair frequencies lie
    within 5 sqrt(p (1 - p) / K) + 1 / K of the enumerated fp64 posterior (five sigma of a binomial
    count with a one-count floor).
  * path_log_posterior: the 8 paths of a 2-state, 3-frame model sum to 1 within 1e-5; joint and
    log-likelihood terms match the fp64 model to 2e-6 relative (the project's loglik bound).
Shapes: every padding of the state count and both sides of it (1, 5, 64 | 65, 128 | 129, 200,
256), T = 1, 2 and 70 (more than one 64-step chunk and a tail of the 8-deep load ring), more
samples than a workgroup has waves (37) and than the grid spreads over blockIdx.y (B = 256).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffbs_numpy as fm  # noqa: E402
from oracle import hmm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


def pad(N):
    return 64 if N <= 64 else (128 if N <= 128 else 256)


def matrix(N, kind, rng):
    """ergodic: rand**4 rows (a wide spread of weights); ltr: stay / next / skip with exact zeros."""
    if kind == "ergodic":
        A = rng.random((N, N)) ** 4 + 1e-12
    else:
        A = np.zeros((N, N))
        for i in range(N):
            for j, p in ((i, 0.5), (i + 1, 0.3), (i + 2, 0.2)):
                A[i, min(j, N - 1)] += p
    return A / A.sum(1, keepdims=True)


def log32(A):
    with np.errstate(divide="ignore"):
        return np.log(A).astype(np.float32)


def rows_case(N, T, kind, seed, B=3, zero_emissions=False):
    """(fwd32 view (B,T,N) of a (B,T,NP) buffer padded with 7.0, log_P32) from the fp64 filter."""
    rng = np.random.default_rng(seed)
    A = matrix(N, kind, rng)
    e = rng.random((B, T, N)) + 1e-3
    p0 = np.full(N, 1.0 / N)
    if zero_emissions:
        e[:, :, 1::3] = 0.0
        p0 = np.zeros(N)
        p0[0] = 1.0
    alpha, _ = fm.forward_filter(e, A, p0)
    buf = np.full((B, T, pad(N)), 7.0, np.float32)
    buf[..., :N] = alpha.astype(np.float32)
    return buf, log32(A)


def run_ffbs(buf, N, lP32, u, lengths=None):
    fwd = t(buf)[..., :N]
    assert fwd.stride(1) == buf.shape[-1]
    return ops().ffbs(fwd, t(lP32), t(u), None if lengths is None else torch.tensor(lengths)).cpu().numpy()


# ------------------------------------------------------------------ 1. kernel given rows
@pytest.mark.parametrize("kind", ["ergodic", "ltr"])
@pytest.mark.parametrize("T", [1, 2, 70])
@pytest.mark.parametrize("N", [1, 5, 64, 65, 128, 129, 200, 256])
def test_kernel_given_rows(N, T, kind):
    B, K = 3, 5
    buf, lP32 = rows_case(N, T, kind, seed=1000 * N + T)
    rng = np.random.default_rng(7 * N + T)
    for lengths in (None, [1, T, T // 2 + 1]):
        u = rng.random((B, K, T), dtype=np.float32)
        rows = buf.copy()
        if lengths is not None:
            for b, n in enumerate(lengths):   # padded frames are never read
                rows[b, n:] = np.nan
                u[b, :, n:] = np.nan
        states = run_ffbs(rows, N, lP32, u, lengths)
        assert states.shape == (B, K, T) and states.dtype == np.int64
        ok, msg = fm.intervals_ok(states, u, rows, lP32, lengths)
        assert ok, msg
        valid = np.ones((B, T), bool) if lengths is None else np.arange(T)[None, :] < np.asarray(lengths)[:, None]
        v = np.broadcast_to(valid[:, None, :], states.shape)
        assert (states[v] >= 0).all() and (states[v] < N).all() and (states[~v] == -1).all()


# ------------------------------------------------------------------------ 2. exact cases
def test_exact_dyadic_rows():
    N, K = 4, 6
    row = np.array([0.25, 0.0, 0.5, 0.25], np.float32)
    u1 = np.array([0.0, 0.25, 0.75, 1.0 - 2.0 ** -24, 0.5, 0.2499999], np.float32)
    want = np.array([0, 2, 3, 3, 2, 0])
    lP = np.zeros((N, N), np.float32)  # A = 1 exactly
    for T in (1, 2, 3):
        buf = np.full((1, T, 64), 7.0, np.float32)
        buf[0, :, :N] = row
        u = np.repeat(u1[None, :, None], T, 2)
        states = run_ffbs(buf, N, lP, u)
        assert (states[0] == want[:, None]).all(), states[0]


def test_exact_degenerate_rows():
    N, T, K = 4, 2, 3
    buf = np.full((3, T, 64), 7.0, np.float32)
    buf[0, :, :N] = 0.0                                  # all zeros: state 0
    buf[1, :, :N] = [1e38, 3e38, 3e38, 0.0]              # the total overflows: the first argmax
    buf[2, :, :N] = [0.0, 0.0, 0.0, 2.0]                 # one positive weight
    u = np.random.default_rng(3).random((3, K, T), dtype=np.float32)
    states = run_ffbs(buf, N, np.zeros((N, N), np.float32), u)
    assert (states[0] == 0).all() and (states[1] == 1).all() and (states[2] == 3).all()


# ------------------------------------------------------------------------ 3. exact zeros
@pytest.mark.parametrize("N", [70, 200])
def test_exact_zeros_keep_left_to_right_paths(N):
    B, K, T = 3, 5, 70
    buf, lP32 = rows_case(N, T, "ltr", seed=N, zero_emissions=True)
    assert np.isneginf(lP32).any() and (buf[:, :, 1:N:3] == 0).all()
    u = np.random.default_rng(N + 1).random((B, K, T), dtype=np.float32)
    u[:, 0] = 0.0                      # the smallest and the largest uniform on every frame
    u[:, 1] = 1.0 - 2.0 ** -24
    states = run_ffbs(buf, N, lP32, u)
    ok, msg = fm.intervals_ok(states, u, buf, lP32)   # includes w[z] > 0 for every draw
    assert ok, msg
    assert (np.diff(states, axis=2) >= 0).all() and (np.diff(states, axis=2) <= 2).all()
    assert (states % 3 != 1).all() and (states[:, :, 0] == 0).all()


# --------------------------------------------------------- 4. samples and determinism
@pytest.mark.parametrize("B,K,T,N", [(3, 1, 70, 65), (3, 37, 70, 65), (256, 37, 2, 5)])
def test_sample_counts_and_repeatability(B, K, T, N):
    buf, lP32 = rows_case(N, T, "ergodic", seed=K + B, B=B)
    u = np.random.default_rng(K).random((B, K, T), dtype=np.float32)
    fwd, lP, ut = t(buf)[..., :N], t(lP32), t(u)
    a = ops().ffbs(fwd, lP, ut)
    b = ops().ffbs(fwd, lP, ut)
    assert torch.equal(a, b)
    ok, msg = fm.intervals_ok(a.cpu().numpy(), u, buf, lP32)
    assert ok, msg
    # every sample reads its own uniforms: permuting them permutes the paths
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(0)).to(DEV)
    assert torch.equal(ops().ffbs(fwd, lP, ut[:, perm].contiguous()), a[:, perm])


def test_side_stream_matches_default_stream():
    """The launches and the workspace follow the current stream: the same call on a side stream,
    queued behind a large matrix product there, gives the default stream's result."""
    B, K, T, N = 3, 9, 70, 129
    buf, lP32 = rows_case(N, T, "ergodic", seed=5)
    u = t(np.random.default_rng(6).random((B, K, T), dtype=np.float32))
    fwd, lP = t(buf)[..., :N], t(lP32)
    want = ops().ffbs(fwd, lP, u)
    big = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _ = big @ big
        got = ops().ffbs(fwd, lP, u)
    side.synchronize()
    assert torch.equal(want, got)


# --------------------------------------------------------------------------- 5. pipeline
@pytest.mark.parametrize("case", ["dense", "banded", "obs_log", "lengths"])
@pytest.mark.parametrize("N", [5, 128, 200])
def test_posterior_sample_is_ffbs_on_the_kept_rows(N, case):
    from pytorch_hmm_amd import autograd
    o = ops()
    B, K, T = 3, 4, 70
    rng = np.random.default_rng(N)
    if case == "banded":   # the reference's left-to-right model: log(P + 1e-8), a banded plan
        lP, l0 = (x.to(DEV) for x in O.hmm_params(O.left_to_right_matrix(N, 0.7)))
    else:
        lP = t(np.log(matrix(N, "ergodic", rng) + 1e-8).astype(np.float32))
        l0 = t(np.log(np.full(N, 1.0 / N) + 1e-8).astype(np.float32))
    obs = rng.random((B, T, N), dtype=np.float32)
    mode = o.OBS_PROB
    if case == "obs_log":
        obs, mode = np.log(obs + 1e-3) * 5, o.OBS_LOG
    obs = t(obs)
    lengths = [T, 1, 37] if case == "lengths" else None
    plan = o.make_plan(lP, dense=(case == "dense"))
    if case == "banded":
        assert plan._hmm355_banded is True
    u = t(rng.random((B, K, T), dtype=np.float32))
    states, loglik = o.posterior_sample(obs, lP, l0, mode, K, uniforms=u, lengths=lengths, plan=plan)
    lens = o.active_lengths(lengths, B, T, N)
    _, ll, _, U, *_ = autograd._run_fb(obs, lP, l0, mode, plan=None if lens is not None else plan, lengths=lens)
    want = o.ffbs(U, lP, u, lens)
    assert torch.equal(states, want) and torch.equal(loglik, ll)
    assert states.shape == (B, K, T) and states.dtype == torch.int64
    ok, msg = fm.intervals_ok(states.cpu().numpy(), u.cpu().numpy(), U.cpu().numpy(), lP.cpu().numpy(), lengths)
    assert ok, msg


# ---------------------------------------------------------- 6. distribution, end to end
def test_sample_frequencies_match_the_exact_posterior():
    import pytorch_hmm_amd as ph
    N, T, B, K = 5, 6, 2, 2048
    rng = np.random.default_rng(42)
    hmm = ph.HMMPyTorch(matrix(N, "ergodic", rng).astype(np.float32), rng.random(N).astype(np.float32) + 0.1)
    obs = rng.random((B, T, N), dtype=np.float32)
    gen = torch.Generator(device=DEV)
    states = hmm.sample_posterior(t(obs), K, generator=gen.manual_seed(123))
    again = hmm.sample_posterior(t(obs), K, generator=gen.manual_seed(123))
    assert torch.equal(states, again)
    assert not torch.equal(states, hmm.sample_posterior(t(obs), K, generator=gen.manual_seed(124)))
    assert states.shape == (B, K, T) and states.dtype == torch.int64
    z = states.cpu().numpy()
    A = np.exp(hmm.log_P.double().numpy())
    p0 = np.exp(hmm.log_p0.double().numpy())
    bound = lambda p: 5 * np.sqrt(p * (1 - p) / K) + 1.0 / K
    worst = 0.0
    for b in range(B):
        paths, post = fm.enumerate_paths(obs[b].astype(np.float64) + 1e-8, A, p0)
        gamma, xi = fm.marginals(paths, post, N)
        freq = np.stack([np.bincount(z[b, :, tt], minlength=N) for tt in range(T)]) / K
        pair = np.zeros((N, N))
        np.add.at(pair, (z[b, :, 2], z[b, :, 3]), 1.0 / K)
        worst = max(worst, (np.abs(freq - gamma) / bound(gamma)).max(), (np.abs(pair - xi[2]) / bound(xi[2])).max())
        assert (np.abs(freq - gamma) <= bound(gamma)).all(), (freq, gamma)
        assert (np.abs(pair - xi[2]) <= bound(xi[2])).all(), (pair, xi[2])
    print(f"largest deviation / bound = {worst:.3f}")


# ------------------------------------------------------------------------ 7. log-posterior
def test_path_log_posterior_sums_to_one():
    import pytorch_hmm_amd as ph
    rng = np.random.default_rng(8)
    hmm = ph.HMMPyTorch(matrix(2, "ergodic", rng).astype(np.float32) + 0.1)
    obs = t(rng.random((1, 3, 2), dtype=np.float32))
    paths = torch.tensor([[(i >> 2) & 1, (i >> 1) & 1, i & 1] for i in range(8)], device=DEV)[None]
    lp = hmm.path_log_posterior(obs, paths)
    assert lp.shape == (1, 8)
    assert abs(float(torch.exp(lp.double()).sum()) - 1.0) < 1e-5
    assert torch.equal(hmm.path_log_posterior(obs[0], paths[0]), lp[0])          # 2-D observations
    assert torch.equal(hmm.path_log_posterior(obs, paths[:, 3]), lp[:, 3])       # (B,T) states


def test_path_log_posterior_matches_fp64_and_return_log_prob():
    import pytorch_hmm_amd as ph
    N, T, B, K = 5, 70, 3, 4
    rng = np.random.default_rng(9)
    hmm = ph.HMMPyTorch(matrix(N, "ergodic", rng).astype(np.float32))
    obs = rng.random((B, T, N), dtype=np.float32)
    gen = torch.Generator(device=DEV)
    for lengths in (None, [T, 9, 33]):
        states, lp = hmm.sample_posterior(t(obs), K, lengths=lengths, generator=gen.manual_seed(5), return_log_prob=True)
        assert lp.shape == (B, K) and torch.equal(lp, hmm.path_log_posterior(t(obs), states, lengths))
        joint, loglik = hmm._path_terms(t(obs), states, lengths)
        lP, l0 = hmm.log_P.double().numpy(), hmm.log_p0.double().numpy()
        le = np.log((obs + np.float32(1e-8)).astype(np.float64))
        _, ll64 = fm.forward_filter(np.exp(le), np.exp(lP), np.exp(l0), lengths)
        z = states.cpu().numpy()
        want = np.zeros((B, K))
        for b in range(B):
            n = T if lengths is None else lengths[b]
            for k in range(K):
                p = z[b, k, :n]
                want[b, k] = l0[p[0]] + lP[p[:-1], p[1:]].sum() + le[b, np.arange(n), p].sum()
        np.testing.assert_allclose(joint.cpu().numpy(), want, rtol=2e-6)
        np.testing.assert_allclose(loglik.cpu().numpy(), ll64, rtol=2e-6)
        assert (lp <= 1e-4).all()


# ------------------------------------------------------------------------------ 8. layers
def _check_alignment(draw, B, K, T, N, lengths):
    gen = torch.Generator(device=DEV)
    a = draw(K, None, gen.manual_seed(1))
    assert a.shape == (B, K, T) and a.dtype == torch.int64 and a.min() >= 0 and a.max() < N
    assert torch.equal(a, draw(K, None, gen.manual_seed(1)))
    p = draw(K, lengths, gen.manual_seed(1))
    valid = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).to(DEV)[:, None, :].expand(B, K, T)
    assert (p[~valid] == -1).all() and (p[valid] >= 0).all() and (p[valid] < N).all()
    return a


def test_hmm_layer_sample_alignment():
    import pytorch_hmm_amd as ph
    B, K, T, N = 3, 6, 40, 7
    torch.manual_seed(0)
    layer = ph.HMMLayer(N).to(DEV)
    x = torch.randn(B, T, N, device=DEV)
    with torch.no_grad():
        layer._get_hmm(), layer._get_hmm()   # past the first-call renormalisation of _get_hmm
        a = _check_alignment(lambda k, n, g: layer.sample_alignment(x, k, n, g), B, K, T, N, [T, 1, 17])
        one = layer.sample_alignment(x[0], K, generator=torch.Generator(device=DEV).manual_seed(1))
        assert one.shape == (K, T)
        want = layer._get_hmm().sample_posterior(torch.sigmoid(x), K,
                                                 generator=torch.Generator(device=DEV).manual_seed(1))
    assert torch.equal(a, want)
    assert not a.requires_grad


def test_gaussian_layer_sample_alignment():
    import pytorch_hmm_amd as ph
    B, K, T, N, D = 3, 6, 40, 6, 4
    torch.manual_seed(1)
    layer = ph.GaussianHMMLayer(N, D).to(DEV)
    x = torch.randn(B, T, D, device=DEV)
    _check_alignment(lambda k, n, g: layer.sample_alignment(x, k, n, g), B, K, T, N, [T, 1, 17])


def test_mixture_layer_sample_alignment():
    import pytorch_hmm_amd as ph
    B, K, T, N, D = 3, 6, 40, 6, 4
    torch.manual_seed(2)
    layer = ph.MixtureGaussianHMMLayer(N, D, num_components=2).to(DEV)
    x = torch.randn(B, T, D, device=DEV)
    a = _check_alignment(lambda k, n, g: layer.sample_alignment(x, k, n, g), B, K, T, N, [T, 1, 17])
    # the model its Viterbi decodes: OBS_LOG emissions, its log transitions, the uniform start
    with torch.no_grad():
        log_T, _, init, plan = layer._inference_tables(x.device)
        lp = layer.get_observation_log_probs(x)
        u = torch.rand((B, K, T), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
        want, _ = ops().posterior_sample(lp, log_T, init, ops().OBS_LOG, K, uniforms=u, plan=plan)
    assert torch.equal(a, want)
