"""GPU parity of the batch-tiled (wide) Viterbi and forward-backward (csrc/wide.hip,
hmm355_viterbi_wide_f32 / hmm355_forward_backward_wide_f32) for 257..4096 states, and of the
public classes above 256 states.

Contracts:
  * Viterbi given fp32 log-emissions: states and trellis bit-identical to the reference's
    recursion (oracle viterbi_from_log, torch-CPU; the C oracle's back-pointers are uint8 and stop
    at 256 states), first index on ties, also for -inf columns.
  * Forward-backward against the float64 C oracle, at the project's bounds (test_gpu_kernels.py)
    plus a relative bound on the posterior entries above 1e-4: an fp32 model of this scaled
    recursion is within 3.4e-6 relative / 4.5e-7 absolute of float64 on these inputs, so 1e-4
    relative leaves ~30x for the GPU's summation order.
Shapes are the smallest that cross the first column tile (64), leave a ragged last tile, use more
than one batch tile, and T in {1, 2}.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sequences per workgroup of the step kernels (csrc/wide.hip kBT)
BT = int(re.search(r"constexpr int kBT = (\d+);",
                   open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "wide.hip")).read()).group(1))


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------- inputs
def log_params(rng, N, power):
    P = rng.random((N, N), dtype=np.float32) ** power
    lP = np.log(P / P.sum(1, keepdims=True) + np.float32(1e-8)).astype(np.float32)
    init = np.log(np.full(N, 1.0 / N, np.float32) + np.float32(1e-8)).astype(np.float32)
    return lP, init


@functools.lru_cache(maxsize=None)
def vit_case(B, T, N, kind="random"):
    """(lo, lP, init, oracle states, oracle delta), computed once per case and left unchanged."""
    rng = np.random.default_rng(B * 1000 + T * 7 + N)
    lo = np.log(rng.random((B, T, N), dtype=np.float32) + np.float32(1e-8)).astype(np.float32)
    lP, init = log_params(rng, N, 4)
    if kind != "random":
        # multiples of 0.5: every sum is exact, so equal candidates occur in different input
        # slices and column tiles
        lo, lP, init = (np.round(x * 2) / 2 for x in (lo, lP, init))
        lo, lP, init = lo.astype(np.float32), lP.astype(np.float32), init.astype(np.float32)
    if kind == "ties_inf":
        lo[rng.random(lo.shape) < 0.1] = -np.inf
        lo[:, :, N // 3] = -np.inf
    s, d = O.viterbi_from_log(torch.from_numpy(lo), torch.from_numpy(lP), torch.from_numpy(init))
    return lo, lP, init, s.numpy(), d.numpy()


def fb_inputs(B, T, N, kind):
    rng = np.random.default_rng(T * N + B)
    if kind == "peaked":
        obs = rng.random((B, T, N), dtype=np.float32) ** 16
        P = torch.from_numpy(rng.random((N, N), dtype=np.float32) ** 8)
    elif kind == "l2r":
        obs = rng.random((B, T, N), dtype=np.float32) ** 16
        P = O.left_to_right_matrix(N, 0.7)
    else:
        obs = rng.random((B, T, N), dtype=np.float32)
        P = torch.from_numpy(rng.random((N, N), dtype=np.float32))
    lP, lp0 = O.hmm_params(P)
    return obs, lP, lp0


@functools.lru_cache(maxsize=None)
def fb_case(B, T, N, kind):
    """(obs, lP, lp0, fp64 log alpha, log beta, posterior, loglik, the reference's compute_likelihood)."""
    obs, lP, lp0 = fb_inputs(B, T, N, kind)
    la, lb, post64, ll64 = O.c_fb64(np.log(obs + np.float32(1e-8)), lP.numpy(), lp0.numpy())
    lik = O.compute_likelihood(torch.from_numpy(obs), lP, lp0).numpy()
    return obs, lP, lp0, la, lb, post64, ll64, lik


def check_fb(outs, la, lb, post64, ll64, lik=None, what=""):
    """The bounds of the module docstring; every figure is printed before it is asserted."""
    post, fwd, bwd, loglik, lik_ref = (None if x is None else x.detach().cpu().numpy().astype(np.float64) for x in outs)
    big = post64 > 1e-4
    rel = np.abs(post[big] - post64[big]) / post64[big] if big.any() else np.zeros(1)
    print(f"{what} posterior max|err| {np.abs(post - post64).max():.3e} max rel (>1e-4) {rel.max():.3e}"
          f" loglik rel {np.abs((loglik - ll64) / ll64).max():.3e}")
    np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0)
    np.testing.assert_allclose(post[big], post64[big], rtol=1e-4, atol=0)
    np.testing.assert_allclose(loglik, ll64, rtol=2e-6)
    for ours, ref in ((fwd, np.exp(la)), (bwd, np.exp(lb))):
        if ours is None:
            continue
        rep = ref > 1e-30
        np.testing.assert_allclose(ours[rep], ref[rep], rtol=1e-4)
        assert np.all(np.abs(ours[~rep]) < 1e-29)
    if lik is not None:
        np.testing.assert_allclose(lik_ref, lik.reshape(-1), rtol=1e-5, atol=1e-5)


def path_score64(states, lo, lP, init):
    """Score of a state path in float64 from fp32 log inputs."""
    lo, lP, init = (np.asarray(x, np.float64) for x in (lo, lP, init))
    B, T = states.shape
    ar = np.arange(B)
    sc = init[states[:, 0]] + lo[ar, 0, states[:, 0]]
    for k in range(1, T):
        sc = sc + lP[states[:, k - 1], states[:, k]] + lo[ar, k, states[:, k]]
    return sc


def check_viterbi_prob(states, delta, obs, lP, lp0):
    """OBS_PROB decodes: a 1-ulp difference between the correctly rounded log and torch's may move
    a near-tie, so the path is judged by its score, not compared state by state."""
    obs_t = torch.from_numpy(obs)
    s_ref, d_ref = O.viterbi_decode(obs_t, lP, lp0)
    states, delta = states.cpu().numpy(), delta.cpu().numpy()
    np.testing.assert_allclose(delta, d_ref.numpy(), rtol=2e-6, atol=1e-5)
    N = obs.shape[-1]
    assert states.min() >= 0 and states.max() < N
    lo = torch.log(obs_t + 1e-8).numpy()
    best = d_ref.numpy()[:, -1].max(-1).astype(np.float64)
    np.testing.assert_allclose(path_score64(states, lo, lP.numpy(), lp0.numpy()), best, rtol=0, atol=1e-3)


# ------------------------------------------------------------------------------ Viterbi
VIT_SHAPES = [(3, 1, 257), (1, 2, 257), (9, 70, 300), (2, 40, 513), (2, 33, 1024), (BT + 1, 5, 640)]


@pytest.mark.parametrize("B,T,N", VIT_SHAPES)
def test_viterbi_bitexact_log_input(B, T, N):
    lo, lP, init, s_ref, d_ref = vit_case(B, T, N)
    o = ops()
    states, delta, final = o.viterbi(t(lo), t(lP), t(init), o.OBS_LOG)
    assert np.array_equal(states.cpu().numpy(), s_ref)
    assert np.array_equal(bits(delta.cpu().numpy()), bits(d_ref))
    assert np.array_equal(final.cpu().numpy(), d_ref[:, -1].max(-1))


@pytest.mark.parametrize("B,T,N,kind", [(3, 70, 300, "ties"), (2, 33, 1024, "ties"), (3, 70, 300, "ties_inf")])
def test_viterbi_ties_first_index(B, T, N, kind):
    lo, lP, init, s_ref, d_ref = vit_case(B, T, N, kind)
    # the inputs do produce ties: some delta column has two equal best candidates
    cand = d_ref[0, T // 2 - 1, :, None].astype(np.float32) + lP
    assert ((cand == cand.max(0)).sum(0) > 1).any()
    o = ops()
    states, delta, final = o.viterbi(t(lo), t(lP), t(init), o.OBS_LOG)
    assert np.array_equal(states.cpu().numpy(), s_ref)
    assert np.array_equal(bits(delta.cpu().numpy()), bits(d_ref))
    assert np.array_equal(final.cpu().numpy(), d_ref[:, -1].max(-1))


@pytest.mark.parametrize("N", [5, 64, 200, 256])
def test_wide_and_narrow_forms_agree(N):
    B, T = 3, 65
    o = ops()
    lo, lP, init, _, _ = vit_case(B, T, N)
    obs, flP, flp0, la, lb, post64, ll64, lik = fb_case(B, T, N, "peaked")
    for x, mode in ((lo, o.OBS_LOG), (obs, o.OBS_PROB)):
        narrow = o.viterbi(t(x), t(lP), t(init), mode)
        wide = o.viterbi(t(x), t(lP), t(init), mode, wide=True)
        for a, b in zip(narrow, wide):
            assert torch.equal(a, b)
    mask = o.FB_POSTERIOR | o.FB_FORWARD | o.FB_BACKWARD
    check_fb(o.forward_backward(t(obs), t(flP), t(flp0), o.OBS_PROB, mask, wide=True), la, lb, post64, ll64, lik,
             f"wide N={N}")
    check_fb(o.forward_backward(t(obs), t(flP), t(flp0), o.OBS_PROB, mask), la, lb, post64, ll64, lik,
             f"narrow N={N}")


def test_viterbi_prob_input():
    B, T, N = 3, 70, 300
    obs, lP, lp0 = fb_inputs(B, T, N, "uniform")
    o = ops()
    states, delta, final = o.viterbi(t(obs), t(lP), t(lp0), o.OBS_PROB)
    check_viterbi_prob(states, delta, obs, lP, lp0)
    assert torch.equal(final, delta[:, -1].max(-1).values)


# --------------------------------------------------------------------- forward-backward
@pytest.mark.parametrize("B,T,N,kind", [(2, 1, 257, "peaked"), (3, 70, 300, "peaked"), (2, 33, 513, "peaked"),
                                        (2, 40, 1024, "l2r"), (1, 600, 257, "uniform")])
def test_forward_backward_vs_fp64(B, T, N, kind):
    obs, lP, lp0, la, lb, post64, ll64, lik = fb_case(B, T, N, kind)
    o = ops()
    outs = o.forward_backward(t(obs), t(lP), t(lp0), o.OBS_PROB, o.FB_POSTERIOR | o.FB_FORWARD | o.FB_BACKWARD)
    check_fb(outs, la, lb, post64, ll64, lik, f"({B},{T},{N}) {kind}")
    # a likelihood-only call (no output bit) gives the same two likelihoods
    _, _, _, ll, lr = o.forward_backward(t(obs), t(lP), t(lp0), o.OBS_PROB, 0)
    assert torch.equal(ll, outs[3]) and torch.equal(lr, outs[4])


def test_forward_backward_far_negative_log_emissions():
    B, T, N = 2, 70, 300
    rng = np.random.default_rng(6)
    lo = (-300 + 40 * rng.standard_normal((B, T, N))).astype(np.float32)
    _, lP, lp0 = fb_inputs(B, T, N, "peaked")
    la, lb, post64, ll64 = O.c_fb64(lo, lP.numpy(), lp0.numpy())
    o = ops()
    outs = o.forward_backward(t(lo), t(lP), t(lp0), o.OBS_LOG, o.FB_POSTERIOR | o.FB_FORWARD | o.FB_BACKWARD)
    for x in outs:
        assert torch.isfinite(x).all()
    check_fb((outs[0], None, None, outs[3], None), la, lb, post64, ll64, None, "far-negative OBS_LOG")


# ------------------------------------------------------------------------------- layers
def test_hmmpytorch_300_states():
    from pytorch_hmm_amd import HMMPyTorch
    B, T, N = 3, 70, 300
    P = O.left_to_right_matrix(N, 0.7)
    lP, lp0 = O.hmm_params(P)
    hmm = HMMPyTorch(P)
    obs = np.random.default_rng(7).random((B, T, N), dtype=np.float32)
    x = t(obs)
    states, delta = hmm.viterbi_decode(x)
    assert states.shape == (B, T) and delta.shape == (B, T, N)
    check_viterbi_prob(states, delta, obs, lP, lp0)
    la, lb, post64, ll64 = O.c_fb64(np.log(obs + np.float32(1e-8)), lP.numpy(), lp0.numpy())
    lik = O.compute_likelihood(torch.from_numpy(obs), lP, lp0).numpy()
    post, fwd, bwd = hmm.forward_backward(x)
    ll = hmm.log_likelihood(x)
    lr = hmm.compute_likelihood(x)
    check_fb((post, fwd, bwd, ll, lr), la, lb, post64, ll64, lik, "HMMPyTorch(300)")
    assert torch.equal(hmm.posteriors(x), post)
    # 2-D input: Viterbi and the likelihoods are squeezed, forward_backward is not (hmm.py)
    s1, d1 = hmm.viterbi_decode(x[0])
    assert s1.shape == (T,) and d1.shape == (T, N)
    assert torch.equal(s1, states[0]) and torch.equal(d1, delta[0])
    assert hmm.compute_likelihood(x[0]).shape == () and hmm.log_likelihood(x[0]).shape == ()
    assert torch.equal(hmm.compute_likelihood(x[0]), lr[0]) and torch.equal(hmm.log_likelihood(x[0]), ll[0])
    assert hmm.forward_backward(x[0])[0].shape == (1, T, N)


def test_mixture_layer_300_states():
    from pytorch_hmm_amd import MixtureGaussianHMMLayer
    torch.manual_seed(3)
    S, D, B, T = 300, 8, 2, 40
    layer = MixtureGaussianHMMLayer(S, D, num_components=2).to(DEV).eval()
    x = torch.randn(B, T, D, device=DEV)
    states, scores = layer(x, return_log_probs=True)
    with torch.no_grad():
        lp = layer.get_observation_log_probs(x).cpu()
        log_T = layer._safe_log(layer.get_transition_matrix()).cpu()
    s_ref, d_ref = O.viterbi_from_log(lp, log_T, O.mixture_init_vector(S))
    assert torch.equal(states.cpu(), s_ref)
    assert torch.equal(scores.cpu(), d_ref[:, -1].max(-1).values)


@pytest.mark.parametrize("viterbi_inference", [True, False])
def test_hmmlayer_300_states_eval(viterbi_inference):
    from pytorch_hmm_amd import HMMLayer
    torch.manual_seed(4)
    B, T, N = 2, 40, 300
    layer = HMMLayer(N, viterbi_inference=viterbi_inference).to(DEV).eval()
    with torch.no_grad():
        post = layer(torch.randn(B, T, N, device=DEV))
        states, delta = layer.align(torch.randn(B, T, N, device=DEV))
    assert post.shape == (B, T, N)
    assert torch.allclose(post.sum(-1), torch.ones(B, T, device=DEV), atol=1e-5, rtol=0)
    assert states.shape == (B, T) and delta.shape == (B, T, N)
    assert int(states.min()) >= 0 and int(states.max()) < N


def test_gaussian_layer_300_states_eval():
    from pytorch_hmm_amd import GaussianHMMLayer
    torch.manual_seed(5)
    B, T, N, D = 2, 40, 300, 4
    layer = GaussianHMMLayer(N, D).to(DEV).eval()
    with torch.no_grad():
        post = layer(torch.randn(B, T, D, device=DEV))
    assert post.shape == (B, T, N)
    assert torch.allclose(post.sum(-1), torch.ones(B, T, device=DEV), atol=1e-5, rtol=0)


def test_gradients_above_256_states_are_refused():
    from pytorch_hmm_amd import HMMPyTorch
    hmm = HMMPyTorch(O.left_to_right_matrix(300, 0.7))
    obs = torch.rand(2, 10, 300, device=DEV).requires_grad_()
    with pytest.raises(NotImplementedError, match="256"):
        hmm.forward_backward(obs)
    with pytest.raises(NotImplementedError, match="256"):
        hmm.compute_likelihood(obs)


# ------------------------------------------------------------------------- stream order
def test_side_stream_matches_default_stream():
    """The per-step launches and the workspace follow the current stream: the same calls on a side
    stream, queued behind a large matrix product there, give the default stream's results."""
    B, T, N = 2, 70, 300
    lo, lP, init, _, _ = vit_case(B, T, N)
    obs, flP, flp0 = fb_inputs(B, T, N, "peaked")
    o = ops()
    args_v = (t(lo), t(lP), t(init), o.OBS_LOG)
    args_f = (t(obs), t(flP), t(flp0), o.OBS_PROB, o.FB_POSTERIOR | o.FB_FORWARD | o.FB_BACKWARD)
    want_v, want_f = o.viterbi(*args_v), o.forward_backward(*args_f)
    big = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _ = big @ big
        got_v, got_f = o.viterbi(*args_v), o.forward_backward(*args_f)
    side.synchronize()
    for a, b in zip(want_v + want_f, got_v + got_f):
        assert torch.equal(a, b)
