"""GPU: forward-backward, Viterbi and their gradients over padded batches with per-sequence
lengths (csrc/ragged.hip, hmm355_viterbi_ragged_f32 / hmm355_forward_backward_ragged_f32, the
`lengths` keyword of the public classes).

Contracts (the oracle is tests/ragged_model.py: the project's oracle on each obs[b, :len_b]):
  * Viterbi: states and log_delta of every valid prefix are bit-identical to ops.viterbi on the
    slice alone and, for log inputs, to the reference's recursion (oracle viterbi_from_log);
    padded frames are -1 / -inf.
  * Forward-backward against the float64 C oracle per slice at the project's bounds
    (test_gpu_wide.py check_fb): posterior 2e-5 absolute and 1e-4 relative on entries > 1e-4,
    loglik 2e-6 relative, forward / backward 1e-4 relative where representable, lik_ref 1e-5;
    padded rows exactly 0.
  * Nothing depends on what the padded frames hold (NaN, 1e30); two calls return the same bits.
  * Gradients against float64 autograd through the reference loops per slice, each tensor within
    1e-4 of its largest entry (test_gpu_autograd.py close); grad_obs exactly 0 in padded frames.
Shapes: every padding of the state count (N = 5, 64 | 70, 128 | 200, 256), lengths around the
8-deep load ring (7, 8, 9) and the 64-row backtrace chunk (63, 64, 65), 1 and 2, more than two
chunks (131).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_model as rm  # noqa: E402
from oracle import hmm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
STATES = [5, 64, 70, 128, 200, 256]
TMAX = 131
VIT_LENGTHS = (1, 2, 63, 64, 65, 131)
FB_LENGTHS = (1, 2, 7, 8, 9, 64, 65, 131)


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


def valid_mask(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def fill_padding(x, lengths, value):
    """A copy of x (B,T,...) with the frames >= lengths[b] set to `value`."""
    y = np.array(x, copy=True)
    y[~valid_mask(lengths, x.shape[1])] = value
    return y


# ------------------------------------------------------------------------------- inputs
def log_params(rng, N, power):
    P = rng.random((N, N), dtype=np.float32) ** power
    lP = np.log(P / P.sum(1, keepdims=True) + np.float32(1e-8)).astype(np.float32)
    init = np.log(np.full(N, 1.0 / N, np.float32) + np.float32(1e-8)).astype(np.float32)
    return lP, init


@functools.lru_cache(maxsize=None)
def vit_case(N, kind, lengths=VIT_LENGTHS, T=TMAX):
    """(lo, lP, init, model states, delta, final): test_gpu_wide.py's generators, the model
    computed once per case and left unchanged."""
    B = len(lengths)
    rng = np.random.default_rng(B * 1000 + T * 7 + N)
    lo = np.log(rng.random((B, T, N), dtype=np.float32) + np.float32(1e-8)).astype(np.float32)
    lP, init = log_params(rng, N, 4)
    if kind != "random":
        # multiples of 0.5: every sum is exact, so equal candidates occur in both input halves
        lo, lP, init = ((np.round(x * 2) / 2).astype(np.float32) for x in (lo, lP, init))
    if kind == "ties_inf":
        lo[rng.random(lo.shape) < 0.1] = -np.inf
        lo[:, :, N // 3] = -np.inf
    s, d, f = rm.viterbi_from_log(lo, lP, init, lengths)
    return lo, lP, init, s, d, f


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
def fb_case(N, kind, lengths=FB_LENGTHS, T=TMAX):
    """(obs, lP, lp0, fp64 log alpha, log beta, posterior, loglik, the reference's compute_likelihood)."""
    obs, lP, lp0 = fb_inputs(len(lengths), T, N, kind)
    la, lb, post64, ll64 = rm.fb64(np.log(obs + np.float32(1e-8)), lP.numpy(), lp0.numpy(), lengths)
    lik = rm.compute_likelihood(obs, lP, lp0, lengths).numpy()
    return obs, lP, lp0, la, lb, post64, ll64, lik


def check_fb(outs, mask, lengths, la, lb, post64, ll64, lik, what=""):
    """check_fb of test_gpu_wide.py on the valid frames, exact zeros in the padded ones; every
    figure is printed before it is asserted."""
    post, fwd, bwd, loglik, lik_ref = (x.detach().cpu().numpy().astype(np.float64) for x in outs)
    val = valid_mask(lengths, la.shape[1])
    print(f"{what} mask {mask} loglik rel {np.abs((loglik - ll64) / ll64).max():.3e}"
          f" lik_ref max|err| {np.abs(lik_ref - lik.reshape(-1)).max():.3e}")
    np.testing.assert_allclose(loglik, ll64, rtol=2e-6)
    np.testing.assert_allclose(lik_ref, lik.reshape(-1), rtol=1e-5, atol=1e-5)
    if mask & 1:
        big = post64 > 1e-4
        rel = np.abs(post[big] - post64[big]) / post64[big] if big.any() else np.zeros(1)
        print(f"{what} posterior max|err| {np.abs(post - post64).max():.3e} max rel (>1e-4) {rel.max():.3e}")
        np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0)
        np.testing.assert_allclose(post[big], post64[big], rtol=1e-4, atol=0)
        assert np.all(post[~val] == 0)
    else:
        assert post.shape == (0,)
    for bit, ours, ref, name in ((2, fwd, np.exp(la), "forward"), (4, bwd, np.exp(lb), "backward")):
        if not mask & bit:
            assert ours.shape == (0,)
            continue
        rep = ref > 1e-30
        err = np.abs(ours[rep] - ref[rep]) / ref[rep]
        print(f"{what} {name} max rel (representable) {err.max():.3e}")
        np.testing.assert_allclose(ours[rep], ref[rep], rtol=1e-4)
        assert np.all(np.abs(ours[~rep]) < 1e-29)
        assert np.all(ours[~val] == 0)


# ------------------------------------------------------------------------------ Viterbi
@pytest.mark.parametrize("kind", ["random", "ties", "ties_inf"])
@pytest.mark.parametrize("N", STATES)
def test_viterbi_log_input_bitexact(N, kind):
    lo, lP, init, s_ref, d_ref, f_ref = vit_case(N, kind)
    if kind != "random":
        # the inputs do produce ties: some delta column has two equal best candidates
        cand = d_ref[-1, :-1, :, None].numpy() + lP[None]   # the longest sequence: (T-1, i, j)
        assert ((cand == cand.max(1, keepdims=True)).sum(1) > 1).any()
    o = ops()
    lens = torch.tensor(VIT_LENGTHS)
    states, delta, final = o.viterbi_ragged(t(lo), t(lP), t(init), o.OBS_LOG, lens)
    assert torch.equal(states.cpu(), s_ref)
    assert torch.equal(delta.cpu().view(torch.int32), d_ref.view(torch.int32))
    assert torch.equal(final.cpu(), f_ref)
    for b, n in enumerate(VIT_LENGTHS):   # and the tuned decode of the slice alone
        s1, d1, f1 = o.viterbi(t(lo[b:b + 1, :n]), t(lP), t(init), o.OBS_LOG)
        assert torch.equal(states[b, :n], s1[0]) and torch.equal(delta[b, :n], d1[0]) and torch.equal(final[b], f1[0])
        assert (states[b, n:] == -1).all() and (delta[b, n:] == float("-inf")).all()


@pytest.mark.parametrize("kind", ["random", "ties", "ties_inf"])
@pytest.mark.parametrize("N", STATES)
def test_viterbi_prob_input_bitexact(N, kind):
    lo, lP, init, _, _, _ = vit_case(N, kind)
    obs = np.exp(lo).astype(np.float32)   # probabilities (0 where the log is -inf)
    o = ops()
    states, delta, final = o.viterbi_ragged(t(obs), t(lP), t(init), o.OBS_PROB, torch.tensor(VIT_LENGTHS))
    for b, n in enumerate(VIT_LENGTHS):
        s1, d1, f1 = o.viterbi(t(obs[b:b + 1, :n]), t(lP), t(init), o.OBS_PROB)
        assert torch.equal(states[b, :n], s1[0]) and torch.equal(delta[b, :n], d1[0]) and torch.equal(final[b], f1[0])
        assert (states[b, n:] == -1).all() and (delta[b, n:] == float("-inf")).all()


# --------------------------------------------------------------------- forward-backward
@pytest.mark.parametrize("kind", ["random", "peaked", "l2r"])
@pytest.mark.parametrize("N", STATES)
def test_forward_backward_vs_fp64(N, kind):
    obs, lP, lp0, la, lb, post64, ll64, lik = fb_case(N, kind)
    o = ops()
    lens = torch.tensor(FB_LENGTHS)
    for mask in (7, 1, 0):
        outs = o.forward_backward_ragged(t(obs), t(lP), t(lp0), o.OBS_PROB, lens, mask)
        check_fb(outs, mask, FB_LENGTHS, la, lb, post64, ll64, lik, f"N={N} {kind}")


def test_forward_backward_log_input():
    """OBS_LOG: log-emissions far below the exp range are shifted by their row maximum."""
    N, lengths = 70, (1, 9, 64, 131)
    rng = np.random.default_rng(6)
    lo = (-300 + 40 * rng.standard_normal((len(lengths), TMAX, N))).astype(np.float32)
    _, lP, lp0 = fb_inputs(2, TMAX, N, "peaked")
    la, lb, post64, ll64 = rm.fb64(lo, lP.numpy(), lp0.numpy(), lengths)
    o = ops()
    post, fwd, bwd, loglik, lik_ref = o.forward_backward_ragged(t(lo), t(lP), t(lp0), o.OBS_LOG,
                                                                torch.tensor(lengths), 7)
    for x in (post, fwd, bwd, loglik, lik_ref):
        assert torch.isfinite(x).all()
    post, loglik = post.cpu().numpy().astype(np.float64), loglik.cpu().numpy().astype(np.float64)
    big = post64 > 1e-4
    print(f"OBS_LOG posterior max|err| {np.abs(post - post64).max():.3e} max rel (>1e-4) "
          f"{(np.abs(post[big] - post64[big]) / post64[big]).max():.3e} loglik rel {np.abs((loglik - ll64) / ll64).max():.3e}")
    np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0)
    np.testing.assert_allclose(post[big], post64[big], rtol=1e-4, atol=0)
    np.testing.assert_allclose(loglik, ll64, rtol=2e-6)
    assert np.all(post[~valid_mask(lengths, TMAX)] == 0)


def test_long_sequence():
    """2000 steps of scaling at N = 128, left-to-right 0.7."""
    lengths, T, N = (1, 777, 2000), 2000, 128
    obs, lP, lp0, la, lb, post64, ll64, lik = fb_case(N, "l2r", lengths, T)
    o = ops()
    outs = o.forward_backward_ragged(t(obs), t(lP), t(lp0), o.OBS_PROB, torch.tensor(lengths), 7)
    check_fb(outs, 7, lengths, la, lb, post64, ll64, lik, "long N=128")


# ----------------------------------------------------------------- padding independence
@pytest.mark.parametrize("mode", ["log", "prob"])
def test_viterbi_ignores_the_padding(mode):
    lo, lP, init, _, _, _ = vit_case(70, "random")
    o = ops()
    x, m = (lo, o.OBS_LOG) if mode == "log" else (np.exp(lo).astype(np.float32), o.OBS_PROB)
    lens = torch.tensor(VIT_LENGTHS)
    want = o.viterbi_ragged(t(x), t(lP), t(init), m, lens)
    again = o.viterbi_ragged(t(x), t(lP), t(init), m, lens)
    for a, b in zip(want, again):
        assert torch.equal(a, b)
    for value in (np.nan, 1e30):
        got = o.viterbi_ragged(t(fill_padding(x, VIT_LENGTHS, value)), t(lP), t(init), m, lens)
        for a, b in zip(want, got):
            assert torch.equal(a, b)


@pytest.mark.parametrize("mode", ["prob", "log"])
def test_forward_backward_ignores_the_padding(mode):
    obs, lP, lp0 = fb_case(70, "random")[:3]
    o = ops()
    x, m = (obs, o.OBS_PROB) if mode == "prob" else (np.log(obs + np.float32(1e-8)), o.OBS_LOG)
    lens = torch.tensor(FB_LENGTHS)
    want = o.forward_backward_ragged(t(x), t(lP), t(lp0), m, lens, 7)
    again = o.forward_backward_ragged(t(x), t(lP), t(lp0), m, lens, 7)
    for a, b in zip(want, again):
        assert torch.equal(a, b)
    for value in (np.nan, 1e30):
        got = o.forward_backward_ragged(t(fill_padding(x, FB_LENGTHS, value)), t(lP), t(lp0), m, lens, 7)
        for a, b in zip(want, got):
            assert torch.isfinite(b).all() and torch.equal(a, b)


# ----------------------------------------------------------------------------- dispatch
def test_equal_lengths_take_the_tuned_path():
    from pytorch_hmm_amd import HMMPyTorch
    B, T, N = 3, 40, 70
    obs, lP, lp0 = fb_inputs(B, T, N, "l2r")
    hmm = HMMPyTorch(O.left_to_right_matrix(N, 0.7))
    x = t(obs)
    full = [T] * B
    for a, b in zip(hmm.forward_backward(x), hmm.forward_backward(x, lengths=full)):
        assert torch.equal(a, b)
    for a, b in zip(hmm.viterbi_decode(x), hmm.viterbi_decode(x, lengths=torch.tensor(full, device=DEV))):
        assert torch.equal(a, b)
    assert torch.equal(hmm.posteriors(x), hmm.posteriors(x, lengths=np.array(full)))
    assert torch.equal(hmm.compute_likelihood(x), hmm.compute_likelihood(x, lengths=full))
    assert torch.equal(hmm.log_likelihood(x), hmm.log_likelihood(x, lengths=full))
    # one common shorter length (B == 1 included): the tuned ops on the slice, padded
    o = ops()
    L0 = 17
    for rows in (slice(0, B), slice(0, 1)):
        xs = x[rows]
        n = xs.shape[0]
        s, d, f = o.viterbi_ragged(xs, t(lP), t(lp0), o.OBS_PROB, torch.tensor([L0] * n))
        s1, d1, f1 = o.viterbi(xs[:, :L0], t(lP), t(lp0), o.OBS_PROB)
        assert torch.equal(s[:, :L0], s1) and torch.equal(d[:, :L0], d1) and torch.equal(f, f1)
        assert (s[:, L0:] == -1).all() and (d[:, L0:] == float("-inf")).all()
        outs = o.forward_backward_ragged(xs, t(lP), t(lp0), o.OBS_PROB, torch.tensor([L0] * n), 7)
        ref = o.forward_backward(xs[:, :L0], t(lP), t(lp0), o.OBS_PROB, 7)
        for a, b in zip(outs[:3], ref[:3]):
            assert torch.equal(a[:, :L0], b) and (a[:, L0:] == 0).all()
        assert torch.equal(outs[3], ref[3]) and torch.equal(outs[4], ref[4])


# ---------------------------------------------------------------------------- gradients
GRAD_LENGTHS = (1, 9, 30)
GRAD_T = 33


def close(a, b, rel=1e-4):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    print(f"max|diff| {np.abs(a - b).max():.3e} scale {scale:.3e}")
    assert np.abs(a - b).max() <= rel * scale, (np.abs(a - b).max(), scale)


def grad_inputs(N):
    rng = np.random.default_rng(GRAD_T * N)
    P = O.left_to_right_matrix(N, 0.7) if N != 70 else torch.from_numpy(rng.random((N, N), dtype=np.float32))
    lP, lp0 = O.hmm_params(P)
    obs = torch.from_numpy(rng.random((len(GRAD_LENGTHS), GRAD_T, N), dtype=np.float32) * 0.9 + 0.1)
    return obs, lP, lp0


def log_alpha64(lo, lP, lp0):
    la = [lp0 + lo[:, 0]]
    for k in range(1, lo.shape[1]):
        la.append(torch.logsumexp(la[-1][:, :, None] + lP[None], dim=1) + lo[:, k])
    return la


def oracle_grads(obs, lP, lp0, kind, lengths):
    """test_gpu_autograd.py oracle_grads on each slice: float64 autograd through the reference's
    loops (hmm.py:89-101), the loss sum_b w_b ll_b."""
    obs = obs.double().requires_grad_(True)
    lP = lP.double().requires_grad_(True)
    lp0 = lp0.double().requires_grad_(True)
    B = obs.shape[0]
    w = torch.linspace(0.5, 1.5, B, dtype=torch.float64)
    lls = []
    for b, n in enumerate(lengths):
        a = log_alpha64(torch.log(obs[b:b + 1, :n] + 1e-8), lP, lp0)[-1]
        lls.append(torch.logsumexp(torch.log(torch.exp(a) + 1e-8) if kind == "ref" else a, dim=-1)[0])
    ll = torch.stack(lls)
    (ll * w).sum().backward()
    return ll.detach(), obs.grad, lP.grad, lp0.grad, w


@pytest.mark.parametrize("pad", ["data", "nan"])
@pytest.mark.parametrize("kind", ["ref", "exact"])
@pytest.mark.parametrize("N", [5, 70, 200])
def test_loglik_gradients(N, kind, pad):
    from pytorch_hmm_amd.autograd import SequenceLogLik
    o = ops()
    obs, lP, lp0 = grad_inputs(N)
    ll_ref, g_obs, g_lP, g_lp0, w = oracle_grads(obs, lP, lp0, kind, GRAD_LENGTHS)
    x = obs if pad == "data" else torch.from_numpy(fill_padding(obs.numpy(), GRAD_LENGTHS, np.nan))
    x = x.to(DEV).requires_grad_(True)
    P_ = lP.to(DEV).requires_grad_(True)
    p0 = lp0.to(DEV).requires_grad_(True)
    lens = o.ragged_lengths(list(GRAD_LENGTHS), len(GRAD_LENGTHS), GRAD_T, N)
    ll = SequenceLogLik.apply(x, P_, p0, o.OBS_PROB, kind, None, lens)
    (ll * w.float().to(DEV)).sum().backward()
    np.testing.assert_allclose(ll.detach().cpu().numpy(), ll_ref.numpy(), rtol=2e-5, atol=2e-5)
    for g in (x.grad, P_.grad, p0.grad):
        assert torch.isfinite(g).all()
    assert (x.grad.cpu()[torch.from_numpy(~valid_mask(GRAD_LENGTHS, GRAD_T))] == 0).all()
    close(x.grad.cpu(), g_obs)
    close(P_.grad.cpu(), g_lP)
    close(p0.grad.cpu(), g_lp0)


def posterior64(lo, lP, lp0):
    """hmm.py:86-130 in float64 autograd (test_gpu_autograd.py fb_ref64), the posterior only."""
    B, T, K = lo.shape
    la = log_alpha64(lo, lP, lp0)
    lb = [torch.zeros(B, K, dtype=lo.dtype)]
    for k in range(T - 2, -1, -1):
        lb.insert(0, torch.logsumexp(lP[None] + lo[:, k + 1, None, :] + lb[0][:, None, :], dim=2))
    lp = torch.stack(la, 1) + torch.stack(lb, 1)
    return torch.exp(lp - torch.logsumexp(lp, dim=-1, keepdim=True))


@pytest.mark.parametrize("pad", ["data", "nan"])
@pytest.mark.parametrize("N", [16, 70])
def test_masked_posterior_loss_gradients(N, pad):
    from pytorch_hmm_amd import HMMPyTorch
    rng = np.random.default_rng(N)
    B = len(GRAD_LENGTHS)
    P = torch.softmax(torch.randn(N, N, generator=torch.Generator().manual_seed(N)), -1)
    obs = torch.from_numpy(rng.random((B, GRAD_T, N), dtype=np.float32) * 0.9 + 0.1)
    val = torch.from_numpy(valid_mask(GRAD_LENGTHS, GRAD_T))
    Gp = torch.from_numpy(rng.standard_normal((B, GRAD_T, N)).astype(np.float32)) * val[..., None]
    # float64 reference: the loss sum Gp * posterior over the valid frames, per slice
    hmm64 = HMMPyTorch(P)
    lP64 = hmm64.log_P.double().requires_grad_(True)
    lp064 = hmm64.log_p0.double().requires_grad_(True)
    o64 = obs.double().requires_grad_(True)
    loss = 0
    for b, n in enumerate(GRAD_LENGTHS):
        loss = loss + (posterior64(torch.log(o64[b:b + 1, :n] + 1e-8), lP64, lp064) * Gp[b:b + 1, :n].double()).sum()
    loss.backward()

    hmm = HMMPyTorch(P).to(DEV)
    hmm.log_P.requires_grad_(True)
    hmm.log_p0.requires_grad_(True)
    x = obs if pad == "data" else torch.from_numpy(fill_padding(obs.numpy(), GRAD_LENGTHS, np.nan))
    x = x.to(DEV).requires_grad_(True)
    post = hmm.posteriors(x, lengths=list(GRAD_LENGTHS))
    assert (post[~val.to(DEV)] == 0).all()
    (post * Gp.to(DEV)).sum().backward()
    for g in (x.grad, hmm.log_P.grad, hmm.log_p0.grad):
        assert torch.isfinite(g).all()
    assert (x.grad.cpu()[~val] == 0).all()
    close(x.grad.cpu(), o64.grad)
    close(hmm.log_P.grad.cpu(), lP64.grad)
    close(hmm.log_p0.grad.cpu(), lp064.grad)


# ------------------------------------------------------------------------------- layers
def test_hmmlayer_training_step_with_lengths():
    import pytorch_hmm_amd as ph
    torch.manual_seed(0)
    layer = ph.HMMLayer(5).to(DEV)
    obs = torch.rand(3, 10, 5, device=DEV)
    lengths = [10, 4, 1]
    opt = torch.optim.Adam(layer.parameters(), lr=0.01)
    before = layer.get_transition_matrix().detach().clone()
    layer.train()
    loss = layer.compute_loss(obs, lengths=lengths)
    opt.zero_grad()
    loss.backward()
    assert torch.isfinite(loss)
    assert layer.log_transition_logits.grad is not None and torch.isfinite(layer.log_transition_logits.grad).all()
    assert layer.log_initial_logits.grad is not None and torch.isfinite(layer.log_initial_logits.grad).all()
    opt.step()
    assert not torch.allclose(before, layer.get_transition_matrix())
    # the supervised branch: cross-entropy over the valid frames only, whatever the padding holds
    target = torch.randint(0, 5, (3, 10), device=DEV)
    val = torch.from_numpy(valid_mask(lengths, 10)).to(DEV)
    l1 = layer.compute_loss(obs, target, lengths=lengths)
    l2 = layer.compute_loss(torch.where(val[..., None], obs, torch.full_like(obs, float("nan"))),
                            torch.where(val, target, torch.zeros_like(target)), lengths=lengths)
    assert torch.isfinite(l1) and torch.equal(l1, l2)
    l1.backward()
    assert torch.isfinite(layer.log_transition_logits.grad).all()


def test_hmmlayer_eval_forward_with_lengths():
    import pytorch_hmm_amd as ph
    torch.manual_seed(1)
    layer = ph.HMMLayer(5).to(DEV).eval()
    x = torch.randn(3, 12, 5, device=DEV)
    lengths = [12, 5, 1]
    val = torch.from_numpy(valid_mask(lengths, 12)).to(DEV)
    with torch.no_grad():
        post, ali = layer(x, return_alignment=True, lengths=lengths)
        states, delta = layer.align(x, lengths=lengths)
    assert torch.equal(ali, states)
    assert (ali[~val] == -1).all() and (ali[val] >= 0).all()
    assert (post[~val] == 0).all() and (post[val].sum(-1) == 1).all()
    assert torch.equal(post[val].argmax(-1), ali[val])
    for b, n in enumerate(lengths):   # each sequence decodes as it does alone
        with torch.no_grad():
            _, a1 = layer(x[b:b + 1, :n], return_alignment=True)
        assert torch.equal(a1[0], ali[b, :n])


def test_gaussian_layer_passes_lengths():
    import pytorch_hmm_amd as ph
    torch.manual_seed(2)
    layer = ph.GaussianHMMLayer(6, 4).to(DEV)
    x = torch.randn(2, 9, 4, device=DEV)
    lengths = [9, 3]
    layer.train()
    loss = layer.compute_loss(torch.where(torch.from_numpy(valid_mask(lengths, 9)).to(DEV)[..., None], x,
                                          torch.full_like(x, float("nan"))), lengths=lengths)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(layer.means.grad).all()
    with torch.no_grad():
        post = layer(x, lengths=lengths)
    assert (post[1, 3:] == 0).all() and torch.allclose(post[1, :3].sum(-1), torch.ones(3, device=DEV), atol=1e-5)


def test_mixture_layer_with_lengths_is_the_layer_on_each_slice():
    from pytorch_hmm_amd import MixtureGaussianHMMLayer
    torch.manual_seed(3)
    layer = MixtureGaussianHMMLayer(16, 8, 2).to(DEV).eval()
    lengths = [40, 17, 1, 33]
    x = torch.randn(len(lengths), 40, 8, device=DEV)
    states, scores = layer(x, return_log_probs=True, lengths=lengths)
    for b, n in enumerate(lengths):
        s1, sc1 = layer(x[b:b + 1, :n], return_log_probs=True)
        assert torch.equal(states[b, :n], s1[0]) and (states[b, n:] == -1).all()
        assert torch.equal(scores[b], sc1[0])
