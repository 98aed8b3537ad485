"""GPU: Baum-Welch on the device -- the statistics kernel (csrc/emstats.hip through ops.gmm_stats and
the C entry), em.e_step and the layers' em_step / fit / log_likelihood / reestimate -- against the
fp64 NumPy model tests/em_numpy.py.

Kernel tolerance.  For each output the model also returns A = the sum of its terms' magnitudes; the
kernel's error is E = max |got - want| / A and the bound is max(2 * E32, 2^-22), E32 the same
quantity for the model file's fp32 restatement on the same inputs (two fp32-quality evaluations
differ by about a factor 2 in their maxima over a few thousand outputs; the floor covers inputs
where the restatement happens to be exact).  Each case prints its E and E32.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_numpy as emn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 2.0 ** -22


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def make_case(seed, B, T, S, C, D, signed=False):
    """fp32 inputs with the frames drawn near the components; the components lie about two
    standard deviations apart whatever D is, so every component takes a share of some frames."""
    rng = np.random.default_rng(seed)
    means = f32(rng.normal(size=(S, C, D)) * 2.0 / np.sqrt(D))
    log_vars = f32(rng.normal(size=(S, C, D)) * 0.3)
    log_w = f32(np.log(rng.dirichlet(np.ones(C) * 2, S)))
    pick = rng.integers(0, S * C, size=(B, T))
    x = f32(means.reshape(-1, D)[pick] + np.exp(0.5 * log_vars.reshape(-1, D)[pick]) * rng.normal(size=(B, T, D)))
    weight = f32(rng.normal(size=(B, T, S)) if signed else rng.random((B, T, S)) + 0.05)
    return x, weight, means, log_vars, log_w


def gpu_stats(x, weight, means, log_vars, log_w, mix, lengths=None):
    from pytorch_hmm_amd import ops
    out = ops.gmm_stats(dev(x), dev(weight), dev(means), dev(log_vars), dev(log_w), mix,
                        None if lengths is None else torch.as_tensor(lengths))
    return [o.cpu().numpy() for o in out]


def check_against_model(tag, x, weight, means, log_vars, log_w, mix, lengths):
    want, A = emn.gmm_stats(x, weight, means, log_vars, log_w, mix, lengths)
    ref32 = emn.gmm_stats_f32(x, weight, means, log_vars, log_w, mix, lengths)
    got = gpu_stats(x, weight, means, log_vars, log_w, mix, lengths)
    for name, g, w, a, r in zip(("occ", "sx", "sxx"), got, want, A, ref32):
        assert (a > 0).all(), (tag, name)
        E, E32 = emn.relative_error(g, w, a), emn.relative_error(r, w, a)
        print(f"emstats {tag} {name}: E = {E:.3e}  E32 = {E32:.3e}")
        assert np.isfinite(g).all()
        assert E <= max(2 * E32, FLOOR), (tag, name, E, E32)


SC = [(5, 1), (16, 4), (22, 3), (65, 4)]
# 96 | 97: the dim split of the 64-lane groups (4 lane groups x 3 chunks x 8 dims per blockIdx.z)
DIMS = [1, 7, 8, 9, 80, 96, 97]
RAGGED = (3, 70, (70, 1, 33))


@pytest.mark.parametrize("S,C", SC)
@pytest.mark.parametrize("D", DIMS)
def test_kernel_matches_model_over_shapes(S, C, D):
    B, T, lengths = RAGGED
    x, weight, means, log_vars, log_w = make_case(100 + S + D, B, T, S, C, D)
    check_against_model(f"S{S} C{C} D{D} ragged", x, weight, means, log_vars, log_w, 1, lengths)


# 170 frames = 6 tiles of 32: two spans of 4 tiles (the least a span holds), the second partly filled
@pytest.mark.parametrize("S,C", SC)
@pytest.mark.parametrize("F", [1, 63, 64, 65, 170])
def test_kernel_matches_model_over_frame_counts(S, C, F):
    x, weight, means, log_vars, log_w = make_case(200 + S + F, 1, F, S, C, 9, signed=True)
    check_against_model(f"S{S} C{C} D9 F{F}", x, weight, means, log_vars, log_w, 1, None)


# wider components: 128 lanes (2 lane groups, split at 48 dims) and 256 lanes (1 group, 24 dims)
@pytest.mark.parametrize("S,C,D", [(2, 70, 48), (2, 70, 49), (1, 130, 24), (1, 130, 25), (3, 256, 9)])
def test_kernel_matches_model_wide_components(S, C, D):
    B, T, lengths = RAGGED
    x, weight, means, log_vars, log_w = make_case(300 + C + D, B, T, S, C, D)
    check_against_model(f"S{S} C{C} D{D} ragged", x, weight, means, log_vars, log_w, 1, lengths)


def test_single_gaussian_mode():
    """mix_lse == 0 (C == 1): r = 1 whatever log_w holds."""
    B, T, lengths = RAGGED
    x, weight, means, log_vars, log_w = make_case(400, B, T, 7, 1, 13)
    check_against_model("S7 C1 D13 mix0", x, weight, means, log_vars, np.zeros_like(log_w), 0, lengths)


# ------------------------------------------------------------------------- exact cases
def test_dyadic_inputs_are_bit_exact():
    rng = np.random.default_rng(1)
    B, T, S, D = 2, 100, 5, 11
    means = f32(rng.integers(-3, 4, size=(S, 1, D)))
    log_vars = f32(rng.normal(size=(S, 1, D)))
    z = rng.integers(0, S, size=(B, T))
    x = f32(means[z, 0] + rng.integers(-2, 3, size=(B, T, D)))
    weight = f32(rng.integers(-8, 9, size=(B, T, S)) / 8.0)
    weight[..., 3] = 0.0                                   # a state with all-zero weight
    want, _ = emn.gmm_stats(x, weight, means, log_vars, None, 1)
    for mix in (0, 1):
        got = gpu_stats(x, weight, means, log_vars, np.zeros((S, 1)), mix)
        for g, w in zip(got, want):
            assert (g == w.astype(np.float32)).all() and (w == w.astype(np.float32)).all()
        assert (got[0][3] == 0).all() and (got[1][3] == 0).all() and (got[2][3] == 0).all()


def test_dead_component_gives_exact_zeros():
    x, weight, means, log_vars, log_w = make_case(2, 2, 50, 6, 3, 10)
    log_w[2, 1] = -np.inf
    log_w[4, :] = -np.inf                                  # a whole state without a live component
    got = gpu_stats(x, weight, means, log_vars, log_w, 1)
    for g in got:
        assert np.isfinite(g).all()
        assert (g[2, 1] == 0).all() and (g[4] == 0).all()
    with np.errstate(divide="ignore"):
        want, A = emn.gmm_stats(x, weight, means, log_vars, log_w, 1)
    live = np.ones((6, 3), dtype=bool)
    live[2, 1] = False
    live[4] = False
    for g, w, a in zip(got, want, A):
        assert emn.relative_error(g[live], w[live], a[live]) <= 1e-5
    # one component per state with log_w = -inf and the mixture rule: r = 0
    got1 = gpu_stats(x, weight, means[:, :1], log_vars[:, :1], np.array([[0], [-np.inf]] * 3, dtype=np.float32), 1)
    assert all((g[1::2] == 0).all() and np.isfinite(g).all() for g in got1) and (got1[0][0::2] != 0).all()


def test_far_frame_has_finite_responsibilities():
    S, C, D = 4, 3, 6
    _, _, means, log_vars, log_w = make_case(3, 1, 1, S, C, D)
    x = np.full((1, 1, D), 1e4, dtype=np.float32)          # every comp is about -5e7 * D
    weight = np.ones((1, 1, S), dtype=np.float32)
    occ, sx, sxx = gpu_stats(x, weight, means, log_vars, log_w, 1)
    assert np.isfinite(occ).all() and np.isfinite(sx).all() and np.isfinite(sxx).all()
    assert (occ >= 0).all() and np.abs(occ.sum(-1) - 1).max() <= 1e-6
    want, _ = emn.gmm_stats(x, weight, means, log_vars, log_w, 1)
    assert np.abs(occ - want[0]).max() <= 1e-5


# ----------------------------------------------------------------------------- padding
def test_padding_is_never_read():
    B, T, lengths = RAGGED
    x, weight, means, log_vars, log_w = make_case(4, B, T, 22, 3, 9)
    xn, wn = x.copy(), weight.copy()
    for b, n in enumerate(lengths):
        xn[b, n:] = np.nan
        wn[b, n:] = np.nan
    got = gpu_stats(xn, wn, means, log_vars, log_w, 1, lengths)
    assert all(np.isfinite(g).all() for g in got)
    # the truncated sequences, concatenated: the same frames in the same tiles only when nothing
    # is dropped in between, so compare with zero-weight clean padding, and with each sequence alone
    clean = gpu_stats(x, weight, means, log_vars, log_w, 1, lengths)
    for g, c in zip(got, clean):
        assert (g == c).all()
    one = gpu_stats(xn[1:2, :1], wn[1:2, :1], means, log_vars, log_w, 1)
    pad1 = gpu_stats(xn[1:2], wn[1:2], means, log_vars, log_w, 1, [1])
    for a, b in zip(one, pad1):
        assert (a == b).all()
    full = gpu_stats(xn[:1], wn[:1], means, log_vars, log_w, 1, [70])
    nolen = gpu_stats(x[:1], weight[:1], means, log_vars, log_w, 1)
    for a, b in zip(full, nolen):
        assert (a == b).all()
    cut = gpu_stats(xn[2:, :33], wn[2:, :33], means, log_vars, log_w, 1)
    pad = gpu_stats(xn[2:], wn[2:], means, log_vars, log_w, 1, [33])
    for a, b in zip(cut, pad):
        assert (a == b).all()


# --------------------------------------------------------------------- reproducibility
def test_reproducible_across_calls_streams_and_null_outputs():
    from pytorch_hmm_amd import _native as nat
    B, T, S, C, D = 2, 300, 22, 3, 17
    x, weight, means, log_vars, log_w = make_case(5, B, T, S, C, D)
    t = [dev(a) for a in (x, weight, means, log_vars, log_w)]
    L = nat.lib()
    need = L.hmm355_gmm_stats_workspace_bytes(B, T, D, S, C)
    assert 0 < need < 64 << 20

    def call(want=(True, True, True), stream=None):
        outs = [torch.full(shape, float("nan"), device=DEV) for shape in ((S, C), (S, C, D), (S, C, D))]
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        st = torch.cuda.current_stream() if stream is None else stream
        with torch.cuda.stream(st):
            rc = L.hmm355_gmm_stats_f32(*[nat.ptr(a) for a in t], None, B, T, D, S, C, 1,
                                        *[nat.ptr(o) if w else None for o, w in zip(outs, want)],
                                        nat.ptr(ws), need, ctypes.c_void_p(st.cuda_stream))
        assert rc == 0
        st.synchronize()
        return [o.cpu().numpy() for o in outs]

    first = call()
    assert all(np.isfinite(o).all() for o in first)
    for other in (call(), call(stream=torch.cuda.Stream())):
        for a, b in zip(first, other):
            assert (a == b).all()
    for want in ((True, False, False), (False, True, False), (False, False, True)):
        got = call(want)
        for a, b, w in zip(first, got, want):
            assert (a == b).all() if w else np.isnan(b).all()
    from pytorch_hmm_amd import ops
    via_op = ops.gmm_stats(*t, 1)
    for a, b in zip(first, via_op):
        assert (a == b.cpu().numpy()).all()


# ------------------------------------------------------------------------------ e_step
def left_to_right(rng, N):
    P = np.zeros((N, N))
    for i in range(N):
        hi = min(N, i + 3)
        P[i, i:hi] = rng.dirichlet(np.ones(hi - i) * 2)
    return f32(P)


@pytest.mark.parametrize("N", [5, 64, 65, 200])
@pytest.mark.parametrize("T", [1, 2, 70])
@pytest.mark.parametrize("ragged", [False, True])
def test_e_step_matches_model(N, T, ragged):
    from pytorch_hmm_amd import em
    rng = np.random.default_rng(N * 100 + T)
    B = 3
    P = left_to_right(rng, N)
    with np.errstate(divide="ignore"):
        log_P = f32(np.log(P))
    log_p0 = f32(np.log(rng.dirichlet(np.ones(N))))
    le = f32(rng.normal(size=(B, T, N)) * 2 - 3)
    lengths = None
    if ragged:
        lengths = np.array([T, 1, max(1, T // 2)])
        for b, n in enumerate(lengths):
            le[b, n:] = np.nan
    es = em.e_step(dev(le), dev(log_P), dev(log_p0), lengths)
    want_ll, want_g, want_xi, want_g0 = emn.forward_backward(np.nan_to_num(le), log_P, log_p0, lengths)
    assert es.n_seq == B
    assert np.abs(es.loglik.cpu().numpy() - want_ll).max() <= 2e-6 * np.abs(want_ll).max()
    assert np.abs(es.gamma.cpu().numpy() - want_g).max() <= 2e-5
    xi = es.xi.cpu().numpy()
    assert np.abs(xi - want_xi).max() <= 2e-5 * max(want_xi.sum(), 1e-30)
    assert np.abs(es.gamma0.cpu().numpy() - want_g0).max() <= 2e-5 * want_g0.sum()
    assert (xi[P == 0] == 0).all()
    if T == 1:
        assert (xi == 0).all()


def test_estats_add_up_over_half_batches():
    from pytorch_hmm_amd import em
    rng = np.random.default_rng(9)
    B, T, N = 4, 70, 65
    P = left_to_right(rng, N)
    with np.errstate(divide="ignore"):
        log_P = dev(np.log(P))
    log_p0 = dev(np.log(rng.dirichlet(np.ones(N))))
    le = dev(rng.normal(size=(B, T, N)) * 2)
    lengths = torch.tensor([70, 12, 70, 41])
    whole = em.e_step(le, log_P, log_p0, lengths)
    halves = em.e_step(le[:2], log_P, log_p0, lengths[:2]) + em.e_step(le[2:], log_P, log_p0, lengths[2:])
    assert halves.n_seq == whole.n_seq == B and halves.gamma is None
    for a, b in ((halves.xi, whole.xi), (halves.gamma0, whole.gamma0), (halves.loglik, whole.loglik)):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# -------------------------------------------------------------------------- end to end
S_, C_, D_, B_, T_ = 6, 3, 12, 4, 60
LENS = np.array([60, 47, 9, 60])


def e2e_data(seed=11):
    """Data from one Gaussian-mixture HMM and the (different) starting parameters of the fits."""
    rng = np.random.default_rng(seed)
    true_means = rng.normal(size=(S_, C_, D_)) * 0.8
    true_P = np.full((S_, S_), 0.04) + 0.76 * np.eye(S_)
    x = emn.sample_gmm_hmm(rng, B_, T_, true_P, np.full(S_, 1 / S_), true_means, 1.0, np.full((S_, C_), 1 / C_))
    init = {"means": f32(true_means + 0.5 * rng.normal(size=(S_, C_, D_))),
            "trans": f32(rng.normal(size=(S_, S_)) * 0.3), "init": f32(rng.normal(size=S_) * 0.3),
            "wlog": f32(rng.normal(size=(S_, C_)) * 0.3)}
    return f32(x), init


def log_softmax64(a, axis=-1):
    a = np.asarray(a, dtype=np.float64)
    m = a.max(axis, keepdims=True)
    return a - m - np.log(np.exp(a - m).sum(axis, keepdims=True))


def gaussian_layer(cov, init):
    from pytorch_hmm_amd import GaussianHMMLayer
    layer = GaussianHMMLayer(S_, D_, covariance_type=cov, transition_type="ergodic").to(DEV)
    with torch.no_grad():
        layer.means.copy_(dev(init["means"][:, 0]))
        layer.hmm_layer.log_transition_logits.copy_(dev(init["trans"]))
        layer.hmm_layer.log_initial_logits.copy_(dev(init["init"]))
    return layer


def mixture_layer(cov, init):
    from pytorch_hmm_amd import MixtureGaussianHMMLayer
    layer = MixtureGaussianHMMLayer(S_, D_, C_, covariance_type=cov).to(DEV)
    with torch.no_grad():
        layer.means.copy_(dev(init["means"]))
        layer.transition_logits.copy_(dev(init["trans"]))
        layer.mixture_weights_logits.copy_(dev(init["wlog"]))
    return layer


def close(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert np.allclose(got, want, rtol=1e-4, atol=1e-5), (what, np.abs(got - want).max())


@pytest.mark.parametrize("cov", ["diag", "spherical"])
def test_gaussian_layer_em_step_matches_model(cov):
    x, init = e2e_data()
    layer = gaussian_layer(cov, init)
    lv0 = np.zeros((S_, 1, D_)) if cov == "diag" else np.zeros((S_, 1))
    want = emn.em_iteration(x, LENS, log_softmax64(init["trans"]), log_softmax64(init["init"]),
                            init["means"][:, :1], lv0, np.zeros((S_, 1)), cov, mix_lse=0)
    ll = layer.em_step(dev(x), LENS)
    assert abs(ll - want["loglik"]) <= 2e-6 * abs(want["loglik"])
    close(layer.hmm_layer.get_transition_matrix(), want["P"], "P")
    close(layer.hmm_layer.get_initial_probabilities(), want["p0"], "p0")
    close(layer.means, want["means"][:, 0], "means")
    close(torch.exp(2 * layer.log_scales), np.exp(want["log_vars"]).reshape(layer.log_scales.shape), "variances")


@pytest.mark.parametrize("cov", ["diag", "tied", "spherical"])
def test_mixture_layer_em_step_matches_model(cov):
    x, init = e2e_data()
    layer = mixture_layer(cov, init)
    lv0 = {"diag": np.zeros((S_, C_, D_)), "tied": np.zeros(D_), "spherical": np.zeros((S_, C_))}[cov]
    log_w = np.log(np.maximum(np.exp(log_softmax64(init["wlog"])), 1e-8))
    want = emn.em_iteration(x, LENS, log_softmax64(init["trans"]), np.full(S_, -np.log(S_)), init["means"], lv0,
                            log_w, cov, mix_lse=1)
    ll_before = layer.log_likelihood(dev(x), LENS)
    ll = layer.em_step(dev(x), LENS)
    assert abs(ll - want["loglik"]) <= 2e-6 * abs(want["loglik"])
    assert np.abs(ll_before.cpu().numpy() - want["logliks"]).max() <= 2e-6 * np.abs(want["logliks"]).max()
    close(layer.get_transition_matrix(), want["P"], "P")
    close(layer.means, want["means"], "means")
    close(torch.exp(layer.log_vars), np.exp(want["log_vars"]), "variances")
    close(torch.softmax(layer.mixture_weights_logits, -1), want["weights"], "weights")


def model_fit(x, init, mixture, n_iter):
    """The fp64 model's logliks over n_iter iterations from the layers' starting point."""
    log_P = log_softmax64(init["trans"])
    log_p0 = np.full(S_, -np.log(S_)) if mixture else log_softmax64(init["init"])
    means = init["means"] if mixture else init["means"][:, :1]
    C = means.shape[1]
    lv = np.zeros((S_, C, D_))
    w = np.exp(log_softmax64(init["wlog"])) if mixture else np.ones((S_, 1))
    hist = []
    for _ in range(n_iter):
        out = emn.em_iteration(x, LENS, log_P, log_p0, means, lv, np.log(w), "diag", mix_lse=int(mixture))
        hist.append(out["loglik"])
        log_P = np.log(np.maximum(out["P"], 1e-30))
        if not mixture:
            log_p0 = np.log(np.maximum(out["p0"], 1e-30))
        means, lv, w = out["means"], out["log_vars"], out["weights"]
    return hist


@pytest.mark.parametrize("mixture", [False, True])
def test_fit_raises_the_loglikelihood_and_refreshes_the_decode(mixture):
    x, init = e2e_data()
    want = model_fit(x, init, mixture, 8)
    # the data are chosen so that the fp64 model alone satisfies both conditions
    assert all(b >= a - 2e-6 * abs(a) for a, b in zip(want, want[1:])) and want[-1] > want[0]
    make = mixture_layer if mixture else gaussian_layer
    layer = make("diag", init).eval()
    xd = dev(x)
    decode = (lambda m: m(xd, True, LENS)) if mixture else (lambda m: (m(xd, lengths=LENS), None))
    before = decode(layer)                                    # fills the layers' cached tables
    hist = layer.fit(xd, LENS, n_iter=8, tol=-1.0)
    print("fit logliks", "mixture" if mixture else "gaussian", hist, "model", want)
    assert len(hist) == 8
    assert all(b >= a - 2e-6 * abs(a) for a, b in zip(hist, hist[1:])), hist
    assert hist[-1] > hist[0]
    assert abs(hist[0] - want[0]) <= 2e-6 * abs(want[0])
    # forward() decodes with the updated parameters: the same as a fresh layer holding them (its
    # second call: HMMLayer's first call renormalises P)
    fresh = make("diag", init).eval()
    fresh.load_state_dict(layer.state_dict())
    decode(fresh)
    after, other = decode(layer), decode(fresh)
    assert torch.equal(after[0], other[0])
    if mixture:
        assert torch.equal(after[1], other[1]) and not torch.equal(after[1], before[1])
    # tol stops the iterations: nothing gains 1e9 per frame
    assert len(make("diag", init).fit(xd, LENS, n_iter=8, tol=1e9)) == 2


@pytest.mark.parametrize("mixture", [False, True])
def test_list_of_batches_equals_their_concatenation(mixture):
    x, init = e2e_data()
    make = mixture_layer if mixture else gaussian_layer
    a, b = make("diag", init), make("diag", init)
    xd = dev(x)
    la = a.fit([(xd[:1], LENS[:1]), (xd[1:], LENS[1:])], n_iter=1)
    lb = b.em_step(xd, LENS)
    assert abs(la[0] - lb) <= 1e-5 * abs(lb)
    for (name, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert float((p - q).abs().max()) <= 1e-5 * max(1.0, float(q.abs().max())), name


def test_reestimate_matches_model_and_leaves_the_object_alone():
    from pytorch_hmm_amd import HMMPyTorch
    rng = np.random.default_rng(13)
    K, B, T = 7, 3, 50
    P = left_to_right(rng, K)
    p0 = f32(rng.dirichlet(np.ones(K)))
    hmm = HMMPyTorch(torch.tensor(P), torch.tensor(p0), device=DEV)
    obs = f32(rng.random((B, T, K)))
    lengths = np.array([50, 20, 1])
    keep = [t.clone() for t in (hmm.P, hmm.p0, hmm.log_P, hmm.log_p0)]
    newP, newp0, ll = hmm.reestimate(dev(obs), lengths)
    le = np.log(obs.astype(np.float64) + 1e-8)
    want_ll, _, xi, g0 = emn.forward_backward(le, hmm.log_P.cpu().numpy(), hmm.log_p0.cpu().numpy(), lengths)
    wantP, wantp0 = emn.transition_m_step(xi, g0, B, hmm.P.cpu().numpy(), hmm.p0.cpu().numpy())
    assert np.abs(ll.cpu().numpy() - want_ll).max() <= 2e-6 * np.abs(want_ll).max()
    close(newP, wantP, "P")
    close(newp0, wantp0, "p0")
    assert np.allclose(newP.cpu().numpy().sum(1), 1, atol=1e-5)
    for t, k in zip((hmm.P, hmm.p0, hmm.log_P, hmm.log_p0), keep):
        assert torch.equal(t, k)
    ll2 = hmm.log_likelihood(dev(obs), lengths)
    assert np.abs(ll2.cpu().numpy() - want_ll).max() <= 2e-6 * np.abs(want_ll).max()
