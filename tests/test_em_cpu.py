"""CPU: Baum-Welch (pytorch_hmm_amd/em.py, csrc/emstats.hip) as far as it can be checked without a
device.

  * tests/em_numpy.py (the GPU tests' fp64 model) against brute-force path enumeration and explicit
    loops, and the behaviour EM must show: monotone log-likelihood, dead components and
    unoccupied states keep their parameters.
  * em.transition_m_step / em.gaussian_m_step (pure torch) against the model.
  * The C entry is declared, exported and rejects bad arguments with the documented codes before
    anything is launched (fake pointers).
  * The layers' host logic: 'full' raises, "initial" is refused by the mixture layer, CPU tensors
    raise.
"""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import em_numpy as emn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")


@pytest.fixture(scope="module")
def L():
    from pytorch_hmm_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from pytorch_hmm_amd import build_native
        build_native.build()
    return nat.lib()


@pytest.fixture(scope="module")
def d():
    return dict((m.group(1), int(m.group(2).rstrip("u"), 0))
                for m in re.finditer(r"#define\s+(HMM355_[A-Z0-9_]+)\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+)u?)\)?",
                                     open(HEADER).read()))


# ------------------------------------------------------------------- the model itself
def brute_force(le, log_P, log_p0, lengths):
    """loglik, gamma, xi, gamma0 by enumerating every path of every sequence."""
    B, T, N = le.shape
    loglik, gamma, xi, gamma0 = np.zeros(B), np.zeros((B, T, N)), np.zeros((N, N)), np.zeros(N)
    for b in range(B):
        Lb = int(lengths[b])
        tot, g, x = 0.0, np.zeros((Lb, N)), np.zeros((N, N))
        for path in itertools.product(range(N), repeat=Lb):
            lp = log_p0[path[0]] + le[b, 0, path[0]]
            for t in range(1, Lb):
                lp += log_P[path[t - 1], path[t]] + le[b, t, path[t]]
            p = np.exp(lp)
            tot += p
            for t in range(Lb):
                g[t, path[t]] += p
            for t in range(Lb - 1):
                x[path[t], path[t + 1]] += p
        loglik[b] = np.log(tot)
        gamma[b, :Lb] = g / tot
        xi += x / tot
        gamma0 += g[0] / tot
    return loglik, gamma, xi, gamma0


def test_model_matches_path_enumeration():
    rng = np.random.default_rng(0)
    N, T, B = 3, 4, 2
    lengths = np.array([4, 2])
    P = rng.dirichlet(np.ones(N), N)
    P[2, 0] = 0.0                                        # one exact zero
    P /= P.sum(1, keepdims=True)
    with np.errstate(divide="ignore"):
        log_P = np.log(P)
    log_p0 = np.log(rng.dirichlet(np.ones(N)))
    le = rng.normal(size=(B, T, N)) * 2
    want = brute_force(le, log_P, log_p0, lengths)
    got = emn.forward_backward(le, log_P, log_p0, lengths)
    for g, w in zip(got, want):
        assert np.abs(g - w).max() <= 1e-12
    assert got[2][2, 0] == 0.0 and (got[1][1, 2:] == 0).all()


def _mixture_case(rng, B, T, S, C, D):
    means = rng.normal(size=(S, C, D))
    log_vars = rng.normal(size=(S, C, D)) * 0.3
    log_w = np.log(rng.dirichlet(np.ones(C), S))
    x = means.reshape(-1, D)[rng.integers(0, S * C, size=(B, T))] + 0.7 * rng.normal(size=(B, T, D))
    weight = rng.random((B, T, S))
    return x, weight, means, log_vars, log_w


def test_centred_statistics_equal_loops_and_raw_moments():
    rng = np.random.default_rng(1)
    B, T, S, C, D = 2, 5, 3, 2, 4
    x, weight, means, log_vars, log_w = _mixture_case(rng, B, T, S, C, D)
    lengths = np.array([5, 3])
    (occ, sx, sxx), (a0, a1, a2) = emn.gmm_stats(x, weight, means, log_vars, log_w, 1, lengths)
    o, s1, s2 = np.zeros((S, C)), np.zeros((S, C, D)), np.zeros((S, C, D))
    raw1, raw2 = np.zeros((S, C, D)), np.zeros((S, C, D))
    for b in range(B):
        for t in range(lengths[b]):
            for s in range(S):
                comp = np.array([-0.5 * (((x[b, t] - means[s, c]) ** 2 / np.exp(log_vars[s, c])).sum()
                                         + log_vars[s, c].sum() + D * np.log(2 * np.pi)) + log_w[s, c]
                                 for c in range(C)])
                r = np.exp(comp - comp.max())
                r /= r.sum()
                for c in range(C):
                    w = weight[b, t, s] * r[c]
                    o[s, c] += w
                    s1[s, c] += w * (x[b, t] - means[s, c])
                    s2[s, c] += w * (x[b, t] - means[s, c]) ** 2
                    raw1[s, c] += w * x[b, t]
                    raw2[s, c] += w * x[b, t] ** 2
    assert np.allclose(occ, o, rtol=1e-12) and np.allclose(sx, s1, atol=1e-12) and np.allclose(sxx, s2, rtol=1e-12)
    assert np.allclose(a0, o, rtol=1e-12) and (a1 >= np.abs(s1) - 1e-12).all()
    mean_raw = raw1 / o[..., None]
    var_raw = raw2 / o[..., None] - mean_raw ** 2
    assert np.allclose(means + sx / occ[..., None], mean_raw, rtol=1e-11, atol=1e-12)
    assert np.allclose(sxx / occ[..., None] - (sx / occ[..., None]) ** 2, var_raw, rtol=1e-9, atol=1e-12)


def _em_run(cov, C, n_iter=10, seed=3, dead=False):
    """n_iter fp64 EM iterations on data drawn from another model; the logliks and final state."""
    rng = np.random.default_rng(seed)
    S, D, B, T = 3, 4, 4, 40
    true_means = rng.normal(size=(S, C, D)) * 2.5
    true_P = np.full((S, S), 0.1) + 0.7 * np.eye(S)
    x = emn.sample_gmm_hmm(rng, B, T, true_P, np.full(S, 1 / S), true_means, 0.8, np.full((S, C), 1 / C))
    lengths = np.array([40, 31, 17, 40])
    means = true_means + rng.normal(size=(S, C, D))
    lv = {"diag": np.zeros((S, C, D)), "spherical": np.zeros((S, C)), "tied": np.zeros(D)}[cov]
    log_P = np.log(rng.dirichlet(np.ones(S) * 3, S))
    log_p0 = np.log(np.full(S, 1 / S))
    w = np.full((S, C), 1.0 / C)
    if dead:
        w[1] = 0.0
        w[1, 0] = 1.0
    hist = []
    for _ in range(n_iter):
        with np.errstate(divide="ignore"):
            out = emn.em_iteration(x, lengths, log_P, log_p0, means, lv, np.log(w), cov, mix_lse=1)
        hist.append(out["loglik"])
        with np.errstate(divide="ignore"):
            log_P, log_p0 = np.log(out["P"]), np.log(out["p0"])
        prev = (means, lv, w)
        means, lv, w = out["means"], out["log_vars"], out["weights"]
    return hist, prev, (means, lv, w), out


@pytest.mark.parametrize("cov,C", [("diag", 1), ("spherical", 1), ("diag", 3), ("tied", 3)])
def test_em_never_lowers_the_loglikelihood(cov, C):
    hist, *_ = _em_run(cov, C)
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(hist, hist[1:])), hist
    assert hist[-1] > hist[0]


def test_dead_component_keeps_zero_statistics_and_parameters():
    hist, prev, cur, out = _em_run("diag", 3, n_iter=2, dead=True)
    assert (out["occ"][1, 1:] == 0).all() and (out["sx"][1, 1:] == 0).all() and (out["sxx"][1, 1:] == 0).all()
    assert np.isfinite(out["occ"]).all() and np.isfinite(out["sxx"]).all()
    assert (cur[0][1, 1:] == prev[0][1, 1:]).all() and (cur[1][1, 1:] == prev[1][1, 1:]).all()
    assert (cur[2][1, 1:] == 0).all() and cur[2][1, 0] == 1.0


def test_unoccupied_state_keeps_its_row():
    rng = np.random.default_rng(5)
    N, B, T = 3, 2, 6
    P = rng.dirichlet(np.ones(N), N)
    le = rng.normal(size=(B, T, N))
    le[..., 2] = -np.inf                                   # state 2 can never emit
    with np.errstate(divide="ignore"):
        _, gamma, xi, gamma0 = emn.forward_backward(le, np.log(P), np.log(np.full(N, 1 / N)))
    assert (gamma[..., 2] == 0).all() and (xi[2] == 0).all()
    newP, p0 = emn.transition_m_step(xi, gamma0, B, P, np.full(N, 1 / N))
    assert (newP[2] == P[2]).all() and np.allclose(newP[:2].sum(1), 1) and p0[2] == 0


# ------------------------------------------------------------------ the torch M-steps
def test_transition_m_step_matches_model_and_keeps_zeros():
    from pytorch_hmm_amd import em
    rng = np.random.default_rng(7)
    N = 6
    xi = rng.random((N, N)) * 5
    xi[np.triu_indices(N, 2)] = 0.0
    xi[np.tril_indices(N, -1)] = 0.0
    xi[4] = 0.0                                            # never occupied: keeps the old row
    gamma0 = rng.random(N)
    old_P = rng.dirichlet(np.ones(N), N)
    old_p0 = rng.dirichlet(np.ones(N))
    wantP, wantp0 = emn.transition_m_step(xi, gamma0, 3, old_P, old_p0)
    P, p0 = em.transition_m_step(torch.tensor(xi, dtype=torch.float32), torch.tensor(gamma0, dtype=torch.float32), 3,
                                 torch.tensor(old_P, dtype=torch.float32), torch.tensor(old_p0, dtype=torch.float32))
    assert P.dtype == torch.float32 and np.abs(P.numpy() - wantP).max() <= 1e-6
    assert np.abs(p0.numpy() - wantp0).max() <= 1e-6
    zero = (xi == 0) & (np.arange(N)[:, None] != 4)
    assert (P.numpy()[zero] == 0).all()
    assert np.allclose(P.numpy()[4], old_P[4], atol=1e-7)


@pytest.mark.parametrize("cov", ["diag", "spherical", "tied"])
def test_gaussian_m_step_matches_model(cov):
    from pytorch_hmm_amd import em
    rng = np.random.default_rng(8)
    B, T, S, C, D = 2, 30, 4, 3, 5
    x, weight, means, log_vars, log_w = _mixture_case(rng, B, T, S, C, D)
    log_w[2, 1] = -np.inf                                  # a dead component
    weight[..., 3] = 0.0                                   # a state that is never occupied
    (occ, sx, sxx), _ = emn.gmm_stats(x, weight, means, log_vars, log_w, 1)
    old_lv = {"diag": log_vars, "spherical": log_vars[..., 0], "tied": log_vars[0, 0]}[cov]
    with np.errstate(divide="ignore"):
        old_w = np.exp(log_w)
    want = emn.gaussian_m_step(occ, sx, sxx, means, cov, log_vars=old_lv, weights=old_w)
    t = lambda a: torch.tensor(a, dtype=torch.float32)
    got = em.gaussian_m_step(t(occ), t(sx), t(sxx), t(means), cov, log_vars=t(old_lv), weights=t(old_w))
    for g, w in zip(got, want):
        assert tuple(g.shape) == w.shape
        assert np.abs(g.numpy() - w).max() <= 1e-6 * max(1.0, np.abs(w).max())
    assert got[2][2, 1] == 0 and (got[0][2, 1].numpy() == means[2, 1].astype(np.float32)).all()
    assert np.allclose(got[2][3].numpy(), old_w[3], atol=1e-7)      # the unoccupied state keeps its weights
    with pytest.raises(NotImplementedError):
        em.gaussian_m_step(t(occ), t(sx), t(sxx), t(means), "full")


def test_estats_addition():
    from pytorch_hmm_amd import em
    a = em.EStats(torch.ones(2), torch.zeros(2, 3, 4), torch.ones(4, 4), torch.ones(4), 2)
    b = em.EStats(torch.ones(3) * 2, torch.zeros(3, 3, 4), torch.ones(4, 4) * 2, torch.ones(4) * 3, 3)
    c = a + b
    assert c.n_seq == 5 and float(c.loglik.sum()) == 8 and (c.xi == 3).all() and (c.gamma0 == 4).all()
    assert c.gamma is None


# ------------------------------------------------------------------------------- C ABI
FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
BIG = 1 << 40


def stats(L, x=FAKE, weight=FAKE, means=FAKE, lv=FAKE, B=2, T=10, D=8, S=4, C=2, mix=1, wsp=FAKE, ws=BIG):
    return L.hmm355_gmm_stats_f32(x, weight, means, lv, FAKE, None, B, T, D, S, C, mix, FAKE, FAKE, FAKE, wsp, ws, None)


def test_declared_exported_and_version_bumped(L, d):
    from pytorch_hmm_amd import _native as nat
    header = open(HEADER).read()
    for name in ("hmm355_gmm_stats_workspace_bytes", "hmm355_gmm_stats_f32"):
        assert name in nat.EXPORTS and re.search(rf"\b{name}\(", header)
        assert getattr(L, name).argtypes
    assert L.hmm355_version() >= 12
    assert d["HMM355_GMM_STATS_MAX_DIM"] == nat.GMM_STATS_MAX_DIM >= 256


def test_status_codes(L, d):
    dmax = d["HMM355_GMM_STATS_MAX_DIM"]
    assert stats(L, x=None) == d["HMM355_E_ARG"]
    assert stats(L, weight=None) == d["HMM355_E_ARG"]
    assert stats(L, means=None) == d["HMM355_E_ARG"]
    assert stats(L, lv=None) == d["HMM355_E_ARG"]
    assert stats(L, wsp=None) == d["HMM355_E_ARG"]
    assert stats(L, B=-1) == d["HMM355_E_ARG"]
    assert stats(L, D=dmax + 1) == d["HMM355_E_SHAPE"]
    assert stats(L, T=0) == d["HMM355_E_SHAPE"]
    assert stats(L, B=1 << 16, T=1 << 16) == d["HMM355_E_SHAPE"]
    assert stats(L, S=65536 // 2 + 1, C=2) == d["HMM355_E_STATES"]
    assert stats(L, S=1, C=257) == d["HMM355_E_STATES"]
    assert stats(L, S=0) == d["HMM355_E_ARG"]
    assert stats(L, C=2, mix=0) == d["HMM355_E_ARG"]
    need = L.hmm355_gmm_stats_workspace_bytes(2, 10, 8, 4, 2)
    assert need > 0
    assert stats(L, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    assert stats(L, B=0) == 0
    assert stats(L, B=0, x=None, weight=None, means=None, lv=None, wsp=None, ws=0) == 0
    assert L.hmm355_gmm_stats_workspace_bytes(2, 10, dmax + 1, 4, 2) == 0
    assert L.hmm355_gmm_stats_workspace_bytes(2, 10, 8, 1, 257) == 0


def test_workspace_has_no_per_frame_component_buffer(L):
    B, T, D, S, C = 32, 2000, 80, 128, 4                   # BASELINE config 3
    need = L.hmm355_gmm_stats_workspace_bytes(B, T, D, S, C)
    assert 0 < need < B * T * S * C * 4
    # ten times the frames: longer spans, not more of them (63 or 64 at this shape)
    assert L.hmm355_gmm_stats_workspace_bytes(B, 10 * T, D, S, C) <= need * 64 // 63


# --------------------------------------------------------------------------- host logic
def test_gmm_stats_op_checks_and_fake():
    from pytorch_hmm_amd import ops
    x, w = torch.zeros(2, 5, 3), torch.zeros(2, 5, 4)
    mu, lv, lw = torch.zeros(4, 2, 3), torch.zeros(4, 2, 3), torch.zeros(4, 2)
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        ops.gmm_stats(x, w, mu, lv, lw, 1)
    with pytest.raises(ValueError):
        ops.gmm_stats(x, torch.zeros(2, 5, 5), mu, lv, lw, 1)
    with pytest.raises(ValueError):
        ops.gmm_stats(torch.zeros(2, 5, 4), w, mu, lv, lw, 1)
    with pytest.raises(ValueError):
        ops.gmm_stats(x, w, mu, lv, lw, 0)                # mix_lse == 0 needs C == 1
    with pytest.raises(ValueError):
        ops.gmm_stats(x, w, mu, lv, lw, 1, torch.tensor([5, 6]))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        occ, sx, sxx = torch.ops.hmm355.gmm_stats(torch.empty(2, 5, 3), torch.empty(2, 5, 4), torch.empty(4, 2, 3),
                                                  torch.empty(4, 2, 3), torch.empty(4, 2), 1)
        assert tuple(occ.shape) == (4, 2) and tuple(sx.shape) == tuple(sxx.shape) == (4, 2, 3)


def test_e_step_checks():
    from pytorch_hmm_amd import em
    with pytest.raises(ValueError):
        em.e_step(torch.zeros(5, 3), torch.zeros(3, 3), torch.zeros(3))
    with pytest.raises(ValueError):
        em.e_step(torch.zeros(2, 5, 3), torch.zeros(4, 4), torch.zeros(3))
    with pytest.raises(NotImplementedError):
        em.e_step(torch.zeros(1, 2, 300), torch.zeros(300, 300), torch.zeros(300))
    with pytest.raises(RuntimeError, match="ROCm GPUs only"):
        em.e_step(torch.zeros(2, 5, 3), torch.zeros(3, 3), torch.zeros(3))


def test_layers_host_logic():
    from pytorch_hmm_amd import GaussianHMMLayer, HMMPyTorch, MixtureGaussianHMMLayer
    x = torch.zeros(2, 6, 4)
    with pytest.raises(NotImplementedError):
        GaussianHMMLayer(3, 4, covariance_type="full").em_step(x)
    with pytest.raises(NotImplementedError):
        MixtureGaussianHMMLayer(3, 4, 2, covariance_type="full").em_step(x)
    with pytest.raises(NotImplementedError):
        MixtureGaussianHMMLayer(3, 4, 2, covariance_type="full").log_likelihood(x)
    mix = MixtureGaussianHMMLayer(3, 4, 2)
    with pytest.raises(ValueError, match="initial"):
        mix.em_step(x, update=("initial", "means"))
    with pytest.raises(ValueError):
        mix.em_step(x, update=("covariances",))
    gau = GaussianHMMLayer(3, 4)
    with pytest.raises(ValueError):
        gau.em_step(x, update=("weights",))
    with pytest.raises(ValueError):
        gau.em_step(torch.zeros(2, 6, 5))                  # wrong feature dim
    with pytest.raises(ValueError):
        mix.fit([(x, [6, 7])])                             # a length past T
    for call in (lambda: gau.em_step(x), lambda: mix.em_step(x), lambda: mix.log_likelihood(x), lambda: gau.fit(x),
                 lambda: mix.fit([(x, None), (x, [6, 3])]),
                 lambda: HMMPyTorch(torch.full((3, 3), 1 / 3)).reestimate(torch.rand(2, 6, 3))):
        with pytest.raises(RuntimeError, match="ROCm GPUs only"):
            call()
    before = [p.clone() for p in mix.parameters()]
    assert all((a == b).all() for a, b in zip(before, mix.parameters()))
