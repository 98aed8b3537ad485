"""fp64 NumPy model of Baum-Welch (EM) for Gaussian-(mixture) HMMs: the yardstick of
tests/test_em_cpu.py and tests/test_gpu_em.py (the reference has no EM to compare with).

  forward_backward   scaled forward-backward with per-sequence lengths: loglik, gamma, xi, gamma0
  component_scores   comp[b,t,s,c] of the scorer's model, responsibilities() their softmax over c
  gmm_stats          the centred statistics by their definition, with A = sum |w * term| per output
  gmm_stats_f32      the same definition evaluated in fp32 throughout (independent of the kernel;
                     used only to size the kernel tests' tolerance)
  transition_m_step / gaussian_m_step   the closed-form updates
  em_iteration       one full iteration of a Gaussian-(mixture) HMM
"""
import numpy as np

LOG2PI = 1.8378770664093453


def _lens(lengths, B, T):
    return np.full(B, T, dtype=np.int64) if lengths is None else np.asarray(lengths, dtype=np.int64)


def forward_backward(log_emis, log_P, log_p0, lengths=None):
    """(loglik (B), gamma (B,T,N) zero past the lengths, xi (N,N), gamma0 (N)) in fp64."""
    le = np.asarray(log_emis, dtype=np.float64)
    B, T, N = le.shape
    with np.errstate(divide="ignore"):
        A = np.exp(np.asarray(log_P, dtype=np.float64))
        p0 = np.exp(np.asarray(log_p0, dtype=np.float64))
    lens = _lens(lengths, B, T)
    loglik = np.zeros(B)
    gamma = np.zeros((B, T, N))
    xi = np.zeros((N, N))
    gamma0 = np.zeros(N)
    for b in range(B):
        L = int(lens[b])
        m = le[b, :L].max(-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        e = np.exp(le[b, :L] - m)
        al = np.zeros((L, N))
        c = np.zeros(L)
        a = p0 * e[0]
        c[0] = a.sum()
        al[0] = a / c[0]
        for t in range(1, L):
            a = (al[t - 1] @ A) * e[t]
            c[t] = a.sum()
            al[t] = a / c[t]
        be = np.ones((L, N))
        for t in range(L - 2, -1, -1):
            be[t] = (A @ (e[t + 1] * be[t + 1])) / c[t + 1]
        g = al * be
        gamma[b, :L] = g / g.sum(-1, keepdims=True)
        gamma0 += gamma[b, 0]
        for t in range(L - 1):
            xi += al[t][:, None] * A * (e[t + 1] * be[t + 1])[None, :] / c[t + 1]
        loglik[b] = np.log(c).sum() + m.sum()
    return loglik, gamma, xi, gamma0


def component_scores(x, means, log_vars, log_w, dtype=np.float64):
    """comp (B,T,S,C) = -0.5 (sum_d (x-mu)^2 / exp(lv) + sum_d lv + D log 2pi) + log_w in `dtype`."""
    x, mu, lv = (np.asarray(a, dtype=dtype) for a in (x, means, log_vars))
    D = x.shape[-1]
    diff = x[:, :, None, None, :] - mu[None, None]
    q = (diff * diff * np.exp(-lv)[None, None]).sum(-1, dtype=dtype)
    k = lv.sum(-1, dtype=dtype) + dtype(D * LOG2PI)
    lw = np.zeros(mu.shape[:2], dtype=dtype) if log_w is None else np.asarray(log_w, dtype=dtype)
    return dtype(-0.5) * (q + k[None, None]) + lw[None, None]


def responsibilities(comp, mix_lse=1):
    """softmax over c, shifted by its max; 0 for every c where all components are -inf; 1 when
    mix_lse == 0 (C == 1)."""
    if not mix_lse:
        assert comp.shape[-1] == 1
        return np.ones_like(comp)
    m = comp.max(-1, keepdims=True)
    dead = np.isneginf(m)
    with np.errstate(invalid="ignore"):
        ex = np.exp(comp - np.where(dead, 0, m).astype(comp.dtype))
    se = ex.sum(-1, keepdims=True, dtype=comp.dtype)
    return np.where(dead, 0, ex / np.where(dead, 1, se)).astype(comp.dtype)


def _stats(x, weight, means, log_vars, log_w, mix_lse, lengths, dtype):
    x = np.asarray(x, dtype=dtype)
    B, T, D = x.shape
    lens = _lens(lengths, B, T)
    valid = np.arange(T)[None, :] < lens[:, None]
    x = np.where(valid[..., None], x, 0).astype(dtype)                   # padded frames never enter
    wt = np.where(valid[..., None], np.asarray(weight, dtype=dtype), 0).astype(dtype)
    r = responsibilities(component_scores(x, means, log_vars, log_w, dtype), mix_lse)
    w = wt[..., None] * r                                                # (B,T,S,C)
    diff = x[:, :, None, None, :] - np.asarray(means, dtype=dtype)[None, None]
    t1 = w[..., None] * diff
    t2 = t1 * diff
    s = lambda a: a.sum((0, 1), dtype=dtype)
    return (s(w), s(t1), s(t2)), (s(np.abs(w)), s(np.abs(t1)), s(np.abs(t2)))


def gmm_stats(x, weight, means, log_vars, log_w=None, mix_lse=1, lengths=None):
    """((occ, sx, sxx), (A_occ, A_sx, A_sxx)) in fp64; A = the sum of the terms' magnitudes."""
    return _stats(x, weight, means, log_vars, log_w, mix_lse, lengths, np.float64)


def gmm_stats_f32(x, weight, means, log_vars, log_w=None, mix_lse=1, lengths=None):
    """(occ, sx, sxx) by the same definition with every intermediate in fp32."""
    return _stats(x, weight, means, log_vars, log_w, mix_lse, lengths, np.float32)[0]


def relative_error(got, want, A):
    """max |got - want| / A over the outputs (A > 0 everywhere)."""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want) / A))


def transition_m_step(xi, gamma0, n_seq, old_P, old_p0, min_occupancy=1e-6):
    xi = np.asarray(xi, dtype=np.float64)
    rows = xi.sum(1, keepdims=True)
    ok = rows >= min_occupancy
    P = np.where(ok, xi / np.where(ok, rows, 1.0), np.asarray(old_P, dtype=np.float64))
    p0 = np.asarray(gamma0, dtype=np.float64) / n_seq if n_seq > 0 else np.asarray(old_p0, dtype=np.float64)
    return P, p0


def gaussian_m_step(occ, sx, sxx, means, covariance_type, var_floor=1e-4, min_occupancy=1e-6, log_vars=None,
                    weights=None):
    """(means', log_vars', weights'); log_vars' in the covariance type's shape ((S,C,D), (S,C), (D))."""
    occ, sx, sxx, mu = (np.asarray(a, dtype=np.float64) for a in (occ, sx, sxx, means))
    S, C, D = mu.shape
    ok = occ >= min_occupancy
    od = np.where(ok, occ, 1.0)
    m1 = sx / od[..., None]
    new_mu = np.where(ok[..., None], mu + m1, mu)
    cen = np.where(ok[..., None], sxx - sx * m1, 0.0)
    shape = {"diag": (S, C, D), "spherical": (S, C), "tied": (D,)}[covariance_type]
    old = np.zeros(shape) if log_vars is None else np.asarray(log_vars, dtype=np.float64).reshape(shape)
    if covariance_type == "diag":
        new_lv = np.where(ok[..., None], np.log(np.maximum(cen / od[..., None], var_floor)), old)
    elif covariance_type == "spherical":
        new_lv = np.where(ok, np.log(np.maximum(cen.sum(-1) / (D * od), var_floor)), old)
    else:
        tot = np.where(ok, occ, 0.0).sum()
        new_lv = np.log(np.maximum(cen.sum((0, 1)) / tot, var_floor)) if tot >= min_occupancy else old
    tot_s = occ.sum(-1, keepdims=True)
    oks = tot_s >= min_occupancy
    oldw = np.full((S, C), 1.0 / C) if weights is None else np.asarray(weights, dtype=np.float64)
    new_w = np.where(oks, occ / np.where(oks, tot_s, 1.0), oldw)
    return new_mu, new_lv, new_w


def expand_log_vars(log_vars, covariance_type, S, C, D):
    lv = np.asarray(log_vars, dtype=np.float64)
    if covariance_type == "diag":
        return lv.reshape(S, C, D)
    if covariance_type == "spherical":
        return np.broadcast_to(lv.reshape(S, C, 1), (S, C, D)).copy()
    return np.broadcast_to(lv.reshape(1, 1, D), (S, C, D)).copy()


def emission_logprob(x, means, log_vars, log_w, mix_lse=1):
    """(B,T,S) log-emissions: the LSE over c of comp (the component itself when mix_lse == 0)."""
    comp = component_scores(x, means, log_vars, log_w)
    if not mix_lse:
        return comp[..., 0]
    m = comp.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.log(np.exp(comp - m).sum(-1)) + m[..., 0]


def em_iteration(x, lengths, log_P, log_p0, means, log_vars, log_w, covariance_type, mix_lse=1, var_floor=1e-4,
                 min_occupancy=1e-6):
    """One EM iteration of a Gaussian-(mixture) HMM in fp64.  means (S,C,D), log_vars in the
    covariance type's shape, log_w (S,C) log mixture weights (-inf allowed).  Returns a dict with
    the total log-likelihood before the update and the updated P, p0, means, log_vars, weights."""
    x = np.asarray(x, dtype=np.float64)
    S, C, D = np.asarray(means).shape
    lv = expand_log_vars(log_vars, covariance_type, S, C, D)
    le = emission_logprob(x, means, lv, log_w, mix_lse)
    B, T = x.shape[:2]
    lens = _lens(lengths, B, T)
    le = np.where((np.arange(T)[None, :] < lens[:, None])[..., None], le, 0.0)
    loglik, gamma, xi, gamma0 = forward_backward(le, log_P, log_p0, lens)
    (occ, sx, sxx), _ = gmm_stats(x, gamma, means, lv, log_w, mix_lse, lens)
    with np.errstate(divide="ignore"):
        P, p0 = transition_m_step(xi, gamma0, B, np.exp(log_P), np.exp(log_p0), min_occupancy)
        mu, new_lv, w = gaussian_m_step(occ, sx, sxx, means, covariance_type, var_floor, min_occupancy, log_vars,
                                        np.exp(np.asarray(log_w, dtype=np.float64)))
    return {"loglik": float(loglik.sum()), "logliks": loglik, "P": P, "p0": p0, "means": mu, "log_vars": new_lv,
            "weights": w, "gamma": gamma, "xi": xi, "gamma0": gamma0, "occ": occ, "sx": sx, "sxx": sxx}


def sample_gmm_hmm(rng, B, T, P, p0, means, std, weights):
    """x (B,T,D) drawn from a Gaussian-mixture HMM (means (S,C,D), one std, weights (S,C))."""
    S, C, D = means.shape
    x = np.zeros((B, T, D))
    for b in range(B):
        z = rng.choice(S, p=p0)
        for t in range(T):
            if t:
                z = rng.choice(S, p=P[z])
            c = rng.choice(C, p=weights[z])
            x[b, t] = means[z, c] + std * rng.standard_normal(D)
    return x
