"""The HMM sums in float64 log space: the range-free yardstick of the scaled kernels.

Every other fp64 model of the sum-product paths (tests/em_numpy.py forward_backward,
tests/sparse_numpy.py sums, the oracle's c_fb64) is the kernels' own scaled probability-domain
recursion in a wider type: it shares their one-factor-per-row scaling and so their blind spot, a
state more than the type's range behind its row's leader.  This one is written from the
definitions and never leaves the log domain:

    log alpha_0[j]   = log_p0[j] + log_obs_0[j]
    log alpha_t[j]   = LSE_i(log alpha_{t-1}[i] + log_P[i,j]) + log_obs_t[j]
    log beta_{L-1}   = 0,   log beta_t[i] = LSE_j(log_P[i,j] + log_obs_{t+1}[j] + log beta_{t+1}[j])
    loglik           = LSE_j log alpha_{L-1}[j]
    gamma_t[j]       = exp(log alpha_t[j] + log beta_t[j] - loglik)
    xi[i,j]          = sum_b sum_{t < L_b - 1} exp(log alpha_t[i] + log_P[i,j] + log_obs_{t+1}[j]
                                                 + log beta_{t+1}[j] - loglik_b)

LSE shifts by its maximum m with the explicit rule `m == -inf ? 0 : m`, so -inf arcs, -inf
emissions and sequences without any path give -inf and exact zeros, never NaN.  `brute_force`
enumerates every path (tiny N, T only): what the recursion itself is checked against.
"""
import itertools

import numpy as np

NEG = -np.inf


def lse(x, axis):
    """log sum exp over `axis`; -inf where every term is -inf."""
    x = np.asarray(x, np.float64)
    m = x.max(axis)
    m0 = np.where(m == NEG, 0.0, m)
    with np.errstate(divide="ignore"):
        return m0 + np.log(np.exp(x - np.expand_dims(m0, axis)).sum(axis))


def _lens(lengths, B, T):
    return np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)


def forward_backward(log_obs, log_P, log_p0, lengths=None):
    """dict(loglik (B), log_alpha, log_beta, gamma (B,T,N), xi (N,N), gamma0 (N), xi_seq (B,N,N)).
    Frames past a length are never read (they may hold NaN): log_alpha = log_beta = -inf and
    gamma = 0 there.  A sequence without a path has loglik -inf and contributes exact zeros."""
    obs = np.asarray(log_obs, np.float64)
    lP = np.asarray(log_P, np.float64)
    l0 = np.asarray(log_p0, np.float64)
    B, T, N = obs.shape
    lens = _lens(lengths, B, T)
    la = np.full((B, T, N), NEG)
    lb = np.full((B, T, N), NEG)
    gamma = np.zeros((B, T, N))
    xi_seq = np.zeros((B, N, N))
    loglik = np.zeros(B)
    for b in range(B):
        L = int(lens[b])
        o = obs[b, :L]
        la[b, 0] = l0 + o[0]
        for t in range(1, L):
            la[b, t] = lse(la[b, t - 1][:, None] + lP, 0) + o[t]
        lb[b, L - 1] = 0.0
        for t in range(L - 2, -1, -1):
            lb[b, t] = lse(lP + (o[t + 1] + lb[b, t + 1])[None, :], 1)
        ll = float(lse(la[b, L - 1], 0))
        loglik[b] = ll
        if ll == NEG:
            continue
        gamma[b, :L] = np.exp(la[b, :L] + lb[b, :L] - ll)
        for t in range(L - 1):
            xi_seq[b] += np.exp(la[b, t][:, None] + lP + (o[t + 1] + lb[b, t + 1])[None, :] - ll)
    return dict(loglik=loglik, log_alpha=la, log_beta=lb, gamma=gamma, xi=xi_seq.sum(0), gamma0=gamma[:, 0].sum(0),
                xi_seq=xi_seq)


def densify(src, dst, log_w, N):
    """(N,N) log matrix: log_w on the arcs, -inf elsewhere."""
    P = np.full((N, N), NEG)
    P[np.asarray(src, np.int64), np.asarray(dst, np.int64)] = np.asarray(log_w, np.float64)
    return P


def forward_backward_arcs(log_obs, src, dst, log_w, log_p0, lengths=None):
    """forward_backward of the dense model that is -inf off the arcs; xi and xi_seq come back per
    arc, (E) and (B,E), in the given arc order."""
    N = np.asarray(log_obs).shape[2]
    out = forward_backward(log_obs, densify(src, dst, log_w, N), log_p0, lengths)
    s, d = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    out["xi_seq"] = out["xi_seq"][:, s, d]
    out["xi"] = out["xi"][s, d]
    return out


def brute_force(log_obs, log_P, log_p0, lengths=None):
    """dict(loglik, gamma, xi, gamma0) by enumerating all N^L state paths of every sequence."""
    obs = np.asarray(log_obs, np.float64)
    lP = np.asarray(log_P, np.float64)
    l0 = np.asarray(log_p0, np.float64)
    B, T, N = obs.shape
    lens = _lens(lengths, B, T)
    loglik = np.zeros(B)
    gamma = np.zeros((B, T, N))
    xi = np.zeros((N, N))
    for b in range(B):
        L = int(lens[b])
        paths = list(itertools.product(range(N), repeat=L))
        score = np.empty(len(paths))
        for k, z in enumerate(paths):
            s = l0[z[0]] + obs[b, 0, z[0]]
            for t in range(1, L):
                s = s + lP[z[t - 1], z[t]] + obs[b, t, z[t]]
            score[k] = s
        ll = float(lse(score, 0))
        loglik[b] = ll
        if ll == NEG:
            continue
        w = np.exp(score - ll)
        for k, z in enumerate(paths):
            if w[k] == 0.0:
                continue
            for t in range(L):
                gamma[b, t, z[t]] += w[k]
            for t in range(1, L):
                xi[z[t - 1], z[t]] += w[k]
    return dict(loglik=loglik, gamma=gamma, xi=xi, gamma0=gamma[:, 0].sum(0))
