"""fp64 model of posterior path sampling (forward-filter backward-sample) for the tests of
hmm355_ffbs_f32 / ops.ffbs / HMMPyTorch.sample_posterior.

  forward_filter      the normalised forward rows and the log-likelihood
  conditionals        p(z_t | z_{t+1}, x) of one path under the backward-sampling rule
  intervals_ok        the teacher-forced check of drawn states against their own uniforms
  enumerate_paths     every path's exact posterior by enumeration (tiny models)
  marginals           per-frame and (t, t+1) pair posteriors from the enumeration
"""
import itertools

import numpy as np


def forward_filter(e, A, p0, lengths=None):
    """e (B,T,N) emission probabilities, A (N,N), p0 (N), all taken to fp64.  Returns
    (alpha (B,T,N) with every valid row summing to 1, loglik (B)); rows past lengths[b] are 0."""
    e, A, p0 = (np.asarray(x, np.float64) for x in (e, A, p0))
    B, T, N = e.shape
    lens = [T] * B if lengths is None else [int(x) for x in lengths]
    alpha = np.zeros((B, T, N))
    loglik = np.zeros(B)
    for b in range(B):
        a = p0 * e[b, 0]
        for t in range(lens[b]):
            if t > 0:
                a = (alpha[b, t - 1] @ A) * e[b, t]
            s = a.sum()
            loglik[b] += np.log(s)
            alpha[b, t] = a / s
    return alpha, loglik


def conditionals(alpha, A, path):
    """prod_t p(z_t | z_{t+1}, x) for one sequence: alpha (T,N) forward rows (any scale), path (T)."""
    T = alpha.shape[0]
    p = 1.0
    for t in range(T - 1, -1, -1):
        w = alpha[t] if t == T - 1 else alpha[t] * A[:, path[t + 1]]
        p *= w[path[t]] / w.sum()
    return p


def enumerate_paths(e, A, p0):
    """One sequence e (T,N): (paths (N^T,T) int, posterior (N^T) = joint / Z)."""
    e, A, p0 = (np.asarray(x, np.float64) for x in (e, A, p0))
    T, N = e.shape
    paths = np.array(list(itertools.product(range(N), repeat=T)), dtype=np.int64)
    joint = p0[paths[:, 0]] * e[0, paths[:, 0]]
    for t in range(1, T):
        joint = joint * A[paths[:, t - 1], paths[:, t]] * e[t, paths[:, t]]
    return paths, joint / joint.sum()


def marginals(paths, post, N):
    """(gamma (T,N), xi (T-1,N,N)) of an enumerated posterior."""
    T = paths.shape[1]
    gamma = np.zeros((T, N))
    xi = np.zeros((max(T - 1, 0), N, N))
    for t in range(T):
        np.add.at(gamma[t], paths[:, t], post)
    for t in range(T - 1):
        np.add.at(xi[t], (paths[:, t], paths[:, t + 1]), post)
    return gamma, xi


def epsilon(N):
    """The interval slack of intervals_ok: bounds the fp32 prefix sum of N non-negative terms, the
    product fwd * A, expf and u * total, with a factor of two for numerator and denominator."""
    return (N + 16) * 2.0 ** -23


def intervals_ok(states, uniforms, fwd32, log_P32, lengths=None):
    """Teacher-forced check of every draw.  states (B,K,T) int, uniforms (B,K,T), fwd32 (B,T,>=N)
    fp32 rows as the kernel read them, log_P32 (N,N) fp32.  For every (b,k,t < L) takes the drawn
    z_{t+1}, forms w in fp64 from the fp32 inputs and F = cumsum(w) / sum(w), and requires
    0 <= z_t < N, w[z_t] > 0 and F[z_t - 1] - eps <= u <= F[z_t] + eps; a row without a positive
    finite total must give the first argmax of the fwd row; frames t >= L must hold -1.
    Returns (ok, message)."""
    states = np.asarray(states)
    u = np.asarray(uniforms, np.float64)
    N = log_P32.shape[0]
    B, K, T = states.shape
    with np.errstate(over="ignore"):
        A = np.exp(np.asarray(log_P32, np.float32).astype(np.float64))
    f = np.asarray(fwd32, np.float32)[..., :N]
    eps = epsilon(N)
    lens = [T] * B if lengths is None else [int(x) for x in lengths]
    ks = np.arange(K)
    for b in range(B):
        L = lens[b]
        if not (states[b, :, L:] == -1).all():
            return False, f"sequence {b}: a padded frame is not -1"
        for t in range(L - 1, -1, -1):
            z = states[b, :, t]
            if z.min() < 0 or z.max() >= N:
                return False, f"({b},:,{t}): state outside [0, {N - 1}]: {z.min()} .. {z.max()}"
            row32 = f[b, t]
            w = np.repeat(row32.astype(np.float64)[:, None], K, 1)          # (N,K)
            tot32 = np.full(K, row32.sum(dtype=np.float32), np.float32)
            if t < L - 1:
                w = w * A[:, states[b, :, t + 1]]
                with np.errstate(over="ignore"):
                    tot32 = (row32[:, None] * A[:, states[b, :, t + 1]].astype(np.float32)).sum(0, dtype=np.float32)
            tot = w.sum(0)
            good = (tot > 0) & np.isfinite(tot) & np.isfinite(tot32)
            if (~good).any():
                want = int(np.argmax(row32))
                if not (z[~good] == want).all():
                    return False, f"({b},:,{t}): degenerate row must give the first argmax {want}, got {z[~good]}"
            if good.any():
                g = ks[good]
                wg, zg, ug = w[:, g], z[g], u[b, g, t]
                F = np.cumsum(wg, 0) / tot[g]
                hi = F[zg, np.arange(len(g))]
                lo = np.where(zg > 0, F[np.maximum(zg - 1, 0), np.arange(len(g))], 0.0)
                wz = wg[zg, np.arange(len(g))]
                bad = ~((wz > 0) & (lo - eps <= ug) & (ug <= hi + eps))
                if bad.any():
                    j = int(np.flatnonzero(bad)[0])
                    return False, (f"({b},{g[j]},{t}): state {zg[j]} weight {wz[j]:.3e} u {ug[j]!r} not in "
                                   f"[{lo[j]!r}, {hi[j]!r}] +- {eps:.2e}")
    return True, ""
