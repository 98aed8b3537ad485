"""numpy restatements of the transcript forced-alignment lattice (csrc/forced.hip), fp32 or fp64.

Sequence b has S_b = state_lengths[b] positions; position s emits e[t,s] = lp[b,t,ids[b,s]] (-inf
for an id outside [0, C); ids None: id_s = s) and stays / advances / skips with the weights
stay[b,s], next[b,s], skip[b,s] of the source position (None: 0, 0, -inf).

  alpha[0,0] = e[0,0];  alpha[t,s] = e[t,s] + LSE(alpha[t-1,s] + stay[s], alpha[t-1,s-1] + next[s-1],
                                                  alpha[t-1,s-2] + skip[s-2]);  loglik = alpha[T_b-1,S_b-1]
  beta[T_b-1,S_b-1] = 0;  beta[t,s] = LSE(stay[s] + e[t+1,s] + beta[t+1,s], next[s] + e[t+1,s+1] + beta[t+1,s+1],
                                          skip[s] + e[t+1,s+2] + beta[t+1,s+2])

-inf candidates drop out of the log-sum-exp.  viterbi is the same lattice as max-plus: every
candidate is one add of value and weight, the candidates are taken in the order stay, s-1, s-2
with strict >, the cell is one more add of the emission: in fp32 it is what the kernel must
reproduce bit for bit.  occupancy gives gamma and the four gradients of loglik.

Shapes: lp (B,T,C), ids (B,Smax) or None, lengths (B), weights (B,Smax) or None; tables (B,T,Smax).
"""
import numpy as np

EPS24 = 2.0 ** -24


def width(lp, ids, *weights):
    if ids is not None:
        return np.asarray(ids).shape[1]
    for w in weights:
        if w is not None:
            return np.asarray(w).shape[1]
    return np.asarray(lp).shape[2]


def weights_of(Smax, B, stay, nxt, skip, dtype):
    """The three (B,Smax) weight arrays in `dtype`, absent ones at their defaults."""
    out = []
    for w, default in ((stay, 0.0), (nxt, 0.0), (skip, -np.inf)):
        out.append(np.full((B, Smax), default, dtype=dtype) if w is None else np.asarray(w, dtype=dtype))
    return out


def emissions(lp, ids, b, Sb, dtype):
    """e (T,Sb) of sequence b in `dtype`; -inf in the columns of ids outside [0, C)."""
    lp = np.asarray(lp)
    T, C = lp.shape[1], lp.shape[2]
    c = np.arange(Sb) if ids is None else np.asarray(ids)[b, :Sb].astype(np.int64)
    ok = (c >= 0) & (c < C)
    e = np.full((T, Sb), -np.inf, dtype=dtype)
    e[:, ok] = lp[b][:, c[ok]].astype(dtype)
    return e


def _lse(cands, dtype):
    """log-sum-exp over axis 0 in `dtype`; -inf where every candidate is"""
    with np.errstate(all="ignore"):
        m = cands.max(axis=0)
        ms = np.where(np.isneginf(m), dtype(0), m).astype(dtype)
        s = np.zeros_like(ms)
        for c in cands:
            s = (s + np.exp((c - ms).astype(dtype)).astype(dtype)).astype(dtype)
        r = (ms + np.log(s).astype(dtype)).astype(dtype)
    return np.where(np.isneginf(m), dtype(-np.inf), r).astype(dtype)


def _shift(v, n, fill):
    """out[s] = v[s - n]"""
    out = np.full_like(v, fill)
    if n < len(v):
        out[n:] = v[:len(v) - n]
    return out


def _cands(prev, ws, wn, wk, dtype):
    """The three candidates of every position from the previous row: one add each."""
    NINF = dtype(-np.inf)
    with np.errstate(all="ignore"):
        return [(prev + ws).astype(dtype), _shift((prev + wn).astype(dtype), 1, NINF),
                _shift((prev + wk).astype(dtype), 2, NINF)]


def alpha(lp, ids, input_lengths, state_lengths, stay=None, nxt=None, skip=None, dtype=np.float32):
    """(alpha (B,T,Smax), loglik (B)) in `dtype`."""
    B, T, _ = np.asarray(lp).shape
    Smax = width(lp, ids, stay, nxt, skip)
    W = weights_of(Smax, B, stay, nxt, skip, dtype)
    NINF = dtype(-np.inf)
    A = np.full((B, T, Smax), NINF, dtype=dtype)
    ll = np.full(B, NINF, dtype=dtype)
    for b in range(B):
        Tb, Sb = int(input_lengths[b]), int(state_lengths[b])
        e = emissions(lp, ids, b, Sb, dtype)
        ws, wn, wk = (w[b, :Sb] for w in W)
        row = np.full(Sb, NINF, dtype=dtype)
        row[0] = e[0, 0]
        A[b, 0, :Sb] = row
        for t in range(1, Tb):
            r = _lse(np.stack(_cands(row, ws, wn, wk, dtype)), dtype)
            with np.errstate(all="ignore"):
                row = (r + e[t]).astype(dtype)
            A[b, t, :Sb] = row
        ll[b] = row[Sb - 1]
    return A, ll


def beta(lp, ids, input_lengths, state_lengths, stay=None, nxt=None, skip=None, dtype=np.float32):
    """beta (B,T,Smax) in `dtype`: its own frame's emission is left out."""
    B, T, _ = np.asarray(lp).shape
    Smax = width(lp, ids, stay, nxt, skip)
    W = weights_of(Smax, B, stay, nxt, skip, dtype)
    NINF = dtype(-np.inf)
    Bt = np.full((B, T, Smax), NINF, dtype=dtype)
    for b in range(B):
        Tb, Sb = int(input_lengths[b]), int(state_lengths[b])
        e = emissions(lp, ids, b, Sb, dtype)
        ws, wn, wk = (w[b, :Sb] for w in W)
        row = np.full(Sb, NINF, dtype=dtype)
        row[Sb - 1] = 0
        Bt[b, Tb - 1, :Sb] = row
        for t in range(Tb - 2, -1, -1):
            with np.errstate(all="ignore"):
                q = (row + e[t + 1]).astype(dtype)
                # from s + 1 and s + 2, with the weights of s itself
                q1 = np.full(Sb, NINF, dtype=dtype)
                q1[:Sb - 1] = q[1:]
                q2 = np.full(Sb, NINF, dtype=dtype)
                if Sb > 2:
                    q2[:Sb - 2] = q[2:]
                c = np.stack([(q + ws).astype(dtype), (q1 + wn).astype(dtype), (q2 + wk).astype(dtype)])
            row = _lse(c, dtype)
            Bt[b, t, :Sb] = row
    return Bt


def viterbi(lp, ids, input_lengths, state_lengths, stay=None, nxt=None, skip=None):
    """(path (B,T) int32, -1 past input_lengths[b] and for a pair with no path; score (B) fp32;
    durations (B,Smax) int32) of the best single path, in fp32."""
    f = np.float32
    B, T, _ = np.asarray(lp).shape
    Smax = width(lp, ids, stay, nxt, skip)
    W = weights_of(Smax, B, stay, nxt, skip, f)
    NINF = f(-np.inf)
    path = np.full((B, T), -1, dtype=np.int32)
    score = np.full(B, NINF, dtype=f)
    dur = np.zeros((B, Smax), dtype=np.int32)
    for b in range(B):
        Tb, Sb = int(input_lengths[b]), int(state_lengths[b])
        e = emissions(lp, ids, b, Sb, f)
        ws, wn, wk = (w[b, :Sb] for w in W)
        v = np.full(Sb, NINF, dtype=f)
        v[0] = e[0, 0]
        back = np.zeros((Tb, Sb), dtype=np.int64)
        for t in range(1, Tb):
            c0, c1, c2 = _cands(v, ws, wn, wk, f)
            best, d = c0, np.zeros(Sb, dtype=np.int64)
            take = c1 > best
            best, d = np.where(take, c1, best), np.where(take, 1, d)
            take = c2 > best
            best, d = np.where(take, c2, best), np.where(take, 2, d)
            with np.errstate(all="ignore"):
                v = (best + e[t]).astype(f)
            back[t] = d
        score[b] = v[Sb - 1]
        if v[Sb - 1] > NINF:
            s = Sb - 1
            for t in range(Tb - 1, -1, -1):
                path[b, t] = s
                dur[b, s] += 1
                s -= back[t, s]
    return path, score, dur


def occupancy(lp, ids, input_lengths, state_lengths, stay=None, nxt=None, skip=None, dtype=np.float64, tables=None):
    """(gamma (B,T,Smax), grad_lp (B,T,C), g_stay, g_next, g_skip (B,Smax)): the posteriors and
    the gradients of loglik; all 0 past either length and for a pair with no path.  tables: the
    (alpha, beta, loglik) of these inputs in `dtype`, if the caller has them already."""
    lp = np.asarray(lp, dtype=dtype)
    B, T, C = lp.shape
    Smax = width(lp, ids, stay, nxt, skip)
    W = weights_of(Smax, B, stay, nxt, skip, dtype)
    if tables is None:
        A, ll = alpha(lp, ids, input_lengths, state_lengths, stay, nxt, skip, dtype)
        Bt = beta(lp, ids, input_lengths, state_lengths, stay, nxt, skip, dtype)
    else:
        A, Bt, ll = tables
    gamma = np.zeros((B, T, Smax), dtype=dtype)
    grad = np.zeros((B, T, C), dtype=dtype)
    gw = [np.zeros((B, Smax), dtype=dtype) for _ in range(3)]
    for b in range(B):
        if not np.isfinite(ll[b]):
            continue
        Tb, Sb = int(input_lengths[b]), int(state_lengths[b])
        e = emissions(lp, ids, b, Sb, dtype)
        with np.errstate(all="ignore"):
            g = np.exp(A[b, :Tb, :Sb] + Bt[b, :Tb, :Sb] - ll[b])
        g = np.where(np.isfinite(g), g, 0)
        gamma[b, :Tb, :Sb] = g
        c = np.arange(Sb) if ids is None else np.asarray(ids)[b, :Sb].astype(np.int64)
        for s in range(Sb):
            if 0 <= c[s] < C:
                grad[b, :Tb, c[s]] += g[:, s]
        for d in range(3):
            n = Sb - d
            if n <= 0 or Tb < 2:
                continue
            with np.errstate(all="ignore"):
                x = (A[b, :Tb - 1, :n] + W[d][b, :n][None, :] + e[1:Tb, d:] + Bt[b, 1:Tb, d:Sb] - ll[b])
                x = np.where(np.isnan(x), -np.inf, x)
                gw[d][b, :n] = np.exp(x).sum(0)
    return gamma, grad, gw[0], gw[1], gw[2]


# ------------------------------------------------------------------ the acceptance bounds
def alpha_steps(T, B):
    """(B,T,1): recursion steps behind alpha[b,t,:], t + 1"""
    return np.broadcast_to(np.arange(1, T + 1)[None, :, None], (B, T, 1))


def beta_steps(T, input_lengths):
    """(B,T,1): recursion steps behind beta[b,t,:], T_b - t: beta runs down from frame T_b - 1"""
    return np.maximum(np.asarray(input_lengths)[:, None, None] - np.arange(T)[None, :, None], 1)


def step_bound(x64, steps):
    """5 n 2^-24 max(1, |x_64|): CTC's 4 n plus one rounding per step for the added weight"""
    x64 = np.asarray(x64, dtype=np.float64)
    ref = np.where(np.isfinite(x64), x64, 0.0)
    return 5 * steps * EPS24 * np.maximum(1.0, np.abs(ref))


def step_bound_excess(x, x64, steps):
    """max over the finite entries of |x - x64| / step_bound: <= 1 passes.  inf when the -inf
    patterns differ or x holds anything else that is not finite."""
    x, x64 = np.asarray(x), np.asarray(x64)
    if not np.array_equal(np.isneginf(x), np.isneginf(x64)) or not np.isfinite(x[np.isfinite(x64)]).all():
        return np.inf
    fin = np.isfinite(x64)
    ref = np.where(fin, x64, 0.0)
    err = np.abs(np.where(fin, x.astype(np.float64) - ref, 0.0))
    return float((err / step_bound(x64, steps)).max(initial=0.0))
