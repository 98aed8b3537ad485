"""numpy restatements of the CTC lattice of pytorch_hmm.alignment.ctc, in fp32 or fp64.

alpha / beta follow ctc_forward_algorithm (ctc.py:32-121) and ctc_backward_algorithm (:124-199)
cell for cell, vectorised over the positions of a frame: beta leaves the frame's own emission
out, -inf candidates drop out of the log-sum-exp, a cell with no finite candidate stays -inf.
viterbi is the same lattice as max-plus (candidates stay, s-1, s-2 with strict >; the end is
S'-1 unless S'-2 is strictly greater): an exact max and one add per cell, so in fp32 it is what the
kernel must reproduce bit for bit.  occupancy gives gamma = exp(alpha + beta - loglik) and the
class gradient d loglik / d log_probs.  test_ctc_cpu.py holds all of them to the fixtures the
reference wrote (tests/golden/ctc_*.npz, make_golden_ctc.py).

Shapes: lp (T,B,C), targets (B,Lmax), input_lengths / target_lengths (B); tables (B,T,2 Lmax+1).
"""
import numpy as np

FIXTURES = ("basic", "empty", "one_frame", "infeasible", "neginf", "blank3", "blank_label", "long")


def expand(targets, blank):
    targets = np.asarray(targets)
    B, L = targets.shape
    ext = np.full((B, 2 * L + 1), blank, dtype=np.int64)
    ext[:, 1::2] = targets
    return ext


def _skip(ext_b, Sb):
    """skip[s]: position s may take from s - 2"""
    sk = np.zeros(len(ext_b), dtype=bool)
    if Sb > 2:
        sk[2:Sb] = ext_b[2:Sb] != ext_b[:Sb - 2]
    return sk


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
    out = np.full_like(v, fill)
    out[n:] = v[:len(v) - n]
    return out


def alpha(lp, targets, input_lengths, target_lengths, blank=0, dtype=np.float32):
    """(alpha (B,T,S'), loglik (B)) in `dtype`."""
    lp = np.asarray(lp, dtype=dtype)
    T, B, _ = lp.shape
    ext = expand(targets, blank)
    S = ext.shape[1]
    NINF = dtype(-np.inf)
    A = np.full((B, T, S), NINF, dtype=dtype)
    ll = np.full(B, NINF, dtype=dtype)
    for b in range(B):
        Tb, Sb = int(input_lengths[b]), 2 * int(target_lengths[b]) + 1
        sk = _skip(ext[b], Sb)
        A[b, 0, 0] = lp[0, b, blank]
        if Sb >= 2:
            A[b, 0, 1] = lp[0, b, ext[b, 1]]
        for t in range(1, Tb):
            prev = A[b, t - 1]
            p2 = np.where(sk, _shift(prev, 2, NINF), NINF)
            r = _lse(np.stack([prev, _shift(prev, 1, NINF), p2]), dtype)
            with np.errstate(all="ignore"):
                row = (lp[t, b, ext[b]] + r).astype(dtype)
            row[np.isneginf(r)] = NINF
            row[Sb:] = NINF
            A[b, t] = row
        ends = [A[b, Tb - 1, Sb - 1]] + ([A[b, Tb - 1, Sb - 2]] if Sb >= 2 else [])
        ll[b] = _lse(np.array(ends, dtype=dtype)[:, None], dtype)[0]
    return A, ll


def beta(lp, targets, input_lengths, target_lengths, blank=0, dtype=np.float32):
    """beta (B,T,S') in `dtype`, the reference's convention."""
    lp = np.asarray(lp, dtype=dtype)
    T, B, _ = lp.shape
    ext = expand(targets, blank)
    S = ext.shape[1]
    NINF = dtype(-np.inf)
    Bt = np.full((B, T, S), NINF, dtype=dtype)
    for b in range(B):
        Tb, Sb = int(input_lengths[b]), 2 * int(target_lengths[b]) + 1
        Bt[b, Tb - 1, Sb - 1] = 0
        if Sb >= 2:
            Bt[b, Tb - 1, Sb - 2] = 0
        # mirrored: u = Sb - 1 - s turns "take from s + 1, s + 2" into "take from u - 1, u - 2"
        em = ext[b, :Sb][::-1]
        sk = _skip(em, Sb)
        for t in range(Tb - 2, -1, -1):
            nxt = Bt[b, t + 1, :Sb][::-1]
            with np.errstate(all="ignore"):
                q = (nxt + lp[t + 1, b, em]).astype(dtype)
            q[np.isneginf(nxt)] = NINF
            p2 = np.where(sk, _shift(q, 2, NINF), NINF)
            r = _lse(np.stack([q, _shift(q, 1, NINF), p2]), dtype)
            Bt[b, t, :Sb] = r[::-1]
    return Bt


def viterbi(lp, targets, input_lengths, target_lengths, blank=0):
    """(positions (B,T) int64, -1 past input_lengths[b] and for a pair with no alignment;
    score (B) fp32) of the best single path, in fp32."""
    f = np.float32
    lp = np.asarray(lp, dtype=f)
    T, B, _ = lp.shape
    ext = expand(targets, blank)
    S = ext.shape[1]
    NINF = f(-np.inf)
    pos = np.full((B, T), -1, dtype=np.int64)
    score = np.full(B, NINF, dtype=f)
    for b in range(B):
        Tb, Sb = int(input_lengths[b]), 2 * int(target_lengths[b]) + 1
        sk = _skip(ext[b], Sb)
        v = np.full(S, NINF, dtype=f)
        v[0] = lp[0, b, blank]
        if Sb >= 2:
            v[1] = lp[0, b, ext[b, 1]]
        back = np.zeros((Tb, S), dtype=np.int64)
        for t in range(1, Tb):
            best, d = v.copy(), np.zeros(S, dtype=np.int64)
            p1 = _shift(v, 1, NINF)
            p2 = np.where(sk, _shift(v, 2, NINF), NINF)
            take = p1 > best
            best, d = np.where(take, p1, best), np.where(take, 1, d)
            take = p2 > best
            best, d = np.where(take, p2, best), np.where(take, 2, d)
            with np.errstate(all="ignore"):
                v = (best + lp[t, b, ext[b]]).astype(f)
            v[Sb:] = NINF
            back[t] = d
        s = Sb - 1
        if Sb >= 2 and v[Sb - 2] > v[Sb - 1]:
            s = Sb - 2
        score[b] = v[s]
        if v[s] > NINF:
            for t in range(Tb - 1, -1, -1):
                pos[b, t] = s
                s -= back[t, s]
    return pos, score


def occupancy(lp, targets, input_lengths, target_lengths, blank=0, dtype=np.float64):
    """(gamma (B,T,S'), grad (T,B,C)): gamma = exp(alpha + beta - loglik), 0 where either is -inf,
    and grad[t,b,c] = d loglik[b] / d lp[t,b,c] = the sum of gamma over the positions of class c.
    Both are 0 past input_lengths[b] and for a pair with no alignment."""
    lp = np.asarray(lp, dtype=dtype)
    T, B, C = lp.shape
    A, ll = alpha(lp, targets, input_lengths, target_lengths, blank, dtype)
    Bt = beta(lp, targets, input_lengths, target_lengths, blank, dtype)
    ext = expand(targets, blank)
    gamma = np.zeros(A.shape, dtype=dtype)
    grad = np.zeros((T, B, C), dtype=dtype)
    for b in range(B):
        if not np.isfinite(ll[b]):
            continue
        fin = np.isfinite(A[b]) & np.isfinite(Bt[b])
        with np.errstate(all="ignore"):
            g = np.where(fin, np.exp(np.where(fin, A[b] + Bt[b] - ll[b], 0)), 0)
        gamma[b] = g
        Sb = 2 * int(target_lengths[b]) + 1
        for s in range(Sb):
            grad[:, b, ext[b, s]] += g[:, s]
    return gamma, grad


def posterior_positions(A, Bt, input_lengths):
    """Per frame the lowest position of largest alpha + beta; -1 past input_lengths[b]."""
    with np.errstate(all="ignore"):
        tot = A + Bt
    pos = tot.argmax(axis=2).astype(np.int64)
    for b in range(pos.shape[0]):
        pos[b, int(input_lengths[b]):] = -1
    return pos


def tokens(pos, targets, input_lengths, blank=0):
    ext = expand(targets, blank)
    return [ext[b, np.maximum(pos[b, :int(input_lengths[b])], 0)] for b in range(pos.shape[0])]


# ------------------------------------------------------------------ the acceptance bound
EPS24 = 2.0 ** -24


def alpha_steps(T, B):
    """(B,T,1): recursion steps behind alpha[b,t,:], t + 1"""
    return np.broadcast_to(np.arange(1, T + 1)[None, :, None], (B, T, 1))


def beta_steps(T, input_lengths):
    """(B,T,1): recursion steps behind beta[b,t,:], T_b - t: beta runs down from frame T_b - 1"""
    return np.maximum(np.asarray(input_lengths)[:, None, None] - np.arange(T)[None, :, None], 1)


def step_bound_excess(x, x64, steps):
    """max over the finite entries of |x - x64| / (4 steps 2^-24 max(1, |x64|)): <= 1 passes.
    Each step is an exact max, a few fp32 roundings at the magnitude of the value and an
    expf / logf on O(1) arguments.  inf when the -inf patterns differ."""
    x, x64 = np.asarray(x), np.asarray(x64)
    if not np.array_equal(np.isneginf(x), np.isneginf(x64)) or not np.isfinite(x[np.isfinite(x64)]).all():
        return np.inf
    fin = np.isfinite(x64)
    ref = np.where(fin, x64, 0.0)
    err = np.abs(np.where(fin, x.astype(np.float64) - ref, 0.0))
    return float((err / (4 * steps * EPS24 * np.maximum(1.0, np.abs(ref)))).max(initial=0.0))
