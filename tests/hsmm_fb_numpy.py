"""The explicit-duration (HSMM) forward-backward in numpy: the yardstick of the GPU op
(ops.hsmm_forward_backward, csrc/hsmm_fb.hip) and of its tolerances.

The model is the segment Viterbi's (hmm355_hsmm_viterbi_f32) with sums in place of maxima: a
segmentation (s_1,d_1)..(s_K,d_K) of T frames has sum d_k = T exactly, 1 <= d_k <= Dmax and
s_k != s_k+1 (log_T's diagonal is never used); its score is

    sum_k dur_lp[s_k, d_k-1] + (lp over its frames) + (k = 1 ? log_init[s_1] : log_T[s_k-1, s_k]).

hsmm_fb() runs the recursions of include/hmm355.h in `dtype` (float64: the reference values;
float32: the error an fp32 implementation of the same recursions makes, from which the GPU
tests take their allowances).  Frame t is shifted by M_t = max_s lp[t,s] (0 for a row without
a finite maximum); the sum of M_t is carried in float64 and added to loglik.  The running sums
behind gamma are float64 in either mode, as in the kernel.  enumerate_segmentations() is the brute
force for tiny shapes.
"""
import numpy as np

NINF = -np.inf


def lse(a, axis=0):
    """log-sum-exp along `axis` with the slice's own maximum; -inf entries drop out and a slice
    without a finite entry gives -inf (no NaN, no warning)."""
    a = np.asarray(a)
    m = np.max(a, axis=axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0).astype(a.dtype)
    with np.errstate(divide="ignore"):
        r = ms + np.log(np.sum(np.exp(a - ms), axis=axis, keepdims=True, dtype=a.dtype))
    r = np.where(m == NINF, NINF, r).astype(a.dtype)
    return np.squeeze(r, axis=axis)


def _safe_exp(x):
    """exp with -inf (and NaN from -inf - -inf, which callers mask) -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.exp(np.where(np.isfinite(x), x, 0)), 0).astype(x.dtype)


def hsmm_fb_one(lp, dur_lp, log_T, log_init=None, dtype=np.float64, shift=True, counts=True):
    """One sequence.  lp (T,S), dur_lp (S,Dmax), log_T (S,S), log_init (S) or None (zeros).
    -> dict(loglik, gamma (T,S), dur_counts (S,Dmax), trans_counts (S,S), init_post (S))."""
    lp = np.asarray(lp, dtype=dtype)
    du = np.asarray(dur_lp, dtype=dtype)
    T, S = lp.shape
    Dm = du.shape[1]
    lt = np.array(log_T, dtype=dtype)
    lt[np.arange(S), np.arange(S)] = NINF
    li = np.zeros(S, dtype) if log_init is None else np.asarray(log_init, dtype=dtype)
    if shift:
        M = lp.max(axis=1)
        M = np.where(np.isfinite(M), M, 0).astype(dtype)
    else:
        M = np.zeros(T, dtype)
    with np.errstate(invalid="ignore"):
        x = (lp - M[:, None]).astype(dtype)
    sum_m = float(np.sum(M.astype(np.float64)))

    begin = np.full((T, S), NINF, dtype)
    F = np.full((T, S), NINF, dtype)
    Bend = np.full((T, S), NINF, dtype)
    Bbeg = np.full((T, S), NINF, dtype)
    # forward: open[:, k] = begin + emissions so far of the segment that started at step k mod Dm
    open_ = np.full((S, Dm), NINF, dtype)
    begin[0] = li
    for t in range(T):
        open_[:, t % Dm] = begin[t]
        open_ += x[t][:, None]
        d = (t - np.arange(Dm)) % Dm  # duration - 1 of slot k (slots not yet started are -inf)
        F[t] = lse(open_ + du[np.arange(S)[:, None], d[None, :]], axis=1)
        if t + 1 < T:
            begin[t + 1] = lse(F[t][:, None] + lt, axis=0)
    ll = lse(F[T - 1], axis=0)
    # backward: the same on reversed time
    open_ = np.full((S, Dm), NINF, dtype)
    Bend[T - 1] = 0
    for u in range(T):
        t = T - 1 - u
        open_[:, u % Dm] = Bend[t]
        open_ += x[t][:, None]
        d = (u - np.arange(Dm)) % Dm
        Bbeg[t] = lse(open_ + du[np.arange(S)[:, None], d[None, :]], axis=1)
        if t > 0:
            Bend[t - 1] = lse(lt + Bbeg[t][None, :], axis=1)
    out = {"loglik": dtype(ll) + dtype(sum_m) if np.isfinite(ll) else dtype(NINF),
           "loglik64": float(ll) + sum_m if np.isfinite(ll) else NINF,
           "ll_shifted": ll, "ll_backward": lse(li + Bbeg[0], axis=0)}
    if not counts:
        return out
    gamma = np.zeros((T, S), dtype)
    dur_counts = np.zeros((S, Dm), dtype)
    trans_counts = np.zeros((S, S), dtype)
    init_post = np.zeros(S, dtype)
    if np.isfinite(ll):
        with np.errstate(invalid="ignore"):
            pb = _safe_exp(begin + Bbeg - ll).astype(np.float64)
            pe = _safe_exp(F + Bend - ll).astype(np.float64)
            init_post = _safe_exp(li + Bbeg[0] - ll)
        cb = np.cumsum(pb, axis=0)
        ce = np.cumsum(pe, axis=0)
        g = cb.copy()
        g[1:] -= ce[:-1]
        gamma = g.astype(dtype)
        dc = np.zeros((S, Dm), np.float64)
        acc = np.zeros((T, S), dtype)  # acc[a] = O(a..a+d-1), every start a at once
        for d in range(1, min(Dm, T) + 1):
            n = T - d + 1
            acc[:n] = acc[:n] + x[d - 1:d - 1 + n]
            with np.errstate(invalid="ignore"):
                term = _safe_exp(begin[:n] + acc[:n] + du[:, d - 1][None, :] + Bend[d - 1:d - 1 + n] - ll)
            dc[:, d - 1] = np.sum(term, axis=0, dtype=np.float64)
        dur_counts = dc.astype(dtype)
        tc = np.zeros((S, S), np.float64)
        for t in range(T - 1):
            with np.errstate(invalid="ignore"):
                tc += _safe_exp(F[t][:, None] + lt + Bbeg[t + 1][None, :] - ll)
        trans_counts = tc.astype(dtype)
    out.update(gamma=gamma, dur_counts=dur_counts, trans_counts=trans_counts, init_post=init_post)
    return out


def hsmm_fb(lp, dur_lp, log_T, log_init=None, dtype=np.float64, shift=True, counts=True):
    """A batch: lp (B,T,S).  Stacks hsmm_fb_one's outputs along a leading batch axis."""
    rows = [hsmm_fb_one(lp[b], dur_lp, log_T, log_init, dtype, shift, counts) for b in range(len(lp))]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def enumerate_segmentations(lp, dur_lp, log_T, log_init=None):
    """Brute force over every segmentation of one tiny sequence, float64: the same outputs as
    hsmm_fb_one."""
    lp = np.asarray(lp, np.float64)
    du = np.asarray(dur_lp, np.float64)
    lt = np.asarray(log_T, np.float64)
    T, S = lp.shape
    Dm = du.shape[1]
    li = np.zeros(S) if log_init is None else np.asarray(log_init, np.float64)
    segs = []

    def rec(t, prev, score, path):
        if t == T:
            segs.append((score, list(path)))
            return
        for s in range(S):
            if s == prev:
                continue
            for d in range(1, min(Dm, T - t) + 1):
                sc = score + du[s, d - 1] + lp[t:t + d, s].sum() + (li[s] if prev < 0 else lt[prev, s])
                if sc == NINF:
                    continue
                path.append((s, d))
                rec(t + d, s, sc, path)
                path.pop()

    rec(0, -1, 0.0, [])
    gamma = np.zeros((T, S))
    dur_counts = np.zeros((S, Dm))
    trans_counts = np.zeros((S, S))
    init_post = np.zeros(S)
    if not segs:
        return {"loglik": NINF, "gamma": gamma, "dur_counts": dur_counts, "trans_counts": trans_counts,
                "init_post": init_post}
    scores = np.array([s for s, _ in segs])
    ll = float(lse(scores, axis=0))
    for sc, path in segs:
        w = np.exp(sc - ll)
        t = 0
        init_post[path[0][0]] += w
        for k, (s, d) in enumerate(path):
            gamma[t:t + d, s] += w
            dur_counts[s, d - 1] += w
            if k > 0:
                trans_counts[path[k - 1][0], s] += w
            t += d
    return {"loglik": ll, "gamma": gamma, "dur_counts": dur_counts, "trans_counts": trans_counts,
            "init_post": init_post}
