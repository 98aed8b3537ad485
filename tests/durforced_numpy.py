"""Numpy model of explicit-duration forced alignment (csrc/durforced.hip; the recursions are spelled
out in include/hmm355.h): every output of ops.durforced / ops.durforced_grad.

model(..., dtype=np.float64) is the reference of the tests.  With dtype=np.float32 the same code
keeps its tables in float32 the way the kernels do (exponents of the posteriors and counts formed in
float64 from the float32 tables, sums over time in float64): tools/measure_durforced_tolerance.py
takes the GPU tests' allowances from the distance between the two.  brute_force() enumerates every
segmentation of a tiny pair and shares no code with the recursions.
"""
import itertools

import numpy as np

NINF = -np.inf


def emissions(lp_b, ids_b, Tb, Lb):
    """e (Tb,Lb) float64: log_probs[t, id_l], -inf for an id outside [0, C).  ids_b None: id_l = l."""
    C = lp_b.shape[1]
    ids = np.arange(Lb) if ids_b is None else np.asarray(ids_b[:Lb]).astype(np.int64)
    ok = (ids >= 0) & (ids < C)
    e = np.full((Tb, Lb), NINF)
    e[:, ok] = lp_b[:Tb][:, ids[ok]].astype(np.float64)
    return e, ids, ok


def frame_shift(e):
    """M_t: the maximum over the chain's positions, 0 where there is no finite one."""
    with np.errstate(invalid="ignore"):
        m = e.max(axis=1)
    return np.where(np.isfinite(m), m, 0.0)


def _lse(c, dtype):
    """log-sum-exp over the last axis in `dtype`; -inf candidates drop out, all -inf gives -inf"""
    m = c.max(axis=-1)
    ms = np.where(m == NINF, dtype(0), m).astype(dtype)
    with np.errstate(divide="ignore"):
        s = np.exp((c - ms[..., None]).astype(dtype)).astype(dtype).sum(axis=-1, dtype=dtype)
        r = (ms + np.log(s).astype(dtype)).astype(dtype)
    return np.where(m == NINF, dtype(NINF), r).astype(dtype)


def chain(x, du, dtype, viterbi=False):
    """The forward recursion over x (Tb,Lb) shifted emissions and du (Lb,Dm): (begin, F) and, with
    viterbi, the chosen d - 1 per cell.  seg[l, j] is the open segment of position l that has
    lasted j + 1 frames."""
    Tb, Lb = x.shape
    Dm = du.shape[1]
    x = x.astype(dtype)
    du = du.astype(dtype)
    seg = np.full((Lb, Dm), NINF, dtype)
    begin = np.full((Tb, Lb), NINF, dtype)
    F = np.full((Tb, Lb), NINF, dtype)
    arg = np.zeros((Tb, Lb), np.int64)
    beg = np.full(Lb, NINF, dtype)
    beg[0] = 0
    for t in range(Tb):
        begin[t] = beg
        seg[:, 1:] = seg[:, :-1].copy()
        seg[:, 0] = beg
        seg = (seg + x[t][:, None]).astype(dtype)
        cand = (seg + du).astype(dtype)
        if viterbi:
            arg[t] = cand.argmax(axis=1)   # the first maximum: the smaller d wins a tie
            F[t] = cand.max(axis=1)
        else:
            F[t] = _lse(cand, dtype)
        beg = np.full(Lb, NINF, dtype)
        beg[1:] = F[t, :-1]
    return begin, F, arg


def model(lp, ids, il, sl, dur, dtype=np.float64, viterbi=True):
    """Every output for a batch: log_probs (B,T,C), ids (B,Lmax) or None, lengths (B), dur
    (B,Lmax,Dmax).  Returns a dict of loglik, loglik_shifted (B); begin, F, Bend, Bbeg, gamma
    (B,T,Lmax); frame_shift (B,T); dur_post (B,Lmax,Dmax); grad_lp (B,T,C); and with viterbi score
    (B), durations (B,Lmax), path (B,T)."""
    lp = np.asarray(lp)
    dur = np.asarray(dur)
    B, T, C = lp.shape
    Lm, Dm = dur.shape[1], dur.shape[2]
    f = dtype
    out = dict(loglik=np.full(B, NINF), loglik_shifted=np.full(B, NINF), frame_shift=np.zeros((B, T)),
               gamma=np.zeros((B, T, Lm)), dur_post=np.zeros((B, Lm, Dm)), grad_lp=np.zeros((B, T, C)),
               score=np.full(B, NINF), durations=np.zeros((B, Lm), np.int64), path=np.full((B, T), -1, np.int64))
    for name in ("begin", "F", "Bend", "Bbeg"):
        out[name] = np.full((B, T, Lm), NINF)
    for b in range(B):
        Tb, Lb = int(il[b]), int(sl[b])
        e, cls, ok = emissions(lp[b], None if ids is None else ids[b], Tb, Lb)
        M = frame_shift(e)
        if dtype == np.float32:
            M = M.astype(np.float32).astype(np.float64)
            x = (e.astype(np.float32) - M.astype(np.float32)[:, None]).astype(np.float32)
        else:
            x = e - M[:, None]
        du = dur[b, :Lb].astype(np.float64)
        begin, F, _ = chain(x, du, f)
        bend_r, bbeg_r, _ = chain(x[::-1, ::-1], du[::-1], f)
        Bend, Bbeg = bend_r[::-1, ::-1], bbeg_r[::-1, ::-1]
        out["frame_shift"][b, :Tb] = M
        for name, tab in (("begin", begin), ("F", F), ("Bend", Bend), ("Bbeg", Bbeg)):
            out[name][b, :Tb, :Lb] = tab
        lls = float(F[Tb - 1, Lb - 1])
        out["loglik_shifted"][b] = lls
        if viterbi:
            _, Fv, arg = chain(x, du, f, viterbi=True)
            best = float(Fv[Tb - 1, Lb - 1])
            if best > NINF:
                out["score"][b] = f(best + M.sum())
                t = Tb - 1
                for q in range(Lb - 1, -1, -1):
                    d = int(arg[t, q]) + 1
                    out["durations"][b, q] = d
                    out["path"][b, t - d + 1:t + 1] = q
                    t -= d
                assert t == -1
        if not lls > NINF:
            continue
        out["loglik"][b] = f(lls + M.sum())
        # posteriors: the running sum of P(begins at t) - P(ended at t - 1), exponents in float64
        b64, f64, e64, g64 = (a.astype(np.float64) for a in (begin, F, Bend, Bbeg))
        with np.errstate(invalid="ignore"):
            pb = np.where(np.isfinite(b64) & np.isfinite(g64), np.exp(b64 + g64 - lls), 0.0)
            pe = np.where(np.isfinite(f64) & np.isfinite(e64), np.exp(f64 + e64 - lls), 0.0)
        delta = pb.copy()
        delta[1:] -= pe[:-1]
        gamma = np.cumsum(delta, axis=0).astype(f).astype(np.float64)
        out["gamma"][b, :Tb, :Lb] = gamma
        np.add.at(out["grad_lp"][b, :Tb], (slice(None), cls[ok]), gamma[:, ok])
        # expected (l, d) counts: O(a..t,l) from prefix sums of the finite x and a count of -inf frames
        x64 = x.astype(np.float64)
        fin = np.isfinite(x64)
        P = np.vstack([np.zeros((1, Lb)), np.cumsum(np.where(fin, x64, 0.0), axis=0)])
        Cn = np.vstack([np.zeros((1, Lb), np.int64), np.cumsum(~fin, axis=0)])
        for d in range(min(Dm, Tb)):
            t = np.arange(d, Tb)
            st = t - d
            with np.errstate(invalid="ignore"):
                expo = b64[st] + (P[t + 1] - P[st]) + du[None, :, d] + e64[t] - lls
            live = np.isfinite(b64[st]) & np.isfinite(e64[t]) & (Cn[t + 1] == Cn[st]) & np.isfinite(du[None, :, d])
            if dtype == np.float32:
                term = np.exp(np.where(live, expo, 0.0).astype(np.float32)).astype(np.float64)
            else:
                term = np.exp(np.where(live, expo, 0.0))
            out["dur_post"][b, :Lb, d] = np.where(live, term, 0.0).sum(axis=0)
    if dtype == np.float32:
        for k in ("gamma", "dur_post", "grad_lp"):
            out[k] = out[k].astype(np.float32).astype(np.float64)
    return out


def rescore(lp_b, ids_b, dur_b, durations, Tb, Lb):
    """The float64 score of a segmentation d_0 .. d_{Lb-1} (sum must be Tb)."""
    e, _, _ = emissions(lp_b, ids_b, Tb, Lb)
    s, t = 0.0, 0
    for q in range(Lb):
        d = int(durations[q])
        s += float(dur_b[q, d - 1]) + float(e[t:t + d, q].sum())
        t += d
    assert t == Tb
    return s


def brute_force(lp_b, ids_b, Tb, Lb, dur_b):
    """One pair by enumeration of every segmentation: dict of loglik, gamma (Tb,Lb), dur_post
    (Lb,Dm), best score, best durations (the tie rule: of equal scores the one with the smallest
    d_{Lb-1}, then the smallest d_{Lb-2}, ...), or loglik -inf and None for an infeasible pair."""
    Dm = dur_b.shape[1]
    e, _, _ = emissions(lp_b, ids_b, Tb, Lb)
    segs, scores = [], []
    for ds in itertools.product(range(1, Dm + 1), repeat=Lb):
        if sum(ds) != Tb:
            continue
        s, t = 0.0, 0
        for q, d in enumerate(ds):
            s += float(dur_b[q, d - 1]) + float(e[t:t + d, q].sum())
            t += d
        if s > NINF:
            segs.append(ds)
            scores.append(s)
    if not segs:
        return dict(loglik=NINF, gamma=np.zeros((Tb, Lb)), dur_post=np.zeros((Lb, Dm)), score=NINF, durations=None)
    scores = np.array(scores)
    m = scores.max()
    ll = m + np.log(np.exp(scores - m).sum())
    w = np.exp(scores - ll)
    gamma = np.zeros((Tb, Lb))
    dp = np.zeros((Lb, Dm))
    for ds, p in zip(segs, w):
        t = 0
        for q, d in enumerate(ds):
            gamma[t:t + d, q] += p
            dp[q, d - 1] += p
            t += d
    best = min((ds for ds, s in zip(segs, scores) if s == m), key=lambda ds: ds[::-1])
    return dict(loglik=ll, gamma=gamma, dur_post=dp, score=m, durations=np.array(best))
