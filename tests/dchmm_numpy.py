"""numpy restatement of the duration-penalty Viterbi (include/hmm355.h, "Duration-constrained
Viterbi"): the GPU tests' oracle on shapes without a fixture, itself pinned to the reference's
fixtures in tests/test_dchmm_cpu.py.

Every arithmetic step is one numpy float32 operation, i.e. one fp32 rounding, in the order the
reference takes them: (delta + lT) + e, then + penalty; the penalty is one fp32 product and an
absent penalty is no add at all.  `viterbi` is vectorised over the predecessor p and the state s
(one (G,S,S) candidate block per step); `viterbi_loops` is the same thing as three plain loops.
`group` is the number of consecutive sequences that share their penalties (None: the whole
batch, as the reference does; 1: every sequence alone).
"""
import math

import numpy as np

FIXTURES = ("b1", "b3", "ties", "neginf", "t1", "long")
F32 = np.float32
NINF = F32(-np.inf)


def _backtrace(delta, psi):
    B, T, _ = delta.shape
    states = np.zeros((B, T), dtype=np.int64)
    states[:, T - 1] = np.argmax(delta[:, T - 1], axis=1)  # the first maximum
    for t in range(T - 2, -1, -1):
        states[:, t] = psi[np.arange(B), t + 1, states[:, t + 1]]
    return states


def _groups(B, group):
    G = B if group is None else int(group)
    return [slice(k, min(B, k + G)) for k in range(0, B, G)]


def viterbi(e, lT, min_duration, max_duration, w=0.1, group=None, stats=None):
    """(states (B,T) int64, delta (B,T,S) float32, dur (B,T,S) int32); a dict given as `stats`
    gets "ties": how many cells were decided by the first-index rule"""
    e, lT = np.asarray(e, dtype=F32), np.asarray(lT, dtype=F32)
    B, T, S = e.shape
    negw = F32(-F32(w))
    delta = np.full((B, T, S), NINF, dtype=F32)
    psi = np.zeros((B, T, S), dtype=np.int64)
    dur = np.zeros((B, T, S), dtype=np.int32)
    delta[:, 0] = e[:, 0] - F32(math.log(S))
    dur[:, 0] = 1
    diag = np.arange(S)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in _groups(B, group):
            for t in range(1, T):
                dp, up, et = delta[g, t - 1], dur[g, t - 1], e[g, t]
                dmax1, dmin = up.max(axis=0) + 1, up.min(axis=0)
                has_self, has_from = dmax1 > max_duration, dmin < min_duration
                pen_self = negw * (dmax1 - max_duration).astype(F32)
                pen_from = negw * (min_duration - dmin).astype(F32)
                cand = (dp[:, :, None] + lT[None, :, :]) + et[:, None, :]          # [b, p, s]
                cand = np.where(has_from[None, :, None], cand + pen_from[None, :, None], cand)
                own = dp + et
                own = np.where(has_self[None, :], own + pen_self[None, :], own)
                cand[:, diag, diag] = own
                arg = np.argmax(cand, axis=1)                                        # first maximum
                best = np.take_along_axis(cand, arg[:, None, :], axis=1)[:, 0, :]
                dead = best == NINF
                if stats is not None:   # live cells whose best score more than one predecessor attains
                    stats["ties"] = stats.get("ties", 0) + int((((cand == best[:, None, :]).sum(axis=1) > 1) & ~dead).sum())
                delta[g, t] = best
                psi[g, t] = np.where(dead, 0, arg)
                dur[g, t] = np.where(dead, 0, np.where(arg == diag[None, :], up + 1, 1))
    return _backtrace(delta, psi), delta, dur


def viterbi_loops(e, lT, min_duration, max_duration, w=0.1, group=None):
    """the same recursion cell by cell"""
    e, lT = np.asarray(e, dtype=F32), np.asarray(lT, dtype=F32)
    B, T, S = e.shape
    negw = F32(-F32(w))
    delta = np.full((B, T, S), NINF, dtype=F32)
    psi = np.zeros((B, T, S), dtype=np.int64)
    dur = np.zeros((B, T, S), dtype=np.int32)
    delta[:, 0] = e[:, 0] - F32(math.log(S))
    dur[:, 0] = 1
    for g in _groups(B, group):
        for t in range(1, T):
            dmax1 = dur[g, t - 1].max(axis=0) + 1
            dmin = dur[g, t - 1].min(axis=0)
            for b in range(g.start, g.stop):
                for s in range(S):
                    best, arg, run = NINF, 0, 0
                    for p in range(S):
                        if p == s:
                            x = F32(delta[b, t - 1, s] + e[b, t, s])
                            if dmax1[s] > max_duration:
                                x = F32(x + F32(negw * F32(dmax1[s] - max_duration)))
                            new = dur[b, t - 1, s] + 1
                        else:
                            x = F32(F32(delta[b, t - 1, p] + lT[p, s]) + e[b, t, s])
                            if dmin[p] < min_duration:
                                x = F32(x + F32(negw * F32(min_duration - dmin[p])))
                            new = 1
                        if x > best:
                            best, arg, run = x, p, new
                    delta[b, t, s], psi[b, t, s], dur[b, t, s] = best, arg, run
    return _backtrace(delta, psi), delta, dur
