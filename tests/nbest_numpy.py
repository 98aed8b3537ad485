"""The N-best Viterbi contract of include/hmm355.h (hmm355_viterbi_nbest_f32) in numpy fp32: the
model the GPU tests compare against bit for bit, and a brute-force enumerator that validates it.
Not a test file.

All arithmetic is fp32.  The tie order (value descending, then source state, then source rank) is
a stable descending sort of the (N*K, N) candidate block whose row index is i*K + r.
"""
import itertools

import numpy as np

NEG = np.float32(-np.inf)


def nbest_one(lo, log_P, init, K, length=None):
    """lo (T,N) log-emissions, log_P (N,N), init (N), all fp32.  Returns (paths (K,T) int64, scores
    (K) fp32, count): the frames >= length and the ranks >= max(count, 1) hold -1 / -inf."""
    lo, log_P, init = (np.asarray(a, np.float32) for a in (lo, log_P, init))
    T, N = lo.shape
    L = T if length is None else int(length)
    d = np.full((N, K), NEG, np.float32)
    d[:, 0] = init + lo[0]
    ptr = np.zeros((L, N, K), np.int64)
    for t in range(1, L):
        cand = (d[:, :, None] + log_P[:, None, :]).reshape(N * K, N)      # row i*K + r, column j
        order = np.argsort(-cand, axis=0, kind="stable")[:K]              # (K,N)
        d = (np.take_along_axis(cand, order, axis=0) + lo[t][None, :]).T.astype(np.float32).copy()
        ptr[t] = order.T
    flat = d.reshape(N * K)                                               # index j*K + k
    order = np.argsort(-flat, kind="stable")[:K]
    scores = flat[order].astype(np.float32)
    count = int((scores > NEG).sum())
    paths = np.full((K, T), -1, np.int64)
    for m in range(max(count, 1)):
        j, k = divmod(int(order[m]), K)
        for t in range(L - 1, 0, -1):
            paths[m, t] = j
            j, k = divmod(int(ptr[t, j, k]), K)
        paths[m, 0] = j
    scores[max(count, 1):] = NEG
    return paths, scores, count


def nbest(lo, log_P, init, K, lengths=None):
    """Batch form: lo (B,T,N) -> (paths (B,K,T) int64, scores (B,K) fp32, count (B) int32)."""
    B = lo.shape[0]
    out = [nbest_one(lo[b], log_P, init, K, None if lengths is None else lengths[b]) for b in range(B)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.array([o[2] for o in out], np.int32))


def fold(path, lo, log_P, init):
    """The left-folded fp32 score fl(fl(s + log_P[z_{t-1}][z_t]) + lo_t[z_t]) of one path."""
    s = np.float32(init[path[0]]) + np.float32(lo[0, path[0]])
    for t in range(1, len(path)):
        s = np.float32(s + np.float32(log_P[path[t - 1], path[t]]))
        s = np.float32(s + np.float32(lo[t, path[t]]))
    return np.float32(s)


def enumerate_scores(lo, log_P, init):
    """The left-folded fp32 scores of all N^T paths, (N,)*T: entry [z_0, .., z_{T-1}]."""
    lo, log_P, init = (np.asarray(a, np.float32) for a in (lo, log_P, init))
    T, N = lo.shape
    s = (init + lo[0]).astype(np.float32)                                 # (N)
    for t in range(1, T):
        s = ((s[..., None] + log_P) + lo[t]).astype(np.float32)           # (.., z_{t-1}, z_t)
    return s


def top_scores(lo, log_P, init, K):
    """The K largest enumerated scores, descending, padded with -inf when N^T < K."""
    s = np.sort(enumerate_scores(lo, log_P, init).reshape(-1))[::-1][:K]
    return np.concatenate([s, np.full(K - s.size, NEG, np.float32)]).astype(np.float32)


def viterbi_first_index(lo, log_P, init):
    """Plain Viterbi with the first index on ties (a column without a finite candidate takes index
    0, the last frame its first argmax): (states (T), final score)."""
    lo, log_P, init = (np.asarray(a, np.float32) for a in (lo, log_P, init))
    T, N = lo.shape
    delta = (init + lo[0]).astype(np.float32)
    psi = np.zeros((T, N), np.int64)
    for t in range(1, T):
        cand = delta[:, None] + log_P
        psi[t] = np.argmax(cand, axis=0)
        delta = (cand[psi[t], np.arange(N)] + lo[t]).astype(np.float32)
    states = np.zeros(T, np.int64)
    states[-1] = int(np.argmax(delta))
    for t in range(T - 1, 0, -1):
        states[t - 1] = psi[t, states[t]]
    return states, np.float32(delta[states[-1]])


def all_paths(N, T):
    return itertools.product(range(N), repeat=T)
