"""The ragged results as the oracle applied to each obs[b, :len_b] and padded by the convention
of include/hmm355.h: posterior / forward / backward 0, log_delta -inf and states -1 in frames
>= len_b.  Shared by tests/test_ragged_cpu.py and tests/test_gpu_ragged.py."""
import numpy as np
import torch

from oracle import hmm_oracle as O


def viterbi_from_log(lo, lP, init, lengths):
    """(states (B,T) int64, delta (B,T,N) fp32, final (B) fp32) as torch tensors."""
    lo = torch.as_tensor(lo)
    B, T, N = lo.shape
    states = torch.full((B, T), -1, dtype=torch.int64)
    delta = torch.full((B, T, N), float("-inf"))
    final = torch.zeros(B)
    for b, n in enumerate(int(x) for x in lengths):
        s, d = O.viterbi_from_log(lo[b:b + 1, :n], torch.as_tensor(lP), torch.as_tensor(init))
        states[b, :n], delta[b, :n] = s[0], d[0]
        final[b] = d[0, -1].max()
    return states, delta, final


def forward_backward(obs, lP, lp0, lengths):
    """(posterior, forward, backward) fp32 (B,T,N) through the oracle's restatement of hmm.py:66-130."""
    obs = torch.as_tensor(obs)
    outs = [torch.zeros(obs.shape) for _ in range(3)]
    for b, n in enumerate(int(x) for x in lengths):
        res = O.forward_backward(obs[b:b + 1, :n], lP, lp0)
        for o, r in zip(outs, res[:3]):
            o[b, :n] = r[0]
    return tuple(outs)


def fb64(lo, lP, lp0, lengths):
    """The float64 C oracle per slice: (log alpha, log beta) padded with -inf, posterior with 0,
    loglik (B)."""
    lo = np.asarray(lo, np.float32)
    B, T, N = lo.shape
    la = np.full((B, T, N), -np.inf)
    lb = np.full((B, T, N), -np.inf)
    post = np.zeros((B, T, N))
    ll = np.zeros(B)
    for b, n in enumerate(int(x) for x in lengths):
        a, bb, p, l = O.c_fb64(lo[b:b + 1, :n], np.asarray(lP), np.asarray(lp0))
        la[b, :n], lb[b, :n], post[b, :n], ll[b] = a[0], bb[0], p[0], l[0]
    return la, lb, post, ll


def compute_likelihood(obs, lP, lp0, lengths):
    obs = torch.as_tensor(obs)
    return torch.stack([O.compute_likelihood(obs[b:b + 1, :int(n)], lP, lp0)[0] for b, n in enumerate(lengths)])
