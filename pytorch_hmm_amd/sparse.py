"""HMMs whose transitions are an arc list: a sparse transition matrix (csrc/sparse.hip).

A left-to-right, skip-state, phone-loop or pronunciation-graph model of N states has a few arcs
per state, not N^2.  `SparseTransitions` holds such a graph sorted the two ways the kernels read
it, and `SparseHMM` decodes, sums, differentiates and re-estimates over it at a cost proportional
to the arcs, up to 8192 states and 2^20 arcs.  The semantics are exactly those of the dense model
whose log_P is -inf off the arcs; emissions are log-emissions (B,T,N).  Tensors passed to the
computing methods must be on a ROCm GPU; building and validating a graph works on any device.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from . import ops
from . import range_guard as rg
from .autograd import SparseLogLik

MAX_STATES = ops.SPARSE_MAX_STATES
MAX_ARCS = ops.SPARSE_MAX_ARCS


def _ids(t, name):
    t = torch.as_tensor(t)
    if t.numel() == 0:
        t = t.to(torch.int64)   # an empty list has no dtype of its own
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{name} must hold integers; got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{name} must be one-dimensional; got {tuple(t.shape)}")
    return t.detach().to("cpu", torch.int64)


class SparseTransitions:
    """The arcs (src[e], dst[e], log_w[e]) of an N-state model, validated on the host and sorted
    once: by (dst, src) for Viterbi and the forward chain, by (src, dst) for the backward chain.

    src, dst: E integer state ids in [0, num_states); log_w: E log weights (-inf allowed; may
    require grad).  Self-loops are allowed; a repeated (src, dst) pair, an id out of range,
    mismatched lengths, num_states outside [1, 8192] or E outside [1, 2^20] is a ValueError.

    Kept, on log_w's device: src, dst (int32, the caller's order), perm_in / perm_out (int64: the
    caller's index of the k-th arc in each sorted order), inv_in / inv_out (the inverse
    permutations), in_ptr / in_src / in_dst and out_ptr / out_src / out_dst (int32); on the host:
    in_ptr_host, out_ptr_host (int32 (N+1), the row pointers the library validates)."""

    def __init__(self, src, dst, log_w: Tensor, num_states: int):
        N = int(num_states)
        if N < 1 or N > MAX_STATES:
            raise ValueError(f"num_states must lie in [1, {MAX_STATES}]; got {num_states}")
        s, d = _ids(src, "src"), _ids(dst, "dst")
        log_w = torch.as_tensor(log_w)
        if log_w.dim() != 1 or not log_w.dtype.is_floating_point:
            raise ValueError(f"log_w must be a one-dimensional floating tensor; got {tuple(log_w.shape)} {log_w.dtype}")
        E = log_w.numel()
        if s.numel() != E or d.numel() != E:
            raise ValueError(f"src, dst and log_w must have one entry per arc; got {s.numel()}, {d.numel()}, {E}")
        if E < 1 or E > MAX_ARCS:
            raise ValueError(f"the number of arcs must lie in [1, {MAX_ARCS}]; got {E}")
        if int(s.min()) < 0 or int(s.max()) >= N or int(d.min()) < 0 or int(d.max()) >= N:
            raise ValueError(f"state ids must lie in [0, {N}); got src in [{int(s.min())}, {int(s.max())}], "
                             f"dst in [{int(d.min())}, {int(d.max())}]")
        key_in = d * N + s
        perm_in = torch.argsort(key_in)
        sorted_in = key_in[perm_in]
        dup = sorted_in[1:] == sorted_in[:-1]
        if bool(dup.any()):
            k = int(sorted_in[1:][dup][0])
            raise ValueError(f"the arc ({k % N} -> {k // N}) appears more than once")
        perm_out = torch.argsort(s * N + d)
        dev = log_w.device
        self.num_states, self.num_arcs = N, E
        self.log_w = log_w
        i32 = torch.int32

        def ptr(ids):
            p = torch.zeros(N + 1, dtype=torch.int64)
            p[1:] = torch.cumsum(torch.bincount(ids, minlength=N), 0)
            return p.to(i32).contiguous()
        self.in_ptr_host, self.out_ptr_host = ptr(d), ptr(s)
        self.src, self.dst = s.to(i32).to(dev), d.to(i32).to(dev)
        self.perm_in, self.perm_out = perm_in.to(dev), perm_out.to(dev)
        self.inv_in, self.inv_out = torch.argsort(perm_in).to(dev), torch.argsort(perm_out).to(dev)
        self.in_ptr, self.out_ptr = self.in_ptr_host.to(dev), self.out_ptr_host.to(dev)
        self.in_src, self.in_dst = s[perm_in].to(i32).to(dev), d[perm_in].to(i32).to(dev)
        self.out_src, self.out_dst = s[perm_out].to(i32).to(dev), d[perm_out].to(i32).to(dev)

    _DEVICE_FIELDS = ("src", "dst", "perm_in", "perm_out", "inv_in", "inv_out", "in_ptr", "out_ptr", "in_src",
                      "in_dst", "out_src", "out_dst", "log_w")

    def to(self, device) -> "SparseTransitions":
        """The same graph with its tensors on `device` (the sort is not repeated)."""
        other = object.__new__(SparseTransitions)
        other.__dict__.update(self.__dict__)
        for f in self._DEVICE_FIELDS:
            setattr(other, f, getattr(self, f).to(device))
        return other

    @classmethod
    def from_dense(cls, log_P: Tensor) -> "SparseTransitions":
        """The arcs of a dense (N,N) log matrix: every entry above -inf, row-major."""
        if log_P.dim() != 2 or log_P.shape[0] != log_P.shape[1]:
            raise ValueError(f"log_P must be (N, N); got {tuple(log_P.shape)}")
        idx = torch.nonzero(log_P.detach() > -float("inf"))
        return cls(idx[:, 0], idx[:, 1], log_P[idx[:, 0], idx[:, 1]], log_P.shape[0])

    def to_dense(self, log_w: Optional[Tensor] = None) -> Tensor:
        """The (N,N) log matrix: log_w on the arcs, -inf elsewhere."""
        w = self.log_w if log_w is None else log_w
        out = w.new_full((self.num_states, self.num_states), -float("inf"))
        return out.index_put((self.src.long(), self.dst.long()), w)

    def max_in_degree(self) -> int:
        return int((self.in_ptr_host[1:] - self.in_ptr_host[:-1]).max())

    def max_out_degree(self) -> int:
        return int((self.out_ptr_host[1:] - self.out_ptr_host[:-1]).max())


def sparse_viterbi(transitions: SparseTransitions, log_obs: Tensor, log_p0: Tensor, log_w: Optional[Tensor] = None,
                   lengths=None) -> Tuple[Tensor, Tensor, Tensor]:
    """(states (B,T) int64, log_delta (B,T,N), final_score (B)) over the arcs: the bits of
    ops.viterbi / ops.viterbi_ragged on transitions.to_dense()."""
    tr = transitions
    w = tr.log_w if log_w is None else log_w
    return ops.sparse_viterbi(log_obs, tr.in_ptr_host, tr.in_ptr, tr.in_src, w.detach().to(torch.float32)[tr.perm_in],
                              log_p0, lengths)


def sparse_e_step(transitions: SparseTransitions, log_obs: Tensor, log_p0: Tensor, log_w: Optional[Tensor] = None,
                  lengths=None, weight: Optional[Tensor] = None, want_posterior: bool = True,
                  want_counts: bool = True, range_guard: bool = True
                  ) -> Tuple[Tensor, Optional[Tensor], Optional[Tensor]]:
    """(loglik (B), gamma (B,T,N) or None, xi (E) fp64 in the caller's arc order or None): one
    forward-backward call and, for xi, one arc-count call over the rows it leaves.

    range_guard (default on): the sequences that left the kernels' fp32 range
    (range_guard.out_of_range over the workspace's rows -- an arc list is a table of exact zeros,
    where that can happen) are recomputed in float64 log space and their loglik, gamma and share
    of xi replaced; the others keep the kernels' bits.  One host read of a flag per call; skipped
    while a CUDA graph is being captured."""
    tr = transitions
    w = (tr.log_w if log_w is None else log_w).detach().to(torch.float32)
    host = None if lengths is None else ops.ragged_lengths(lengths, log_obs.shape[0], log_obs.shape[1])
    obs = log_obs.detach().to(torch.float32).contiguous()
    loglik, post, ws = ops.sparse_forward_backward(obs, tr.in_ptr_host, tr.in_ptr, tr.in_src, w[tr.perm_in],
                                                   tr.out_ptr_host, tr.out_ptr, tr.out_dst, w[tr.perm_out], log_p0,
                                                   want_posterior, host)
    bad = rg.sparse_flagged(ws, obs, host) if range_guard and obs.shape[0] else None
    xi = None
    if want_counts:
        # the destination order: neighbouring threads read neighbouring states
        xi = ops.sparse_arc_counts(obs, tr.in_src, tr.in_dst, w[tr.perm_in], ws, weight, host)[tr.inv_in]
    if bad is not None:
        ll, g, x = rg.logspace_forward_backward(obs[bad], log_p0, src=tr.src, dst=tr.dst, log_w=w,
                                                lengths=None if host is None else host.to(obs.device)[bad],
                                                weight=None if weight is None else weight[bad], want_xi=want_counts)
        loglik = loglik.index_copy(0, bad, ll.to(loglik.dtype))
        if want_posterior:
            post = post.index_copy(0, bad, g.to(post.dtype))
        if want_counts:
            xi = xi + x
    return loglik, (post if want_posterior else None), xi


def sparse_transition_m_step(xi: Tensor, src: Tensor, old_log_w: Tensor, num_states: int,
                             min_occupancy: float = 1e-6) -> Tensor:
    """log_w' (E): xi normalised over the arcs that share a source, in fp64.  A source whose total
    count is below min_occupancy keeps its old weights (as em.transition_m_step keeps a row); an
    exact zero of xi stays an exact zero probability (log_w' = -inf).  Pure torch, any device."""
    x = xi.to(torch.float64)
    s = src.long()
    tot = torch.zeros(num_states, dtype=torch.float64, device=x.device).index_add_(0, s, x)[s]
    ok = tot >= min_occupancy
    new = torch.log(x / torch.where(ok, tot, torch.ones_like(tot)))
    return torch.where(ok, new, old_log_w.to(torch.float64)).to(old_log_w.dtype)


class SparseHMM(nn.Module):
    """An HMM over an arc list.  log_w (E, the caller's arc order) and log_p0 (N) are parameters
    (trainable=True, the default) or buffers; the graph itself is fixed.

        hmm = SparseHMM(SparseTransitions(src, dst, log_w, N), log_p0).cuda()
        states, score = hmm.viterbi_decode(log_obs, lengths=lengths)
        loss = -hmm.log_likelihood(log_obs).sum(); loss.backward()
        hmm.reestimate(log_obs)                      # one Baum-Welch update

    log_obs is (B,T,N) log-emissions on the GPU (a (T,N) sequence is taken as a batch of one);
    lengths is accepted throughout, in any form ops.ragged_lengths takes."""

    _GRAPH = ("src", "dst", "perm_in", "perm_out", "inv_in", "inv_out", "in_ptr", "out_ptr", "in_src", "in_dst",
              "out_src", "out_dst")

    def __init__(self, transitions: SparseTransitions, log_p0: Optional[Tensor] = None, trainable: bool = True):
        super().__init__()
        tr = transitions
        self.num_states, self.num_arcs = tr.num_states, tr.num_arcs
        w = tr.log_w.detach().clone().to(torch.float32)
        if log_p0 is None:
            log_p0 = torch.full((tr.num_states,), -float(torch.log(torch.tensor(float(tr.num_states)))))
        p0 = torch.as_tensor(log_p0).detach().clone().to(torch.float32).to(w.device)
        if p0.shape != (tr.num_states,):
            raise ValueError(f"log_p0 must be ({tr.num_states},); got {tuple(p0.shape)}")
        if trainable:
            self.log_w, self.log_p0 = nn.Parameter(w), nn.Parameter(p0)
        else:
            self.register_buffer("log_w", w)
            self.register_buffer("log_p0", p0)
        for f in self._GRAPH:
            self.register_buffer("_" + f, getattr(tr, f), persistent=False)
        self._in_ptr_host, self._out_ptr_host = tr.in_ptr_host, tr.out_ptr_host

    @classmethod
    def from_dense(cls, log_P: Tensor, log_p0: Optional[Tensor] = None, trainable: bool = True) -> "SparseHMM":
        return cls(SparseTransitions.from_dense(log_P), log_p0, trainable)

    @property
    def transitions(self) -> SparseTransitions:
        """The graph with the module's current weights, on the module's device."""
        tr = object.__new__(SparseTransitions)
        tr.num_states, tr.num_arcs = self.num_states, self.num_arcs
        tr.in_ptr_host, tr.out_ptr_host = self._in_ptr_host, self._out_ptr_host
        for f in self._GRAPH:
            setattr(tr, f, getattr(self, "_" + f))
        tr.log_w = self.log_w
        return tr

    def to_dense(self) -> Tensor:
        return self.transitions.to_dense()

    @staticmethod
    def _batch(log_obs):
        if log_obs.dim() == 2:
            return log_obs.unsqueeze(0), True
        return log_obs, False

    def viterbi_decode(self, log_obs: Tensor, lengths=None) -> Tuple[Tensor, Tensor]:
        """(states (B,T) int64, final_score (B)): the most probable state path of every sequence;
        padded frames get state -1."""
        obs, squeeze = self._batch(log_obs)
        states, _, score = sparse_viterbi(self.transitions, obs, self.log_p0.detach(), lengths=lengths)
        return (states.squeeze(0), score.squeeze(0)) if squeeze else (states, score)

    def forward_backward(self, log_obs: Tensor, lengths=None) -> Tuple[Tensor, Tensor]:
        """(posterior (B,T,N), loglik (B)); no gradients."""
        obs, squeeze = self._batch(log_obs)
        loglik, post, _ = sparse_e_step(self.transitions, obs, self.log_p0.detach(), lengths=lengths, want_counts=False)
        return (post.squeeze(0), loglik.squeeze(0)) if squeeze else (post, loglik)

    def posteriors(self, log_obs: Tensor, lengths=None) -> Tensor:
        return self.forward_backward(log_obs, lengths)[0]

    def log_likelihood(self, log_obs: Tensor, lengths=None) -> Tensor:
        """loglik (B), differentiable in log_obs, log_w and log_p0 (autograd.SparseLogLik)."""
        obs, squeeze = self._batch(log_obs)
        host = None if lengths is None else ops.ragged_lengths(lengths, obs.shape[0], obs.shape[1])
        ll = SparseLogLik.apply(obs, self.log_w, self.log_p0, self.transitions, host)
        return ll.squeeze(0) if squeeze else ll

    forward = log_likelihood

    def e_step(self, log_obs: Tensor, lengths=None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """(loglik (B), gamma (B,T,N), xi (E) fp64 in the caller's arc order, gamma0 (N) fp64: the
        initial-state counts).  Sequences with no path contribute zeros."""
        obs, _ = self._batch(log_obs)
        loglik, post, xi = sparse_e_step(self.transitions, obs, self.log_p0.detach(), lengths=lengths)
        return loglik, post, xi, post[:, 0].to(torch.float64).sum(0)

    @torch.no_grad()
    def reestimate(self, log_obs: Tensor, lengths=None, min_occupancy: float = 1e-6) -> Tensor:
        """One Baum-Welch update of log_w and log_p0 in place from one padded batch; returns the
        batch's log-likelihoods (B) under the parameters before the update.  Sequences with no
        path are left out of the initial-state estimate."""
        loglik, _, xi, g0 = self.e_step(log_obs, lengths)
        n_seq = int((loglik > -float("inf")).sum())
        self.log_w.copy_(sparse_transition_m_step(xi, self._src, self.log_w, self.num_states, min_occupancy))
        if n_seq > 0:
            self.log_p0.copy_(torch.log(g0 / n_seq).to(self.log_p0.dtype))
        return loglik
