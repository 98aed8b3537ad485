"""The fp32 range of the scaled forward-backward kernels: a detector and a log-space fallback.

The sum-product kernels keep state probabilities in fp32, rescaled once per step by one factor for
the whole row, and shift a frame's log-emissions by their maximum over all states.  A state more
than about 87 nats behind its row's leader is therefore exactly 0.  With floored tables
(log(P + 1e-8)) the leader refills every state each step and nothing is lost; with exact zeros in
the table the leader may be a state that no path reaches, or that leads nowhere, and then the
states that carry the sequence's whole probability are flushed: a feasible sequence comes out
infeasible, or (both chains surviving in different components) with a finite wrong likelihood.

out_of_range() reads the rows a forward-backward call leaves anyway and flags the sequences
whose result cannot be trusted; logspace_forward_backward() recomputes those alone in float64
log space with plain torch.  The guarded entry points (em.e_step, sparse.sparse_e_step,
autograd.SequenceLogLik / SparseLogLik and what calls them) replace the flagged sequences' results
and keep every other sequence's bits.  The raw ops (ops.forward_backward, ...) are in-range only
(include/hmm355.h).

The bound ("fp32 range").  A value lost to flushing is below 2^-126 in a row whose
leader the kernels keep near 1.  The detector asks, at every valid frame, that
    f_t = sum_j (A^T U_{t-1})_j e_t[j] / sum U_{t-1}      (the share of the forward mass that survives e_t)
    b_t = sum_j e_t[j] V_t[j] / max V_t                   (the same for the backward row)
    r_t = max_i (A (e_t V_t))_i / sum_j e_t[j] V_t[j]      (the best state's reach into that row)
    o_t = sum_j U_t[j] V_t[j] / (max U_t max V_t)          (the overlap of the two rows)
all be finite and at least theta.  Then each row's leader is above theta / N of what its
predecessor passed on, and the posterior mass of a frame that flushing can have removed is below
N 2^-126 / theta^2: 2^-33 at theta = 2^-40 and N = 8192.  A floored table bottoms out at
e^-18.4 = 2^-26.6 per step, above theta, so floored models are never flagged for the table's sake.
In the chains that normalise by the row sum (ragged, sparse, time-varying) f_t = sum U_t and
b_t >= sum e_t V_t, r_t = max V_{t-1}: the four quantities are the rows' own normalisers.
"""
from typing import Optional, Tuple

import torch
from torch import Tensor

THETA = 2.0 ** -40


def capturing() -> bool:
    """A CUDA graph is being captured: the guard's one host read is impossible, so it is skipped."""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def out_of_range(U: Tensor, V: Tensor, CA: Tensor, lengths: Optional[Tensor] = None, theta: float = THETA, *,
                 E: Optional[Tensor] = None, CB: Optional[Tensor] = None) -> Tensor:
    """(B,) bool on U's device: sequence b left the kernels' fp32 range.

    U, V (B,T,N): the scaled forward / backward rows; CA (B,T): the forward step normalisers
    (U_{t+1} = A^T U_t e_{t+1} / CA_t); lengths (B) or None; E (B,T,N): the shifted emissions
    exp(obs - rowmax) the chains multiplied by; CB (B,T): the backward step normalisers
    (V_{t-1} = A e_t V_t / CB_t), needed only where they are not sum e_t V_t.  Without E the
    backward row sums are taken to be CB; without both the b / r checks are left out.
    Pure torch (any device), no synchronisation."""
    B, T, N = U.shape
    dev = U.device
    f64 = torch.float64
    mu, mv = U.amax(-1), V.amax(-1)                                   # NaN rows stay NaN
    su = U.sum(-1).to(f64)
    ov = ((U / mu[..., None]) * (V / mv[..., None])).sum(-1).to(f64)
    t = torch.arange(T, device=dev)[None, :]
    valid = torch.ones(B, T, dtype=torch.bool, device=dev) if lengths is None else t < lengths.to(dev)[:, None]
    step = valid & (t >= 1)                                           # frames t - 1 and t both valid
    one = torch.ones(B, T, dtype=f64, device=dev)
    checks = [(torch.cat([su[:, :1], su[:, 1:] * CA[:, :-1].to(f64) / su[:, :-1]], 1), valid), (ov, valid)]
    x = (E * V).sum(-1).to(f64) if E is not None else (CB.to(f64) if CB is not None else None)
    if x is not None:
        cb = CB.to(f64) if CB is not None else x
        mv64 = mv.to(f64)
        checks.append((x / mv64, step))
        checks.append((torch.cat([one[:, :1], mv64[:, :-1] * cb[:, 1:] / x[:, 1:]], 1), step))
    else:
        checks.append((mv.to(f64), valid))
    bad = torch.zeros(B, T, dtype=torch.bool, device=dev)
    for q, where in checks:
        bad |= where & ~(torch.isfinite(q) & (q >= theta))
    return bad.any(1)


def flagged(U, V, CA, lengths=None, theta: float = THETA, *, E=None, CB=None) -> Optional[Tensor]:
    """The indices (int64, on the device) of the sequences out_of_range() flags, or None when there
    are none -- one bool(flag.any()) read, the guard's only synchronisation -- or while a CUDA
    graph is being captured (no host read is possible there: the call is unguarded)."""
    if capturing():
        return None
    flag = out_of_range(U, V, CA, lengths, theta, E=E, CB=CB)
    if not bool(flag.any()):
        return None
    return torch.nonzero(flag).flatten()


def sparse_rows(ws: Tensor, B: int, T: int, N: int) -> dict:
    """Views of the pieces ops.sparse_forward_backward leaves in its workspace (csrc/sparse.hip
    sp_fb_layout: U, V (B,T,N); CA, rmax, Q1, Q2 (B,T); fp32, each piece 256-byte aligned)."""
    fl = ws.view(torch.float32)
    rows = B * T
    up = lambda nbytes: (nbytes + 255) // 256 * 256
    out, at = {}, 0
    for name, n, shape in (("U", rows * N, (B, T, N)), ("V", rows * N, (B, T, N)), ("CA", rows, (B, T)),
                           ("rmax", rows, (B, T)), ("Q1", rows, (B, T)), ("Q2", rows, (B, T))):
        out[name] = fl[at // 4: at // 4 + n].view(shape)
        at += up(n * 4)
    return out


def sparse_flagged(ws: Tensor, obs: Tensor, lengths: Optional[Tensor], theta: float = THETA) -> Optional[Tensor]:
    """flagged() over a sparse forward-backward workspace.  The flagged sequences' rows are then
    neutralised in place (U = V = Q1 = Q2 = 0, CA = 1), so that ops.sparse_arc_counts over the
    workspace counts exactly 0 for them whatever the chains left there (NaN included)."""
    B, T, N = obs.shape
    r = sparse_rows(ws, B, T, N)
    lens = None if lengths is None else lengths.to(obs.device)
    bad = flagged(r["U"], r["V"], r["CA"], lens, theta, E=torch.exp(obs - r["rmax"][..., None]))
    if bad is not None:
        for name in ("U", "V", "Q1", "Q2"):
            r[name].index_fill_(0, bad, 0.0)
        r["CA"].index_fill_(0, bad, 1.0)
    return bad


def _lse_scatter(cand: Tensor, idx: Tensor, N: int) -> Tensor:
    """(B,N): log sum exp of cand (B,E) over the arcs that share idx[e]; -inf where there is no
    finite term (the shift is `m == -inf ? 0 : m`)."""
    B, E = cand.shape
    m = torch.full((B, N), -float("inf"), dtype=cand.dtype, device=cand.device)
    m = m.scatter_reduce(1, idx.expand(B, E), cand, "amax", include_self=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.zeros_like(m).index_add_(1, idx, torch.exp(cand - m0[:, idx]))
    return m0 + torch.log(s)


_TABLE_CAP = 1 << 25     # elements of the gathered (B, N, degree) candidates of one step


def _arc_table(idx: Tensor, N: int, B: int) -> Optional[Tensor]:
    """(N, D) arc ids grouped by idx[e], rows padded with E (D the largest group): with it a step's
    sums are plain reductions, the same bits on every call (index_add_ adds in any order).  None
    when B * N * D would pass _TABLE_CAP elements (a hub of a large graph): _lse_scatter then."""
    E = idx.numel()
    counts = torch.bincount(idx, minlength=N)
    D = int(counts.max()) if E else 0
    if D == 0 or B * N * D > _TABLE_CAP:
        return None
    order = torch.argsort(idx, stable=True)
    sidx = idx[order]
    pos = torch.arange(E, device=idx.device) - (torch.cumsum(counts, 0) - counts)[sidx]
    table = torch.full((N, D), E, dtype=torch.int64, device=idx.device)
    table[sidx, pos] = order
    return table


def _lse_arcs(cand: Tensor, idx: Tensor, N: int, table: Optional[Tensor]) -> Tensor:
    if table is None:
        return _lse_scatter(cand, idx, N)
    pad = torch.full((cand.shape[0], 1), -float("inf"), dtype=cand.dtype, device=cand.device)
    return _lse(torch.cat([cand, pad], 1)[:, table])


def _lse(x: Tensor) -> Tensor:
    m = x.amax(-1)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    return m0 + torch.log(torch.exp(x - m0[..., None]).sum(-1))


@torch.no_grad()
def logspace_forward_backward(log_obs: Tensor, log_p0: Tensor, log_P: Optional[Tensor] = None, *,
                              src: Optional[Tensor] = None, dst: Optional[Tensor] = None,
                              log_w: Optional[Tensor] = None, lengths: Optional[Tensor] = None,
                              weight: Optional[Tensor] = None, want_xi: bool = True
                              ) -> Tuple[Tensor, Tensor, Optional[Tensor]]:
    """(loglik (B), gamma (B,T,N), xi) in float64 on log_obs's device: the forward-backward sums by
    log-sum-exp recursions, a loop over T in plain torch.  The transitions are a dense log_P (N,N)
    -- xi is (N,N) -- or the arcs src / dst / log_w (E) -- xi is (E), in their order; -inf entries
    are forbidden transitions.  lengths (B) or None: frames past a length are never used (gamma is
    0 there).  xi is summed over the sequences with `weight` (B) or 1.  A sequence without a path
    gets loglik -inf and exact zeros.  Meant for the few sequences out_of_range() flags: it is
    orders of magnitude slower than the kernels."""
    dev = log_obs.device
    f64 = torch.float64
    B, T, N = log_obs.shape
    dense = log_P is not None
    if dense:
        lP = log_P.detach().to(f64)
        nz = torch.nonzero(lP > -float("inf"))
        src, dst, w = nz[:, 0], nz[:, 1], lP[nz[:, 0], nz[:, 1]]
    else:
        src, dst, w = src.long().to(dev), dst.long().to(dev), log_w.detach().to(f64)
    E = w.numel()
    lens = torch.full((B,), T, dtype=torch.int64, device=dev) if lengths is None else lengths.to(dev).long()
    t_idx = torch.arange(T, device=dev)
    valid = t_idx[None, :] < lens[:, None]                             # (B,T)
    obs = torch.where(valid[..., None], log_obs.detach().to(f64), torch.zeros((), dtype=f64, device=dev))
    la = torch.empty(B, T, N, dtype=f64, device=dev)
    lb = torch.zeros(B, T, N, dtype=f64, device=dev)
    la[:, 0] = log_p0.detach().to(f64) + obs[:, 0]
    by_dst, by_src = _arc_table(dst, N, B), _arc_table(src, N, B)
    for t in range(1, T):
        nxt = _lse_arcs(la[:, t - 1][:, src] + w, dst, N, by_dst) + obs[:, t]
        la[:, t] = torch.where(valid[:, t, None], nxt, la[:, t - 1])     # past the end: carried along
    loglik = _lse(la[:, T - 1])
    for t in range(T - 2, -1, -1):
        prv = _lse_arcs(w + (obs[:, t + 1] + lb[:, t + 1])[:, dst], src, N, by_src)
        lb[:, t] = torch.where(valid[:, t + 1, None], prv, torch.zeros_like(prv))
    ok = torch.isfinite(loglik)
    ll = torch.where(ok, loglik, torch.zeros_like(loglik))
    live = (valid & ok[:, None])[..., None]
    gamma = torch.where(live, torch.exp(la + lb - ll[:, None, None]), torch.zeros((), dtype=f64, device=dev))
    xi = None
    if want_xi:
        g = torch.ones(B, dtype=f64, device=dev) if weight is None else weight.detach().to(f64)
        acc = torch.zeros(E, dtype=f64, device=dev)
        for t in range(T - 1):
            pair = (valid[:, t + 1] & ok)[:, None]
            term = torch.exp(la[:, t][:, src] + w + (obs[:, t + 1] + lb[:, t + 1])[:, dst] - ll[:, None])
            acc += (torch.where(pair, term, torch.zeros_like(term)) * g[:, None]).sum(0)
        xi = torch.zeros(N, N, dtype=f64, device=dev).index_put_((src, dst), acc) if dense else acc
    return loglik, gamma, xi
