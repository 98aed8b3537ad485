"""Baum-Welch (EM) re-estimation on the GPU.

The reference trains its layers by autograd only (its documentation lists Baum-Welch,
docs/01_hmm_theory.md, but its code has none).  Here one EM iteration is

  E-step  e_step(): one forward-backward call (autograd._run_fb, OBS_LOG) gives the exact
          log-likelihood, the state posteriors gamma and -- from the scaled rows the chains leave in
          their workspace, with the expressions of autograd.SequenceLogLik.backward at G = 1 -- the
          expected transition counts xi.  ops.gmm_stats (csrc/emstats.hip) turns gamma into the
          occupancy-weighted moments of the Gaussian (mixture) emissions, centred on the current means.
  M-step  transition_m_step() / gaussian_m_step(): closed-form updates in fp64 on the small tables.

Everything is additive over sequences: EStats and the three statistics tensors of several batches
are summed before one M-step (fit() with a list of batches).
"""
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _native as nat
from . import ops
from . import range_guard as rg
from .autograd import _require_narrow, _run_fb, _staged_emissions, valid_frames

__all__ = ["EStats", "e_step", "sequence_loglik", "transition_m_step", "gaussian_m_step"]


@dataclass
class EStats:
    """The chain half of the E-step.  loglik (B,) exact log-likelihoods; gamma (B,T,N) state
    posteriors, 0 in padded frames; xi (N,N) = sum_b sum_{t < len_b - 1} p(z_t = i, z_{t+1} = j | x_b);
    gamma0 (N) = sum_b gamma[b,0]; n_seq the number of sequences.

    a + b accumulates two batches: xi, gamma0 and n_seq are summed and loglik is concatenated (its
    sum is the total); gamma belongs to one batch (it weights that batch's frames in ops.gmm_stats)
    and is None in a sum."""
    loglik: Tensor
    gamma: Optional[Tensor]
    xi: Tensor
    gamma0: Tensor
    n_seq: int

    def __add__(self, other: "EStats") -> "EStats":
        if not isinstance(other, EStats):
            return NotImplemented
        return EStats(torch.cat([self.loglik, other.loglik]), None, self.xi + other.xi, self.gamma0 + other.gamma0,
                      self.n_seq + other.n_seq)


def e_step(log_emis: Tensor, log_P: Tensor, log_p0: Tensor, lengths=None, plan: Optional[Tensor] = None,
           range_guard: bool = True) -> EStats:
    """Posteriors and expected counts of the chain for log-emissions log_emis (B,T,N), log_P (N,N)
    (-inf for a forbidden transition: xi is exactly 0 there) and log_p0 (N); lengths as
    ops.ragged_lengths (frames past a length are never read).  One forward-backward call, no
    autograd.  N <= 256.

    range_guard (default on): the sequences that left the kernels' fp32 range
    (range_guard.out_of_range over the rows the call leaves: possible only with exact zeros in
    log_P) are recomputed in float64 log space (range_guard.logspace_forward_backward) and their
    loglik, gamma and share of xi / gamma0 replaced; every other sequence keeps the kernels' bits.
    This costs one host read of a flag per call, and nothing else while no sequence is flagged.  It
    is skipped while a CUDA graph is being captured.  Callers whose tables are floored by
    construction (log(P + 1e-8)) pass False."""
    if log_emis.dim() != 3:
        raise ValueError(f"log_emis must be (B, T, N); got {tuple(log_emis.shape)}")
    B, T, N = log_emis.shape
    if tuple(log_P.shape) != (N, N) or tuple(log_p0.shape) != (N,):
        raise ValueError(f"log_P must be ({N}, {N}) and log_p0 ({N},); got {tuple(log_P.shape)}, {tuple(log_p0.shape)}")
    if T < 1:
        raise ValueError("log_emis must hold at least one frame")
    _require_narrow(N, "the Baum-Welch E-step")
    lens = ops.active_lengths(lengths, B, T, N)
    nat.require_gpu(log_emis, log_P, log_p0)
    dev = log_emis.device
    with torch.no_grad():
        obs, lP, l0 = (t.detach().to(torch.float32).contiguous() for t in (log_emis, log_P, log_p0))
        if B == 0:
            return EStats(torch.zeros(0, device=dev), torch.zeros(0, T, N, device=dev), torch.zeros(N, N, device=dev),
                          torch.zeros(N, device=dev), 0)
        post, loglik, _, U, V, _, _, CA, CB = _run_fb(obs, lP, l0, nat.OBS_LOG, posterior=True,
                                                      plan=None if lens is not None else plan, lengths=lens)
        valid = valid_frames(lens, T, dev)
        e = _staged_emissions(obs, nat.OBS_LOG, valid) if T > 1 or range_guard else None
        bad = rg.flagged(U, V, CA, lens, E=e, CB=CB) if range_guard else None
        xi = torch.zeros(N, N, device=dev)
        if T > 1:
            # SequenceLogLik.backward's X (x) Y with G = 1 (the terminal backward vector is 1)
            S = (U * V).sum(-1)
            den = (CA[:, :-1] * S[:, 1:]).unsqueeze(-1)
            if valid is None:
                X = U[:, :-1] / den
            else:
                pair = valid[:, 1:, None]                         # frames t and t + 1 both valid
                X = torch.where(pair, U[:, :-1] / torch.where(pair, den, torch.ones_like(den)),
                                torch.zeros_like(U[:, :-1]))
            Y = e[:, 1:] * V[:, 1:]
            if bad is not None:
                # the flagged sequences' rows may hold anything (NaN included): out of both factors
                X, Y = X.index_fill(0, bad, 0.0), Y.index_fill(0, bad, 0.0)
            xi = torch.exp(lP) * torch.einsum("bti,btj->ij", X, Y)
        if bad is not None:
            ll, g, x = rg.logspace_forward_backward(obs[bad], l0, lP, lengths=None if lens is None else lens.to(dev)[bad])
            loglik = loglik.index_copy(0, bad, ll.to(loglik.dtype))
            post = post.index_copy(0, bad, g.to(post.dtype))
            xi = xi + x.to(xi.dtype)
        gamma0 = post[:, 0].sum(0)
    return EStats(loglik, post, xi, gamma0, B)


def sequence_loglik(log_emis: Tensor, log_P: Tensor, log_p0: Tensor, lens: Optional[Tensor] = None,
                    range_guard: bool = True) -> Tensor:
    """(B,) exact log-likelihoods for log-emissions (B,T,N), without posteriors or autograd: the
    likelihood half of e_step, with its guard (a sequence range_guard.out_of_range flags over the
    rows the call leaves takes its value from the float64 log-space loop; the others keep the
    kernels' bits).  lens: active lengths (ops.active_lengths) or None.  Above 256 states the
    batch-tiled form runs, which leaves no such rows: unguarded there, in range only (hmm355.h)."""
    B, T, N = log_emis.shape
    with torch.no_grad():
        obs, lP, l0 = (t.detach().to(torch.float32).contiguous() for t in (log_emis, log_P, log_p0))
        if N > nat.NARROW_MAX_STATES or B == 0:
            return ops.forward_backward(obs, lP, l0, nat.OBS_LOG, 0)[3]
        _, loglik, _, U, V, _, _, CA, CB = _run_fb(obs, lP, l0, nat.OBS_LOG, lengths=lens)
        if range_guard:
            e = _staged_emissions(obs, nat.OBS_LOG, valid_frames(lens, T, obs.device))
            bad = rg.flagged(U, V, CA, lens, E=e, CB=CB)
            if bad is not None:
                ll, _, _ = rg.logspace_forward_backward(obs[bad], l0, lP, want_xi=False,
                                                        lengths=None if lens is None else lens.to(obs.device)[bad])
                loglik = loglik.index_copy(0, bad, ll.to(loglik.dtype))
    return loglik


def transition_m_step(xi: Tensor, gamma0: Tensor, n_seq: int, old_P: Tensor, old_p0: Tensor,
                      min_occupancy: float = 1e-6) -> Tuple[Tensor, Tensor]:
    """(P', p0'): the rows of xi normalised (a row whose sum is below min_occupancy keeps its row
    of old_P) and gamma0 / n_seq (old_p0 without sequences).  Divisions in fp64; exact zeros of xi
    stay exact zeros.  Pure torch, any device."""
    x = xi.to(torch.float64)
    rows = x.sum(1, keepdim=True)
    ok = rows >= min_occupancy
    P = torch.where(ok, x / torch.where(ok, rows, torch.ones_like(rows)), old_P.to(torch.float64))
    p0 = gamma0.to(torch.float64) / n_seq if n_seq > 0 else old_p0.to(torch.float64)
    return P.to(old_P.dtype), p0.to(old_p0.dtype)


def gaussian_m_step(occ: Tensor, sx: Tensor, sxx: Tensor, means: Tensor, covariance_type: str,
                    var_floor: float = 1e-4, min_occupancy: float = 1e-6, *, log_vars: Optional[Tensor] = None,
                    weights: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """(means', log_vars', weights') from the centred statistics occ (S,C), sx, sxx (S,C,D) of
    ops.gmm_stats and the means (S,C,D) they were centred on:
        means' = means + sx / occ
        'diag'       var' (S,C,D) = sxx / occ - (sx / occ)^2
        'spherical'  var' (S,C)   = sum_d (sxx - sx^2 / occ) / (D occ)
        'tied'       var' (D)     = sum_{s,c} (sxx - sx^2 / occ) / sum_{s,c} occ
        weights'[s,c] = occ[s,c] / sum_c occ[s,c]
    with var' floored at var_floor.  A component whose occupancy is below min_occupancy keeps its
    parameters (and stays out of the tied sums); a state whose total occupancy is below it keeps
    its weights.  The kept values are the optional `log_vars` (in the covariance type's shape) and
    `weights` (S,C); without them such entries get log_vars' = 0 and uniform weights.  Divisions in
    fp64; pure torch, any device."""
    if covariance_type not in ("diag", "spherical", "tied"):
        if covariance_type == "full":
            raise NotImplementedError("EM re-estimation covers 'diag', 'spherical' and 'tied' covariances, not 'full'")
        raise ValueError(f"Unknown covariance_type: {covariance_type}")
    S, C, D = means.shape
    f64 = torch.float64
    o, s1, s2, mu = occ.to(f64), sx.to(f64), sxx.to(f64), means.to(f64)
    ok = o >= min_occupancy                                        # (S,C)
    od = torch.where(ok, o, torch.ones_like(o))
    m1 = s1 / od[..., None]
    new_means = torch.where(ok[..., None], mu + m1, mu)
    cen = s2 - s1 * m1                                             # occ * var, per dim
    cen = torch.where(ok[..., None], cen, torch.zeros_like(cen))
    if covariance_type == "diag":
        old = torch.zeros(S, C, D, dtype=f64, device=o.device) if log_vars is None else log_vars.to(f64)
        var = (cen / od[..., None]).clamp(min=var_floor)
        new_lv = torch.where(ok[..., None], torch.log(var), old)
    elif covariance_type == "spherical":
        old = torch.zeros(S, C, dtype=f64, device=o.device) if log_vars is None else log_vars.to(f64).reshape(S, C)
        var = (cen.sum(-1) / (D * od)).clamp(min=var_floor)
        new_lv = torch.where(ok, torch.log(var), old)
    else:
        old = torch.zeros(D, dtype=f64, device=o.device) if log_vars is None else log_vars.to(f64).reshape(D)
        tot = torch.where(ok, o, torch.zeros_like(o)).sum()
        good = tot >= min_occupancy
        var = (cen.sum((0, 1)) / torch.where(good, tot, torch.ones_like(tot))).clamp(min=var_floor)
        new_lv = torch.where(good, torch.log(var), old)
    tot_s = o.sum(-1, keepdim=True)
    oks = tot_s >= min_occupancy
    oldw = torch.full((S, C), 1.0 / C, dtype=f64, device=o.device) if weights is None else weights.to(f64)
    new_w = torch.where(oks, o / torch.where(oks, tot_s, torch.ones_like(tot_s)), oldw)
    dt = means.dtype
    return new_means.to(dt), new_lv.to(dt), new_w.to(dt)


# ---------------------------------------------------------------- the layers' EM driver
def as_batches(observations, lengths) -> List[Tuple[Tensor, Optional[Tensor]]]:
    """[(x (B,T,D), lengths or None)] from one batch or a list of (x, lengths) pairs; checks shapes
    (ValueError) and devices before anything is launched."""
    if isinstance(observations, (list, tuple)):
        if lengths is not None:
            raise ValueError("with a list of batches the lengths go inside the (x, lengths) pairs")
        pairs = [(p[0], p[1]) if isinstance(p, (list, tuple)) else (p, None) for p in observations]
        if not pairs:
            raise ValueError("fit needs at least one batch")
    else:
        pairs = [(observations, lengths)]
    return pairs


def check_batch(x, lengths, D: int, N: int):
    """The checked (x, active lengths or None, number of frames) of one batch."""
    if not isinstance(x, Tensor) or x.dim() != 3 or x.shape[2] != D:
        raise ValueError(f"observations must be (B, T, {D}); got {tuple(x.shape) if isinstance(x, Tensor) else type(x)}")
    B, T, _ = x.shape
    if B < 1 or T < 1:
        raise ValueError(f"observations must hold at least one sequence and one frame; got {tuple(x.shape)}")
    lens = ops.active_lengths(lengths, B, T, N)
    nat.require_gpu(x)
    frames = B * T if lens is None else int(lens.sum())
    return x, lens, frames


def accumulate(batches, D, N, score, stats, log_P, log_p0, plan=None, want_stats=True, range_guard=True):
    """The E-step over `batches`: score(x) -> log-emissions (B,T,N), stats(x, gamma, lens) -> (occ,
    sx, sxx).  Returns (EStats summed, [occ, sx, sxx] summed or None, frames).  Padded frames of x
    are zeroed (selected) before they are scored; the chain and the statistics kernel never read
    them.  range_guard as e_step's: on for the layers' em_step / fit, whose tables may hold exact
    zeros (a fixed transition_matrix) and whose Gaussian log-densities differ by hundreds of nats
    between states (MixtureGaussianHMMLayer.log_likelihood goes through sequence_loglik)."""
    checked = [check_batch(x, lens, D, N) for x, lens in batches]
    total, sums, frames = None, None, 0
    for x, lens, nf in checked:
        if lens is not None:
            valid = valid_frames(lens, x.shape[1], x.device)
            x = torch.where(valid[..., None], x, torch.zeros_like(x))
        es = e_step(score(x), log_P, log_p0, lens, plan, range_guard)
        if want_stats:
            part = stats(x, es.gamma, lens)
            sums = list(part) if sums is None else [a + b for a, b in zip(sums, part)]
        total = es if total is None else total + es
        frames += nf
    return total, sums, frames


def run_fit(step, n_iter: int, tol: float) -> List[float]:
    """step() -> (total log-likelihood before the update, frames); iterates until n_iter or until the
    gain per frame drops below tol."""
    hist: List[float] = []
    for it in range(int(n_iter)):
        ll, frames = step()
        hist.append(ll)
        if it > 0 and (hist[-1] - hist[-2]) / max(frames, 1) < tol:
            break
    return hist


def log_of(P: Tensor) -> Tensor:
    """log P with -inf at exact zeros (a fixed transition matrix buffer)."""
    return torch.where(P > 0, torch.log(torch.where(P > 0, P, torch.ones_like(P))), torch.full_like(P, -math.inf))


def check_update(update: Sequence[str], allowed: Sequence[str], what: str):
    bad = [u for u in update if u not in allowed]
    if bad:
        raise ValueError(f"{what}: update may contain {tuple(allowed)}; got {tuple(bad)}")
