"""Explicit-duration forced alignment: align an utterance to its own transcript where every position
has its own duration distribution.

Every utterance b has a chain of L_b positions, the tokens of its transcript in order; position l
emits class state_ids[b, l] of log_probs (B,T,C) and lasts d_l frames, 1 <= d_l <= Dmax, scored by
dur_lp[b, l, d_l - 1] (B,Lmax,Dmax; -inf forbids a duration, which is how a minimum duration is
written).  Every position is visited once, in order, and the durations add up to
input_lengths[b] exactly; batches are ragged in both lengths.  A pair with no such segmentation
(fewer frames than positions, more than L_b Dmax, or ruled out by the -inf entries) is infeasible:
score / loglik -inf, path -1, durations 0, posteriors and gradients 0.  The recursions are the HIP
kernels of csrc/durforced.hip (ops.durforced / ops.durforced_grad / autograd.DurForcedLogLik) and
take tensors on a ROCm GPU only.

  duration_forced_align       the best segmentation: the position of every frame, d_l, its score
  duration_forced_loglik      the log of the sum over all segmentations, differentiable in
                              log_probs and dur_lp: the marginal likelihood a duration predictor
                              is trained by
  duration_forced_posteriors  gamma[b,t,l] and the posterior of "position l lasts d frames"
  DurationForcedAligner       a module with per-token duration logits, or driven by a duration
                              predictor's dur_lp
"""
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from .. import _native as nat
from .. import ops
from ..autograd import DurForcedLogLik


def duration_forced_align(log_probs: torch.Tensor, state_ids: Optional[torch.Tensor], input_lengths: torch.Tensor,
                          state_lengths: torch.Tensor,
                          dur_lp: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(path, durations, score) of the best segmentation of every utterance.  path (B,T) int32: the
    chain position of each frame, -1 past input_lengths[b]; durations (B,Lmax) int32: d_l, 0 past
    state_lengths[b]; score (B,) float32.  Of equally good segmentations the one whose last
    position is shortest wins, then the one before it, and so on."""
    nat.require_gpu(log_probs, dur_lp)
    out = ops.durforced(log_probs, state_ids, input_lengths, state_lengths, dur_lp, viterbi=True)
    return out[7], out[9], out[8]


def duration_forced_loglik(log_probs: torch.Tensor, state_ids: Optional[torch.Tensor], input_lengths: torch.Tensor,
                           state_lengths: torch.Tensor, dur_lp: torch.Tensor) -> torch.Tensor:
    """The log (B,) float32 of the sum over every segmentation; -inf for an infeasible pair.  When
    log_probs or dur_lp requires grad the result is differentiable (autograd.DurForcedLogLik);
    otherwise this is the value-only kernel call, which writes no table."""
    nat.require_gpu(log_probs, dur_lp)
    if torch.is_grad_enabled() and (log_probs.requires_grad or dur_lp.requires_grad):
        return DurForcedLogLik.apply(log_probs, state_ids, input_lengths, state_lengths, dur_lp)
    return ops.durforced(log_probs, state_ids, input_lengths, state_lengths, dur_lp)[0]


def duration_forced_posteriors(log_probs: torch.Tensor, state_ids: Optional[torch.Tensor],
                               input_lengths: torch.Tensor, state_lengths: torch.Tensor,
                               dur_lp: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(gamma (B,T,Lmax), dur_post (B,Lmax,Dmax)) float32: the posterior probability of position l
    at frame t, and of position l lasting d frames.  Each used frame of gamma and each used
    position of dur_post sums to 1 for a feasible pair; everything past either length and every
    infeasible pair is 0."""
    nat.require_gpu(log_probs, dur_lp)
    args = (log_probs, state_ids, input_lengths, state_lengths, dur_lp)
    out = ops.durforced(*args, tables=True)
    gamma, _, dur_post = ops.durforced_grad(*out[1:7], *args, want_gamma=True, want_grad=False, want_dur=True)
    return gamma, dur_post


class DurationForcedAligner(nn.Module):
    """Forced alignment of token transcripts with one state and one duration distribution per token.

    Token k is class k of log_probs (B,T,num_tokens) and has duration logits over 1..max_duration
    frames, turned into dur_lp by a log-softmax and gathered per chain position with ordinary
    indexing, so autograd carries the gradient of the marginal likelihood back to the logits.
    Every method also takes dur_lp= (B,Lmax,max_duration), which replaces the module's own table:
    the scores of a duration predictor, trained through forward().

    Args:
        num_tokens: size of the token inventory
        max_duration: Dmax, the longest segment of a position in frames
        learnable_durations: the logits are a Parameter (else a buffer); initialised uniform
    """

    def __init__(self, num_tokens: int, max_duration: int, learnable_durations: bool = True):
        super().__init__()
        if num_tokens < 1 or max_duration < 1:
            raise ValueError("num_tokens and max_duration must be at least 1")
        if max_duration > ops.DURFORCED_MAX_DURATION:
            raise ValueError(f"max_duration above {ops.DURFORCED_MAX_DURATION} is not supported; got {max_duration}")
        self.num_tokens = int(num_tokens)
        self.max_duration = int(max_duration)
        logits = torch.zeros(self.num_tokens, self.max_duration)
        if learnable_durations:
            self.duration_logits = nn.Parameter(logits)
        else:
            self.register_buffer("duration_logits", logits)

    def chain(self, tokens: torch.Tensor, token_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """tokens (B,Lmax) integers, token_lengths (B) -> (state_ids (B,Lmax) int32, state_lengths
        (B) int32).  A used token outside [0, num_tokens) raises ValueError."""
        if tokens.dim() != 2 or tokens.dtype.is_floating_point or tokens.dtype == torch.bool:
            raise ValueError(f"tokens must be (B, Lmax) integers; got {tuple(tokens.shape)} {tokens.dtype}")
        B, Lmax = tokens.shape
        tl = torch.as_tensor(token_lengths).detach().reshape(-1).to("cpu", torch.int64)
        if tl.numel() != B or Lmax < 1 or int(tl.min()) < 1 or int(tl.max()) > Lmax:
            raise ValueError(f"token_lengths must hold {B} values in [1, {Lmax}]; got {tl.tolist()}")
        used = torch.arange(Lmax)[None, :] < tl[:, None]
        tk = tokens.detach().to(torch.int64)
        if bool((((tk < 0) | (tk >= self.num_tokens)).cpu() & used).any()):
            raise ValueError(f"tokens hold values outside [0, {self.num_tokens})")
        return tk.to(torch.int32), tl.to(torch.int32)

    def duration_log_probs(self, state_ids: torch.Tensor) -> torch.Tensor:
        """dur_lp (B,Lmax,max_duration): the log-softmax of the token's logits at every position."""
        lsm = torch.log_softmax(self.duration_logits.float(), dim=1)
        return lsm[state_ids.to(lsm.device).long().clamp(0, self.num_tokens - 1)]

    def _args(self, log_probs, tokens, token_lengths, dur_lp):
        if log_probs.dim() != 3 or log_probs.shape[2] != self.num_tokens:
            raise ValueError(f"log_probs must be (B, T, {self.num_tokens}); got {tuple(log_probs.shape)}")
        ids, sl = self.chain(tokens, token_lengths)
        ids = ids.to(log_probs.device)
        if dur_lp is None:
            dur_lp = self.duration_log_probs(ids)
        elif dur_lp.dim() != 3 or tuple(dur_lp.shape[:2]) != tuple(ids.shape) or dur_lp.shape[2] > self.max_duration:
            raise ValueError(f"dur_lp must be (B, Lmax, D <= {self.max_duration}) over tokens {tuple(ids.shape)}; "
                             f"got {tuple(dur_lp.shape)}")
        return ids, sl, dur_lp

    def forward(self, log_probs: torch.Tensor, tokens: torch.Tensor, input_lengths: torch.Tensor,
                token_lengths: torch.Tensor, dur_lp: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-loglik (B,): the marginal alignment loss of every utterance, differentiable in
        log_probs and the duration logits (or the dur_lp given); +inf for an infeasible pair (its
        gradient is 0)."""
        ids, sl, du = self._args(log_probs, tokens, token_lengths, dur_lp)
        return -duration_forced_loglik(log_probs, ids, input_lengths, sl, du)

    @torch.no_grad()
    def align(self, log_probs: torch.Tensor, tokens: torch.Tensor, input_lengths: torch.Tensor,
              token_lengths: torch.Tensor, dur_lp: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """{"path" (B,T) int32 index into the transcript of every frame, "token_durations" (B,Lmax)
        int32 frames per token, "score" (B,)}."""
        ids, sl, du = self._args(log_probs, tokens, token_lengths, dur_lp)
        path, dur, score = duration_forced_align(log_probs, ids, input_lengths, sl, du)
        return {"path": path, "token_durations": dur, "score": score}

    @torch.no_grad()
    def posteriors(self, log_probs: torch.Tensor, tokens: torch.Tensor, input_lengths: torch.Tensor,
                   token_lengths: torch.Tensor,
                   dur_lp: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(gamma (B,T,Lmax), dur_post (B,Lmax,D)): the posterior of every position at every frame
        and of every duration of every position."""
        ids, sl, du = self._args(log_probs, tokens, token_lengths, dur_lp)
        return duration_forced_posteriors(log_probs, ids, input_lengths, sl, du)
