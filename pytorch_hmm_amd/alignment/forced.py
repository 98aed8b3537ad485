"""Transcript forced alignment: align an utterance to its own left-to-right chain of states.

Every utterance b has a chain of S_b positions, the states of its transcript in order; position s
emits class state_ids[b, s] of log_probs (B,T,C) -- the per-class log-densities that
GaussianHMMLayer / MixtureGaussianHMMLayer.get_observation_log_probs produce -- and either stays,
advances to s + 1 or (optionally) skips to s + 2, with per-position log-weights log_stay, log_next
and log_skip (B,Smax) indexed by the source position (absent: 0, 0 and -inf).  A path starts in
position 0 at frame 0 and ends in position S_b - 1 at frame input_lengths[b] - 1; batches are
ragged in both lengths.  The recursions are the HIP kernels of csrc/forced.hip (ops.forced /
ops.forced_grad / autograd.ForcedLogLik) and take tensors on a ROCm GPU only.

  forced_align                 the best path, the frames it spends in each position, its score
  forced_alignment_loglik      the log of the sum over all paths ("forward-sum"), differentiable
  forced_alignment_posteriors  gamma[b,t,s], the probability of position s at frame t
  monotonic_alignment_search   forced_align over value (B,T,S) itself: position s emits column s,
                               no weights, no skips (the search TTS models run in their training loop)
  ForcedAligner                a module with per-class stay / next / skip logits over
                               num_tokens x states_per_token classes
"""
import math
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn

from .. import _native as nat
from .. import ops
from ..autograd import ForcedLogLik


def forced_align(log_probs: torch.Tensor, state_ids: Optional[torch.Tensor], input_lengths: torch.Tensor,
                 state_lengths: torch.Tensor, log_stay: Optional[torch.Tensor] = None,
                 log_next: Optional[torch.Tensor] = None,
                 log_skip: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(path, durations, score) of the best path of every utterance through its chain.
    path (B,T) int32: the chain position of each frame, -1 past input_lengths[b]; durations
    (B,Smax) int32: the frames spent in each position (0 for a skipped one and past
    state_lengths[b]); score (B,) float32.  Ties go to stay, then s-1, then s-2.  A pair with no
    path (more positions than frames and no skips, for example) has -1 everywhere, durations 0
    and score -inf."""
    nat.require_gpu(log_probs)
    _, _, _, path, score, dur = ops.forced(log_probs, state_ids, input_lengths, state_lengths, log_stay, log_next,
                                           log_skip, viterbi=True)
    return path, dur, score


def forced_alignment_loglik(log_probs: torch.Tensor, state_ids: Optional[torch.Tensor], input_lengths: torch.Tensor,
                            state_lengths: torch.Tensor, log_stay: Optional[torch.Tensor] = None,
                            log_next: Optional[torch.Tensor] = None,
                            log_skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The log (B,) float32 of the sum over every path; -inf for a pair with no path.  When
    log_probs or a weight tensor requires grad the result is differentiable
    (autograd.ForcedLogLik); otherwise this is the value-only kernel call, which writes no table."""
    nat.require_gpu(log_probs)
    diff = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                           for t in (log_probs, log_stay, log_next, log_skip))
    if diff:
        return ForcedLogLik.apply(log_probs, state_ids, input_lengths, state_lengths, log_stay, log_next, log_skip)
    return ops.forced(log_probs, state_ids, input_lengths, state_lengths, log_stay, log_next, log_skip)[0]


def forced_alignment_posteriors(log_probs: torch.Tensor, state_ids: Optional[torch.Tensor],
                                input_lengths: torch.Tensor, state_lengths: torch.Tensor,
                                log_stay: Optional[torch.Tensor] = None, log_next: Optional[torch.Tensor] = None,
                                log_skip: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gamma (B,T,Smax) float32: the posterior probability of position s at frame t given that the
    utterance traverses its whole chain.  Each frame of a pair with a path sums to 1; frames and
    positions past either length and pairs with no path are 0."""
    nat.require_gpu(log_probs)
    args = (state_ids, input_lengths, state_lengths, log_stay, log_next, log_skip)
    loglik, alpha, beta, _, _, _ = ops.forced(log_probs, *args, alpha=True, beta=True)
    return ops.forced_grad(alpha, beta, loglik, log_probs, *args, want_gamma=True, want_grad=False)[0]


def monotonic_alignment_search(value: torch.Tensor, input_lengths: torch.Tensor,
                               state_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """forced_align over value (B,T,S) with position s emitting column s, unit weights and no
    skips: (path (B,T) int32, durations (B,S) int32, score (B,))."""
    return forced_align(value, None, input_lengths, state_lengths)


class ForcedAligner(nn.Module):
    """Forced alignment of token transcripts with left-to-right token models.

    Token k owns the classes k K .. k K + K - 1 (K = states_per_token), in that order; a
    transcript expands to the chain of its tokens' states.  Every class has stay / next (/ skip)
    logits, turned into log-weights by a log-softmax and gathered per chain position.

    Args:
        num_tokens: size of the token inventory
        states_per_token: K, states of every token's left-to-right model
        allow_skip: a position may also skip the next one (s -> s + 2)
        learnable_transitions: the logits are a Parameter (else a buffer)
        self_loop_prob: initial stay probability (create_left_to_right_matrix's default); the
            rest goes to next, or 0.8 / 0.2 of it to next / skip with allow_skip
    """

    def __init__(self, num_tokens: int, states_per_token: int = 1, allow_skip: bool = False,
                 learnable_transitions: bool = True, self_loop_prob: float = 0.7):
        super().__init__()
        if num_tokens < 1 or states_per_token < 1:
            raise ValueError("num_tokens and states_per_token must be at least 1")
        if not 0.0 < self_loop_prob < 1.0:
            raise ValueError(f"self_loop_prob must lie in (0, 1); got {self_loop_prob}")
        self.num_tokens = int(num_tokens)
        self.states_per_token = int(states_per_token)
        self.num_classes = self.num_tokens * self.states_per_token
        self.allow_skip = bool(allow_skip)
        rest = 1.0 - self_loop_prob
        probs = [self_loop_prob, 0.8 * rest, 0.2 * rest] if allow_skip else [self_loop_prob, rest]
        logits = torch.tensor([math.log(p) for p in probs]).repeat(self.num_classes, 1)
        if learnable_transitions:
            self.transition_logits = nn.Parameter(logits)
        else:
            self.register_buffer("transition_logits", logits)

    def expand(self, tokens: torch.Tensor, token_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """tokens (B,Lmax) integers, token_lengths (B) -> (state_ids (B, Lmax K) int32,
        state_lengths (B) int32).  A used token outside [0, num_tokens) raises ValueError."""
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
        K = self.states_per_token
        ids = (tk[:, :, None] * K + torch.arange(K, device=tk.device)).reshape(B, Lmax * K)
        return ids.to(torch.int32), (tl * K).to(torch.int32)

    def transition_weights(self, state_ids: torch.Tensor):
        """(log_stay, log_next, log_skip or None), each (B,Smax): the log-softmax of the class's
        logits at every chain position."""
        lsm = torch.log_softmax(self.transition_logits.float(), dim=1)
        idx = state_ids.to(lsm.device).long().clamp(0, self.num_classes - 1)
        w = lsm[idx]
        return w[..., 0], w[..., 1], (w[..., 2] if self.allow_skip else None)

    def _chain(self, log_probs, tokens, token_lengths):
        if log_probs.dim() != 3 or log_probs.shape[2] != self.num_classes:
            raise ValueError(f"log_probs must be (B, T, {self.num_classes}); got {tuple(log_probs.shape)}")
        ids, sl = self.expand(tokens, token_lengths)
        ids = ids.to(log_probs.device)
        return (ids, sl) + tuple(self.transition_weights(ids))

    def forward(self, log_probs: torch.Tensor, tokens: torch.Tensor, input_lengths: torch.Tensor,
                token_lengths: torch.Tensor) -> torch.Tensor:
        """-loglik (B,): the forward-sum alignment loss of every utterance, differentiable in
        log_probs and the transition logits; +inf for a pair with no path (its gradient is 0)."""
        ids, sl, ws, wn, wk = self._chain(log_probs, tokens, token_lengths)
        return -forced_alignment_loglik(log_probs, ids, input_lengths, sl, ws, wn, wk)

    @torch.no_grad()
    def align(self, log_probs: torch.Tensor, tokens: torch.Tensor, input_lengths: torch.Tensor,
              token_lengths: torch.Tensor) -> Dict[str, torch.Tensor]:
        """{"path" (B,T) int32 chain positions (position // states_per_token is the token's index
        in the transcript), "token_durations" (B,Lmax) int32 frames per token, "score" (B,)}."""
        ids, sl, ws, wn, wk = self._chain(log_probs, tokens, token_lengths)
        path, dur, score = forced_align(log_probs, ids, input_lengths, sl, ws, wn, wk)
        B, Lmax = tokens.shape
        return {"path": path, "token_durations": dur.reshape(B, Lmax, self.states_per_token).sum(2).to(torch.int32),
                "score": score}

    @torch.no_grad()
    def posteriors(self, log_probs: torch.Tensor, tokens: torch.Tensor, input_lengths: torch.Tensor,
                   token_lengths: torch.Tensor) -> torch.Tensor:
        """gamma (B,T,Lmax K): the posterior of every chain position at every frame."""
        ids, sl, ws, wn, wk = self._chain(log_probs, tokens, token_lengths)
        return forced_alignment_posteriors(log_probs, ids, input_lengths, sl, ws, wn, wk)
