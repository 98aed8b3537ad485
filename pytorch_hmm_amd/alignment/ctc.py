"""CTC alignment with the reference's interface (pytorch_hmm/alignment/ctc.py).

The lattice recursions (alpha, beta, the best path, the occupancies and their gradient) are the
HIP kernels behind ops.ctc / ops.ctc_grad / autograd.CTCLogLik (csrc/ctc.hip) and take tensors on
a ROCm GPU only.  Everything else here (expanding, collapsing, greedy decoding, segmentation) is
plain vectorised torch and runs wherever its tensors are.

Kept from the reference, quirks included:
  * beta leaves the frame's own emission out (ctc.py:164-197), so alpha + beta is the log of the
    joint probability of the targets and "position s at frame t";
  * alpha's first frame is set whatever input_lengths says;
  * ctc_alignment_path's default method="reference" returns what the reference returns.  Its
    log_alpha is allocated and never filled (ctc.py:224), every alpha + beta is -inf, no position
    beats the initial best_pos = 0, and each frame maps to expanded position 0: the result is
    input_lengths[b] copies of blank_id.  It is built here without running a kernel;
  * CTCAligner.forward is the reference's nn.CTCLoss wrapper, with torch's gradient convention;
  * decode's "beam search" is the greedy decode; _estimate_segment_text assumes 1000 frames.
Departures:
  * method="posterior" and method="viterbi" (and ctc_forced_align) give the alignments the
    reference's code was written to give;
  * lengths outside [1, T] / [0, Lmax] and labels outside [0, C) raise ValueError where the
    reference would silently index row -1;
  * segment_and_align returns its frame bounds as Python ints.
"""
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from .. import _native as nat
from .. import ops
from ..autograd import CTCLogLik

METHODS = ("reference", "posterior", "viterbi")


def expand_targets_with_blank(targets: torch.Tensor, blank_id: int) -> torch.Tensor:
    """targets (B,L) -> (B,2L+1) int64: blank_id at the even positions, the labels at the odd ones."""
    batch_size, target_length = targets.shape
    expanded = torch.full((batch_size, 2 * target_length + 1), blank_id, device=targets.device)
    expanded[:, 1::2] = targets
    return expanded


def ctc_forward_algorithm(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                          target_lengths: torch.Tensor, blank_id: int = 0) -> torch.Tensor:
    """The log-likelihood (B,) float32 of the targets under log_probs (T,B,C) (ctc.py:32-121).
    -inf for a pair with no alignment.  When log_probs requires grad the result is differentiable
    (autograd.CTCLogLik: the true gradient, see its docstring); otherwise this is the value-only
    kernel call, which writes no (B,T,S') table."""
    nat.require_gpu(log_probs, targets)
    if torch.is_grad_enabled() and log_probs.requires_grad:
        return CTCLogLik.apply(log_probs, targets, input_lengths, target_lengths, blank_id)
    return ops.ctc(log_probs, targets, input_lengths, target_lengths, blank_id)[0]


def ctc_backward_algorithm(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                           target_lengths: torch.Tensor, blank_id: int = 0) -> torch.Tensor:
    """The beta table (B,T,2 Lmax+1) float32 in the reference's convention (ctc.py:124-199):
    beta[b,t,s] is the log-probability of finishing the targets over frames t+1 .. T_b-1 from
    position s at frame t, the emission of frame t left out; -inf past either length."""
    nat.require_gpu(log_probs, targets)
    return ops.ctc(log_probs, targets, input_lengths, target_lengths, blank_id, beta=True)[2]


def _lengths(t, B):
    return [int(v) for v in torch.as_tensor(t).reshape(B).tolist()]


def _tokens(positions, targets, input_lengths, blank_id):
    """Expanded positions (B,T) -> per-sequence int64 token tensors of the true lengths."""
    ext = expand_targets_with_blank(targets, blank_id).long()
    tok = torch.gather(ext, 1, positions.clamp(min=0))
    return [tok[b, :n] for b, n in enumerate(_lengths(input_lengths, targets.shape[0]))]


def ctc_forced_align(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                     target_lengths: torch.Tensor, blank_id: int = 0,
                     method: str = "viterbi") -> Tuple[torch.Tensor, List[torch.Tensor], torch.Tensor]:
    """(positions, tokens, score) of the forced alignment of targets to log_probs (T,B,C).
    positions (B,T) int64: the expanded position (0 .. 2 L_b) of every frame, -1 past
    input_lengths[b]; tokens: per sequence the int64 labels of those positions (blank_id at the
    even ones), of length input_lengths[b]; score (B,) float32.
      method="viterbi"    the single best path (ties: stay, then s-1, then s-2; the path ends in
                          the last position unless the one before it scores strictly higher);
                          score is its log-probability.  A pair with no alignment has -1 in every
                          frame (its tokens are all blank_id) and score -inf.
      method="posterior"  per frame the position of largest alpha + beta, the lowest on ties
                          (what ctc.py:238-252 computes once alpha is filled); score is loglik."""
    nat.require_gpu(log_probs, targets)
    if method == "viterbi":
        _, _, _, path, score = ops.ctc(log_probs, targets, input_lengths, target_lengths, blank_id, viterbi=True)
        positions = path.long()
    elif method == "posterior":
        score, alpha, beta, _, _ = ops.ctc(log_probs, targets, input_lengths, target_lengths, blank_id,
                                           alpha=True, beta=True)
        total = alpha + beta
        S = total.shape[2]
        idx = torch.arange(S, device=total.device)
        # the lowest index that attains the maximum (argmax alone does not promise which)
        positions = torch.where(total == total.max(dim=2, keepdim=True).values, idx, S).min(dim=2).values
        T = total.shape[1]
        il = torch.as_tensor(input_lengths).to(total.device).reshape(-1, 1)
        positions = torch.where(torch.arange(T, device=total.device)[None, :] < il, positions, -1)
    else:
        raise ValueError(f"ctc_forced_align: method must be 'viterbi' or 'posterior'; got {method!r}")
    return positions, _tokens(positions, targets, input_lengths, blank_id), score


def ctc_alignment_path(log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                       target_lengths: torch.Tensor, blank_id: int = 0, *,
                       method: str = "reference") -> List[torch.Tensor]:
    """Per sequence the int64 token of every frame, of length input_lengths[b] (ctc.py:202-256).
    method="reference" (the default) reproduces the reference: it never fills its alpha, so every
    frame comes out as blank_id (see the module docstring); no kernel runs.  "posterior" and
    "viterbi" are ctc_forced_align's tokens."""
    if method == "reference":
        B = log_probs.shape[1]
        return [torch.full((n,), blank_id, dtype=torch.int64, device=log_probs.device) if n > 0
                else torch.tensor([], device=log_probs.device) for n in _lengths(input_lengths, B)]
    if method not in METHODS:
        raise ValueError(f"ctc_alignment_path: method must be one of {METHODS}; got {method!r}")
    return ctc_forced_align(log_probs, targets, input_lengths, target_lengths, blank_id, method)[1]


class CTCAligner(nn.Module):
    """The reference's CTC aligner (ctc.py:259-381): forward is nn.CTCLoss, decode is greedy, align
    is ctc_alignment_path.

    Args:
        num_classes: number of classes, blank included
        blank_id: the blank's class
        reduction: 'mean', 'sum' or 'none' (nn.CTCLoss)
    """

    def __init__(self, num_classes: int, blank_id: int = 0, reduction: str = 'mean'):
        super().__init__()
        self.num_classes = num_classes
        self.blank_id = blank_id
        self.reduction = reduction
        self.ctc_loss = nn.CTCLoss(blank=blank_id, reduction=reduction, zero_infinity=True)

    def forward(self, log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                target_lengths: torch.Tensor) -> torch.Tensor:
        """The CTC loss of nn.CTCLoss over the concatenated targets (ctc.py:285-308); its backward is
        torch's (the log_softmax Jacobian folded in), not CTCLogLik's."""
        used = torch.arange(targets.shape[1], device=targets.device)[None, :] < \
            torch.as_tensor(target_lengths).to(targets.device).reshape(-1, 1)
        return self.ctc_loss(log_probs, targets[used], input_lengths, target_lengths)

    def decode(self, log_probs: torch.Tensor, input_lengths: torch.Tensor, beam_width: int = 1) -> List[torch.Tensor]:
        """Per sequence the decoded labels.  As in the reference, any beam_width decodes greedily."""
        if beam_width == 1:
            return self._greedy_decode(log_probs, input_lengths)
        return self._beam_search_decode(log_probs, input_lengths, beam_width)

    def _greedy_decode(self, log_probs: torch.Tensor, input_lengths: torch.Tensor) -> List[torch.Tensor]:
        """Best class per frame, repeats collapsed, blanks dropped: int64 tensors; an empty result is
        torch.tensor([]) (float32), as the reference's torch.tensor(list) gives."""
        best = torch.argmax(log_probs, dim=2)  # (T,B)
        changed = torch.ones_like(best, dtype=torch.bool)
        changed[1:] = best[1:] != best[:-1]
        keep = changed & (best != self.blank_id)
        out = []
        for b, n in enumerate(_lengths(input_lengths, log_probs.shape[1])):
            seq = best[:n, b][keep[:n, b]]
            out.append(seq if seq.numel() else torch.tensor([], device=log_probs.device))
        return out

    def _beam_search_decode(self, log_probs: torch.Tensor, input_lengths: torch.Tensor,
                            beam_width: int) -> List[torch.Tensor]:
        return self._greedy_decode(log_probs, input_lengths)

    def align(self, log_probs: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
              target_lengths: torch.Tensor, method: str = "reference") -> List[torch.Tensor]:
        """Per sequence the token of every frame: ctc_alignment_path(..., method=method)."""
        return ctc_alignment_path(log_probs, targets, input_lengths, target_lengths, self.blank_id, method=method)


class CTCSegmentationAligner(CTCAligner):
    """The reference's segmenting aligner (ctc.py:384-460): cuts a long recording at fixed
    intervals and gives each piece a proportional share of the transcript."""

    def __init__(self, num_classes: int, min_segment_length: int = 50, max_segment_length: int = 1000, **kwargs):
        super().__init__(num_classes=num_classes, **kwargs)
        self.min_segment_length = min_segment_length
        self.max_segment_length = max_segment_length

    def segment_and_align(self, log_probs: torch.Tensor, full_transcript: torch.Tensor,
                          segment_boundaries: Optional[torch.Tensor] = None
                          ) -> List[Tuple[torch.Tensor, torch.Tensor, int, int]]:
        """log_probs (time, C), full_transcript (length,) -> [(frames, labels, start, end), ...]: a
        boundary closes a segment when at least min_segment_length frames lie before it."""
        if segment_boundaries is None:
            segment_boundaries = self._detect_segment_boundaries(log_probs, full_transcript)
        segments = []
        start = 0
        for end in (int(v) for v in torch.as_tensor(segment_boundaries).reshape(-1).tolist()):
            if end - start >= self.min_segment_length:
                audio = log_probs[start:end]
                segments.append((audio, self._estimate_segment_text(audio, full_transcript, start, end), start, end))
                start = end
        return segments

    def _detect_segment_boundaries(self, log_probs: torch.Tensor, transcript: torch.Tensor) -> torch.Tensor:
        """A boundary every max_segment_length frames, from frame 0."""
        return torch.arange(0, log_probs.shape[0], self.max_segment_length)

    def _estimate_segment_text(self, segment_audio: torch.Tensor, full_transcript: torch.Tensor, start_frame: int,
                               end_frame: int) -> torch.Tensor:
        """The transcript's share of frames start_frame .. end_frame, with the recording taken as
        1000 frames long: the reference looks for self.log_probs, which is never set."""
        ratio = len(full_transcript) / 1000
        return full_transcript[int(start_frame * ratio):int(end_frame * ratio)]


def remove_ctc_blanks(sequence: torch.Tensor, blank_id: int = 0) -> torch.Tensor:
    """sequence without its blank_id entries."""
    return sequence[sequence != blank_id]


def collapse_repeated_tokens(sequence: torch.Tensor) -> torch.Tensor:
    """Runs of equal tokens replaced by one of them.  An empty sequence is returned as it is;
    otherwise integer tokens come back int64 and floating ones in the default dtype, as the
    reference's torch.tensor(list) gives."""
    if len(sequence) == 0:
        return sequence
    keep = torch.ones(len(sequence), dtype=torch.bool, device=sequence.device)
    keep[1:] = sequence[1:] != sequence[:-1]
    out = sequence[keep]
    if out.dtype.is_floating_point:
        return out.to(torch.get_default_dtype())
    return out if out.dtype == torch.bool else out.to(torch.int64)


def ctc_decode_sequence(sequence: torch.Tensor, blank_id: int = 0) -> torch.Tensor:
    """collapse_repeated_tokens, then remove_ctc_blanks."""
    return remove_ctc_blanks(collapse_repeated_tokens(sequence), blank_id)
