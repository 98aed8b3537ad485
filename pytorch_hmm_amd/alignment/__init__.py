"""pytorch_hmm_amd.alignment — drop-in for pytorch_hmm.alignment: dynamic time warping and CTC.

DTW (dtw.py): compute_dtw_path, DTWAligner, ConstrainedDTWAligner, dtw_alignment, dtw_distance and
phoneme_audio_alignment keep the reference's signatures and return conventions; their per-cell
Python loops run as HIP kernels (csrc/dtw.hip: one workgroup per pair, one launch per call, a
batch in one launch), and soft-DTW is differentiable through its own gradient kernel
(autograd.SoftDTW).

CTC (ctc.py): ctc_forward_algorithm and ctc_backward_algorithm, four-deep Python loops in the
reference, are one launch of csrc/ctc.hip (one workgroup per sequence and direction);
ctc_forward_algorithm is differentiable (autograd.CTCLogLik, the occupancy kernel).
ctc_alignment_path and CTCAligner.align return by default what the reference returns -- all
blank_id, because its alpha is never filled -- and with method="posterior" or "viterbi" the forced
alignment it was written to give; ctc_forced_align also returns the expanded positions and the
score.  CTCAligner.forward stays the reference's nn.CTCLoss wrapper; decoding, collapsing and
CTCSegmentationAligner are plain torch on any device.

Transcript forced alignment (forced.py) has no counterpart in the reference: every utterance is
aligned to its own left-to-right chain of transcript states (stay / next / optional skip, ragged
in both lengths) in one launch of csrc/forced.hip -- the best path with per-position durations
(forced_align, monotonic_alignment_search), the differentiable sum over all paths
(forced_alignment_loglik, autograd.ForcedLogLik), the posteriors, and the ForcedAligner module.

Explicit-duration forced alignment (durforced.py) is the same chain with a duration distribution
per position in the place of stay / next weights (dur_lp (B,Lmax,Dmax), -inf for a forbidden
duration), one launch of csrc/durforced.hip: the best segmentation (duration_forced_align), the
differentiable sum over all segmentations (duration_forced_loglik, autograd.DurForcedLogLik), the
position and duration posteriors, and the DurationForcedAligner module -- the alignment side of the
reference's phoneme-duration workflows (HSMMLayer, DurationModel, phoneme_audio_alignment).

The kernels take tensors on a ROCm GPU only.  Of the reference package's four listed techniques
(DTW, CTC, attention, monotonic) it implements the first two; this package adds the monotonic one.
"""
from .ctc import (CTCAligner, CTCSegmentationAligner, collapse_repeated_tokens, ctc_alignment_path,
                  ctc_backward_algorithm, ctc_decode_sequence, ctc_forced_align, ctc_forward_algorithm,
                  expand_targets_with_blank, remove_ctc_blanks)
from .dtw import (ConstrainedDTWAligner, DTWAligner, compute_distance_matrix, compute_dtw_path, dtw_alignment,
                  dtw_distance, extract_phoneme_durations, phoneme_audio_alignment)
from .durforced import (DurationForcedAligner, duration_forced_align, duration_forced_loglik,
                        duration_forced_posteriors)
from .forced import (ForcedAligner, forced_align, forced_alignment_loglik, forced_alignment_posteriors,
                     monotonic_alignment_search)

__all__ = ["DTWAligner", "ConstrainedDTWAligner", "compute_distance_matrix", "compute_dtw_path", "dtw_alignment",
           "dtw_distance", "phoneme_audio_alignment", "extract_phoneme_durations",
           "CTCAligner", "CTCSegmentationAligner", "ctc_forward_algorithm", "ctc_backward_algorithm",
           "ctc_alignment_path", "ctc_forced_align", "expand_targets_with_blank", "remove_ctc_blanks",
           "collapse_repeated_tokens", "ctc_decode_sequence",
           "ForcedAligner", "forced_align", "forced_alignment_loglik", "forced_alignment_posteriors",
           "monotonic_alignment_search",
           "DurationForcedAligner", "duration_forced_align", "duration_forced_loglik", "duration_forced_posteriors"]
