"""pytorch_hmm_amd.alignment — drop-in for pytorch_hmm.alignment's dynamic time warping.

compute_dtw_path, DTWAligner, ConstrainedDTWAligner, dtw_alignment, dtw_distance and
phoneme_audio_alignment keep the reference's signatures and return conventions; their per-cell
Python loops run as HIP kernels (csrc/dtw.hip: one workgroup per pair, one launch per call, a
batch in one launch), and soft-DTW is differentiable through its own gradient kernel
(autograd.SoftDTW).  The kernels take tensors on a ROCm GPU only.

The reference's CTC alignment (pytorch_hmm.alignment.ctc) is out of scope here: CTCAligner wraps
nn.CTCLoss, which already runs on the GPU, and ctc_alignment_path never fills its log_alpha.
"""
from .dtw import (ConstrainedDTWAligner, DTWAligner, compute_distance_matrix, compute_dtw_path, dtw_alignment,
                  dtw_distance, extract_phoneme_durations, phoneme_audio_alignment)

__all__ = ["DTWAligner", "ConstrainedDTWAligner", "compute_distance_matrix", "compute_dtw_path", "dtw_alignment",
           "dtw_distance", "phoneme_audio_alignment", "extract_phoneme_durations"]
