"""pytorch_hmm_amd — MI355X (gfx950) native HMM inference core.

Drop-in for the hot path of crlotwhite/pytorch_hmm: HMMPyTorch.forward_backward /
viterbi_decode / compute_likelihood, HMMLayer, GaussianHMMLayer,
MixtureGaussianHMMLayer and HSMMLayer, and the next rows of that path (NeuralHMM,
SemiMarkovHMM, StreamingHMMProcessor, DurationConstrainedHMM), with the per-time-step loops replaced by
hand-written HIP kernels (csrc/) behind the C ABI in include/hmm355.h and the
torch.library ops in ops.py.  Tensors must be on a ROCm GPU; there is no CPU path.
"""
from .hmm import HMM, HMMPyTorch
from .utils import create_left_to_right_matrix, create_transition_matrix
from . import ops

__all__ = ["HMM", "HMMPyTorch", "create_left_to_right_matrix", "create_transition_matrix", "ops"]

from .hmm_layer import HMMLayer, GaussianHMMLayer
from .mixture_gaussian import MixtureGaussianHMMLayer
from .hsmm import HSMMLayer
from .neural import NeuralHMM, ContextualNeuralHMM
from .semi_markov import DurationModel, SemiMarkovHMM, AdaptiveDurationHSMM
from .streaming import AdaptiveLatencyController, StreamingHMMProcessor, StreamingResult

__all__ += ["HMMLayer", "GaussianHMMLayer", "MixtureGaussianHMMLayer", "HSMMLayer", "NeuralHMM",
            "ContextualNeuralHMM", "DurationModel", "SemiMarkovHMM", "AdaptiveDurationHSMM",
            "StreamingHMMProcessor", "StreamingResult", "AdaptiveLatencyController"]

from . import alignment
from .alignment import (ConstrainedDTWAligner, CTCAligner, CTCSegmentationAligner, DTWAligner,
                        DurationForcedAligner, ForcedAligner, duration_forced_align, duration_forced_loglik,
                        duration_forced_posteriors,
                        forced_align, forced_alignment_loglik, forced_alignment_posteriors,
                        monotonic_alignment_search)

__all__ += ["alignment", "DTWAligner", "ConstrainedDTWAligner", "CTCAligner", "CTCSegmentationAligner",
            "ForcedAligner", "forced_align", "forced_alignment_loglik", "forced_alignment_posteriors",
            "monotonic_alignment_search", "DurationForcedAligner", "duration_forced_align",
            "duration_forced_loglik", "duration_forced_posteriors"]

from .hsmm import DurationConstrainedHMM
from .utils import compute_state_durations, create_duration_constrained_matrix

__all__ += ["DurationConstrainedHMM", "compute_state_durations", "create_duration_constrained_matrix"]

from .ops import posterior_sample

__all__ += ["posterior_sample"]

from . import em
from .em import EStats, e_step, gaussian_m_step, transition_m_step

__all__ += ["em", "EStats", "e_step", "transition_m_step", "gaussian_m_step"]

from . import sparse
from .sparse import SparseHMM, SparseTransitions, sparse_transition_m_step

__all__ += ["sparse", "SparseHMM", "SparseTransitions", "sparse_transition_m_step"]

from . import range_guard

__all__ += ["range_guard"]
