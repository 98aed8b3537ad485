"""HSMMLayer — drop-in for the reference's explicit-duration HMM layer (hsmm.py:20-470) — and
DurationConstrainedHMM (hsmm.py:475-590), at the end of this file.

Parameters keep the reference's names, shapes and initialisation (``transition_logits``,
``observation_means``, ``observation_log_vars``, ``duration_shape``/``duration_rate``
(gamma), ``duration_lambda`` (poisson), ``duration_scale``/``duration_concentration``
(weibull), ``duration_means`` and ``duration_range`` buffers; hsmm.py:61-106).  The duration
and transition tables are the reference's torch expressions (tiny, S x Dmax); the
observation scores run in the gfx950 GMM scorer (one component) and the segment Viterbi
(hsmm.py:208-354) in the HSMM kernels (csrc/hsmm.hip, csrc/hsmm_wide.hip), bit-exact given the
same tables at every supported size: the segment sums follow torch.sum's CPU cascade order
(csrc/tsum.h), pinned to torch.sum for every length 1..1024 and to a reference fixture with
83- and 82-frame segments (tests/golden/hsmm_d96.npz).

``log_likelihood``, ``state_posteriors`` and ``compute_loss`` are additions (the reference's layer
can only decode): the sum over the decoder's segmentations and its gradients, on the same
tables (csrc/hsmm_fb.hip, autograd.HsmmLogLik).
"""
import math
import warnings
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._native import DCHMM_MAX_STATES
from ._native import require_gpu as nat_require_gpu
from .autograd import GmmLogProb, HsmmLogLik, needs_grad


class HSMMLayer(nn.Module):
    def __init__(self, num_states: int, feature_dim: int, duration_distribution: str = "gamma",
                 max_duration: int = 50, learnable_duration_params: bool = True, min_duration: int = 1):
        super().__init__()
        # the segment-Viterbi kernels (csrc/hsmm.hip): S <= 64 with Dmax <= 71, or S <= 128 with
        # Dmax <= 63, keep every open segment in registers; larger layers, up to S <= 1024 and
        # Dmax <= 1024, take the general form of csrc/hsmm_wide.hip (M history and segment sums
        # in HBM).  The reference has no limit; beyond these sizes the layer is rejected here, at
        # construction, rather than at the first forward (BASELINE config 5 is S = 64, Dmax = 40).
        # The general form costs time and memory: at S = 64, T = 2000, B = 32 the decode takes
        # 4.8 ms with 36 MiB of workspace at Dmax = 71 and 23 ms with 1.58 GiB at Dmax = 100
        # (B*T*S*(Dmax+1) fp32; ops.hsmm_viterbi decodes the batch in slices that fit the free
        # memory; INTEGRATION.md "Supported sizes", profiles/r5u_hsmm_wide_edge.log).
        if not 1 <= num_states <= 1024:
            raise ValueError(f"HSMMLayer on gfx950 supports 1 <= num_states <= 1024, got {num_states}")
        if not 1 <= max_duration <= 1024:
            raise ValueError(f"HSMMLayer on gfx950 supports 1 <= max_duration <= 1024, got {max_duration}")
        self.num_states = num_states
        self.feature_dim = feature_dim
        self.duration_distribution = duration_distribution
        self.max_duration = max_duration
        self.min_duration = min_duration
        self.learnable_duration_params = learnable_duration_params
        self.eps = 1e-8
        self._init_parameters()
        self.register_buffer("duration_range",
                             torch.arange(self.min_duration, self.max_duration + 1, dtype=torch.float))

    def _init_parameters(self):
        S, D = self.num_states, self.feature_dim
        self.transition_logits = nn.Parameter(torch.randn(S, S) * 0.1)
        self.observation_means = nn.Parameter(torch.randn(S, D) * 0.1)
        self.observation_log_vars = nn.Parameter(torch.zeros(S, D))
        if self.learnable_duration_params:
            if self.duration_distribution == "gamma":
                self.duration_shape = nn.Parameter(torch.ones(S) * 2.0)
                self.duration_rate = nn.Parameter(torch.ones(S) * 0.2)
            elif self.duration_distribution == "poisson":
                self.duration_lambda = nn.Parameter(torch.ones(S) * 10.0)
            elif self.duration_distribution == "weibull":
                self.duration_scale = nn.Parameter(torch.ones(S) * 10.0)
                self.duration_concentration = nn.Parameter(torch.ones(S) * 2.0)
            else:
                raise ValueError(f"Unknown duration distribution: {self.duration_distribution}")
        else:
            self.register_buffer("duration_means", torch.ones(S) * 10.0)

    # -- parameter tables (reference expressions, hsmm.py:108-179) ----------------------
    def get_transition_matrix(self) -> torch.Tensor:
        logits = self.transition_logits.clone()
        logits.fill_diagonal_(float("-inf"))
        return F.softmax(logits, dim=-1)

    def get_duration_probabilities(self) -> torch.Tensor:
        d = self.duration_range.unsqueeze(0)
        if self.duration_distribution == "gamma":
            shape = F.softplus(self.duration_shape).unsqueeze(1)
            rate = F.softplus(self.duration_rate).unsqueeze(1)
            lp = ((shape - 1) * torch.log(d + self.eps) - rate * d - torch.lgamma(shape)
                  + shape * torch.log(rate + self.eps))
        elif self.duration_distribution == "poisson":
            lam = F.softplus(self.duration_lambda).unsqueeze(1)
            lp = d * torch.log(lam + self.eps) - lam - torch.lgamma(d + 1)
        elif self.duration_distribution == "weibull":
            scale = F.softplus(self.duration_scale).unsqueeze(1)
            conc = F.softplus(self.duration_concentration).unsqueeze(1)
            lp = (torch.log(conc + self.eps) - conc * torch.log(scale + self.eps)
                  + (conc - 1) * torch.log(d + self.eps) - (d / scale) ** conc)
        else:
            return None
        lp = torch.where(d >= self.min_duration, lp, torch.full_like(lp, float("-inf")))
        return torch.exp(lp)

    def get_observation_log_probs(self, observations: torch.Tensor) -> torch.Tensor:
        """(B,T,D) -> (B,T,S) diagonal-Gaussian log-densities (hsmm.py:181-206)."""
        S = self.num_states
        zeros = torch.zeros(S, 1, device=observations.device)
        if needs_grad(observations, self.observation_means, self.observation_log_vars):
            return GmmLogProb.apply(observations, self.observation_means.unsqueeze(1),
                                    self.observation_log_vars.unsqueeze(1), zeros, 0)
        with torch.no_grad():
            return ops.gmm_diag_logprob(observations, self.observation_means.unsqueeze(1),
                                        self.observation_log_vars.unsqueeze(1), zeros, 0)

    # -- decoding (hsmm.py:208-354) -------------------------------------------------------
    def viterbi_decode_hsmm(self, observations: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(states (B,T) int64, best segmentation score (B,))."""
        B, T, _ = observations.shape
        if T > 1000:
            warnings.warn(f"Long sequence ({T} frames) may cause memory issues in HSMM decoding.")
        with torch.no_grad():  # the segment Viterbi is not differentiated (as in the reference)
            obs_log_probs = self.get_observation_log_probs(observations)
            dur_lp = torch.log(self.get_duration_probabilities() + self.eps)
            log_T = torch.log(self.get_transition_matrix() + self.eps)
        if dur_lp.shape[1] < self.max_duration:
            # the reference indexes duration_log_probs[s, d-1] for d up to max_duration
            raise IndexError(f"index {dur_lp.shape[1]} is out of bounds for dimension 1 with size {dur_lp.shape[1]}")
        return ops.hsmm_viterbi(obs_log_probs, dur_lp[:, :self.max_duration], log_T)

    def forward(self, observations: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.viterbi_decode_hsmm(observations)

    # -- likelihood, posteriors, training loss (csrc/hsmm_fb.hip; not in the reference) -------
    def _segment_tables(self, observations: torch.Tensor):
        """The decoder's tables (viterbi_decode_hsmm), built under the caller's grad mode."""
        S, Dm = self.num_states, self.max_duration
        if not ops.hsmm_fb_supported(S, Dm):
            raise ValueError(
                f"HSMMLayer's likelihood and posteriors on gfx950 support num_states <= "
                f"{ops.HSMM_FB_MAX_STATES}, max_duration <= {ops.HSMM_FB_MAX_DURATION} and num_states * "
                f"max_duration <= {ops.HSMM_FB_MAX_CELLS}; got {S} and {Dm}")
        nat_require_gpu(observations)
        obs_log_probs = self.get_observation_log_probs(observations)
        dur_lp = torch.log(self.get_duration_probabilities() + self.eps)
        log_T = torch.log(self.get_transition_matrix() + self.eps)
        if dur_lp.shape[1] < Dm:
            raise IndexError(f"index {dur_lp.shape[1]} is out of bounds for dimension 1 with size {dur_lp.shape[1]}")
        return obs_log_probs, dur_lp[:, :Dm], log_T

    def log_likelihood(self, observations: torch.Tensor) -> torch.Tensor:
        """(B,T,D) -> (B,) log of the sum over all segmentations of the score viterbi_decode_hsmm
        maximises; differentiable in every parameter and in the observations."""
        lp, dur_lp, log_T = self._segment_tables(observations)
        if needs_grad(lp, dur_lp, log_T):
            return HsmmLogLik.apply(lp, dur_lp, log_T, None)
        return ops.hsmm_forward_backward(lp, dur_lp, log_T)[0]

    def state_posteriors(self, observations: torch.Tensor) -> torch.Tensor:
        """(B,T,D) -> (B,T,S) P(state at frame t is s | observations); rows sum to 1."""
        with torch.no_grad():
            lp, dur_lp, log_T = self._segment_tables(observations)
            return ops.hsmm_forward_backward(lp, dur_lp, log_T, want_gamma=True)[1]

    def compute_loss(self, observations: torch.Tensor) -> torch.Tensor:
        """Mean negative log-likelihood (as GaussianHMMLayer.compute_loss)."""
        return -self.log_likelihood(observations).mean()

    def get_expected_durations(self) -> torch.Tensor:
        if self.duration_distribution == "gamma":
            return F.softplus(self.duration_shape) / F.softplus(self.duration_rate)
        if self.duration_distribution == "poisson":
            return F.softplus(self.duration_lambda)
        if self.duration_distribution == "weibull":
            scale = F.softplus(self.duration_scale)
            conc = F.softplus(self.duration_concentration)
            return scale * torch.exp(torch.lgamma(1 + 1 / conc))
        return self.duration_means

    def get_model_info(self) -> dict:
        total = sum(p.numel() for p in self.parameters())
        trainable = sum(p.numel() for p in self.parameters() if p.requires_grad)
        return {"num_states": self.num_states, "feature_dim": self.feature_dim,
                "duration_distribution": self.duration_distribution, "max_duration": self.max_duration,
                "min_duration": self.min_duration, "expected_durations": self.get_expected_durations().tolist(),
                "total_parameters": total, "trainable_parameters": trainable}


class DurationConstrainedHMM(nn.Module):
    """Drop-in for the reference's DurationConstrainedHMM (hsmm.py:475-590): an HMM decoder whose
    Viterbi pass tracks how long each path has stayed in its state and subtracts
    ``duration_penalty_weight`` per frame for a self-loop past ``max_duration`` and for leaving a
    state before ``min_duration`` (soft constraints).

    Parameters keep the reference's names, shapes and creation order (``transition_logits``, then
    ``emission_net`` = Linear(feature_dim, 128), ReLU, Linear(128, num_states), LogSoftmax), so
    the same seed gives the same initial parameters and the reference's ``state_dict`` loads.
    The emission network and the transition log-softmax run in torch on the GPU; the recursion
    (the reference's Python loops over t, s and prev_s) runs in one HIP launch
    (ops.duration_constrained_viterbi, csrc/dchmm.hip) and decodes the reference's states given
    the same emission log-probs.

    The reference takes the run lengths that decide a step's penalties as .max() / .min() over
    the whole batch, so a sequence's decode depends on what it is batched with.  That is kept
    (the batch then runs in one workgroup: B * num_states <= 4096).  ``per_sequence=True`` is an
    extension: every sequence gets the penalties of its own run lengths, i.e. what the
    reference returns when called on one sequence at a time, with no limit on B.
    """

    def __init__(self, num_states: int, feature_dim: int, min_duration: int = 3, max_duration: int = 30, *,
                 per_sequence: bool = False):
        super().__init__()
        if not 1 <= num_states <= DCHMM_MAX_STATES:
            raise ValueError(f"DurationConstrainedHMM on gfx950 supports 1 <= num_states <= "
                             f"{DCHMM_MAX_STATES}, got {num_states}")
        self.num_states = num_states
        self.feature_dim = feature_dim
        self.min_duration = min_duration
        self.max_duration = max_duration
        self.per_sequence = bool(per_sequence)
        self.transition_logits = nn.Parameter(torch.randn(num_states, num_states) * 0.1)
        self.emission_net = nn.Sequential(nn.Linear(feature_dim, 128), nn.ReLU(), nn.Linear(128, num_states),
                                          nn.LogSoftmax(dim=-1))
        self.duration_penalty_weight = 0.1

    def forward(self, observations: torch.Tensor) -> torch.Tensor:
        """(B,T,D) observations -> (B,T) int64 decoded states."""
        emission_log_probs = self.emission_net(observations)
        log_transitions = torch.log(F.softmax(self.transition_logits, dim=-1) + 1e-8)
        return self._constrained_viterbi(emission_log_probs, log_transitions)

    def _constrained_viterbi(self, emission_log_probs: torch.Tensor, log_transitions: torch.Tensor) -> torch.Tensor:
        """(B,T,S) emission log-probs and (S,S) log-transitions -> (B,T) int64 states."""
        states, _, _, _ = ops.duration_constrained_viterbi(
            emission_log_probs, log_transitions, self.min_duration, self.max_duration,
            self.duration_penalty_weight, self.per_sequence)
        return states
