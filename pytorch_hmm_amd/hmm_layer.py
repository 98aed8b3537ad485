"""HMMLayer / GaussianHMMLayer — nn.Module drop-ins for the reference's layers
(hmm_layer.py:11-217 and :220-363).

Same constructor arguments, parameter names and shapes (state_dict compatible:
``log_transition_logits`` / ``transition_matrix``, ``log_initial_logits``, ``means``,
``log_scales``), same train/eval dispatch, same first-call quirk of ``_get_hmm`` (call 1
builds an HMMPyTorch, which renormalises P; later calls assign log(P + 1e-8) directly,
hmm_layer.py:75-89).  The recursions run in the HIP kernels (ops.py); the Gaussian
emission of GaussianHMMLayer runs in the gfx950 GMM scorer (single component).
"""
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .autograd import GmmLogProb, valid_frames, needs_grad
from .hmm import HMMPyTorch
from .utils import create_left_to_right_matrix, create_transition_matrix


class HMMLayer(nn.Module):
    """HMM as a layer over per-frame state scores x (B,T,K) (reference hmm_layer.py:11-217)."""

    def __init__(self, num_states: int, learnable_transitions: bool = True,
                 transition_type: str = "left_to_right", self_loop_prob: float = 0.7,
                 viterbi_inference: bool = True, apply_sigmoid: bool = True):
        super().__init__()
        self.num_states = num_states
        self.viterbi_inference = viterbi_inference
        self.apply_sigmoid = apply_sigmoid
        if transition_type == "left_to_right":
            P_init = create_left_to_right_matrix(num_states, self_loop_prob)
        else:
            P_init = create_transition_matrix(num_states, transition_type, self_loop_prob)
        if learnable_transitions:
            self.log_transition_logits = nn.Parameter(torch.log(P_init + 1e-8))   # :48
        else:
            self.register_buffer("transition_matrix", P_init)                      # :51
            self.log_transition_logits = None
        p0_init = torch.ones(num_states) / num_states
        self.log_initial_logits = nn.Parameter(torch.log(p0_init + 1e-8))        # :55-56
        self._hmm = None

    # -- parameters (hmm_layer.py:61-89) ---------------------------------------------
    def _get_transition_matrix(self) -> torch.Tensor:
        if self.log_transition_logits is not None:
            return F.softmax(self.log_transition_logits, dim=1)
        return self.transition_matrix

    def _get_initial_probabilities(self) -> torch.Tensor:
        return F.softmax(self.log_initial_logits, dim=0)

    def _param_key(self):
        """Identity + version of the tensors P and p0 derive from (and whether autograd is
        recording through them)."""
        src = self.log_transition_logits if self.log_transition_logits is not None else self.transition_matrix
        init = self.log_initial_logits
        grad = torch.is_grad_enabled() and (src.requires_grad or init.requires_grad)
        return (src, src._version, src.device, init, init._version, grad)

    def _get_hmm(self) -> HMMPyTorch:
        if self._hmm is not None:
            # later calls assign log(P + 1e-8) (hmm_layer.py:83-86).  With the parameters
            # unchanged since the previous later call and no autograd, the assigned tensors
            # would be bit-identical: keep them, so HMMPyTorch's device copies and transition
            # plan stay cached (no per-call softmax/log/plan launches).
            key = self._param_key()
            old = self.__dict__.get("_hmm_key")
            if (old is not None and not key[5] and old[0] is key[0] and old[3] is key[3]
                    and old[1:3] == key[1:3] and old[4:] == key[4:]):
                return self._hmm
        P = self._get_transition_matrix()
        p0 = self._get_initial_probabilities()
        device = P.device
        if self._hmm is None:
            self._hmm = HMMPyTorch(P, p0, device=str(device))
            self.__dict__["_hmm_key"] = None   # call 2 must re-derive (first-call quirk)
        else:
            self._hmm.P = P
            self._hmm.log_P = torch.log(P + 1e-8)
            self._hmm.p0 = p0
            self._hmm.log_p0 = torch.log(p0 + 1e-8)
            self._hmm.device = str(device)
            self.__dict__["_hmm_key"] = self._param_key()
        return self._hmm

    # -- forward (hmm_layer.py:91-142) -------------------------------------------------
    def forward(self, x: torch.Tensor, return_alignment: bool = False,
                lengths=None) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """lengths (None = every sequence has T frames): one length per sequence of a padded batch
        (HMMPyTorch.forward_backward).  The frames past a sequence's length are never read; their
        posterior / one-hot rows are zero and the alignment is -1 there."""
        if self.apply_sigmoid:
            x = torch.sigmoid(x)
        if x.dim() == 2:
            x = x.unsqueeze(0)
        B, T, K = x.shape
        if K != self.num_states:
            raise ValueError(f"Input feature dim {K} must match num_states {self.num_states}")
        hmm = self._get_hmm()
        lens = ops.active_lengths(lengths, B, T, K)
        valid = None if lens is None else valid_frames(lens, T, x.device)
        if self.training:
            posteriors = hmm.posteriors(x, lens)
        elif self.viterbi_inference:
            states, _ = hmm.viterbi_decode(x, lens)
            if valid is None:
                posteriors = F.one_hot(states, num_classes=self.num_states).float()
            else:
                posteriors = F.one_hot(states.clamp(min=0), num_classes=self.num_states).float() * valid[..., None]
        else:
            posteriors = hmm.posteriors(x, lens)
        if return_alignment and not self.training:
            if self.viterbi_inference:
                alignment = states
            else:
                alignment = torch.argmax(posteriors, dim=-1)
                if valid is not None:
                    alignment = torch.where(valid, alignment, torch.full_like(alignment, -1))
            return posteriors, alignment
        return posteriors

    def compute_loss(self, observations: torch.Tensor, target_alignment: Optional[torch.Tensor] = None,
                     lengths=None) -> torch.Tensor:
        """Cross-entropy on posteriors when a target alignment is given, else -mean of
        compute_likelihood (hmm_layer.py:144-173).  With lengths the cross-entropy runs over the
        valid frames only and the likelihood of sequence b is that of its lengths[b] frames."""
        hmm = self._get_hmm()
        if target_alignment is not None:
            posteriors = self.forward(observations, lengths=lengths)
            lens = ops.active_lengths(lengths, posteriors.shape[0], posteriors.shape[1], self.num_states)
            if lens is not None:
                valid = valid_frames(lens, posteriors.shape[1], posteriors.device)
                return F.cross_entropy(posteriors[valid], target_alignment.reshape(valid.shape)[valid])
            return F.cross_entropy(posteriors.view(-1, self.num_states), target_alignment.view(-1))
        if self.apply_sigmoid:
            observations = torch.sigmoid(observations)
        return -hmm.compute_likelihood(observations, lengths).mean()

    def align(self, observations: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(states, log_delta) by Viterbi (hmm_layer.py:175-191)."""
        hmm = self._get_hmm()
        if self.apply_sigmoid:
            observations = torch.sigmoid(observations)
        return hmm.viterbi_decode(observations, lengths)

    def sample_alignment(self, x: torch.Tensor, num_samples: int = 1, lengths=None,
                         generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """num_samples alignments per sequence drawn from p(z | x) (HMMPyTorch.sample_posterior) on
        the emissions align() decodes: (B,K,T) int64, (K,T) for 2-D input, -1 in the frames past a
        sequence's length.  No gradients."""
        hmm = self._get_hmm()
        if self.apply_sigmoid:
            x = torch.sigmoid(x)
        return hmm.sample_posterior(x, num_samples, lengths, generator)

    def nbest_alignment(self, x: torch.Tensor, num_paths: int, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The num_paths most probable alignments per sequence, in order (HMMPyTorch.viterbi_nbest),
        on the emissions align() decodes: (paths (B,K,T) int64, scores (B,K)), (K,T) and (K) for 2-D
        input.  Rank 0 is align()'s path; -1 in the frames past a sequence's length and in a rank
        that does not exist.  No gradients."""
        hmm = self._get_hmm()
        if self.apply_sigmoid:
            x = torch.sigmoid(x)
        return hmm.viterbi_nbest(x, num_paths, lengths)

    def sample(self, seq_length: int, batch_size: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._get_hmm().sample(seq_length, batch_size)

    def get_transition_matrix(self) -> torch.Tensor:
        return self._get_transition_matrix()

    def get_initial_probabilities(self) -> torch.Tensor:
        return self._get_initial_probabilities()

    def extra_repr(self) -> str:
        return f"num_states={self.num_states}, viterbi_inference={self.viterbi_inference}"


def _gaussian_component_params(log_scales: torch.Tensor, covariance_type: str, D: int):
    """(K,1,D) log-variances for the GMM scorer from GaussianHMMLayer.log_scales
    (hmm_layer.py:286-319: log_var = 2*log_scales; 'full' uses the diagonal; 'spherical'
    one value per state)."""
    if covariance_type == "full":
        lv = 2 * torch.diagonal(log_scales, dim1=-2, dim2=-1)
    elif covariance_type == "spherical":
        lv = (2 * log_scales).expand(-1, D)
    else:
        lv = 2 * log_scales
    return lv.unsqueeze(1)


class GaussianHMMLayer(nn.Module):
    """Gaussian emissions + HMMLayer(apply_sigmoid=False) (reference hmm_layer.py:220-363)."""

    def __init__(self, num_states: int, feature_dim: int, covariance_type: str = "diag",
                 learnable_transitions: bool = True, transition_type: str = "left_to_right"):
        super().__init__()
        self.num_states = num_states
        self.feature_dim = feature_dim
        self.covariance_type = covariance_type
        self.hmm_layer = HMMLayer(num_states=num_states, learnable_transitions=learnable_transitions,
                                  transition_type=transition_type, apply_sigmoid=False)
        self.means = nn.Parameter(torch.randn(num_states, feature_dim))
        if covariance_type == "full":
            self.log_scales = nn.Parameter(torch.zeros(num_states, feature_dim, feature_dim))
        elif covariance_type == "diag":
            self.log_scales = nn.Parameter(torch.zeros(num_states, feature_dim))
        elif covariance_type == "spherical":
            self.log_scales = nn.Parameter(torch.zeros(num_states, 1))
        else:
            raise ValueError(f"Unknown covariance_type: {covariance_type}")

    def _compute_gaussian_log_probs(self, observations: torch.Tensor) -> torch.Tensor:
        """(B,T,D) -> (B,T,K) Gaussian log-densities on the gfx950 scorer
        (hmm_layer.py:270-323)."""
        B, T, D = observations.shape
        log_w = torch.zeros(self.num_states, 1, device=self.means.device)
        if needs_grad(observations, self.means, self.log_scales):
            lv = _gaussian_component_params(self.log_scales, self.covariance_type, D)
            return GmmLogProb.apply(observations, self.means.unsqueeze(1), lv, log_w, 0)
        lv = _gaussian_component_params(self.log_scales.detach(), self.covariance_type, D)
        return ops.gmm_diag_logprob(observations.detach(), self.means.detach().unsqueeze(1), lv, log_w, 0)

    def _observation_probs(self, observations, lengths):
        """exp of the Gaussian log-densities.  With lengths the padded frames are zeroed first
        (selected, not multiplied), so whatever they hold stays out of the parameters' gradients."""
        if lengths is not None:
            B, T = observations.shape[:2]
            lens = ops.active_lengths(lengths, B, T, self.num_states)
            if lens is not None:
                valid = valid_frames(lens, T, observations.device)
                observations = torch.where(valid[..., None], observations, torch.zeros_like(observations))
        return torch.exp(self._compute_gaussian_log_probs(observations))

    def forward(self, observations: torch.Tensor, lengths=None) -> torch.Tensor:
        return self.hmm_layer(self._observation_probs(observations, lengths), lengths=lengths)

    def compute_loss(self, observations: torch.Tensor, lengths=None) -> torch.Tensor:
        observation_probs = self._observation_probs(observations, lengths)
        hmm = self.hmm_layer._get_hmm()
        return -hmm.compute_likelihood(observation_probs, lengths).mean()

    def sample_alignment(self, x: torch.Tensor, num_samples: int = 1, lengths=None,
                         generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """num_samples alignments per sequence drawn from p(z | x) under the Gaussian emissions
        (HMMLayer.sample_alignment on the observation probabilities): (B,K,T) int64, -1 in the
        frames past a sequence's length.  No gradients."""
        with torch.no_grad():
            probs = self._observation_probs(x, lengths)
        return self.hmm_layer.sample_alignment(probs, num_samples, lengths, generator)

    # -- Baum-Welch (em.py) ----------------------------------------------------------------
    _EM_UPDATES = ("transitions", "initial", "means", "variances")

    def nbest_alignment(self, x: torch.Tensor, num_paths: int, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The num_paths most probable alignments per sequence under the Gaussian emissions
        (HMMLayer.nbest_alignment on the observation probabilities): (paths (B,K,T) int64, scores
        (B,K)).  No gradients."""
        with torch.no_grad():
            probs = self._observation_probs(x, lengths)
        return self.hmm_layer.nbest_alignment(probs, num_paths, lengths)

    def _em_model(self):
        """(log_P, log_p0) of the E-step: log_softmax of the logits, or log of the fixed
        transition matrix with -inf at its zeros."""
        from . import em
        hl = self.hmm_layer
        if hl.log_transition_logits is not None:
            log_P = F.log_softmax(hl.log_transition_logits, dim=1)
        else:
            log_P = em.log_of(hl.transition_matrix)
        return log_P, F.log_softmax(hl.log_initial_logits, dim=0)

    def _em_iteration(self, batches, update, var_floor):
        """One EM iteration over `batches` ([(x, lengths)]); (total log-likelihood under the
        parameters before the update, frames)."""
        from . import em
        if self.covariance_type == "full":
            raise NotImplementedError("em_step covers covariance_type 'diag' and 'spherical', not 'full'")
        em.check_update(update, self._EM_UPDATES, "GaussianHMMLayer.em_step")
        S, D = self.num_states, self.feature_dim
        hl = self.hmm_layer
        with torch.no_grad():
            mu = self.means.detach().unsqueeze(1)
            lv = _gaussian_component_params(self.log_scales.detach(), self.covariance_type, D).contiguous()
            log_w = torch.zeros(S, 1, device=mu.device)
            log_P, log_p0 = self._em_model()
            score = lambda x: ops.gmm_diag_logprob(x, mu, lv, log_w, 0)
            stats = lambda x, gamma, lens: ops.gmm_stats(x, gamma, mu, lv, log_w, 0, lens)
            want = "means" in update or "variances" in update
            es, sums, frames = em.accumulate(batches, D, S, score, stats, log_P, log_p0, want_stats=want)
            if "transitions" in update or "initial" in update:
                P, p0 = em.transition_m_step(es.xi, es.gamma0, es.n_seq, torch.exp(log_P), torch.exp(log_p0))
                if "transitions" in update:
                    if hl.log_transition_logits is not None:
                        hl.log_transition_logits.copy_(torch.log(P.clamp(min=1e-30)))
                    else:
                        hl.transition_matrix.copy_(P)
                if "initial" in update:
                    hl.log_initial_logits.copy_(torch.log(p0.clamp(min=1e-30)))
            if want:
                old_lv = (2 * self.log_scales.detach()).reshape(S, 1, -1) if self.covariance_type == "diag" else \
                    (2 * self.log_scales.detach()).reshape(S, 1)
                new_mu, new_lv, _ = em.gaussian_m_step(*sums, mu, self.covariance_type, var_floor, log_vars=old_lv)
                if "means" in update:
                    self.means.copy_(new_mu.squeeze(1))
                if "variances" in update:
                    self.log_scales.copy_(0.5 * new_lv.reshape(self.log_scales.shape))
        return float(es.loglik.sum(dtype=torch.float64)), frames

    def em_step(self, observations: torch.Tensor, lengths=None, *,
                update=("transitions", "initial", "means", "variances"), var_floor: float = 1e-4) -> float:
        """One Baum-Welch iteration on observations (B,T,D) (lengths: one length per sequence of a
        padded batch, or None); returns the total log-likelihood under the parameters BEFORE the
        update.  E-step model: the scorer's Gaussian log-densities as log-emissions, log_P =
        log_softmax(log_transition_logits) (or the log of the fixed transition_matrix, -inf at its
        zeros), log_p0 = log_softmax(log_initial_logits).  The M-step writes, in place and for the
        names in `update`: log_transition_logits = log(clamp(P', 1e-30)) (or the transition_matrix
        buffer), log_initial_logits likewise, means, and log_scales = log(var') / 2 with var' floored
        at var_floor.  covariance_type 'diag' and 'spherical'; 'full' raises NotImplementedError."""
        from . import em
        return self._em_iteration(em.as_batches(observations, lengths), tuple(update), var_floor)[0]

    def fit(self, observations, lengths=None, n_iter: int = 10, tol: float = 1e-4):
        """Up to n_iter EM iterations (em_step); returns the total log-likelihood before each
        iteration and stops once the gain per frame drops below tol.  observations may be a list of
        (x, lengths) pairs: their statistics are summed before each M-step."""
        from . import em
        batches = em.as_batches(observations, lengths)
        return em.run_fit(lambda: self._em_iteration(batches, self._EM_UPDATES, 1e-4), n_iter, tol)

    def extra_repr(self) -> str:
        return (f"num_states={self.num_states}, feature_dim={self.feature_dim}, "
                f"covariance_type={self.covariance_type}")
