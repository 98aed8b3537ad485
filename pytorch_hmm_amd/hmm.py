"""HMM / HMMPyTorch — drop-in for the reference's core recursions (hmm.py:7-254).

Parameter preparation is the reference's own arithmetic (renormalise P, log(P + 1e-8),
uniform or renormalised p0, hmm.py:20-55), done once on the device the parameters are
given on, so the kernels see the reference's log_P / log_p0 bits.  The per-time-step
loops are replaced by the gfx950 kernels behind torch.ops.hmm355 (see ops.py,
pytorch_hmm_amd/csrc/*.hip); observations must live on a ROCm GPU.
"""
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from .autograd import SequenceLogLik, forward_backward_with_grad, needs_grad


class HMM:
    """Base class: transition matrix P (K,K) and initial distribution p0 (K)
    (reference hmm.py:7-55; same validation and the same ValueError messages)."""

    def __init__(self, P: Union[np.ndarray, torch.Tensor], p0: Optional[Union[np.ndarray, torch.Tensor]] = None,
                 device: str = "cpu"):
        if isinstance(P, np.ndarray):
            P = torch.from_numpy(P).float()
        P = P.to(device)
        self.K = P.shape[0]
        self.device = device
        if len(P.shape) != 2:
            raise ValueError(f"P shape should have length 2. found {len(P.shape)}")
        if P.shape[0] != P.shape[1]:
            raise ValueError(f"P should be square, found {P.shape}")
        P = P / P.sum(dim=1, keepdim=True)
        self.P = P
        self.log_P = torch.log(P + 1e-8)
        if p0 is None:
            self.p0 = torch.ones(self.K, device=device) / self.K
        else:
            if isinstance(p0, np.ndarray):
                p0 = torch.from_numpy(p0).float()
            p0 = p0.to(device)
            if len(p0) != self.K:
                raise ValueError(f"dimensions of p0 {p0.shape} must match P[0] {P.shape[0]}")
            self.p0 = p0 / p0.sum()
        self.log_p0 = torch.log(self.p0 + 1e-8)


class HMMPyTorch(HMM):
    """Forward-backward, Viterbi and likelihood on MI355X (reference hmm.py:58-254)."""

    # -- helpers -------------------------------------------------------------------
    def _device_params(self, dev):
        """(log_P, log_p0, plan) on device `dev`.  Device copies and the transition plan
        (ops.make_plan: the banded structure of log_P, measured once) are cached while log_P /
        log_p0 are unchanged."""
        lp, l0 = self.log_P, self.log_p0
        # The entry holds the source tensors themselves: a hit needs the SAME objects at the
        # same version (a freed host buffer's address can be reused by a new tensor).
        cache = self.__dict__.setdefault("_dev_cache", {})
        hit = cache.get(str(dev))
        if (hit is None or hit[0] is not lp or hit[1] is not l0 or hit[2] != (lp._version, l0._version)
                or lp.requires_grad or l0.requires_grad):
            lpd = lp if lp.device == dev else lp.to(dev)
            l0d = l0 if l0.device == dev else l0.to(dev)
            # A plan re-formed every call (log_P requires grad: a training step changes it)
            # skips the host read of its structure, so a training forward never waits on the
            # device (ops.make_plan read_banded=False).
            grad = lp.requires_grad or l0.requires_grad
            plan = ops.make_plan(lpd.detach(), read_banded=not grad) if dev.type == "cuda" else None
            hit = (lp, l0, (lp._version, l0._version), lpd, l0d, plan)
            if not grad:
                cache[str(dev)] = hit
        return hit[3], hit[4], hit[5]

    @staticmethod
    def _as_batch(observations):
        if observations.dim() == 2:
            return observations.unsqueeze(0), True
        return observations, False

    # -- reference API -------------------------------------------------------------
    def forward_backward(self, observations: torch.Tensor,
                         lengths=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(posterior, forward, backward), each (B,T,K) — 2-D input is NOT squeezed, as in
        the reference (hmm.py:66-130).  forward/backward are exp(log alpha)/exp(log beta) and
        underflow to 0 for long sequences exactly as the reference's do.

        lengths (here and in the methods below; None = every sequence has T frames): one length
        per sequence of a padded batch, a tensor, list or numpy array of B integers in [1, T].
        Sequence b is observations[b, :lengths[b]]; the frames past it are never read and get
        posterior = forward = backward = 0, log_delta = -inf and state -1."""
        obs, _ = self._as_batch(observations)
        B, T, K = obs.shape
        assert K == self.K, f"Observation dim {K} must match model states {self.K}"
        log_P, log_p0, plan = self._device_params(obs.device)
        mask = ops.FB_POSTERIOR | ops.FB_FORWARD | ops.FB_BACKWARD
        lens = ops.active_lengths(lengths, B, T, K)
        if lens is not None:
            return self._fb_ragged(obs, log_P, log_p0, mask, lens)
        if needs_grad(obs, log_P, log_p0):
            # differentiable through all three outputs (autograd.ForwardBackwardFn)
            return forward_backward_with_grad(obs, log_P, log_p0, ops.OBS_PROB, mask, plan)
        post, fwd, bwd, _, _ = ops.forward_backward(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB,
                                                    mask, plan)
        return post, fwd, bwd

    @staticmethod
    def _fb_ragged(obs, log_P, log_p0, mask, lens):
        """The outputs of `mask` for a padded batch with lengths `lens` (ops.active_lengths)."""
        if needs_grad(obs, log_P, log_p0):
            return forward_backward_with_grad(obs, log_P, log_p0, ops.OBS_PROB, mask, None, lens)
        outs = ops.forward_backward_ragged(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB, lens, mask)
        return tuple(o for bit, o in zip((ops.FB_POSTERIOR, ops.FB_FORWARD, ops.FB_BACKWARD), outs) if mask & bit)

    def posteriors(self, observations: torch.Tensor, lengths=None) -> torch.Tensor:
        """Posterior only (what HMMLayer needs); skips the forward/backward outputs."""
        obs, _ = self._as_batch(observations)
        assert obs.shape[-1] == self.K, f"Observation dim {obs.shape[-1]} must match model states {self.K}"
        log_P, log_p0, plan = self._device_params(obs.device)
        lens = ops.active_lengths(lengths, obs.shape[0], obs.shape[1], self.K)
        if lens is not None:
            return self._fb_ragged(obs, log_P, log_p0, ops.FB_POSTERIOR, lens)[0]
        if needs_grad(obs, log_P, log_p0):
            return forward_backward_with_grad(obs, log_P, log_p0, ops.OBS_PROB, ops.FB_POSTERIOR, plan)[0]
        return ops.forward_backward(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB,
                                    ops.FB_POSTERIOR, plan)[0]

    def viterbi_decode(self, observations: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(states (B,T) int64, log_delta (B,T,K)); 2-D input squeezed (hmm.py:132-184)."""
        obs, squeeze = self._as_batch(observations)
        B, T, K = obs.shape
        assert K == self.K, f"Observation dim {K} must match model states {self.K}"
        log_P, log_p0, plan = self._device_params(obs.device)
        lens = ops.active_lengths(lengths, B, T, K)
        if lens is not None:
            states, delta, _ = ops.viterbi_ragged(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB, lens)
        else:
            states, delta, _ = ops.viterbi(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB, plan)
        if squeeze:
            return states.squeeze(0), delta.squeeze(0)
        return states, delta

    def viterbi_nbest(self, observations: torch.Tensor, num_paths: int,
                      lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Extension: the num_paths (at most 16) most probable state paths of every sequence, in
        order, by list Viterbi (ops.viterbi_nbest, csrc/nbest.hip): (paths (B,K,T) int64, scores
        (B,K)), (K,T) and (K) for 2-D input.  scores[b, k] is the fp32 log joint
        log p0[z_0] + sum log P[z_{t-1}, z_t] + sum log(obs + 1e-8)[t, z_t] of path k, non-increasing
        in k; rank 0 is viterbi_decode's path bit for bit.  A rank that does not exist (fewer than
        num_paths paths with a score above -inf) has score -inf and states -1, as have the frames
        past a sequence's length.  Takes no gradients (the inputs are detached).  For normalised
        scores, log p(z | x), pass the paths to path_log_posterior."""
        obs, squeeze = self._as_batch(observations)
        B, T, K = obs.shape
        assert K == self.K, f"Observation dim {K} must match model states {self.K}"
        log_P, log_p0, _ = self._device_params(obs.device)
        lens = ops.active_lengths(lengths, B, T, K)
        paths, scores, _ = ops.viterbi_nbest(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB,
                                             num_paths, lens)
        if squeeze:
            return paths.squeeze(0), scores.squeeze(0)
        return paths, scores

    def _likelihood(self, observations, lengths, kind):
        """compute_likelihood ('ref') / log_likelihood ('exact'), taken at frame lengths[b] - 1."""
        obs, squeeze = self._as_batch(observations)
        B, T, K = obs.shape
        assert K == self.K, f"Observation dim {K} must match model states {self.K}"
        log_P, log_p0, plan = self._device_params(obs.device)
        lens = ops.active_lengths(lengths, B, T, K)
        if needs_grad(obs, log_P, log_p0):
            ll = SequenceLogLik.apply(obs, log_P, log_p0, ops.OBS_PROB, kind, None, lens)
        elif lens is not None:
            ll = ops.forward_backward_ragged(obs, log_P, log_p0, ops.OBS_PROB, lens, 0)[4 if kind == "ref" else 3]
        else:
            ll = ops.forward_backward(obs, log_P, log_p0, ops.OBS_PROB, 0, plan)[4 if kind == "ref" else 3]
        return ll.squeeze(0) if squeeze else ll

    def compute_likelihood(self, observations: torch.Tensor, lengths=None) -> torch.Tensor:
        """The reference's value logsumexp(log(forward[:, -1] + 1e-8)) (hmm.py:186-211),
        including its saturation at log(K*1e-8) once exp(log alpha) underflows."""
        return self._likelihood(observations, lengths, "ref")

    def log_likelihood(self, observations: torch.Tensor, lengths=None) -> torch.Tensor:
        """Extension: the well-defined sequence log-likelihood log sum_j alpha_{T-1}[j]
        (what compute_likelihood would return without exp() underflow)."""
        return self._likelihood(observations, lengths, "exact")

    def sample_posterior(self, observations: torch.Tensor, num_samples: int = 1, lengths=None,
                         generator: Optional[torch.Generator] = None, return_log_prob: bool = False):
        """Extension: num_samples state paths per sequence drawn from p(z | x) by forward-filter
        backward-sample (ops.posterior_sample, csrc/ffbs.hip): (B,K,T) int64, (K,T) for 2-D input,
        -1 in the frames past a sequence's length.  Unlike per-frame draws from posteriors() these
        are paths: consecutive states follow the transition matrix.  generator: a torch.Generator
        on the observations' device for the uniform numbers (None: the default one).  Takes no
        gradients (the inputs are detached).  return_log_prob=True also returns log p(z | x) of
        every drawn path (path_log_posterior), (B,K) or (K)."""
        obs, squeeze = self._as_batch(observations)
        assert obs.shape[-1] == self.K, f"Observation dim {obs.shape[-1]} must match model states {self.K}"
        log_P, log_p0, plan = self._device_params(obs.device)
        states, _ = ops.posterior_sample(obs.detach(), log_P.detach(), log_p0.detach(), ops.OBS_PROB, num_samples,
                                         lengths=lengths, plan=plan, generator=generator)
        if not return_log_prob:
            return states.squeeze(0) if squeeze else states
        with torch.no_grad():
            lp = self.path_log_posterior(obs, states, lengths)
        return (states.squeeze(0), lp.squeeze(0)) if squeeze else (states, lp)

    def _path_terms(self, obs, states, lengths):
        """(log joint (B,K), log-likelihood (B)) of the paths `states` (B,K,T): log p0[z_0] + sum of
        log P[z_{t-1}, z_t] + sum of log(obs + 1e-8)[t, z_t] over the valid frames, by torch gathers."""
        B, T, K = obs.shape
        log_P, log_p0, _ = self._device_params(obs.device)
        log_P, log_p0, obs = log_P.detach(), log_p0.detach(), obs.detach()
        lens = ops.active_lengths(lengths, B, T, K)
        valid = torch.ones(B, T, dtype=torch.bool, device=obs.device) if lens is None else (
            torch.arange(T, device=obs.device)[None, :] < lens.to(obs.device)[:, None])
        z = states.to(obs.device).clamp(min=0)                            # padded frames: any state, masked below
        on = valid[:, None, :]                                            # (B,1,T)
        le = torch.log(obs + 1e-8)                                        # the reference's emissions (hmm.py:86)
        emis = torch.gather(le[:, None].expand(B, z.shape[1], T, K), 3, z.unsqueeze(-1)).squeeze(-1)
        # the T terms are summed in fp64 (the fp32 terms themselves are the model's)
        joint = torch.where(on, emis, torch.zeros_like(emis)).sum(-1, dtype=torch.float64) + log_p0[z[:, :, 0]]
        if T > 1:
            trans = log_P[z[:, :, :-1], z[:, :, 1:]]
            joint = joint + torch.where(on[:, :, 1:], trans, torch.zeros_like(trans)).sum(-1, dtype=torch.float64)
        return joint.to(torch.float32), self.log_likelihood(obs, lengths)

    def path_log_posterior(self, observations: torch.Tensor, states: torch.Tensor, lengths=None) -> torch.Tensor:
        """Extension: log p(z | x) = log p0[z_0] + sum log P[z_{t-1}, z_t] + sum log e_t[z_t] -
        log_likelihood of the state paths `states` ((B,K,T) -> (B,K), or (B,T) -> (B); with 2-D
        observations (K,T) -> (K) or (T) -> a scalar).  Emissions are the reference's
        log(obs + 1e-8); frames past a sequence's length are ignored (any value, -1 included)."""
        obs, squeeze = self._as_batch(observations)
        assert obs.shape[-1] == self.K, f"Observation dim {obs.shape[-1]} must match model states {self.K}"
        st = states.unsqueeze(0) if squeeze else states
        single = st.dim() == 2
        if single:
            st = st.unsqueeze(1)
        if st.dim() != 3 or st.shape[0] != obs.shape[0] or st.shape[2] != obs.shape[1]:
            raise ValueError(f"states must be (B, K, T) or (B, T) for observations {tuple(obs.shape)}; "
                             f"got {tuple(states.shape)}")
        joint, loglik = self._path_terms(obs, st, lengths)
        out = joint - loglik[:, None]
        if single:
            out = out.squeeze(1)
        return out.squeeze(0) if squeeze else out

    def reestimate(self, observations: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Extension: one Baum-Welch re-estimation of the chain for given emissions (em.e_step and
        em.transition_m_step): (P_new (K,K), p0_new (K), loglik (B,)) with loglik the exact
        log-likelihood under the current parameters.  The emissions are the class's own,
        log(observations + 1e-8), with log_P and log_p0 as the recursions use them.  The object is
        not modified; a state that is never occupied keeps its row of P.  At most 256 states."""
        from . import em
        obs, _ = self._as_batch(observations)
        if obs.dim() != 3 or obs.shape[-1] != self.K:
            raise ValueError(f"observations must be (B, T, {self.K}); got {tuple(observations.shape)}")
        from . import _native as nat
        nat.require_gpu(obs)
        log_P, log_p0, plan = self._device_params(obs.device)
        with torch.no_grad():
            # log(P + 1e-8) and log(obs + 1e-8) are floored by construction: in the kernels' range
            es = em.e_step(torch.log(obs.detach() + 1e-8), log_P.detach(), log_p0.detach(), lengths, plan,
                           range_guard=False)
            P, p0 = em.transition_m_step(es.xi, es.gamma0, es.n_seq, self.P.detach().to(obs.device),
                                         self.p0.detach().to(obs.device))
        return P, p0, es.loglik

    def sample(self, seq_length: int, batch_size: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """Sample (states, one-hot observations) — reference hmm.py:213-245 (not on the hot
        path; plain torch sampling on the parameters' device)."""
        dev = self.P.device
        states = torch.zeros(batch_size, seq_length, dtype=torch.long, device=dev)
        observations = torch.zeros(batch_size, seq_length, self.K, device=dev)
        states[:, 0] = torch.distributions.Categorical(self.p0).sample((batch_size,))
        for t in range(seq_length):
            if t > 0:
                states[:, t] = torch.distributions.Categorical(self.P[states[:, t - 1]]).sample()
            observations[torch.arange(batch_size, device=dev), t, states[:, t]] = 1.0
        return states, observations

    def to(self, device: str):
        """Move parameters (reference hmm.py:247-254)."""
        self.device = device
        self.P = self.P.to(device)
        self.log_P = self.log_P.to(device)
        self.p0 = self.p0.to(device)
        self.log_p0 = self.log_p0.to(device)
        return self
