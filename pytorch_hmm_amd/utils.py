"""Transition-matrix factories used to build the hot path's inputs.

Same names, arguments and results as the reference's factories (utils.py:9-103) so that
`HMMPyTorch(create_left_to_right_matrix(128, 0.7))` builds bit-identical parameters; and the two
duration helpers that go with DurationConstrainedHMM (utils.py:289-341, 447-474).
"""
from typing import Optional

import torch


def create_transition_matrix(num_states: int, transition_type: str = "ergodic",
                             self_loop_prob: float = 0.5, forward_prob: float = 0.4,
                             skip_prob: float = 0.1, device: str = "cpu") -> torch.Tensor:
    """Row-stochastic (K, K) matrix of type 'ergodic' | 'left_to_right' |
    'left_to_right_skip' | 'circular' (reference utils.py:9-77)."""
    K = num_states
    if transition_type == "ergodic":
        P = torch.ones(K, K, device=device) + torch.eye(K, device=device) * self_loop_prob * K
    elif transition_type in ("left_to_right", "left_to_right_skip", "circular"):
        P = torch.zeros(K, K, device=device)
        idx = torch.arange(K, device=device)
        if transition_type == "circular":
            P[idx, idx] = self_loop_prob
            P[idx, (idx + 1) % K] = forward_prob
        else:
            last = 1 if transition_type == "left_to_right" else 2
            body = idx[: max(K - last, 0)]
            P[body, body] = self_loop_prob
            P[body, body + 1] = forward_prob
            if transition_type == "left_to_right_skip":
                P[body, body + 2] = skip_prob
                if K >= 2:
                    P[K - 2, K - 2] = self_loop_prob
                    P[K - 2, K - 1] = forward_prob
            P[K - 1, K - 1] = 1.0
    else:
        raise ValueError(f"Unknown transition_type: {transition_type}")
    return P / P.sum(dim=1, keepdim=True)


def create_left_to_right_matrix(num_states: int, self_loop_prob: float = 0.7,
                                device: str = "cpu") -> torch.Tensor:
    """Bakis left-to-right matrix (reference utils.py:80-103)."""
    return create_transition_matrix(num_states, "left_to_right", self_loop_prob,
                                    1.0 - self_loop_prob, device=device)


def create_duration_constrained_matrix(num_states: int, min_duration: int = 1, max_duration: Optional[int] = None,
                                       device: str = "cpu") -> torch.Tensor:
    """The reference's expanded duration matrix (utils.py:289-341): (K*D, K*D) with D =
    max_duration (3 * min_duration when None); row (state, d) is d + 1 frames into the state.
    Below min_duration it moves to (state, d + 1) with probability 1; from there to D - 1 it
    stays with 0.7 and enters (state + 1, 0) with 0.3 (the last state has nowhere to go: its
    rows keep 0.7); at d = D - 1 it must leave (the last state stays where it is).  Rows are
    the reference's values, not renormalised."""
    K, m = num_states, min_duration
    D = m * 3 if max_duration is None else max_duration
    P = torch.zeros(K * D, K * D, device=device)
    if K * D == 0:
        return P
    state = torch.arange(K, device=device).repeat_interleave(D)
    d = torch.arange(D, device=device).repeat(K)
    idx = state * D + d
    nxt = ((state + 1) * D).clamp(max=K * D - 1)
    inner = d < D - 1
    forced = inner & (d < m - 1)
    free = inner & ~(d < m - 1)
    leave = free & (state < K - 1)
    P[idx[forced], idx[forced] + 1] = 1.0
    P[idx[free], idx[free] + 1] = 0.7
    P[idx[leave], nxt[leave]] = 0.3
    last = ~inner & ~(d < m - 1)
    out = last & (state < K - 1)
    stay = last & (state == K - 1)
    P[idx[out], nxt[out]] = 1.0
    P[idx[stay], idx[stay]] = 1.0
    return P


def compute_state_durations(state_sequence: torch.Tensor) -> torch.Tensor:
    """Run lengths of a (T,) state sequence in order (reference utils.py:447-474), int64 on the
    sequence's device; an empty sequence gives the reference's empty float tensor.  No loop over
    T: the run boundaries are found with one comparison, so a GPU tensor stays on the GPU."""
    state_sequence = torch.as_tensor(state_sequence)
    T = state_sequence.shape[0] if state_sequence.dim() else 0
    if T == 0:
        return torch.tensor([])
    dev = state_sequence.device
    change = torch.ones(T, dtype=torch.bool, device=dev)
    change[1:] = state_sequence[1:] != state_sequence[:-1]
    starts = torch.nonzero(change).flatten()
    ends = torch.cat([starts[1:], torch.tensor([T], device=dev)])
    return ends - starts
