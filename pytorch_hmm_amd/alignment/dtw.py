"""Dynamic time warping with the reference's interface (pytorch_hmm/alignment/dtw.py).

The distance matrix is plain torch on the device; the O(N*M) recursions, the backtrace and the
soft-DTW gradient are the HIP kernels behind ops.dtw / ops.soft_dtw / autograd.SoftDTW.
"""
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native as nat
from .. import ops
from ..autograd import SoftDTW

# elements of the (rows, M, D) difference tensor formed at once for euclidean / manhattan
_CHUNK_ELEMS = 1 << 24


def compute_distance_matrix(x: torch.Tensor, y: torch.Tensor, distance_fn: str = 'euclidean') -> torch.Tensor:
    """Distances between the frames of x (N,D) and y (M,D): (N,M); also (B,N,D), (B,M,D) -> (B,N,M).
    The reference's three formulae (dtw.py:22-39); euclidean and manhattan are formed in row chunks,
    so the (rows,M,D) temporary stays bounded."""
    if distance_fn == 'cosine':
        x_norm = F.normalize(x, p=2, dim=-1)
        y_norm = F.normalize(y, p=2, dim=-1)
        return 1 - torch.matmul(x_norm, y_norm.transpose(-1, -2))
    if distance_fn not in ('euclidean', 'manhattan'):
        raise ValueError(f"Unknown distance function: {distance_fn}")
    N, M, D = x.shape[-2], y.shape[-2], x.shape[-1]
    batch = x.shape[0] if x.dim() == 3 else 1
    rows = max(1, _CHUNK_ELEMS // max(1, batch * M * D))
    y_expanded = y.unsqueeze(-3)
    pieces = []
    for r0 in range(0, max(N, 1), rows):
        diff = x[..., r0:r0 + rows, :].unsqueeze(-2) - y_expanded
        pieces.append(torch.norm(diff, dim=-1) if distance_fn == 'euclidean' else torch.sum(torch.abs(diff), dim=-1))
    return pieces[0] if len(pieces) == 1 else torch.cat(pieces, dim=-2)


def _paths(path_i, path_j, path_len):
    """Per-pair int64 paths of the true length: one host read of path_len for the batch."""
    lens = path_len.tolist()
    pi, pj = path_i.long(), path_j.long()
    return [pi[b, :n] for b, n in enumerate(lens)], [pj[b, :n] for b, n in enumerate(lens)]


def compute_dtw_path(distance_matrix: torch.Tensor,
                     step_pattern: str = 'symmetric') -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(path_i, path_j, cost_matrix) of one (N,M) distance matrix (dtw.py:47-152): int64 paths of the
    true length from (0,0) to (N-1,M-1), the (N,M) fp32 cost matrix."""
    nat.require_gpu(distance_matrix)
    cost, _, path_i, path_j, path_len = ops.dtw(distance_matrix.unsqueeze(0), ops.dtw_pattern(step_pattern))
    pi, pj = _paths(path_i, path_j, path_len)
    return pi[0], pj[0], cost[0]


def dtw_distance(x: torch.Tensor, y: torch.Tensor, distance_fn: str = 'euclidean',
                 step_pattern: str = 'symmetric') -> torch.Tensor:
    """The DTW cost of x (N,D) against y (M,D): the value-only kernel call (no cost table, no path)."""
    nat.require_gpu(x, y)
    dist = compute_distance_matrix(x, y, distance_fn)
    _, total, _, _, _ = ops.dtw(dist.unsqueeze(0), ops.dtw_pattern(step_pattern), None, None, False, False)
    return total[0]


def _align_hard(x, y, distance_fn, step_pattern):
    """Batched hard alignment: x (B,N,D), y (B,M,D) -> lists of paths and the totals (B)."""
    nat.require_gpu(x, y)
    dist = compute_distance_matrix(x, y, distance_fn)
    _, total, path_i, path_j, path_len = ops.dtw(dist, ops.dtw_pattern(step_pattern), None, None, False, True)
    pi, pj = _paths(path_i, path_j, path_len)
    return pi, pj, total


def dtw_alignment(x: torch.Tensor, y: torch.Tensor, distance_fn: str = 'euclidean',
                  step_pattern: str = 'symmetric') -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(path_i, path_j, total_cost) of x (N,D) against y (M,D) (dtw.py:178-202)."""
    pi, pj, total = _align_hard(x.unsqueeze(0), y.unsqueeze(0), distance_fn, step_pattern)
    return pi[0], pj[0], total[0]


class DTWAligner(nn.Module):
    """The reference's DTWAligner (dtw.py:205-305).  forward(x, y) with (N,D), (M,D) returns
    (path_i, path_j, total_cost); with (B,N,D), (B,M,D) two lists of paths and the stacked costs (B),
    from one batched kernel launch and one host read of the path lengths.  soft_dtw=True returns the
    soft-DTW value, differentiable in x and y, with the reference's placeholder path (arange(N) and
    the rounded linspace).  `bandwidth` is stored and, as in the reference, not used."""

    def __init__(self, distance_fn: str = 'euclidean', step_pattern: str = 'symmetric',
                 bandwidth: Optional[int] = None, soft_dtw: bool = False, gamma: float = 0.1):
        super().__init__()
        self.distance_fn = distance_fn
        self.step_pattern = step_pattern
        self.bandwidth = bandwidth
        self.soft_dtw = soft_dtw
        self.gamma = gamma

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        if x.dim() == 3:
            return self._align_batch(x, y)
        pi, pj, cost = self._align_batch(x.unsqueeze(0), y.unsqueeze(0))
        return pi[0], pj[0], cost[0]

    def _align_batch(self, x, y):
        if self.soft_dtw:
            return self._soft_dtw_align(x, y)
        return _align_hard(x, y, self.distance_fn, self.step_pattern)

    def _soft_dtw_align(self, x, y):
        nat.require_gpu(x, y)
        dist = compute_distance_matrix(x, y, self.distance_fn)
        B, N, M = dist.shape
        total = SoftDTW.apply(dist, self.gamma, None, None)
        path_i = torch.arange(N, device=dist.device)
        path_j = torch.round(torch.linspace(0, M - 1, N, device=dist.device)).long()
        return [path_i] * B, [path_j] * B, total


class ConstrainedDTWAligner(DTWAligner):
    """The reference's ConstrainedDTWAligner (dtw.py:308-340).  The reference builds a band mask
    over the distance matrix in an O(N*M) Python loop and then discards it: it calls
    dtw_alignment(x, y, ...), which recomputes the distances.  Its results are therefore those of
    the unconstrained hard DTWAligner (also with soft_dtw=True), and that is what this class
    returns, without the mask loop.  For a real band fill the distance matrix with +inf outside it
    and call ops.dtw."""

    def __init__(self, bandwidth: int = 10, monotonic: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.bandwidth = bandwidth
        self.monotonic = monotonic

    def _align_batch(self, x, y):
        return _align_hard(x, y, self.distance_fn, self.step_pattern)


def phoneme_audio_alignment(phoneme_features: torch.Tensor, audio_features: torch.Tensor,
                            phoneme_durations: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(alignment (num_frames) int64: the phoneme of each frame; boundaries: 0, the frame at which
    the path enters each further phoneme, num_frames) from the cosine / asymmetric DTW path
    (dtw.py:344-384), as vectorised torch on the device."""
    aligner = DTWAligner(distance_fn='cosine', step_pattern='asymmetric')
    path_i, path_j, _ = aligner(phoneme_features, audio_features)
    num_frames = audio_features.shape[0]
    dev = audio_features.device
    # the reference writes alignment[frame] = phoneme in path order; the path's phoneme index never
    # decreases, so the last write of a frame is the largest
    alignment = torch.zeros(num_frames, dtype=torch.long, device=dev)
    alignment.scatter_reduce_(0, path_j, path_i, reduce='amax', include_self=True)
    entered = path_i[1:] > path_i[:-1]
    edge = torch.tensor([0, num_frames], device=dev, dtype=torch.long)
    boundaries = torch.cat([edge[:1], path_j[1:][entered], edge[1:]])
    return alignment, boundaries


def extract_phoneme_durations(alignment: torch.Tensor, num_phonemes: int) -> torch.Tensor:
    """Frames per phoneme (num_phonemes) int64 (dtw.py:387-403); indices >= num_phonemes are not counted."""
    return torch.bincount(alignment, minlength=num_phonemes)[:num_phonemes]
