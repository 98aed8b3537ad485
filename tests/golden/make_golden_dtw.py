"""Writes tests/golden/dtw_*.npz from the reference's pytorch_hmm.alignment.dtw (torch-CPU).

    python tests/golden/make_golden_dtw.py /path/to/reference

The fixtures hold data only: inputs x, y, dist; for the three step patterns the reference's cost
matrix, path and total (compute_dtw_path); for soft-DTW at gamma in {1, 0.1, 0.01} the total of
the reference's loop (DTWAligner._soft_dtw_align) in fp32 and fp64, d total / d dist of that loop
in fp64 and the reference's own fp32 gradient (grad_ref32); the three distance formulae; and the
outputs of phoneme_audio_alignment / extract_phoneme_durations on well-separated features.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATTERNS = ("symmetric", "asymmetric", "rabiner_juang")
GAMMAS = (("1", 1.0), ("0p1", 0.1), ("0p01", 0.01))


def soft(ref, dist, gamma, dtype):
    """total and d total / d dist of the reference's soft-DTW loop run in `dtype`."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    leaf = dist.to(dtype).clone().requires_grad_()
    keep = ref.compute_distance_matrix
    ref.compute_distance_matrix = lambda x, y, fn="euclidean": leaf
    try:
        _, _, total = ref.DTWAligner(soft_dtw=True, gamma=gamma)(leaf, leaf)
        total.backward()
    finally:
        ref.compute_distance_matrix = keep
        torch.set_default_dtype(old)
    return total.detach().numpy(), leaf.grad.numpy()


def soft_xy(ref, x, y, gamma, dtype):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        xl, yl = x.to(dtype).clone().requires_grad_(), y.to(dtype).clone().requires_grad_()
        _, _, total = ref.DTWAligner(soft_dtw=True, gamma=gamma)(xl, yl)
        total.backward()
    finally:
        torch.set_default_dtype(old)
    return total.detach().numpy(), xl.grad.numpy(), yl.grad.numpy()


def hard(ref, dist, out):
    for p in PATTERNS:
        pi, pj, cost = ref.compute_dtw_path(dist, p)
        out["cost_" + p] = cost.numpy()
        out["path_i_" + p] = pi.numpy().astype(np.int64)
        out["path_j_" + p] = pj.numpy().astype(np.int64)
        out["total_" + p] = cost[-1, -1].numpy()


def main():
    sys.path.insert(0, sys.argv[1])
    import pytorch_hmm.alignment.dtw as ref
    rng = np.random.default_rng(20)
    D = 4
    cases = {}
    for N, M in ((1, 1), (1, 7), (7, 1), (13, 9), (40, 40)):
        x = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32))
        y = torch.from_numpy(rng.standard_normal((M, D)).astype(np.float32))
        cases[f"{N}x{M}"] = (x, y, ref.compute_distance_matrix(x, y, "euclidean"), "euclidean", True)
    # integer-valued distances (manhattan over integer features): real ties
    x = torch.from_numpy(rng.integers(0, 4, (20, 1)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 4, (33, 1)).astype(np.float32))
    cases["ties"] = (x, y, ref.compute_distance_matrix(x, y, "manhattan"), "manhattan", True)
    # +inf outside |i - j| <= 5, and an all-inf last row (the end cell is unreachable)
    x = torch.from_numpy(rng.standard_normal((24, D)).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((24, D)).astype(np.float32))
    d = ref.compute_distance_matrix(x, y, "euclidean")
    ii, jj = np.indices((24, 24))
    band = d.clone()
    band[torch.from_numpy(np.abs(ii - jj) > 5)] = float("inf")
    cases["band"] = (x, y, band, "euclidean", False)
    noend = d.clone()
    noend[-1, :] = float("inf")
    cases["noend"] = (x, y, noend, "euclidean", False)

    for name, (x, y, dist, fn, finite) in cases.items():
        out = {"x": x.numpy(), "y": y.numpy(), "dist": dist.numpy(), "distance_fn": np.array(fn)}
        for f in ("euclidean", "cosine", "manhattan"):
            out["dist_" + f] = ref.compute_distance_matrix(x, y, f).numpy()
        hard(ref, dist, out)
        if finite:
            for tag, g in GAMMAS:
                t32, g32 = soft(ref, dist, g, torch.float32)
                t64, g64 = soft(ref, dist, g, torch.float64)
                out["soft_total32_" + tag], out["grad_ref32_" + tag] = t32, g32
                out["soft_total64_" + tag], out["soft_grad64_" + tag] = t64, g64
        np.savez(os.path.join(HERE, f"dtw_{name}.npz"), **out)

    # soft-DTW through the euclidean distance matrix: gradients on x and y
    x = torch.from_numpy(rng.standard_normal((9, D)).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((13, D)).astype(np.float32))
    out = {"x": x.numpy(), "y": y.numpy()}
    for tag, g in GAMMAS:
        t32, gx32, gy32 = soft_xy(ref, x, y, g, torch.float32)
        t64, gx64, gy64 = soft_xy(ref, x, y, g, torch.float64)
        out["total32_" + tag], out["xgrad_ref32_" + tag], out["ygrad_ref32_" + tag] = t32, gx32, gy32
        out["total64_" + tag], out["xgrad64_" + tag], out["ygrad64_" + tag] = t64, gx64, gy64
    np.savez(os.path.join(HERE, "dtw_xgrad.npz"), **out)

    # phoneme / audio alignment on well-separated features: each phoneme is its own direction,
    # every frame a noisy copy of its phoneme
    P, F, Df = 6, 40, 8
    ph = torch.eye(P, Df) * 3 + 0.05 * torch.from_numpy(rng.standard_normal((P, Df)).astype(np.float32))
    durs = np.array([5, 9, 3, 8, 7, 8])
    owner = np.repeat(np.arange(P), durs)
    au = ph[owner] + 0.05 * torch.from_numpy(rng.standard_normal((F, Df)).astype(np.float32))
    alignment, boundaries = ref.phoneme_audio_alignment(ph, au)
    np.savez(os.path.join(HERE, "dtw_phoneme.npz"), phoneme_features=ph.numpy(), audio_features=au.numpy(),
             alignment=alignment.numpy(), boundaries=boundaries.numpy(),
             durations=ref.extract_phoneme_durations(alignment, P).numpy())


if __name__ == "__main__":
    main()
