"""CPU: the dynamic-time-warping feature without a device.

  * The numpy restatements in tests/dtw_numpy.py (the GPU tests' oracle on shapes without a
    fixture) reproduce every fixture the reference wrote (tests/golden/dtw_*.npz,
    make_golden_dtw.py): cost-matrix bits and paths for the three step patterns, including real
    ties, a +inf band and an unreachable end cell; the closed-form soft-DTW gradient recursion in
    fp64 equals the reference's autograd gradient to 1e-10.
  * The C ABI (include/hmm355.h, csrc/dtw.hip) declares and exports the DTW entry points, reports
    version >= 3 and rejects bad arguments with the documented codes before any launch.
  * pytorch_hmm_amd.alignment imports without a GPU and refuses CPU tensors by name.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_numpy as dn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("pattern", dn.PATTERNS)
@pytest.mark.parametrize("name", dn.FIXTURES)
def test_restatement_reproduces_fixture(gold, name, pattern):
    g = gold("dtw_" + name)
    C, pi, pj = dn.hard_dtw(g["dist"], pattern)
    assert np.array_equal(bits(C), bits(g["cost_" + pattern]))
    assert np.array_equal(pi, g["path_i_" + pattern]) and np.array_equal(pj, g["path_j_" + pattern])
    assert dn.path_is_valid(pi, pj, *g["dist"].shape)
    # (rabiner_juang walks back by raw cost, which is not its forward pass's own argmin: dtw.py:127-143)
    if pattern != "rabiner_juang" and np.isfinite(g["total_" + pattern]):
        assert abs(dn.path_cost(g["dist"], pi, pj, pattern) - float(g["total_" + pattern])) <= 1e-4


def test_fixtures_hold_what_they_are_for(gold):
    t = gold("dtw_ties")
    assert np.array_equal(t["dist"], np.round(t["dist"]))
    # real ties: some interior cell has two equal smallest predecessors
    C = t["cost_symmetric"]
    three = np.stack([C[:-1, :-1], C[:-1, 1:], C[1:, :-1]])
    s = np.sort(three, axis=0)
    assert (s[0] == s[1]).any()
    b = gold("dtw_band")["dist"]
    ii, jj = np.indices(b.shape)
    assert np.isinf(b[np.abs(ii - jj) > 5]).all() and np.isfinite(b[np.abs(ii - jj) <= 5]).all()
    assert np.isfinite(gold("dtw_band")["total_symmetric"])
    for p in dn.PATTERNS:
        assert np.isposinf(gold("dtw_noend")["total_" + p])


@pytest.mark.parametrize("tag,gamma", dn.GAMMAS)
@pytest.mark.parametrize("name", dn.SOFT_FIXTURES)
def test_closed_form_gradient_equals_reference_autograd(gold, name, tag, gamma):
    g = gold("dtw_" + name)
    R = dn.soft_forward(g["dist"], gamma)
    n, m = g["dist"].shape
    assert abs(R[n, m] - float(g["soft_total64_" + tag])) <= 1e-10 * max(1.0, abs(R[n, m]))
    E = dn.soft_grad(g["dist"], R, gamma)
    assert np.abs(E - g["soft_grad64_" + tag]).max() <= 1e-10
    assert E.min() >= 0.0 and E.max() <= 1.0 + 1e-10


# ---------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def L():
    from pytorch_hmm_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from pytorch_hmm_amd import build_native
        build_native.build()
    return nat.lib()


@pytest.fixture(scope="module")
def d():
    return dict((m.group(1), int(m.group(2).rstrip("u"), 0))
                for m in re.finditer(r"#define\s+(HMM355_[A-Z0-9_]+)\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+)u?)\)?",
                                     open(HEADER).read()))


FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
BIG = 1 << 40
DTW_SYMBOLS = ("hmm355_dtw_workspace_bytes", "hmm355_dtw_f32", "hmm355_softdtw_f32", "hmm355_softdtw_grad_f32")


def hard(L, dist=FAKE, B=1, N=10, M=12, pattern=0, flags=1, ws=BIG, paths=FAKE):
    return L.hmm355_dtw_f32(dist, None, None, B, N, M, pattern, flags, FAKE, FAKE, paths, paths, paths, FAKE, ws, None)


def soft(L, dist=FAKE, B=1, N=10, M=12, gamma=0.1):
    return L.hmm355_softdtw_f32(dist, None, None, B, N, M, gamma, FAKE, FAKE, None)


def grad(L, dist=FAKE, B=1, N=10, M=12, gamma=0.1):
    return L.hmm355_softdtw_grad_f32(dist, FAKE, None, None, B, N, M, gamma, FAKE, None)


def test_header_exports_and_version(L, d):
    from pytorch_hmm_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hmm355_[a-z0-9_]+)\s*\(", src))
    for name in DTW_SYMBOLS:
        assert name in declared and name in nat.EXPORTS and hasattr(L, name)
    assert declared == set(nat.EXPORTS)
    assert L.hmm355_version() >= 3
    assert (d["HMM355_DTW_SYMMETRIC"], d["HMM355_DTW_ASYMMETRIC"], d["HMM355_DTW_RABINER_JUANG"]) == \
        (nat.DTW_SYMMETRIC, nat.DTW_ASYMMETRIC, nat.DTW_RABINER_JUANG)
    assert d["HMM355_DTW_PATH"] == nat.DTW_PATH


def test_hard_dtw_argument_checks(L, d):
    assert hard(L, pattern=3) == d["HMM355_E_ARG"] and hard(L, pattern=-1) == d["HMM355_E_ARG"]
    assert hard(L, flags=2) == d["HMM355_E_ARG"]
    assert hard(L, N=0) == d["HMM355_E_SHAPE"] and hard(L, M=0) == d["HMM355_E_SHAPE"]
    assert hard(L, B=-1) == d["HMM355_E_ARG"]
    assert hard(L, dist=None) == d["HMM355_E_ARG"]
    assert hard(L, paths=None) == d["HMM355_E_ARG"]          # HMM355_DTW_PATH needs the path outputs
    assert hard(L, B=2, ws=16) == d["HMM355_E_WORKSPACE"]
    need = L.hmm355_dtw_workspace_bytes(2, 10, 12, 1)
    assert hard(L, B=2, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    assert hard(L, N=1 << 30, M=1 << 30) == d["HMM355_E_SHAPE"]   # sizes are checked in size_t
    assert hard(L, B=0) == 0
    assert L.hmm355_dtw_f32(None, None, None, 0, 10, 12, 0, 0, None, None, None, None, None, None, 0, None) == 0


@pytest.mark.parametrize("call", [soft, grad])
def test_soft_dtw_argument_checks(L, d, call):
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert call(L, gamma=g) == d["HMM355_E_ARG"]
    assert call(L, N=0) == d["HMM355_E_SHAPE"] and call(L, M=0) == d["HMM355_E_SHAPE"]
    assert call(L, dist=None) == d["HMM355_E_ARG"]
    assert call(L, B=0) == 0


def test_workspace_sizes(L):
    B, N, M = 3, 100, 70
    q = (M + 3) // 4
    value_only = L.hmm355_dtw_workspace_bytes(B, N, M, 0)
    with_path = L.hmm355_dtw_workspace_bytes(B, N, M, 1)
    assert 0 < value_only < B * N * M            # no N x M table without the path
    assert with_path >= value_only + B * N * q + 2 * B * (N + M - 1) * 4
    assert L.hmm355_dtw_workspace_bytes(B, 0, M, 1) == 0 and L.hmm355_dtw_workspace_bytes(B, N, 0, 1) == 0
    assert L.hmm355_dtw_workspace_bytes(-1, N, M, 1) == 0
    assert L.hmm355_dtw_workspace_bytes(B, N, M, 2) == 0
    assert L.hmm355_dtw_workspace_bytes(B, 1 << 30, 1 << 30, 1) == 0


# ------------------------------------------------------------------------------- Python
def test_alignment_imports_without_a_gpu():
    import pytorch_hmm_amd
    import pytorch_hmm_amd.alignment as al
    for name in ("compute_distance_matrix", "compute_dtw_path", "dtw_distance", "dtw_alignment", "DTWAligner",
                 "ConstrainedDTWAligner", "phoneme_audio_alignment", "extract_phoneme_durations"):
        assert hasattr(al, name)
    assert pytorch_hmm_amd.DTWAligner is al.DTWAligner
    assert pytorch_hmm_amd.ConstrainedDTWAligner is al.ConstrainedDTWAligner
    assert "CTC" in al.__doc__
    for op in ("dtw", "soft_dtw"):
        assert hasattr(torch.ops.hmm355, op)


def test_cpu_tensors_are_refused_by_name():
    import pytorch_hmm_amd.alignment as al
    from pytorch_hmm_amd import ops
    from pytorch_hmm_amd.autograd import SoftDTW
    x, y = torch.rand(5, 3), torch.rand(7, 3)
    dist = torch.rand(1, 5, 7)
    for call in (lambda: al.compute_dtw_path(dist[0]), lambda: al.dtw_distance(x, y), lambda: al.dtw_alignment(x, y),
                 lambda: al.DTWAligner()(x, y), lambda: al.DTWAligner(soft_dtw=True)(x, y),
                 lambda: al.ConstrainedDTWAligner()(x, y), lambda: al.phoneme_audio_alignment(x, y),
                 lambda: ops.dtw(dist, ops.DTW_SYMMETRIC), lambda: ops.soft_dtw(dist, 0.1),
                 lambda: SoftDTW.apply(dist, 0.1, None, None)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()
    with pytest.raises(ValueError):
        ops.dtw_pattern("diagonal")


def test_distance_matrix_formulae_and_chunking(gold, monkeypatch):
    """compute_distance_matrix is plain torch: on the fixture host's formulae it reproduces the
    reference (same ops), whole or in row chunks."""
    import pytorch_hmm_amd.alignment.dtw as ad
    g = gold("dtw_13x9")
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    D = x.shape[1]
    for fn in ("euclidean", "cosine", "manhattan"):
        whole = ad.compute_distance_matrix(x, y, fn)
        ref = g["dist_" + fn]
        tol = D * 2.0 ** -23
        assert np.all(np.abs(whole.numpy() - ref) <= tol * np.abs(ref) + (tol if fn == "cosine" else 0.0))
        monkeypatch.setattr(ad, "_CHUNK_ELEMS", 5 * 9 * D)   # 5 rows at a time
        assert torch.equal(ad.compute_distance_matrix(x, y, fn), whole)
        monkeypatch.undo()
    with pytest.raises(ValueError):
        ad.compute_distance_matrix(x, y, "chebyshev")
    assert ad.compute_distance_matrix(x[None], y[None], "euclidean").shape == (1, 13, 9)


def test_extract_phoneme_durations(gold):
    import pytorch_hmm_amd.alignment as al
    g = gold("dtw_phoneme")
    got = al.extract_phoneme_durations(torch.from_numpy(g["alignment"]), len(g["durations"]))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), g["durations"])
    assert np.array_equal(al.extract_phoneme_durations(torch.from_numpy(g["alignment"]), 3).numpy(), g["durations"][:3])
