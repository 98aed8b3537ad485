"""CPU: N-best Viterbi (include/hmm355.h hmm355_viterbi_nbest_f32, csrc/nbest.hip,
pytorch_hmm_amd/ops.py viterbi_nbest) as far as it can be checked without a device.

  * tests/nbest_numpy.py (the GPU tests' model) against the enumeration of all N^T paths: the
    scores are the K largest left-folded path scores bit for bit, the paths behind finite scores
    are distinct and refold to their scores, rank 0 is the first-index Viterbi path.
  * The two entry points are declared, exported and reject bad arguments with the documented
    status codes before anything is launched or dereferenced (fake pointers).
  * hmm355::viterbi_nbest has a shape-only fake and checks its arguments on the host.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nbest_numpy as nm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")
NEG = -np.inf


def make_case(rng, N, T, kind):
    """kind 0: real-valued; 1: with -inf transitions and emissions; 2: small integers (exact ties);
    3: integers with -inf entries."""
    if kind in (0, 1):
        lo = np.log(rng.random((T, N)) + 1e-3).astype(np.float32)
        lP = np.log(rng.random((N, N)) + 1e-3).astype(np.float32)
        init = np.log(rng.random(N) + 1e-3).astype(np.float32)
    else:
        lo = -rng.integers(0, 3, (T, N)).astype(np.float32)
        lP = -rng.integers(0, 3, (N, N)).astype(np.float32)
        init = -rng.integers(0, 2, N).astype(np.float32)
    if kind in (1, 3):
        lo[rng.random((T, N)) < 0.25] = NEG
        lP[rng.random((N, N)) < 0.3] = NEG
        init[rng.random(N) < 0.3] = NEG
    return lo, lP, init


CASES = [(N, T, kind) for N in (2, 3, 4) for T in range(1, 7) for kind in range(4)]


# ------------------------------------------------------------------------ the test model
@pytest.mark.parametrize("N,T,kind", CASES)
def test_model_against_enumeration(N, T, kind):
    rng = np.random.default_rng(1000 * N + 10 * T + kind)
    lo, lP, init = make_case(rng, N, T, kind)
    enum = nm.enumerate_scores(lo, lP, init)
    finite = int((enum > NEG).sum())
    vs, vscore = nm.viterbi_first_index(lo, lP, init)
    for K in range(1, 9):
        paths, scores, count = nm.nbest_one(lo, lP, init, K)
        assert np.array_equal(scores, nm.top_scores(lo, lP, init, K)), (K, scores)
        assert count == min(K, finite)                       # also N^T < K
        assert np.all(scores[:-1] >= scores[1:])
        seen = set()
        for k in range(K):
            if k < max(count, 1):
                assert paths[k].min() >= 0 and paths[k].max() < N
                refolded = nm.fold(paths[k], lo, lP, init)
                assert refolded == scores[k] or (k == 0 and count == 0 and refolded == NEG)
                if k < count:
                    assert tuple(paths[k]) not in seen
                    seen.add(tuple(paths[k]))
            else:
                assert np.all(paths[k] == -1) and scores[k] == NEG
        # rank 0 is the plain first-index Viterbi, ties and -inf columns included
        assert np.array_equal(paths[0], vs) and scores[0] == vscore


def test_model_lengths_and_padding():
    rng = np.random.default_rng(5)
    lo, lP, init = make_case(rng, 3, 6, 0)
    lo_b = np.stack([lo, lo, lo])
    lo_b[1, 1:] = np.nan
    lo_b[2, 3:] = np.nan
    paths, scores, count = nm.nbest(lo_b, lP, init, 4, [6, 1, 3])
    assert paths.shape == (3, 4, 6) and scores.shape == (3, 4) and count.dtype == np.int32
    for b, L in enumerate((6, 1, 3)):
        p1, s1, c1 = nm.nbest_one(lo[:L], lP, init, 4)
        assert np.array_equal(paths[b, :, :L], p1) and np.array_equal(scores[b], s1) and count[b] == c1
        assert np.all(paths[b, :, L:] == -1)
    assert count[1] == 3 and np.all(paths[1, 3] == -1)       # N^1 = 3 < K = 4


# ------------------------------------------------------------------------------- C ABI
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
BIG = 1 << 50


def call(L, obs=FAKE, mode=1, lP=FAKE, init=FAKE, lengths=FAKE, B=2, T=10, N=70, K=3, paths=FAKE, scores=FAKE,
         count=FAKE, wsp=FAKE, ws=BIG):
    return L.hmm355_viterbi_nbest_f32(obs, mode, lP, init, lengths, B, T, N, K, paths, scores, count, wsp, ws, None)


def test_declared_exported_and_version_bumped(L):
    from pytorch_hmm_amd import _native as nat
    from pytorch_hmm_amd import build_native
    header = open(HEADER).read()
    for name in ("hmm355_viterbi_nbest_workspace_bytes", "hmm355_viterbi_nbest_f32"):
        assert name in nat.EXPORTS and re.search(rf"\b{name}\(", header)
        assert getattr(L, name).argtypes
    assert L.hmm355_version() >= 13
    assert "nbest.hip" in build_native.SOURCES


def test_status_codes(L, d):
    from pytorch_hmm_amd import _native as nat
    for mode in (nat.OBS_PROB, nat.OBS_LOG):
        assert call(L, mode=mode, B=0) == 0
    assert call(L, N=0) == d["HMM355_E_STATES"]
    assert call(L, N=257) == d["HMM355_E_STATES"]
    assert call(L, K=17) == d["HMM355_E_STATES"]
    assert call(L, T=0) == d["HMM355_E_SHAPE"]
    assert call(L, K=0) == d["HMM355_E_SHAPE"]
    assert call(L, K=-1) == d["HMM355_E_SHAPE"]
    assert call(L, B=1 << 30, T=1 << 30) == d["HMM355_E_SHAPE"]
    assert call(L, mode=7) == d["HMM355_E_ARG"]
    assert call(L, B=-1) == d["HMM355_E_ARG"]
    for name in ("obs", "lP", "init", "paths", "scores", "wsp"):
        assert call(L, **{name: None}) == d["HMM355_E_ARG"], name
    assert call(L, B=0, obs=None, lP=None, init=None, paths=None, scores=None, wsp=None, ws=0) == 0
    # lengths and count are optional: with them NULL the next check (the workspace) is reached
    assert call(L, lengths=None, count=None, ws=0) == d["HMM355_E_WORKSPACE"]


def test_workspace_size(L, d):
    from pytorch_hmm_amd import _native as nat
    q = L.hmm355_viterbi_nbest_workspace_bytes
    for N, NP in ((1, 64), (64, 64), (65, 128), (128, 128), (129, 256), (256, 256)):
        for K in (1, 5, 16):
            need = q(3, 11, N, K, nat.OBS_LOG)
            assert 3 * 11 * K * NP * 2 <= need < 3 * 11 * K * NP * 2 + 256   # the pointer table: linear
            assert call(L, B=3, T=11, N=N, K=K, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    for bad in ((2, 10, 0, 3, 1), (2, 10, 257, 3, 1), (2, 10, 70, 17, 1), (2, 10, 70, 0, 1), (2, 0, 70, 3, 1),
                (2, 10, 70, 3, 9), (1 << 30, 1 << 30, 70, 3, 1), (-1, 10, 70, 3, 1)):
        assert q(*bad) == 0, bad


# -------------------------------------------------------------------------------- ops
def test_fake_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    B, T, N, K = 3, 9, 70, 5
    from pytorch_hmm_amd import ops  # noqa: F401  (registers the op)
    with FakeTensorMode():
        lP, init = torch.empty(N, N), torch.empty(N)
        # the real op converts fp64 / fp16 inputs and always allocates float32 scores
        for dtype in (torch.float32, torch.float64, torch.float16):
            for lens in (None, torch.empty(B, dtype=torch.int64)):
                obs = torch.empty(B, T, N, dtype=dtype)
                paths, scores, count = torch.ops.hmm355.viterbi_nbest(obs, lP, init, 1, K, lens)
                assert paths.shape == (B, K, T) and paths.dtype == torch.int64
                assert scores.shape == (B, K) and scores.dtype == torch.float32
                assert count.shape == (B,) and count.dtype == torch.int32


def test_schema():
    from pytorch_hmm_amd import ops  # noqa: F401  (registers the op)
    assert str(torch.ops.hmm355.viterbi_nbest.default._schema) == (
        "hmm355::viterbi_nbest(Tensor obs, Tensor log_P, Tensor init, SymInt obs_mode, SymInt num_paths, "
        "Tensor? lengths=None) -> (Tensor, Tensor, Tensor)")


def test_outputs_spec_is_shared():
    from pytorch_hmm_amd import ops
    paths, scores, count = ops._viterbi_nbest_outputs(torch.empty, 2, 7, 4)
    assert paths.shape == (2, 4, 7) and scores.shape == (2, 4) and count.shape == (2,)
    assert "viterbi_nbest" in ops.__doc__


def test_host_value_errors():
    from pytorch_hmm_amd import ops
    obs, lP, l0 = torch.zeros(2, 5, 7), torch.zeros(7, 7), torch.zeros(7)
    for K in (0, 17, -3):
        with pytest.raises(ValueError, match="num_paths"):
            ops.viterbi_nbest(obs, lP, l0, ops.OBS_LOG, K)
    with pytest.raises(ValueError, match="256"):
        ops.viterbi_nbest(torch.zeros(2, 5, 257), torch.zeros(257, 257), torch.zeros(257), ops.OBS_LOG, 2)
    with pytest.raises(ValueError, match=r"\[1, 6\]"):
        ops.viterbi_nbest(obs, lP, l0, ops.OBS_LOG, 2, [1, 6])
    with pytest.raises(ValueError, match=r"\(B, T, N\)"):
        ops.viterbi_nbest(torch.zeros(5, 7), lP, l0, ops.OBS_LOG, 2)


def test_cpu_tensors_are_refused_by_name():
    import pytorch_hmm_amd as ph
    from pytorch_hmm_amd import ops
    obs, lP, l0 = torch.zeros(2, 5, 7), torch.zeros(7, 7), torch.zeros(7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.viterbi_nbest(obs, lP, l0, ops.OBS_LOG, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ph.HMMPyTorch(np.full((7, 7), 1 / 7, np.float32)).viterbi_nbest(obs, 2)
    for layer in (ph.HMMLayer(7), ph.GaussianHMMLayer(7, 4), ph.MixtureGaussianHMMLayer(7, 4)):
        assert callable(layer.nbest_alignment)
