"""CPU: posterior path sampling (include/hmm355.h hmm355_ffbs_f32, csrc/ffbs.hip,
pytorch_hmm_amd/ops.py ffbs / posterior_sample) as far as it can be checked without a device.

  * The two entry points are declared, exported and reject bad arguments with the documented
    status codes before anything is launched or dereferenced (fake pointers).
  * hmm355::ffbs has a shape-only fake; posterior_sample checks its arguments on the host.
  * tests/ffbs_numpy.py (the GPU tests' model): the product of its backward-sampling conditionals
    is the enumerated path posterior.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ffbs_numpy as fm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")


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


def ffbs(L, fwd=FAKE, ld=128, lengths=FAKE, uni=FAKE, B=2, T=10, N=70, K=3, states=FAKE, wsp=FAKE, ws=BIG):
    return L.hmm355_ffbs_f32(fwd, ld, FAKE, lengths, uni, B, T, N, K, states, wsp, ws, None)


# ------------------------------------------------------------------------------- C ABI
def test_declared_exported_and_version_bumped(L):
    from pytorch_hmm_amd import _native as nat
    header = open(HEADER).read()
    for name in ("hmm355_ffbs_workspace_bytes", "hmm355_ffbs_f32"):
        assert name in nat.EXPORTS and re.search(rf"\b{name}\(", header)
        assert getattr(L, name).argtypes
    assert L.hmm355_version() >= 11


def test_status_codes(L, d):
    assert ffbs(L, N=0) == d["HMM355_E_STATES"]
    assert ffbs(L, N=257, ld=300) == d["HMM355_E_STATES"]
    assert ffbs(L, T=0) == d["HMM355_E_SHAPE"]
    assert ffbs(L, K=0) == d["HMM355_E_SHAPE"]
    assert ffbs(L, B=1 << 30, T=1 << 30) == d["HMM355_E_SHAPE"]
    assert ffbs(L, B=1 << 20, T=1 << 20, K=1 << 30) == d["HMM355_E_SHAPE"]
    assert ffbs(L, ld=69) == d["HMM355_E_ARG"]
    assert ffbs(L, fwd=None) == d["HMM355_E_ARG"]
    assert ffbs(L, uni=None) == d["HMM355_E_ARG"]
    assert ffbs(L, states=None) == d["HMM355_E_ARG"]
    assert ffbs(L, wsp=None) == d["HMM355_E_ARG"]
    assert L.hmm355_ffbs_f32(FAKE, 128, None, FAKE, FAKE, 2, 10, 70, 3, FAKE, FAKE, BIG, None) == d["HMM355_E_ARG"]
    assert ffbs(L, B=-1) == d["HMM355_E_ARG"]
    assert ffbs(L, B=0) == 0
    assert ffbs(L, B=0, fwd=None, uni=None, states=None, wsp=None, ws=0) == 0


def test_workspace_size(L, d):
    for N, NP in ((1, 64), (5, 64), (64, 64), (65, 128), (128, 128), (129, 256), (256, 256)):
        need = L.hmm355_ffbs_workspace_bytes(N)
        assert need >= NP * NP * 4
        assert ffbs(L, N=N, ld=256, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    assert L.hmm355_ffbs_workspace_bytes(257) == 0
    assert L.hmm355_ffbs_workspace_bytes(0) == 0


# -------------------------------------------------------------------------------- ops
def test_fake_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    B, T, N, K = 3, 9, 70, 5
    with FakeTensorMode():
        fwd, lP, u = torch.empty(B, T, N), torch.empty(N, N), torch.empty(B, K, T)
        states = torch.ops.hmm355.ffbs(fwd, lP, u)
        assert states.shape == (B, K, T) and states.dtype == torch.int64
        states = torch.ops.hmm355.ffbs(torch.empty(B, T, 128)[..., :N], lP, u, torch.empty(B, dtype=torch.int32))
        assert states.shape == (B, K, T) and states.dtype == torch.int64


def test_row_stride_of_views():
    from pytorch_hmm_amd import ops
    buf = torch.zeros(3, 7, 128)
    assert ops._row_stride(buf[..., :70]) == 128
    assert ops._row_stride(torch.zeros(3, 7, 70)) == 70
    assert ops._row_stride(buf[:, :, ::2]) is None          # last dimension not contiguous
    assert ops._row_stride(buf[:, :5, :70]) is None         # rows of a sequence not T * ld apart
    assert ops._row_stride(buf[:1, :5, :70]) == 128
    assert ops._row_stride(torch.zeros(3, 1, 128)[..., :70]) == 128
    assert ops._row_stride(torch.zeros(3, 7, 1).expand(3, 7, 4)) is None


def test_posterior_sample_value_errors():
    import pytorch_hmm_amd
    from pytorch_hmm_amd import ops
    assert pytorch_hmm_amd.posterior_sample is ops.posterior_sample and "posterior_sample" in pytorch_hmm_amd.__all__
    obs, lP, l0 = torch.zeros(2, 5, 7), torch.zeros(7, 7), torch.zeros(7)
    with pytest.raises(ValueError, match="num_samples"):
        ops.posterior_sample(obs, lP, l0, ops.OBS_PROB, 0)
    with pytest.raises(ValueError, match=r"\(2, 3, 5\)"):
        ops.posterior_sample(obs, lP, l0, ops.OBS_PROB, 3, uniforms=torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match=r"\(2, 3, 5\)"):
        ops.posterior_sample(obs, lP, l0, ops.OBS_PROB, 3, uniforms=torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match="256"):
        ops.posterior_sample(torch.zeros(2, 5, 257), torch.zeros(257, 257), torch.zeros(257), ops.OBS_LOG, 1)
    with pytest.raises(ValueError, match=r"\[1, 6\]"):
        ops.posterior_sample(obs, lP, l0, ops.OBS_PROB, 1, lengths=[1, 6])
    with pytest.raises(ValueError, match="256"):
        ops.ffbs(torch.zeros(2, 5, 257), torch.zeros(257, 257), torch.zeros(2, 1, 5))
    with pytest.raises(ValueError, match="uniforms"):
        ops.ffbs(torch.zeros(2, 5, 7), lP, torch.zeros(2, 1, 4))


def test_cpu_tensors_are_refused_by_name():
    from pytorch_hmm_amd import ops
    obs, lP, l0 = torch.zeros(2, 5, 7), torch.zeros(7, 7), torch.zeros(7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.posterior_sample(obs, lP, l0, ops.OBS_PROB, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ffbs(obs, lP, torch.zeros(2, 3, 5))
    import pytorch_hmm_amd as ph
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ph.HMMPyTorch(np.full((7, 7), 1 / 7, np.float32)).sample_posterior(obs, 2)


# ------------------------------------------------------------------------ the test model
def test_model_conditionals_are_the_path_posterior():
    rng = np.random.default_rng(0)
    N, T = 3, 4
    A = rng.random((N, N))
    A /= A.sum(1, keepdims=True)
    p0 = rng.random(N)
    p0 /= p0.sum()
    e = rng.random((T, N))
    alpha, loglik = fm.forward_filter(e[None], A, p0)
    paths, post = fm.enumerate_paths(e, A, p0)
    assert paths.shape == (81, T) and abs(post.sum() - 1) < 1e-12
    for path, p in zip(paths, post):
        assert abs(fm.conditionals(alpha[0], A, path) - p) < 1e-12
    # any positive scale of the rows gives the same conditionals
    assert abs(fm.conditionals(alpha[0] * 7.5, A, paths[40]) - post[40]) < 1e-12
    gamma, xi = fm.marginals(paths, post, N)
    assert np.allclose(gamma.sum(1), 1) and np.allclose(xi.sum((1, 2)), 1)
    assert np.allclose(xi.sum(2), gamma[:-1]) and np.allclose(xi.sum(1), gamma[1:])


def test_model_intervals_accept_an_exact_sampler_and_reject_a_wrong_state():
    rng = np.random.default_rng(1)
    B, K, T, N = 2, 4, 9, 6
    A = rng.random((N, N)) ** 4
    A /= A.sum(1, keepdims=True)
    e = rng.random((B, T, N))
    alpha, _ = fm.forward_filter(e, A, np.full(N, 1 / N))
    fwd32 = alpha.astype(np.float32)
    lP32 = np.log(A).astype(np.float32)
    A32 = np.exp(lP32.astype(np.float64))
    u = rng.random((B, K, T))
    lens = [T, 5]
    states = np.full((B, K, T), -1, np.int64)
    for b in range(B):
        for k in range(K):
            for t in range(lens[b] - 1, -1, -1):
                w = fwd32[b, t].astype(np.float64)
                if t < lens[b] - 1:
                    w = w * A32[:, states[b, k, t + 1]]
                states[b, k, t] = int(np.searchsorted(np.cumsum(w), u[b, k, t] * w.sum(), side="right"))
    ok, msg = fm.intervals_ok(states, u, fwd32, lP32, lens)
    assert ok, msg
    wrong = states.copy()
    wrong[0, 0, 3] = (wrong[0, 0, 3] + 3) % N
    assert not fm.intervals_ok(wrong, u, fwd32, lP32, lens)[0]
    unpadded = states.copy()
    unpadded[1, 0, 7] = 0
    assert not fm.intervals_ok(unpadded, u, fwd32, lP32, lens)[0]
