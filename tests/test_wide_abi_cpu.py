"""CPU: the batch-tiled (wide) Viterbi / forward-backward entry points of the C ABI
(include/hmm355.h, csrc/wide.hip) validate their arguments with the documented status codes
before anything is launched or dereferenced, report their workspace sizes, and leave the
contract of the narrow entry points (N <= 256) as it was.  No compute calls here."""
import ctypes
import os
import re

import pytest

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


def vit(L, obs=FAKE, mode=1, B=1, T=10, N=300, ws=BIG):
    return L.hmm355_viterbi_wide_f32(obs, mode, FAKE, FAKE, B, T, N, FAKE, FAKE, FAKE, FAKE, ws, None)


def fb(L, obs=FAKE, mode=0, B=1, T=10, N=300, ws=BIG):
    return L.hmm355_forward_backward_wide_f32(obs, mode, FAKE, FAKE, B, T, N, 1, FAKE, None, None, None, None,
                                              FAKE, ws, None)


def test_version_is_bumped(L):
    assert L.hmm355_version() >= 2


@pytest.mark.parametrize("call", [vit, fb])
def test_state_range(L, d, call):
    assert call(L, N=0) == d["HMM355_E_STATES"]
    assert call(L, N=4097) == d["HMM355_E_STATES"]


@pytest.mark.parametrize("call", [vit, fb])
def test_shape_null_workspace_and_empty_batch(L, d, call):
    assert call(L, T=0) == d["HMM355_E_SHAPE"]
    assert call(L, obs=None) == d["HMM355_E_ARG"]
    assert call(L, mode=7) == d["HMM355_E_ARG"]
    assert call(L, B=2, N=300, ws=16) == d["HMM355_E_WORKSPACE"]
    assert call(L, B=0) == 0


def test_null_everything_with_empty_batch(L):
    assert L.hmm355_viterbi_wide_f32(None, 0, None, None, 0, 10, 300, None, None, None, None, 0, None) == 0
    assert L.hmm355_forward_backward_wide_f32(None, 0, None, None, 0, 10, 300, 7, None, None, None, None, None,
                                              None, 0, None) == 0


def test_output_pointer_required_by_mask(L, d):
    rc = L.hmm355_forward_backward_wide_f32(FAKE, 0, FAKE, FAKE, 1, 10, 300, 2, FAKE, None, None, None, None,
                                            FAKE, BIG, None)
    assert rc == d["HMM355_E_ARG"]


def test_workspace_sizes(L):
    B, T, N = 2, 10, 300
    for mode in (0, 1):
        assert L.hmm355_viterbi_wide_workspace_bytes(B, T, N, mode) >= B * T * N * 2   # the uint16 psi table
    # OBS_PROB decodes add the log-emission buffer
    assert (L.hmm355_viterbi_wide_workspace_bytes(B, T, N, 0) - L.hmm355_viterbi_wide_workspace_bytes(B, T, N, 1)
            >= B * T * N * 4)
    assert L.hmm355_viterbi_wide_workspace_bytes(B, T, N, 2) == 0
    # A and its transpose, the raw alpha / beta rows
    assert L.hmm355_fb_wide_workspace_bytes(B, T, N) >= 2 * N * N * 4 + 2 * B * T * N * 4
    assert L.hmm355_viterbi_wide_workspace_bytes(B, T, 4097, 1) == 0
    assert L.hmm355_fb_wide_workspace_bytes(B, T, 4097) == 0
    assert L.hmm355_viterbi_wide_workspace_bytes(B, T, 0, 1) == 0 and L.hmm355_fb_wide_workspace_bytes(B, T, 0) == 0
    assert L.hmm355_viterbi_wide_workspace_bytes(B, T, 4096, 1) > 0 and L.hmm355_fb_wide_workspace_bytes(B, T, 4096) > 0
    # sizes at or below 256 states are accepted (the two forms are compared there)
    assert L.hmm355_viterbi_wide_workspace_bytes(B, T, 5, 1) > 0 and L.hmm355_fb_wide_workspace_bytes(B, T, 5) > 0


def test_narrow_entry_points_keep_their_limit(L, d):
    rc = L.hmm355_viterbi_f32(FAKE, 0, FAKE, FAKE, 1, 10, 300, FAKE, FAKE, FAKE, FAKE, 1 << 30, None)
    assert rc == d["HMM355_E_STATES"]
    rc = L.hmm355_forward_backward_f32(FAKE, 0, FAKE, FAKE, 1, 10, 300, 1, FAKE, None, None, None, None, FAKE,
                                       1 << 30, None)
    assert rc == d["HMM355_E_STATES"]
    assert L.hmm355_plan_bytes(300) == 0
    assert L.hmm355_fb_workspace_bytes(2, 10, 300) == 0 and L.hmm355_viterbi_workspace_bytes(2, 10, 300) == 0
    assert "4096" in L.hmm355_strerror(d["HMM355_E_STATES"]).decode()


def test_make_plan_above_256_is_none_without_a_device():
    """ops.make_plan returns None above 256 states with no native call and no host read, so the
    plan caches of HMMPyTorch / MixtureGaussianHMMLayer hold None there."""
    import torch
    from pytorch_hmm_amd import ops
    assert ops.make_plan(torch.zeros(300, 300)) is None
    assert ops.make_plan(torch.zeros(257, 257), read_banded=False, dense=True) is None


def test_gradients_above_256_are_refused_by_name():
    import torch
    from pytorch_hmm_amd.autograd import SequenceLogLik, forward_backward_with_grad
    obs = torch.rand(1, 4, 300, requires_grad=True)
    lP, l0 = torch.zeros(300, 300), torch.zeros(300)
    with pytest.raises(NotImplementedError, match="256"):
        forward_backward_with_grad(obs, lP, l0, 0, 1)
    with pytest.raises(NotImplementedError, match="256"):
        SequenceLogLik.apply(obs, lP, l0, 0, "ref")
