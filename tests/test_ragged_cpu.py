"""CPU: per-sequence lengths for forward-backward and Viterbi (include/hmm355.h "ragged",
csrc/ragged.hip, pytorch_hmm_amd/ops.py) as far as they can be checked without a device.

  * The three new entry points are declared, exported and reject bad arguments with the
    documented status codes before anything is launched or dereferenced (fake pointers).
  * ops.ragged_lengths validates lengths on the host; the new custom ops have shape-only fakes.
  * tests/ragged_model.py (the GPU tests' oracle) with full lengths is the oracle's batch result.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ragged_model as rm  # noqa: E402
from oracle import hmm_oracle as O  # noqa: E402

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


def vit(L, obs=FAKE, mode=1, lengths=FAKE, B=2, T=10, N=70, ws=BIG, wsp=FAKE, states=FAKE):
    return L.hmm355_viterbi_ragged_f32(obs, mode, FAKE, FAKE, lengths, B, T, N, states, FAKE, FAKE, wsp, ws, None)


def fb(L, obs=FAKE, mode=0, lengths=FAKE, B=2, T=10, N=70, ws=BIG, wsp=FAKE, mask=1, post=FAKE, lbt=None):
    return L.hmm355_forward_backward_ragged_f32(obs, mode, FAKE, FAKE, lbt, lengths, B, T, N, mask, post, None,
                                                None, None, None, wsp, ws, None)


# ------------------------------------------------------------------------------- C ABI
def test_declared_exported_and_version_bumped(L):
    from pytorch_hmm_amd import _native as nat
    header = open(HEADER).read()
    for name in ("hmm355_viterbi_ragged_workspace_bytes", "hmm355_viterbi_ragged_f32",
                 "hmm355_forward_backward_ragged_f32"):
        assert name in nat.EXPORTS and re.search(rf"\b{name}\(", header)
        assert getattr(L, name)
    assert L.hmm355_version() >= 10


@pytest.mark.parametrize("call", [vit, fb])
def test_status_codes(L, d, call):
    assert call(L, N=0) == d["HMM355_E_STATES"]
    assert call(L, N=257) == d["HMM355_E_STATES"]
    assert call(L, T=0) == d["HMM355_E_SHAPE"]
    assert call(L, obs=None) == d["HMM355_E_ARG"]
    assert call(L, lengths=None) == d["HMM355_E_ARG"]
    assert call(L, wsp=None) == d["HMM355_E_ARG"]
    assert call(L, mode=7) == d["HMM355_E_ARG"]
    assert call(L, B=-1) == d["HMM355_E_ARG"]
    assert call(L, ws=16) == d["HMM355_E_WORKSPACE"]
    assert call(L, B=0) == 0
    assert call(L, B=0, obs=None, lengths=None, wsp=None, ws=0) == 0


def test_viterbi_needs_its_outputs(L, d):
    assert vit(L, states=None) == d["HMM355_E_ARG"]


def test_fb_mask_needs_its_pointer(L, d):
    assert fb(L, mask=1, post=None) == d["HMM355_E_ARG"]
    assert fb(L, mask=2) == d["HMM355_E_ARG"]      # forward asked for, no forward pointer
    assert fb(L, mask=4) == d["HMM355_E_ARG"]
    assert fb(L, mask=0x100) == d["HMM355_E_ARG"]  # a hint bit of the tuned chains


def test_fb_workspace_is_the_tuned_layout(L, d):
    B, T, N = 3, 11, 70
    need = L.hmm355_fb_workspace_bytes(B, T, N)
    assert fb(L, B=B, T=T, N=N, ws=need - 1) == d["HMM355_E_WORKSPACE"]


def test_viterbi_workspace_size(L, d):
    for B, T, N, NP in ((3, 131, 5, 64), (3, 131, 64, 64), (2, 7, 70, 128), (1, 9, 200, 256), (4, 1, 256, 256)):
        for mode in (0, 1):
            need = L.hmm355_viterbi_ragged_workspace_bytes(B, T, N, mode)
            assert need >= B * T * NP
            assert vit(L, mode=mode, B=B, T=T, N=N, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    assert L.hmm355_viterbi_ragged_workspace_bytes(2, 10, 257, 1) == 0
    assert L.hmm355_viterbi_ragged_workspace_bytes(2, 10, 0, 1) == 0
    assert L.hmm355_viterbi_ragged_workspace_bytes(2, 0, 5, 1) == 0
    assert L.hmm355_viterbi_ragged_workspace_bytes(2, 10, 5, 2) == 0


# ------------------------------------------------------------------------ length helper
def test_lengths_accepted_forms():
    from pytorch_hmm_amd import ops
    want = [1, 5, 3]
    for given in (want, np.array(want), np.array(want, np.int32), torch.tensor(want, dtype=torch.int32),
                  torch.tensor(want, dtype=torch.int64), torch.tensor(want).view(3, 1)):
        host = ops.ragged_lengths(given, 3, 5, 70)
        assert host.dtype == torch.int64 and host.device.type == "cpu" and host.tolist() == want


@pytest.mark.parametrize("bad,word", [([1, 2], "one length per sequence"), ([1, 2, 3, 4], "one length per sequence"),
                                      ([0, 2, 3], r"\[0, 2, 3\]"), ([1, 6, 3], r"\[1, 6, 3\]"),
                                      ([-1, 2, 3], r"\[-1, 2, 3\]")])
def test_lengths_rejected_by_value(bad, word):
    from pytorch_hmm_amd import ops
    with pytest.raises(ValueError, match=word):
        ops.ragged_lengths(bad, 3, 5, 70)


def test_lengths_rejected_by_dtype_and_states():
    from pytorch_hmm_amd import ops
    with pytest.raises(ValueError, match="float32"):
        ops.ragged_lengths(torch.tensor([1.0, 2.0, 3.0]), 3, 5, 70)
    with pytest.raises(ValueError, match="bool"):
        ops.ragged_lengths(torch.tensor([True, True, True]), 3, 5, 70)
    with pytest.raises(ValueError, match="256"):
        ops.ragged_lengths([1, 2, 3], 3, 5, 257)
    # the ops check on the host before they ask for a device
    with pytest.raises(ValueError, match="256"):
        ops.viterbi_ragged(torch.zeros(3, 5, 257), torch.zeros(257, 257), torch.zeros(257), ops.OBS_LOG,
                           torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match=r"\[1, 2, 6\]"):
        ops.forward_backward_ragged(torch.zeros(3, 5, 7), torch.zeros(7, 7), torch.zeros(7), ops.OBS_PROB,
                                    torch.tensor([1, 2, 6]), 1)


def test_active_lengths():
    from pytorch_hmm_amd import ops
    assert ops.active_lengths(None, 3, 5, 7) is None
    assert ops.active_lengths([5, 5, 5], 3, 5, 7) is None
    assert ops.active_lengths([5, 4, 5], 3, 5, 7).tolist() == [5, 4, 5]


def test_cpu_tensors_are_refused_by_name():
    from pytorch_hmm_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.viterbi_ragged(torch.zeros(2, 5, 7), torch.zeros(7, 7), torch.zeros(7), ops.OBS_LOG, torch.tensor([2, 5]))


# -------------------------------------------------------------------------------- fakes
def test_fakes_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pytorch_hmm_amd import ops
    B, T, N = 3, 9, 70
    with FakeTensorMode():
        obs, lP, v = torch.empty(B, T, N), torch.empty(N, N), torch.empty(N)
        lens = torch.empty(B, dtype=torch.int32)
        post, fwd, bwd, ll, lr = torch.ops.hmm355.forward_backward_ragged(obs, lP, v, ops.OBS_PROB, lens, 5)
        assert post.shape == (B, T, N) and bwd.shape == (B, T, N) and fwd.shape == (0,)
        assert ll.shape == (B,) and lr.shape == (B,)
        assert all(x.dtype == torch.float32 for x in (post, fwd, bwd, ll, lr))
        post, _, _, _, _ = torch.ops.hmm355.forward_backward_ragged(obs, lP, v, ops.OBS_PROB, lens, 1,
                                                                    torch.empty(B, N))
        assert post.shape == (B, T, N)
        states, delta, final = torch.ops.hmm355.viterbi_ragged(obs, lP, v, ops.OBS_LOG, lens)
        assert states.shape == (B, T) and states.dtype == torch.int64
        assert delta.shape == (B, T, N) and delta.dtype == torch.float32
        assert final.shape == (B,) and final.dtype == torch.float32


# ------------------------------------------------------------------------ the test model
def test_model_with_full_lengths_is_the_oracle():
    rng = np.random.default_rng(0)
    B, T, N = 3, 12, 7
    obs = torch.from_numpy(rng.random((B, T, N), dtype=np.float32))
    lP, lp0 = O.hmm_params(O.left_to_right_matrix(N, 0.7))
    lo = torch.log(obs + 1e-8)
    full = [T] * B
    s, dl, final = rm.viterbi_from_log(lo, lP, lp0, full)
    s_ref, d_ref = O.viterbi_from_log(lo, lP, lp0)
    assert torch.equal(s, s_ref) and torch.equal(dl, d_ref) and torch.equal(final, d_ref[:, -1].max(-1).values)
    ref = O.forward_backward(obs, lP, lp0)
    for a, b in zip(rm.forward_backward(obs, lP, lp0, full), ref[:3]):
        assert torch.equal(a, b)
    assert torch.equal(rm.compute_likelihood(obs, lP, lp0, full), O.compute_likelihood(obs, lP, lp0))
    la, lb, post, ll = rm.fb64(lo.numpy(), lP.numpy(), lp0.numpy(), full)
    for a, b in zip((la, lb, post, ll), O.c_fb64(lo.numpy(), lP.numpy(), lp0.numpy())):
        assert np.array_equal(a, b)


def test_model_pads_by_the_convention():
    rng = np.random.default_rng(1)
    B, T, N = 2, 6, 5
    obs = torch.from_numpy(rng.random((B, T, N), dtype=np.float32))
    lP, lp0 = O.hmm_params(O.left_to_right_matrix(N, 0.7))
    s, dl, _ = rm.viterbi_from_log(torch.log(obs + 1e-8), lP, lp0, [2, 6])
    assert (s[0, 2:] == -1).all() and (s[0, :2] >= 0).all() and (s[1] >= 0).all()
    assert torch.isinf(dl[0, 2:]).all() and (dl[0, 2:] < 0).all() and torch.isfinite(dl[1]).all()
    post, fwd, bwd = rm.forward_backward(obs, lP, lp0, [2, 6])
    for x in (post, fwd, bwd):
        assert (x[0, 2:] == 0).all()
    assert torch.allclose(post[0, :2].sum(-1), torch.ones(2), atol=1e-5)
