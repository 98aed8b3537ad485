"""CPU: the numpy model of the HSMM forward-backward (tests/hsmm_fb_numpy.py) against brute-force
enumeration of every segmentation, its identities on the committed HSMM fixtures, and the
argument checks of hmm355_hsmm_fb_f32 (include/hmm355.h), which come before anything is launched
or dereferenced.  No compute calls on the library here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import hsmm_fb_numpy as M  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hmm355.h")
GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("hsmm_s2", "hsmm_s5", "hsmm_s8", "hsmm_d96")
OUTPUTS = ("gamma", "dur_counts", "trans_counts", "init_post")
TINY = [(6, 3, 3), (5, 2, 4), (7, 3, 2), (1, 3, 3), (4, 1, 4)]  # (T, S, Dmax)


def tiny_tables(T, S, Dm, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(-3, 2, (T, S)), rng.normal(-1, 1, (S, Dm)), rng.normal(-1, 1, (S, S)),
            rng.normal(-1, 1, S))


@pytest.mark.parametrize("T,S,Dm", TINY)
@pytest.mark.parametrize("with_init", [False, True])
def test_model_equals_enumeration(T, S, Dm, with_init):
    lp, du, lt, li = tiny_tables(T, S, Dm, 100 * T + 10 * S + Dm)
    li = li if with_init else None
    got = M.hsmm_fb_one(lp, du, lt, li)
    ref = M.enumerate_segmentations(lp, du, lt, li)
    assert abs(got["loglik"] - ref["loglik"]) <= 1e-12 * max(1.0, abs(ref["loglik"]))
    assert abs(got["ll_backward"] - got["ll_shifted"]) <= 1e-12 * max(1.0, abs(got["ll_shifted"]))
    for k in OUTPUTS:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-12, err_msg=k)
    # the unshifted recursion is the same model
    raw = M.hsmm_fb_one(lp, du, lt, li, shift=False)
    assert abs(raw["loglik"] - ref["loglik"]) <= 1e-12 * max(1.0, abs(ref["loglik"]))


def test_model_with_neg_inf_entries_equals_enumeration():
    lp, du, lt, li = tiny_tables(6, 3, 3, 7)
    du[:, 0] = -np.inf      # a minimum duration of 2
    lt[2, :] = -np.inf      # state 2 is a dead end
    lp[3, 1] = -np.inf
    got = M.hsmm_fb_one(lp, du, lt, li)
    ref = M.enumerate_segmentations(lp, du, lt, li)
    assert np.isfinite(ref["loglik"]) and abs(got["loglik"] - ref["loglik"]) <= 1e-12
    for k in OUTPUTS:
        assert np.isfinite(got[k]).all()
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-12, err_msg=k)


def test_infeasible_sequence_gives_neg_inf_and_zeros():
    lp, du, lt, _ = tiny_tables(5, 1, 3, 3)   # one state cannot follow itself: T > Dmax has no segmentation
    for dtype in (np.float64, np.float32):
        got = M.hsmm_fb_one(lp, du, lt, dtype=dtype)
        assert got["loglik"] == -np.inf
        for k in OUTPUTS:
            assert not np.isnan(got[k]).any() and (got[k] == 0).all(), k
    assert M.enumerate_segmentations(lp, du, lt)["loglik"] == -np.inf


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_bound_and_identities(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=True)
    got = M.hsmm_fb(z["log_probs"], z["dur_log_probs"], z["log_T"])
    assert (got["loglik"] >= z["scores"]).all()               # the sum bounds its largest term
    np.testing.assert_allclose(got["gamma"].sum(-1), 1.0, rtol=0, atol=1e-10)
    np.testing.assert_allclose(got["init_post"].sum(-1), 1.0, rtol=0, atol=1e-10)
    segs = got["dur_counts"].sum((1, 2))
    np.testing.assert_allclose(segs, got["trans_counts"].sum((1, 2)) + 1.0, rtol=0, atol=1e-10)
    assert (got["trans_counts"][:, np.arange(z["log_T"].shape[0]), np.arange(z["log_T"].shape[0])] == 0).all()
    np.testing.assert_allclose(got["ll_backward"], got["ll_shifted"], rtol=1e-12)
    # frames of a state = its segments' durations
    d = np.arange(1, z["dur_log_probs"].shape[1] + 1)
    np.testing.assert_allclose(got["gamma"].sum(1), (got["dur_counts"] * d).sum(-1), rtol=0, atol=1e-9)


def test_diagonal_of_log_T_is_never_used():
    z = np.load(os.path.join(GOLDEN, "hsmm_s5.npz"), allow_pickle=True)
    lt = z["log_T"].astype(np.float64).copy()
    a = M.hsmm_fb(z["log_probs"], z["dur_log_probs"], lt)
    lt[np.arange(5), np.arange(5)] = 1000.0
    b = M.hsmm_fb(z["log_probs"], z["dur_log_probs"], lt)
    for k in ("loglik",) + OUTPUTS:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------- the C ABI
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
ALL = 0xF0


def fb(L, lp=FAKE, dur=FAKE, lt=FAKE, li=None, B=2, T=10, S=5, Dm=7, flags=ALL, loglik=FAKE, gamma=FAKE,
       durc=FAKE, trc=FAKE, ip=FAKE, wsp=FAKE, ws=BIG):
    return L.hmm355_hsmm_fb_f32(lp, dur, lt, li, B, T, S, Dm, flags, loglik, gamma, durc, trc, ip, wsp, ws, None)


def test_header_exports_and_version(L, d):
    from pytorch_hmm_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hmm355_[a-z0-9_]+)\s*\(", src))
    for name in ("hmm355_hsmm_fb_workspace_bytes", "hmm355_hsmm_fb_f32"):
        assert name in declared and name in nat.EXPORTS and hasattr(L, name)
    assert declared == set(nat.EXPORTS)
    assert L.hmm355_version() >= 7
    assert (d["HMM355_HSMM_FB_GAMMA"], d["HMM355_HSMM_FB_DUR"], d["HMM355_HSMM_FB_TRANS"],
            d["HMM355_HSMM_FB_INIT"]) == (nat.HSMM_FB_GAMMA, nat.HSMM_FB_DUR, nat.HSMM_FB_TRANS, nat.HSMM_FB_INIT)
    assert (d["HMM355_HSMM_FB_MAX_STATES"], d["HMM355_HSMM_FB_MAX_DURATION"], d["HMM355_HSMM_FB_MAX_CELLS"]) == \
        (nat.HSMM_FB_MAX_STATES, nat.HSMM_FB_MAX_DURATION, nat.HSMM_FB_MAX_CELLS)
    assert nat.HSMM_FB_MAX_STATES >= 256 and nat.HSMM_FB_MAX_DURATION >= 128 and nat.HSMM_FB_MAX_CELLS >= 16384


def test_argument_checks(L, d):
    from pytorch_hmm_amd import _native as nat
    ARG, STATES, SHAPE, DUR = d["HMM355_E_ARG"], d["HMM355_E_STATES"], d["HMM355_E_SHAPE"], d["HMM355_E_DURATION"]
    assert fb(L, S=0) == STATES and fb(L, S=nat.HSMM_FB_MAX_STATES + 1) == STATES
    assert fb(L, Dm=0) == DUR and fb(L, Dm=nat.HSMM_FB_MAX_DURATION + 1) == DUR
    assert fb(L, S=256, Dm=65) == DUR                      # S * Dmax above the LDS ring
    assert fb(L, T=0) == SHAPE
    assert fb(L, B=-1) == ARG and fb(L, flags=0x100) == ARG
    for ptr in ("lp", "dur", "lt", "loglik", "wsp"):
        assert fb(L, **{ptr: None}) == ARG, ptr
    for ptr in ("gamma", "durc", "trc", "ip"):             # each output flag needs its pointer
        assert fb(L, **{ptr: None}) == ARG, ptr
    assert fb(L, wsp=ctypes.c_void_p(0x1004)) == ARG
    need = L.hmm355_hsmm_fb_workspace_bytes(2, 10, 5, 7, ALL)
    assert need > 0 and fb(L, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    assert fb(L, ws=16, flags=0) == d["HMM355_E_WORKSPACE"]
    assert fb(L, B=0) == 0
    assert fb(L, B=nat.HSMM_FB_MAX_BATCH + 1) == SHAPE and fb(L, B=1 << 20, T=1 << 12) == SHAPE
    assert d["HMM355_HSMM_FB_MAX_BATCH"] == nat.HSMM_FB_MAX_BATCH == 65535
    assert L.hmm355_hsmm_fb_f32(None, None, None, None, 0, 10, 5, 7, ALL, None, None, None, None, None, None, 0,
                                None) == 0
    # the shape is checked before the empty batch
    assert fb(L, B=0, S=0) == STATES and fb(L, B=0, T=0) == SHAPE


def test_workspace_sizes(L):
    B, T, S, Dm = 3, 50, 6, 9
    lik = L.hmm355_hsmm_fb_workspace_bytes(B, T, S, Dm, 0)
    gam = L.hmm355_hsmm_fb_workspace_bytes(B, T, S, Dm, 0x10)
    dur = L.hmm355_hsmm_fb_workspace_bytes(B, T, S, Dm, 0x30)
    assert 0 < lik < B * T * S * 4 + 8192                     # likelihood only: no (B,T,S) table
    assert gam >= lik + 4 * B * T * S * 4                     # begin, F, Bend, Bbeg
    assert dur >= gam + B * T * S * 12                        # fp64 prefix sums and -inf counts
    assert L.hmm355_hsmm_fb_workspace_bytes(B, T, 0, Dm, 0) == 0
    assert L.hmm355_hsmm_fb_workspace_bytes(B, T, S, 129, 0) == 0
    assert L.hmm355_hsmm_fb_workspace_bytes(B, 0, S, Dm, 0) == 0
    assert L.hmm355_hsmm_fb_workspace_bytes(B, T, S, Dm, 0x100) == 0
    assert L.hmm355_hsmm_fb_workspace_bytes(B, T, 256, 64, 0xF0) > 0
    assert L.hmm355_hsmm_fb_workspace_bytes(B, T, 64, 40, 0xF1) > 0   # HMM355_FORM_GENERAL is accepted


def test_layer_methods_need_a_gpu_and_a_supported_size():
    import torch
    from pytorch_hmm_amd import HSMMLayer
    layer = HSMMLayer(4, 3, max_duration=6)
    x = torch.randn(1, 8, 3)
    for call in (layer.log_likelihood, layer.state_posteriors, layer.compute_loss):
        with pytest.raises(RuntimeError, match="GPU"):
            call(x)
    big = HSMMLayer(300, 3, max_duration=6)      # construction and decoding keep their limits
    wide = HSMMLayer(256, 3, max_duration=65)
    for layer in (big, wide):
        for call in (layer.log_likelihood, layer.state_posteriors, layer.compute_loss):
            with pytest.raises(ValueError, match="max_duration"):
                call(x)


def test_op_and_autograd_are_registered():
    import torch
    from pytorch_hmm_amd import autograd, ops
    assert hasattr(torch.ops.hmm355, "hsmm_forward_backward") and hasattr(autograd, "HsmmLogLik")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.hsmm_forward_backward(torch.zeros(1, 4, 3), torch.zeros(3, 2), torch.zeros(3, 3))


def test_gpu_pairs_cover_every_table_placement():
    """The chain kernel is instantiated for three placements of log_T and dur_lp; the GPU tests'
    (S, Dmax) pairs run all three and both sides of each switch, by the host code's own
    arithmetic (restated in test_gpu_hsmm_fb.placement with the budget read from the source)."""
    import test_gpu_hsmm_fb as G
    src = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "hsmm_fb.hip")).read()
    budget = int(re.search(r"kHfLdsBudget = (\d+) \* 1024;", src).group(1)) * 1024
    assert "S + sub" in src and "hsmm_fb_chain_kernel<false, false>" not in src
    place = lambda S, Dm: G.placement(S, Dm, budget)
    assert {place(S, Dm) for S, Dm in G.PAIRS} == {(True, True), (True, False), (False, True)}
    assert place(128, 90) == (True, True) and place(128, 91) == (True, False)
    assert place(160, 88) == (True, False) and place(160, 89) == (False, True)
    assert place(128, 128) == (True, False) and place(160, 102) == (False, True)
    assert place(65, 128) == (True, True) and place(256, 64) == (False, True)
    # without log_T the ring and dur_lp always fit: there is no fourth placement
    for S in range(1, 257):
        for Dm in range(1, 129):
            if S * Dm <= G.MAX_CELLS:
                assert place(S, Dm) != (False, False), (S, Dm)
