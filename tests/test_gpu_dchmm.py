"""GPU parity of the duration-penalty Viterbi (csrc/dchmm.hip; ops.duration_constrained_viterbi;
DurationConstrainedHMM).

Contract: bit for bit.  Every value of the recursion is an exact maximum of sums of two or three
fp32 adds taken in the reference's order, and each penalty is one rounded fp32 product, so the
decoded states equal the reference's (tests/golden/dchmm_*.npz) and the whole trellis, log_delta
and durations, equals the numpy restatement's (tests/dchmm_numpy.py, itself pinned to the
fixtures on the CPU) under array_equal, the -inf pattern included.  Only the module's forward has
a tolerance, 1e-5 on the emission log-probs: its GEMMs run on the GPU.

Beyond the fixtures the shapes sit where the kernel changes its path: S across the wave size and
across the point where the transition matrix no longer fits in LDS (S = 200, 256), groups whose
cells fit one pass of 1024 threads with one, two and four sequences per thread (B * S up to 1024,
2048 and beyond; odd B pads the last block), each of those with the matrix in and out of LDS,
the group-size limit itself, and a partial last group.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dchmm_numpy as dn  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _native():
    import pytorch_hmm_amd._native as nat
    nat.lib()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()


def ops():
    from pytorch_hmm_amd import ops as o
    return o


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)    # a copy: the shared cases stay read-only


def run(e, lT, mn, mx, per_sequence=False, w=0.1):
    s, score, delta, dur = ops().duration_constrained_viterbi(dev(e), dev(lT), mn, mx, w, per_sequence, True)
    assert s.dtype == torch.int64 and dur.dtype == torch.int32 and delta.dtype == torch.float32
    return s.cpu().numpy(), score.cpu().numpy(), delta.cpu().numpy(), dur.cpu().numpy()


def check(e, lT, mn, mx, per_sequence=False, states=None):
    """kernel == restatement on states, delta and dur, bit for bit; score = the last row's maximum"""
    want = dn.viterbi(e, lT, mn, mx, group=1 if per_sequence else None)
    s, score, delta, dur = run(e, lT, mn, mx, per_sequence)
    assert np.array_equal(delta, want[1]) and not np.isnan(delta).any()
    assert np.array_equal(dur, want[2])
    assert np.array_equal(s, want[0])
    assert np.array_equal(score, want[1][:, -1].max(axis=1))
    if states is not None:
        assert np.array_equal(s, states)
    return s


@functools.lru_cache(maxsize=None)
def random_case(B, T, S, seed=0, halves=False, neginf=0.0):
    """Shared among the tests, read-only.  Log-softmax emissions that favour one state for 3..9
    frames at a time (paths stay past max_duration and still move on).  halves: scores that are
    multiples of 1/2 in a narrow range instead, with no favoured state: exact ties among a cell's
    candidates, and penalties that decide between paths."""
    rng = np.random.default_rng(100 * S + B + seed)
    x = rng.standard_normal((B, T, S)).astype(np.float32)
    lT = torch.log(torch.softmax(torch.from_numpy(rng.standard_normal((S, S)).astype(np.float32)), 1) + 1e-8).numpy()
    if halves:
        e, lT = (np.round(2 * x) / 2).astype(np.float32), (np.round(2 * lT) / 2).astype(np.float32)
        e[:, 0] = 0.0   # a flat first row: frame 1's candidates differ by lT alone, so many tie exactly
    else:
        for b in range(B):
            t = 0
            while t < T:
                n = int(rng.integers(3, 10))
                x[b, t:t + n, int(rng.integers(0, S))] += 8.0
                t += n
        e = torch.log_softmax(torch.from_numpy(x), 2).numpy()
    if neginf:
        e[rng.random(e.shape) < neginf] = -np.inf
    e.setflags(write=False)
    lT.setflags(write=False)
    return e, lT


# ------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("name", dn.FIXTURES)
def test_fixture(gold, name):
    g = gold("dchmm_" + name)
    e, lT, mn, mx = g["e"], g["lT"], int(g["min_duration"]), int(g["max_duration"])
    check(e, lT, mn, mx, states=g["states"])
    s, score, delta, dur = ops().duration_constrained_viterbi(dev(e), dev(lT), mn, mx)
    assert np.array_equal(s.cpu().numpy(), g["states"])         # the same without the trellis
    assert delta.numel() == 0 and dur.numel() == 0 and score.shape == (e.shape[0],)


# ---------------------------------------------------------------------- sizes beyond them
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 128, 200, 256])
def test_state_counts(S):
    e, lT = random_case(2, 40, S)
    s = check(e, lT, 3, 5)
    if S >= 63:
        _, _, dur = dn.viterbi(e, lT, 3, 5)
        assert dur.max() > 5       # some path outstays max_duration: pen_self was applied
        assert len(np.unique(s)) > 1


def test_group_limit():
    e, lT = random_case(16, 6, 256)         # B * S = 4096: exactly the limit
    check(e, lT, 3, 5)


def test_past_the_limits():
    e, lT = random_case(17, 6, 256)
    o = ops()
    with pytest.raises(ValueError, match="4096"):
        o.duration_constrained_viterbi(dev(e), dev(lT), 3, 5)
    with pytest.raises(ValueError, match="4096"):
        o.duration_constrained_viterbi(dev(e), dev(lT), 3, 5, 0.1, False)
    with pytest.raises(ValueError, match="256"):
        o.duration_constrained_viterbi(torch.zeros(17, 6, 257, device=DEV), torch.zeros(257, 257, device=DEV), 3, 5,
                                       0.1, False)
    with pytest.raises(ValueError, match="256"):
        o.duration_constrained_viterbi(torch.zeros(1, 6, 257, device=DEV), torch.zeros(257, 257, device=DEV), 3, 5,
                                       0.1, True)
    check(e, lT, 3, 5, per_sequence=True)   # past the coupled limit, per_sequence decodes


@pytest.mark.parametrize("B,S", [(3, 40), (5, 40), (7, 130), (12, 100), (11, 120), (9, 200), (5, 256), (33, 100),
                                 (19, 200)])
def test_batch_sizes_around_the_sequences_per_thread(B, S):
    e, lT = random_case(B, 24, S, neginf=0.05)
    check(e, lT, 3, 5)


# -------------------------------------------------------------------------------- groups
def test_per_sequence_on_b3(gold):
    g = gold("dchmm_b3")
    s = check(g["e"], g["lT"], 3, 4, per_sequence=True, states=g["states_alone"])
    assert not np.array_equal(s, g["states"])


@pytest.mark.parametrize("B,S,group", [(5, 6, 2), (5, 70, 2), (11, 33, 4), (6, 256, 5)])
def test_partial_last_group_through_the_c_abi(B, S, group):
    import pytorch_hmm_amd._native as nat
    T, mn, mx = 30, 3, 5
    e, lT = random_case(B, T, S, seed=7, halves=S == 6)
    want = dn.viterbi(e, lT, mn, mx, group=group)
    L = nat.lib()
    de, dl = dev(e), dev(lT)
    states = torch.empty((B, T), dtype=torch.int64, device=DEV)
    score = torch.empty(B, device=DEV)
    delta = torch.empty((B, T, S), device=DEV)
    dur = torch.empty((B, T, S), dtype=torch.int32, device=DEV)
    ws = torch.empty(L.hmm355_dchmm_workspace_bytes(B, T, S), dtype=torch.uint8, device=DEV)
    nat.check(L.hmm355_dchmm_viterbi_f32(nat.ptr(de), nat.ptr(dl), B, T, S, group, mn, mx, 0.1, nat.ptr(states),
                                         nat.ptr(score), nat.ptr(delta), nat.ptr(dur), nat.ptr(ws), ws.numel(),
                                         nat.stream_of(torch.device(DEV, torch.cuda.current_device()))))
    torch.cuda.synchronize()
    assert np.array_equal(delta.cpu().numpy(), want[1]) and np.array_equal(dur.cpu().numpy(), want[2])
    assert np.array_equal(states.cpu().numpy(), want[0])
    assert np.array_equal(score.cpu().numpy(), want[1][:, -1].max(axis=1))
    if S == 6:   # the groups really differ from one coupled batch
        assert not np.array_equal(want[2], dn.viterbi(e, lT, mn, mx)[2])


# ---------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("B,S", [(3, 65), (5, 65), (2, 256)])
def test_quantised_ties(B, S):
    e, lT = random_case(B, 30, S, halves=True)
    stats = {}
    s = dn.viterbi(e, lT, 3, 5, stats=stats)[0]
    assert stats["ties"] > 10 and len(np.unique(s)) > 3     # cells that the first-index rule decides
    check(e, lT, 3, 5)
    check(e, lT, 3, 5, per_sequence=True)


def test_all_equal_scores_take_the_first_index():
    B, T, S = 2, 9, 70
    e, lT = np.zeros((B, T, S), np.float32), np.zeros((S, S), np.float32)
    s = check(e, lT, 1, 100)       # no penalty ever: every candidate of a cell ties
    assert (s == 0).all()


def test_dead_cells_and_dead_sequences():
    e, lT = random_case(3, 12, 20, neginf=0.3)
    e = e.copy()
    e[1, 4] = -np.inf              # sequence 1 dies at frame 4: all of its later cells are -inf
    s = check(e, lT, 3, 4)
    _, _, dur = dn.viterbi(e, lT, 3, 4)
    assert (dur[1, 4:] == 0).all() and (s[1, 3:] == 0).all()
    lT2 = lT.copy()
    lT2[:, 3] = -np.inf            # a state that can only be kept, never entered
    check(e, lT2, 3, 4)


# ---------------------------------------------------------------------------- short runs
def test_one_and_two_frames(gold):
    g = gold("dchmm_t1")
    s = check(g["e"], g["lT"], 3, 4, states=g["states"])
    assert s.shape[1] == 1
    e, lT = random_case(3, 2, 7)
    _, delta, _ = dn.viterbi(e, lT, 3, 1)            # max_duration = 1: pen_self on the first step
    own = (delta[:, 0] + e[:, 1]) + np.float32(-np.float32(0.1)) * np.float32(1)
    assert (delta[:, 1] >= own).all()
    check(e, lT, 3, 1)
    check(e, lT, 3, 1, per_sequence=True)
    check(e[:, :1], lT, 3, 1, per_sequence=True)


# -------------------------------------------------------------------------------- module
def test_module(gold):
    from pytorch_hmm_amd import DurationConstrainedHMM
    g = gold("dchmm_module")
    S, D = g["log_transitions"].shape[0], int(g["feature_dim"])
    m = DurationConstrainedHMM(S, D, int(g["min_duration"]), int(g["max_duration"]))
    m.load_state_dict({str(k): torch.from_numpy(g["sd." + str(k)]) for k in g["sd_keys"]})
    m = m.to(DEV)
    obs = dev(g["obs"])
    with torch.no_grad():
        elp = m.emission_net(obs)
        lT = torch.log(torch.softmax(m.transition_logits, dim=-1) + 1e-8)
        assert np.abs(elp.cpu().numpy() - g["emission_log_probs"]).max() <= 1e-5
        assert np.abs(lT.cpu().numpy() - g["log_transitions"]).max() <= 1e-5
        states = m(obs)
        assert states.dtype == torch.int64 and states.shape == g["states"].shape
        assert torch.equal(states, m._constrained_viterbi(elp, lT))
        fed = m._constrained_viterbi(dev(g["emission_log_probs"]), dev(g["log_transitions"]))
    assert np.array_equal(fed.cpu().numpy(), g["states"])
    alone = DurationConstrainedHMM(S, D, 3, 4, per_sequence=True).to(DEV)
    b3 = gold("dchmm_b3")
    assert np.array_equal(alone._constrained_viterbi(dev(b3["e"]), dev(b3["lT"])).cpu().numpy(), b3["states_alone"])


# ---------------------------------------------------------------- stream and repeatability
def test_stream_repeat_and_layout(gold):
    o = ops()
    e, lT = random_case(4, 40, 65)
    de, dl = dev(e), dev(lT)
    first = o.duration_constrained_viterbi(de, dl, 3, 5, 0.1, False, True)
    again = o.duration_constrained_viterbi(de, dl, 3, 5, 0.1, False, True)
    for x, y in zip(first, again):
        assert torch.equal(x, y)
    side = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        src = (big @ big)[:1, :1].sum() * 0 + de   # the inputs exist only after the matmul, on this stream
        out = o.duration_constrained_viterbi(src, dl, 3, 5, 0.1, False, True)
    side.synchronize()
    for x, y in zip(first, out):
        assert torch.equal(x, y)
    # a transposed view, a strided matrix and fp64 inputs give the contiguous fp32 result
    et = de.transpose(1, 2).contiguous().transpose(1, 2)
    assert not et.is_contiguous()
    lt2 = torch.zeros(65, 130, device=DEV)[:, ::2]
    lt2.copy_(dl)
    assert not lt2.is_contiguous()
    for x, y in zip(first, o.duration_constrained_viterbi(et, lt2, 3, 5, 0.1, False, True)):
        assert torch.equal(x, y)
    for x, y in zip(first, o.duration_constrained_viterbi(de.double(), dl.double(), 3, 5, 0.1, False, True)):
        assert torch.equal(x, y)


def test_registered_op_and_fake():
    e, lT = random_case(2, 40, 2)
    s, score, delta, dur = torch.ops.hmm355.duration_constrained_viterbi(dev(e), dev(lT), 3, 5)
    assert np.array_equal(s.cpu().numpy(), dn.viterbi(e, lT, 3, 5)[0]) and delta.numel() == 0
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        fe, fl = torch.empty(3, 11, 6, device=DEV), torch.empty(6, 6, device=DEV)
        s, score, delta, dur = torch.ops.hmm355.duration_constrained_viterbi(fe, fl, 3, 5, 0.1, False, True)
        assert (s.shape, s.dtype) == ((3, 11), torch.int64) and (score.shape, score.dtype) == ((3,), torch.float32)
        assert (delta.shape, delta.dtype) == ((3, 11, 6), torch.float32)
        assert (dur.shape, dur.dtype) == ((3, 11, 6), torch.int32)
        s, score, delta, dur = torch.ops.hmm355.duration_constrained_viterbi(fe, fl, 3, 5)
        assert delta.numel() == 0 and dur.numel() == 0 and s.shape == (3, 11)
