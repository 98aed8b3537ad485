"""GPU: the end of the Viterbi decode beside a banded chain (follow.h vit_decode_follow).  The
chain's own workgroup takes the first arg-max of the last trellis row from its LDS ring, writes
the final score and hands the end state over with its final count; the follower keeps the
end-state table of the chunks it has composed, so the chunk end states are one row of it.

Contract: states, trellis and final score bit-identical to the C oracle through the plan path.
Shapes: N = 100, 128 (NP = 128, padded and full), 200, 256 (NP = 256); T = 1 (one row, no map),
63 / 64 / 65 and 128 / 129 (the 64-step chunk boundaries: one chunk, a second of one step, two
whole, a third of one step), 700 (eleven chunks, the last short: several composing groups).

Ties: with the ergodic matrix (invariant under any permutation of the states) and a uniform
start, emissions that are equal within each pair of states (2k, 2k + 1) keep the pair's trellis
values equal bit for bit, so the last row's maximum is attained twice and the first arg-max
(the reference's end state) differs from the last one.  The test asserts that on the oracle's
own output, and batch element 0 of every case is such a sequence."""
import functools

import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 3
TS = (1, 63, 64, 65, 128, 129, 700)
NS = (100, 128, 200, 256)
KINDS = ("l2r", "per_row", "ergodic")


def t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def ops():
    from pytorch_hmm_amd import ops as o
    return o


@functools.lru_cache(maxsize=None)
def model(kind, N):
    rng = np.random.default_rng([KINDS.index(kind), N, 5])
    if kind == "l2r":
        lP, lp0 = (x.numpy() for x in O.hmm_params(O.left_to_right_matrix(N, 0.7)))
    elif kind == "ergodic":
        lP, lp0 = (x.numpy() for x in O.hmm_params(O.transition_matrix(N, "ergodic")))
    else:
        lP = M.band_case(M.TRI, N, "per_row", rng)
        p = rng.random(N) + 0.1
        lp0 = np.log(p / p.sum()).astype(np.float32)
    assert M.classify(lP)["banded"], (kind, N)
    return np.ascontiguousarray(lP, np.float32), np.ascontiguousarray(lp0, np.float32)


def log_obs(kind, N, T, salt=0):
    rng = np.random.default_rng([KINDS.index(kind), N, T, salt])
    lo = np.log(rng.random((B, T, N), dtype=np.float32) + np.float32(1e-8)).astype(np.float32)
    if kind == "ergodic":
        # batch element 0: equal emissions within each pair of states, the last row all equal
        lo[0, :, 1::2] = lo[0, :, 0:2 * (N // 2):2]
        lo[0, -1, :] = np.float32(-1.5)
    return lo


def check(o, kind, N, lo, want):
    lP, lp0 = model(kind, N)
    cs, cd = want
    plan = o.make_plan(t(lP))
    assert plan._hmm355_banded
    states, delta, final = o.viterbi(t(lo), t(lP), t(lp0), o.OBS_LOG, plan)
    assert np.array_equal(delta.cpu().numpy(), cd), "trellis"
    assert np.array_equal(states.cpu().numpy(), cs), "states"
    assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), "final score"


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_decode_end_bitexact(kind, N, T):
    lP, lp0 = model(kind, N)
    lo = log_obs(kind, N, T)
    cs, cd, _ = O.c_viterbi(lo, lP, lp0)
    if kind == "ergodic":
        last = cd[0, -1]
        first_arg = int(np.argmax(last))
        last_arg = N - 1 - int(np.argmax(last[::-1]))
        assert first_arg != last_arg, "the tie case has no tie in the last row"
        assert cs[0, -1] == first_arg, "the oracle's end state is the first arg-max"
    check(ops(), kind, N, lo, (cs, cd))


@pytest.mark.parametrize("N", (128, 200))
def test_three_calls_in_a_row(N):
    """three calls back to back on one stream and one workspace: a count or end state of the call
    before would show in the next one's path"""
    o = ops()
    kind, T = "ergodic", 129
    lP, lp0 = model(kind, N)
    los = [log_obs(kind, N, T, salt) for salt in (1, 2, 3)]
    want = [O.c_viterbi(lo, lP, lp0) for lo in los]
    plan = o.make_plan(t(lP))
    tl, tp = t(lP), t(lp0)
    dev = [t(lo) for lo in los]
    torch.cuda.synchronize()
    got = [o.viterbi(x, tl, tp, o.OBS_LOG, plan) for x in dev]
    torch.cuda.synchronize()
    for k in range(3):
        states, delta, final = got[k]
        cs, cd, _ = want[k]
        assert np.array_equal(states.cpu().numpy(), cs), f"call {k} states"
        assert np.array_equal(delta.cpu().numpy(), cd), f"call {k} trellis"
        assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), f"call {k} final score"
