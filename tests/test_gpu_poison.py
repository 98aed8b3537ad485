"""GPU: no op reads or leaves behind uninitialised device memory.

ops.py allocates every output and workspace with torch.empty; the native library allocates nothing.
Each launch form below is called four times on the same inputs -- unpatched, then with every
torch.empty allocation filled with 0x00 bytes, 0xFF bytes (NaN / -1) and 0x3F800000 words (1.0f / a
large int32), tests/poison.py -- and every element of every output (and of the arguments the op
updates in place) must have the same bytes in all four.  No element is masked: one that differs was
never written, an output that differs everywhere was computed from a read before a write.
poison.covers() makes each case fail if the op stops allocating through torch.empty.

A returned tensor that is a workspace handed to another library call (the third output of the
sparse forward-backward op, what the autograd functions save) is not compared itself; what its
consumer produces is (sparse_arc_counts, the gradients).

Each case is the smallest shape that reaches its launch form.
"""
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import range_cases as rc  # noqa: E402
import sparse_numpy as sn  # noqa: E402
from poison import check_four  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = -np.inf
# sequences per workgroup of the batch-tiled step kernels (csrc/wide.hip kBT)
BT = int(re.search(r"constexpr int kBT = (\d+);",
                   open(os.path.join(HERE, "..", "pytorch_hmm_amd", "csrc", "wide.hip")).read()).group(1))


def o():
    from pytorch_hmm_amd import ops
    return ops


def lib():
    from pytorch_hmm_amd import _native
    return _native.lib()


def t(a, dtype=None):
    if a is None:
        return None
    x = torch.as_tensor(np.ascontiguousarray(a))
    return x.to(DEV) if dtype is None else x.to(DEV, dtype)


def l2r_model(N):
    """left-to-right 0.7 (a banded plan) as log tables on the device"""
    from oracle import hmm_oracle as O
    lP, lp0 = O.hmm_params(O.left_to_right_matrix(N, 0.7))
    return lP.to(DEV), lp0.to(DEV)


def dense_model(N, seed):
    rng = np.random.default_rng(seed)
    lP = np.log(rng.dirichlet(np.ones(N), size=N) + 1e-8).astype(np.float32)
    lp0 = np.log(rng.dirichlet(np.ones(N)) + 1e-8).astype(np.float32)
    return t(lP), t(lp0)


def ragged_lengths(T):
    return np.array([T, 1, max(T // 2, 1)], np.int64)


def log_emissions(B, T, N, seed, lengths=None):
    rng = np.random.default_rng(seed)
    e = np.log(rng.dirichlet(np.ones(N), size=(B, T))).astype(np.float32)
    if lengths is not None:
        for b in range(B):
            e[b, int(lengths[b]):] = np.nan      # padded frames are never read
    return e


# ------------------------------------------------------------------ forward-backward
@pytest.mark.parametrize("N", [7, 100, 200])
@pytest.mark.parametrize("form", ["noplan", "dense", "follow", "pair"])
def test_forward_backward(N, form):
    ops = o()
    lP, lp0 = l2r_model(N)
    plan = {"noplan": lambda: None, "dense": lambda: ops.make_plan(lP, dense=True)}.get(form, lambda: ops.make_plan(lP))()
    kw = {"follow": dict(follow=True, pair=False), "pair": dict(pair=True)}.get(form, {})
    if form in ("follow", "pair"):
        assert plan._hmm355_banded is True
    for T, mask in itertools.product((1, 33), (ops.FB_POSTERIOR, 7)):
        x = t(np.random.default_rng(N + T).random((3, T, N), dtype=np.float32))
        check_four(lambda: ops.forward_backward(x, lP, lp0, ops.OBS_PROB, mask, plan, **kw),
                   lib().hmm355_fb_workspace_bytes(3, T, N))


@pytest.mark.parametrize("T", [1, 2, 70])
def test_forward_backward_wide(T):
    ops = o()
    N, B = 257, BT + 1
    lP, lp0 = dense_model(N, 1)
    x = t(np.random.default_rng(T).random((B, T, N), dtype=np.float32))
    for mask in (ops.FB_POSTERIOR, 7):
        check_four(lambda: ops.forward_backward(x, lP, lp0, ops.OBS_PROB, mask, wide=True),
                   lib().hmm355_fb_wide_workspace_bytes(B, T, N))


@pytest.mark.parametrize("N", [7, 200])
@pytest.mark.parametrize("terminal", [False, True])
def test_forward_backward_ragged(N, terminal):
    ops = o()
    T = 33
    lens = ragged_lengths(T)
    lP, lp0 = dense_model(N, 2)
    x = t(log_emissions(3, T, N, 3, lens))
    lbt = t(np.log(np.random.default_rng(4).random((3, N)) + 0.1).astype(np.float32)) if terminal else None
    for mask in (ops.FB_POSTERIOR, 7):
        check_four(lambda: ops.forward_backward_ragged(x, lP, lp0, ops.OBS_LOG, torch.from_numpy(lens), mask, lbt),
                   lib().hmm355_fb_workspace_bytes(3, T, N))


# ---------------------------------------------------------------------------- Viterbi
@pytest.mark.parametrize("N", [7, 128, 200])
@pytest.mark.parametrize("form", ["noplan", "banded-follow", "dense-psi", "unread-plan"])
def test_viterbi(N, form):
    ops = o()
    T = 130
    lP, lp0 = l2r_model(N)
    plan = {"noplan": lambda: None, "banded-follow": lambda: ops.make_plan(lP),
            "dense-psi": lambda: ops.make_plan(lP, dense=True),
            "unread-plan": lambda: ops.make_plan(lP, read_banded=False)}[form]()
    x = t(np.random.default_rng(N).random((3, T, N), dtype=np.float32))
    check_four(lambda: ops.viterbi(x, lP, lp0, ops.OBS_PROB, plan),
               lib().hmm355_viterbi_workspace_bytes_ex(3, T, N, ops.OBS_PROB))


@pytest.mark.parametrize("T", [1, 2, 70])
def test_viterbi_wide(T):
    ops = o()
    N, B = 257, BT + 1
    lP, lp0 = dense_model(N, 5)
    x = t(np.random.default_rng(T).random((B, T, N), dtype=np.float32))
    check_four(lambda: ops.viterbi(x, lP, lp0, ops.OBS_PROB, wide=True),
               lib().hmm355_viterbi_wide_workspace_bytes(B, T, N, ops.OBS_PROB))


@pytest.mark.parametrize("N", [7, 200])
def test_viterbi_ragged(N):
    ops = o()
    T = 33
    lens = ragged_lengths(T)
    lP, lp0 = dense_model(N, 6)
    x = t(log_emissions(3, T, N, 7, lens))
    check_four(lambda: ops.viterbi_ragged(x, lP, lp0, ops.OBS_LOG, torch.from_numpy(lens)),
               lib().hmm355_viterbi_ragged_workspace_bytes(3, T, N, ops.OBS_LOG))


@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("holes", [False, True])
def test_viterbi_nbest(K, holes):
    ops = o()
    T, N = 12, 7
    lens = ragged_lengths(T)
    if holes:   # a chain with one path per start state: count < K
        P = np.full((N, N), NEG, np.float32)
        P[np.arange(N - 1), np.arange(1, N)] = 0.0
        lP, lp0 = t(P), t(np.where(np.arange(N) < 2, 0.0, NEG).astype(np.float32))
    else:
        lP, lp0 = dense_model(N, 8)
    x = t(log_emissions(3, T, N, 9, lens))
    paths, scores, count = check_four(lambda: ops.viterbi_nbest(x, lP, lp0, ops.OBS_LOG, K, lens),
                                      lib().hmm355_viterbi_nbest_workspace_bytes(3, T, N, K, ops.OBS_LOG))
    if holes and K == 16:
        assert int(count.max()) < K


# ------------------------------------------------------------------------------ sparse
SPARSE_NAMES = ["lr-N65-T70-B1", "rand-N65-T70-B3", "hub-N320-T70-B3", "nopath-N64-T3-B1", "lr-N8192-T4-B1"]
SUM_CASES = {c["name"]: c for c in sn.sum_cases()}
VIT_CASES = {c["name"]: c for c in sn.viterbi_cases()}


def sparse_on_gpu(c):
    import pytorch_hmm_amd as ph
    tr = ph.SparseTransitions(c["src"], c["dst"], t(c["log_w"]), c["N"])
    lens = None if c["lengths"] is None else torch.from_numpy(c["lengths"])
    return tr, t(c["log_obs"]), t(c["log_p0"]), lens, t(c["weight"])


@pytest.mark.parametrize("name", SPARSE_NAMES)
def test_sparse_viterbi(name):
    from pytorch_hmm_amd import sparse
    c = VIT_CASES[name]
    tr, obs, p0, lens, _ = sparse_on_gpu(c)
    E = c["src"].size
    check_four(lambda: sparse.sparse_viterbi(tr, obs, p0, lengths=lens),
               lib().hmm355_sparse_viterbi_workspace_bytes(c["B"], c["T"], c["N"], E))


@pytest.mark.parametrize("name", SPARSE_NAMES)
def test_sparse_e_step(name):
    """The workspace the forward-backward op returns is compared through its consumer: xi."""
    from pytorch_hmm_amd import sparse
    c = SUM_CASES[name]
    tr, obs, p0, lens, w = sparse_on_gpu(c)
    E = c["src"].size
    check_four(lambda: sparse.sparse_e_step(tr, obs, p0, lengths=lens, weight=w, range_guard=False),
               lib().hmm355_sparse_forward_backward_workspace_bytes(c["B"], c["T"], c["N"], E), guard=False)

    def ops_call():   # the ops themselves: loglik and posterior guarded, the workspace left out
        ops = o()
        host = None if lens is None else ops.ragged_lengths(lens, c["B"], c["T"])
        wt = tr.log_w.detach().to(torch.float32)
        ll, post, ws = ops.sparse_forward_backward(obs, tr.in_ptr_host, tr.in_ptr, tr.in_src, wt[tr.perm_in],
                                                   tr.out_ptr_host, tr.out_ptr, tr.out_dst, wt[tr.perm_out], p0, True, host)
        xi = ops.sparse_arc_counts(obs, tr.in_src, tr.in_dst, wt[tr.perm_in], ws, w, host)
        return ll, post, xi
    check_four(ops_call, lib().hmm355_sparse_arc_counts_workspace_bytes(c["B"], c["T"], c["N"], E))


# ------------------------------------------------------------------- time-varying matrices
@pytest.mark.parametrize("N", [5, 64])
@pytest.mark.parametrize("static", [False, True])
def test_tv(N, static):
    ops = o()
    B, T = 3, 9
    rng = np.random.default_rng(N)
    x = t(log_emissions(B, T, N, 10))
    if static:
        A = dense_model(N, 11)[0].expand(B, T, N, N)
    else:
        A = t(np.log(rng.dirichlet(np.ones(N), size=(B, T, N)) + 1e-8).astype(np.float32))
    lp0 = dense_model(N, 12)[1]
    for mask in (ops.FB_POSTERIOR, 7):
        check_four(lambda: ops.tv_forward_backward(x, A, lp0, mask), lib().hmm355_tv_fb_workspace_bytes(B, T, N))
    check_four(lambda: ops.tv_viterbi(x, A, lp0), lib().hmm355_tv_viterbi_workspace_bytes(B, T, N))


# ------------------------------------------------------------------------------- HSMM
def hsmm_tables(B, T, S, Dm, seed):
    rng = np.random.default_rng(seed)
    lp = (-(rng.random((B, T, S)) * 20 + 5)).astype(np.float32)
    du = np.log(rng.random((S, Dm)) + 1e-3).astype(np.float32)
    lT = np.log(rng.random((S, S)) + 1e-3).astype(np.float32)
    return t(lp), t(du), t(lT)


# one (S, Dmax) per geometry of hsmm_cfg (csrc/hsmm.hip): 4x16s64, 8x16, 4x16 and, with no
# geometry (S > 64 and Dmax >= 64), the general form of hsmm_wide.hip
@pytest.mark.parametrize("S,Dm", [(16, 12), (7, 70), (128, 63), (65, 64)])
@pytest.mark.parametrize("serial", [False, True])
def test_hsmm_viterbi(S, Dm, serial):
    ops = o()
    lp, du, lT = hsmm_tables(3, 200, S, Dm, S)
    check_four(lambda: ops.hsmm_viterbi(lp, du, lT, ops.FORM_SERIAL_WALK if serial else 0))


@pytest.mark.parametrize("flags", ["register", "general"])
def test_hsmm_viterbi_no_path(flags):
    ops = o()
    S, Dm, T = 4, 20, 90
    lp, du, _ = hsmm_tables(3, T, S, Dm, 1)
    lT = np.full((S, S), NEG, np.float32)
    lT[np.arange(S - 1), np.arange(1, S)] = 0.0
    states, scores = check_four(lambda: ops.hsmm_viterbi(lp, du, t(lT), ops.FORM_GENERAL if flags == "general" else 0))
    assert bool(torch.isneginf(scores).all())


@pytest.mark.parametrize("S,Dm", [(5, 40), (128, 91), (160, 89)])
def test_hsmm_forward_backward(S, Dm):
    ops = o()
    import test_gpu_hsmm_fb as H
    from pytorch_hmm_amd import _native as nat
    lp, du, lt, li = H.random_tables(3, Dm + 1, S, Dm, S)
    for wants, init in itertools.product((True, False), (True, False)):
        kw = dict(want_gamma=wants, want_dur=wants, want_trans=wants, want_init=wants)
        fl = (nat.HSMM_FB_GAMMA | nat.HSMM_FB_DUR | nat.HSMM_FB_TRANS | nat.HSMM_FB_INIT) if wants else 0
        check_four(lambda: ops.hsmm_forward_backward(t(lp), t(du), t(lt), t(li) if init else None, **kw),
                   lib().hmm355_hsmm_fb_workspace_bytes(3, Dm + 1, S, Dm, fl))


# ------------------------------------------------------------------------ semi-Markov
@pytest.mark.parametrize("S,Dm,T", [(4, 10, 50), (70, 10, 60), (4, 10, 3), (70, 10, 3)])
@pytest.mark.parametrize("dead", [False, True])
def test_semimarkov(S, Dm, T, dead):
    ops = o()
    rng = np.random.default_rng(S + T)
    Df = 3
    x = t(rng.standard_normal((3, T, Df)).astype(np.float32))
    means = t(rng.standard_normal((Df, S)).astype(np.float32))
    var = t((rng.random((Df, S)) + 0.5).astype(np.float32))
    (quad,) = check_four(lambda: ops.semimarkov_quad(x, means, var))
    cseg = t(rng.standard_normal(S).astype(np.float32))
    li, lT = dense_model(S, 13)[1], dense_model(S, 14)[0]
    du = np.full((S, Dm), NEG, np.float32) if dead else np.log(rng.random((S, Dm)) + 1e-3).astype(np.float32)
    du = t(du)
    wsb = lib().hmm355_semimarkov_workspace_bytes_ex(3, T, S, Dm, 0)
    check_four(lambda: ops.semimarkov_viterbi(quad, cseg, li, lT, du), wsb)
    for want_alpha in (False, True):
        check_four(lambda: ops.semimarkov_forward(quad, cseg, li, lT, du, want_alpha), wsb)


# ------------------------------------------------------------------ streaming decoders
@pytest.mark.parametrize("N", [7, 200])
def test_stream_greedy(N):
    ops = o()
    lT = dense_model(N, 15)[0]
    e = t(log_emissions(3, 70, N, 16))
    prev = t(np.array([-1, 0, N - 1], np.int32))
    check_four(lambda: ops.stream_greedy(e, lT, prev, 1.5))


@pytest.mark.parametrize("N,K,live", [(7, 5, 5), (200, 12, 12), (2, 5, 1)])
def test_stream_beam(N, K, live):
    """live = 1, N = 2, K = 5 is the under-full beam: the first frame has two expansions."""
    ops = o()
    B, T = 3, 70
    lT = dense_model(N, 17)[0]
    e = t(log_emissions(B, T, N, 18))
    rng = np.random.default_rng(19)
    hs0 = torch.full((B, ops.STREAM_SLOTS), float("-inf"))
    hl0 = torch.zeros((B, ops.STREAM_SLOTS), dtype=torch.int32)
    hs0[:, :live] = torch.from_numpy(np.sort(rng.standard_normal((B, live)).astype(np.float32))[:, ::-1].copy())
    hl0[:, :live] = torch.from_numpy(rng.integers(0, N, (B, live)).astype(np.int32))
    first = t(np.array([1, 0, 1], np.int32))

    def call():
        hs, hl = hs0.to(DEV), hl0.to(DEV)
        cnt = torch.full((B,), live, dtype=torch.int32, device=DEV)
        states, parent, hstate = ops.stream_beam(e, lT, K, hs, hl, cnt, first, live_max=live)
        return states, parent, hstate, hs, hl, cnt
    # the hypotheses are the caller's tensors, updated in place: compared, not guarded
    outs = check_four(call, guard=(0, 1, 2))
    if live == 1:
        parent, hstate = outs[1], outs[2]
        # the steps have min(K, live * N) = 2, 4, 5, 5, ... hypotheses: the other ranks are -1
        for step, kn in ((0, 2), (1, 4), (2, 5)):
            for x in (parent, hstate):
                assert bool((x[:, step, :kn] >= 0).all()) and bool((x[:, step, kn:] == -1).all())
        assert bool((parent[:, 2:] >= 0).all()) and bool((hstate[:, 2:] >= 0).all())


# ------------------------------------------------------------------ dynamic time warping
def dtw_inputs(band):
    rng = np.random.default_rng(20)
    B, N, M = 3, 9, 11
    d = rng.random((B, N, M)).astype(np.float32)
    n_len, m_len = np.array([N, 5, 7], np.int32), np.array([M, 11, 4], np.int32)
    if band:
        d[1, 4, :] = np.inf      # a wall across pair 1: its end cell is unreachable
    return t(d), t(n_len), t(m_len), (B, N, M)


@pytest.mark.parametrize("pattern", ["symmetric", "asymmetric", "rabiner_juang"])
@pytest.mark.parametrize("band", [False, True])
def test_dtw(pattern, band):
    ops = o()
    d, n_len, m_len, (B, N, M) = dtw_inputs(band)
    pat = ops.dtw_pattern(pattern)
    for lens, want_cost, want_path in itertools.product((False, True), (False, True), (False, True)):
        nl, ml = (n_len, m_len) if lens else (None, None)
        check_four(lambda: ops.dtw(d, pat, nl, ml, want_cost, want_path),
                   lib().hmm355_dtw_workspace_bytes(B, N, M, 1 if want_path else 0))


@pytest.mark.parametrize("band", [False, True])
def test_soft_dtw(band):
    ops = o()
    d, n_len, m_len, _ = dtw_inputs(band)
    for nl, ml in ((None, None), (n_len, m_len)):
        R, total = check_four(lambda: ops.soft_dtw(d, 0.5, nl, ml))
        check_four(lambda: ops.soft_dtw_grad(d, R, 0.5, nl, ml))


# ---------------------------------------------------------------------- lattices
def ctc_inputs():
    rng = np.random.default_rng(21)
    T, B, C = 12, 4, 6
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, C)).astype(np.float32)), -1).to(DEV)
    targets = t(np.array([[1, 2, 3], [4, 4, 0], [0, 0, 0], [1, 1, 1]], np.int64))
    il = torch.tensor([12, 9, 5, 2])     # the last pair needs five frames and has two
    tl = torch.tensor([3, 2, 0, 3])      # the third target is empty
    return lp, targets, il, tl, C


def test_ctc():
    ops = o()
    lp, targets, il, tl, C = ctc_inputs()
    T, B = lp.shape[:2]
    for alpha, beta, vit in itertools.product((False, True), repeat=3):
        fl = (ops.CTC_ALPHA if alpha else 0) | (ops.CTC_BETA if beta else 0) | (ops.CTC_VITERBI if vit else 0)
        outs = check_four(lambda: ops.ctc(lp, targets, il, tl, 0, alpha, beta, vit),
                          lib().hmm355_ctc_workspace_bytes(B, T, targets.shape[1], fl))
    loglik, A, Bt = outs[:3]
    assert bool(torch.isneginf(loglik[3])) and bool(torch.isfinite(loglik[:3]).all())
    for want_gamma in (False, True):
        check_four(lambda: ops.ctc_grad(A, Bt, loglik, targets, il, tl, C, 0, want_gamma))


def forced_inputs(variant):
    rng = np.random.default_rng(22)
    B, T, C, S = 3, 9, 7, 3
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)), -1).to(DEV)
    il = torch.tensor([9, 7, 2])         # the last pair has more states than frames
    w = lambda: t(-rng.random((B, S)).astype(np.float32))
    if variant == "ids":
        return lp, t(np.array([[1, 2, 3], [4, 4, 0], [2, 3, 5]], np.int64)), il, torch.tensor([3, 2, 3]), w(), w(), w()
    if variant == "identity":
        return lp, None, il, torch.tensor([7, 5, 3]), None, None, None
    return lp, None, il, torch.tensor([3, 2, 3]), None, w(), None     # identity + weight


@pytest.mark.parametrize("variant", ["ids", "identity", "identity+weight"])
def test_forced(variant):
    import ops_fake_cases as cases
    ops = o()
    lp, ids, il, sl, ws, wn, wk = forced_inputs(variant)
    B, T, C = lp.shape
    S = C if variant == "identity" else 3
    name = "forced" if variant == "ids" else "forced/" + variant
    for on in cases.combos(name):
        sw = {k: k in on for k in cases.SWITCHES[name]}
        fl = ((ops.FORCED_ALPHA if sw["alpha"] else 0) | (ops.FORCED_BETA if sw["beta"] else 0) |
              (ops.FORCED_VITERBI if sw["viterbi"] else 0))
        outs = check_four(lambda: ops.forced(lp, ids, il, sl, ws, wn, wk, **sw),
                          lib().hmm355_forced_workspace_bytes(B, T, S, fl))
    loglik, A, Bt = outs[:3]     # (the last combination has every switch on)
    for on in cases.combos("forced_grad"):
        if ("forced_grad", on) in cases.REFUSED:
            continue
        sw = {k: k in on for k in cases.SWITCHES["forced_grad"]}
        check_four(lambda: ops.forced_grad(A, Bt, loglik, lp, ids, il, sl, ws, wn, wk, **sw))


def test_durforced():
    import ops_fake_cases as cases
    from pytorch_hmm_amd import _native as nat
    ops = o()
    rng = np.random.default_rng(23)
    B, T, C, Lm, Dm = 3, 9, 7, 3, 4
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)), -1).to(DEV)
    ids = t(np.array([[1, 2, 3], [4, 4, 0], [2, 3, 5]], np.int64))
    il, sl = torch.tensor([9, 7, 2]), torch.tensor([3, 2, 3])     # the last pair is infeasible
    du = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, Lm, Dm)).astype(np.float32)), -1).to(DEV)
    for tables, vit in itertools.product((False, True), repeat=2):
        fl = (nat.DURFORCED_TABLES if tables else 0) | (nat.DURFORCED_VITERBI if vit else 0)
        outs = check_four(lambda: ops.durforced(lp, ids, il, sl, du, tables=tables, viterbi=vit),
                          lib().hmm355_durforced_workspace_bytes(B, T, Lm, Dm, fl))
    assert bool(torch.isneginf(outs[0][2]))
    tabs = outs[1:7]
    for on in cases.combos("durforced_grad"):
        if ("durforced_grad", on) in cases.REFUSED:
            continue
        sw = {k: k in on for k in cases.SWITCHES["durforced_grad"]}
        check_four(lambda: ops.durforced_grad(*tabs, lp, ids, il, sl, du, **sw))


@pytest.mark.parametrize("want_trellis", [False, True])
@pytest.mark.parametrize("per_sequence", [False, True])
def test_duration_constrained_viterbi(want_trellis, per_sequence):
    ops = o()
    B, T, S = 3, 40, 7
    e = t(log_emissions(B, T, S, 24))
    lT = dense_model(S, 25)[0]
    check_four(lambda: ops.duration_constrained_viterbi(e, lT, 2, 6, 0.1, per_sequence, want_trellis),
               lib().hmm355_dchmm_workspace_bytes(B, T, S))


# ------------------------------------------------------------------ posterior sampling
def test_ffbs_and_posterior_sample():
    ops = o()
    B, T, N, K = 3, 33, 7, 3
    lens = ragged_lengths(T)
    rng = np.random.default_rng(26)
    lP, lp0 = dense_model(N, 27)
    buf = rng.random((B, T, 64)).astype(np.float32) + 0.01
    for b in range(B):
        buf[b, int(lens[b]):] = np.nan
    fwd = t(buf)[..., :N]                 # a row stride above N
    u = t(rng.random((B, K, T)).astype(np.float32))
    (states,) = check_four(lambda: ops.ffbs(fwd, lP, u, torch.from_numpy(lens)), lib().hmm355_ffbs_workspace_bytes(N))
    assert bool((states[1, :, 1:] == -1).all())
    x = t(log_emissions(B, T, N, 28, lens))
    check_four(lambda: ops.posterior_sample(x, lP, lp0, ops.OBS_LOG, K, uniforms=u, lengths=lens),
               lib().hmm355_fb_workspace_bytes(B, T, N))


# ------------------------------------------------------------------------ GMM emission
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_gmm_diag_logprob(C):
    ops = o()
    rng = np.random.default_rng(C)
    B, T, D, S = 3, 21, 13, 6
    x = t(rng.standard_normal((B, T, D)).astype(np.float32))
    means = t((0.3 * rng.standard_normal((S, C, D))).astype(np.float32))
    lv = t((0.2 * rng.standard_normal((S, C, D))).astype(np.float32))
    lw = t(np.log(rng.dirichlet(np.ones(C), size=S)).astype(np.float32))
    for mix_lse in ((0, 1) if C == 1 else (1,)):
        check_four(lambda: ops.gmm_diag_logprob(x, means, lv, lw, mix_lse), lib().hmm355_gmm_workspace_bytes(B, T, D, S, C))


def test_gmm_stats():
    ops = o()
    rng = np.random.default_rng(29)
    B, T, D, S, C = 3, 21, 13, 6, 2
    lens = ragged_lengths(T)
    xs = rng.standard_normal((B, T, D)).astype(np.float32)
    wt = rng.random((B, T, S)).astype(np.float32)
    for b in range(B):
        xs[b, int(lens[b]):] = np.nan
        wt[b, int(lens[b]):] = np.nan
    means = t((0.3 * rng.standard_normal((S, C, D))).astype(np.float32))
    lv = t((0.2 * rng.standard_normal((S, C, D))).astype(np.float32))
    lw = t(np.log(rng.dirichlet(np.ones(C), size=S)).astype(np.float32))
    check_four(lambda: ops.gmm_stats(t(xs), t(wt), means, lv, lw, 1, torch.from_numpy(lens)),
               lib().hmm355_gmm_stats_workspace_bytes(B, T, D, S, C))


# --------------------------------------------------------------------------- backward
def gradients(fn, *leaves):
    """call() for check_four: the gradients of a fixed weighting of fn's outputs in fresh leaves"""
    def call():
        xs = [x.detach().clone().requires_grad_(True) for x in leaves]
        outs = fn(*xs)
        outs = outs if isinstance(outs, (tuple, list)) else (outs,)
        loss = 0
        for i, y in enumerate(y for y in outs if y is not None and y.numel() and y.requires_grad):
            wgt = torch.linspace(0.5, 1.5, y.numel(), device=y.device).reshape(y.shape) * (i + 1)
            loss = loss + (torch.where(torch.isfinite(y), y, torch.zeros_like(y)) * wgt).sum()
        loss.backward()
        return tuple(x.grad for x in xs)
    return call


def check_gradients(fn, *leaves):
    grads = check_four(gradients(fn, *leaves), guard=False)
    assert all(g is not None for g in grads)
    return grads


@pytest.mark.parametrize("kind", ["ref", "exact"])
def test_backward_sequence_loglik(kind):
    from pytorch_hmm_amd.autograd import SequenceLogLik
    ops = o()
    B, T, N = 3, 33, 7
    lens = ragged_lengths(T)
    lP, lp0 = dense_model(N, 30)
    x = torch.nan_to_num(t(log_emissions(B, T, N, 31)))
    host = ops.ragged_lengths(lens, B, T, N)
    check_gradients(lambda a, b, c: SequenceLogLik.apply(a, b, c, ops.OBS_LOG, kind, None, host), x, lP, lp0)


def test_backward_tv_sequence_loglik():
    from pytorch_hmm_amd.autograd import TvSequenceLogLik
    B, T, N = 3, 9, 5
    A = t(np.log(np.random.default_rng(32).dirichlet(np.ones(N), size=(B, T, N)) + 1e-8).astype(np.float32))
    x, lp0 = t(log_emissions(B, T, N, 33)), dense_model(N, 34)[1]
    check_gradients(lambda a, b, c: TvSequenceLogLik.apply(a, b, c, "exact"), x, A, lp0)


def test_backward_forward_backward_fns():
    from pytorch_hmm_amd import autograd as ag
    ops = o()
    B, T, N = 3, 9, 7
    lP, lp0 = dense_model(N, 35)
    x = t(log_emissions(B, T, N, 36))
    check_gradients(lambda a, b, c: ag.forward_backward_with_grad(a, b, c, ops.OBS_LOG, 7), x, lP, lp0)
    A = t(np.log(np.random.default_rng(37).dirichlet(np.ones(N), size=(B, T, N)) + 1e-8).astype(np.float32))
    check_gradients(lambda a, b, c: ag.tv_forward_backward_with_grad(a, b, c, 7), x, A, lp0)


def test_backward_gmm_logprob():
    from pytorch_hmm_amd.autograd import GmmLogProb
    rng = np.random.default_rng(38)
    B, T, D, S, C = 3, 21, 13, 6, 2
    x = t(rng.standard_normal((B, T, D)).astype(np.float32))
    means = t((0.3 * rng.standard_normal((S, C, D))).astype(np.float32))
    lv = t((0.2 * rng.standard_normal((S, C, D))).astype(np.float32))
    lw = t(np.log(rng.dirichlet(np.ones(C), size=S)).astype(np.float32))
    check_gradients(lambda a, b, c, d: GmmLogProb.apply(a, b, c, d, 1), x, means, lv, lw)


def test_backward_viterbi_score():
    from pytorch_hmm_amd.autograd import ViterbiScore
    B, T, N = 3, 33, 7
    lP, lp0 = dense_model(N, 39)
    check_gradients(lambda a, b, c: ViterbiScore.apply(a, b, c), t(log_emissions(B, T, N, 40)), lP, lp0)


def test_backward_soft_dtw():
    from pytorch_hmm_amd.autograd import SoftDTW
    d, n_len, m_len, _ = dtw_inputs(False)
    check_gradients(lambda a: SoftDTW.apply(a, 0.5, n_len, m_len), d)


def test_backward_ctc():
    from pytorch_hmm_amd.autograd import CTCLogLik
    lp, targets, il, tl, _ = ctc_inputs()
    check_gradients(lambda a: CTCLogLik.apply(a, targets, il, tl, 0), lp)


def test_backward_forced():
    from pytorch_hmm_amd.autograd import ForcedLogLik
    lp, ids, il, sl, ws, wn, wk = forced_inputs("ids")
    check_gradients(lambda a, b, c, d: ForcedLogLik.apply(a, ids, il, sl, b, c, d), lp, ws, wn, wk)


def test_backward_durforced():
    from pytorch_hmm_amd.autograd import DurForcedLogLik
    rng = np.random.default_rng(41)
    B, T, C, Lm, Dm = 3, 9, 7, 3, 4
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32)), -1).to(DEV)
    ids = t(np.array([[1, 2, 3], [4, 4, 0], [2, 3, 5]], np.int64))
    il, sl = torch.tensor([9, 7, 2]), torch.tensor([3, 2, 3])
    du = torch.log_softmax(torch.from_numpy(rng.standard_normal((B, Lm, Dm)).astype(np.float32)), -1).to(DEV)
    check_gradients(lambda a, b: DurForcedLogLik.apply(a, ids, il, sl, b), lp, du)


def test_backward_hsmm():
    from pytorch_hmm_amd.autograd import HsmmLogLik
    import test_gpu_hsmm_fb as H
    lp, du, lt, li = (t(a) for a in H.random_tables(3, 23, 5, 7, 18))
    check_gradients(lambda a, b, c, d: HsmmLogLik.apply(a, b, c, d), lp, du, lt, li)


def test_backward_sparse():
    from pytorch_hmm_amd.autograd import SparseLogLik
    ops = o()
    c = SUM_CASES["rand-N65-T70-B3"]
    tr, obs, p0, lens, _ = sparse_on_gpu(c)
    host = ops.ragged_lengths(lens, c["B"], c["T"])
    obs = torch.nan_to_num(obs)      # (the gradient's leaf; the padded frames are still never read)
    check_gradients(lambda a, b, d: SparseLogLik.apply(a, b, d, tr, host), obs, tr.log_w.detach(), p0)


# ------------------------------------------------------------------------- range guard
def test_range_guard_fallback():
    """A class B case (a sequence outside the kernels' fp32 range) with lengths: the E-step's
    float64 log-space fallback allocates its own table with torch.empty."""
    from pytorch_hmm_amd import em
    c = next(x for x in rc.b_cases() if x["name"] == "B-batch")
    T = c["T"]
    lens = np.array([T, T, T - 3, T], np.int64)
    obs = c["log_obs"].copy()
    obs[2, T - 3:] = np.nan
    x, lP, lp0 = t(obs), t(c["log_P"]), t(c["log_p0"])

    def call():
        s = em.e_step(x, lP, lp0, lengths=lens)
        return s.loglik, s.gamma, s.xi, s.gamma0
    ll, *_ = check_four(call, lib().hmm355_fb_workspace_bytes(c["B"], T, c["N"]), guard=False)
    assert bool(torch.isfinite(ll[rc.BATCH_OUT])) and bool(torch.isneginf(ll[rc.BATCH_INFEASIBLE]))
