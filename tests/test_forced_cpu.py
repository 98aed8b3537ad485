"""CPU: transcript forced alignment without a device.

  * The numpy restatements in tests/forced_numpy.py (the GPU tests' oracle) agree with brute-force
    enumeration of every path of small lattices (T <= 7, S <= 5, with and without skips): loglik,
    the best path and its score, gamma and the transition gradients as path-posterior counts.
  * Pairs with no path give -inf and zeros; the gradient invariants hold (every frame of the
    log_probs gradient sums to 1, the three transition gradients together to T_b - 1).
  * The C ABI (include/hmm355.h, csrc/forced.hip) declares and exports the entry points, reports
    version >= 8 and rejects bad arguments with the documented codes before any launch.
  * The Python layer raises ValueError on bad lengths and shapes, refuses CPU tensors by name,
    and ForcedAligner.expand lays the token states out as documented.
"""
import ctypes
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forced_numpy as fz  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")


# ----------------------------------------------------------------- brute-force enumeration
def all_paths(T, S, skips):
    """Every path of T frames from position 0 to S - 1 with steps 0, 1 (and 2)."""
    out = []
    for steps in itertools.product((0, 1, 2) if skips else (0, 1), repeat=T - 1):
        if sum(steps) == S - 1:
            out.append(np.concatenate([[0], np.cumsum(steps)]).astype(np.int64))
    return out if (T > 1 or S == 1) else []


def enumerate_lattice(e, ws, wn, wk, skips):
    """(loglik, gamma (T,S), counts (3,S), best path or None, best score) over every path, fp64"""
    T, S = e.shape
    W = (ws, wn, wk)
    paths, lw = all_paths(T, S, skips), []
    for p in paths:
        v = e[np.arange(T), p].sum()
        for t in range(1, T):
            d = p[t] - p[t - 1]
            v = v + W[d][p[t - 1]]
        lw.append(v)
    lw = np.array(lw, dtype=np.float64)
    gamma, counts = np.zeros((T, S)), np.zeros((3, S))
    if len(lw) == 0 or not np.isfinite(lw.max()):
        return -np.inf, gamma, counts, None, -np.inf
    ll = lw.max() + np.log(np.exp(lw - lw.max()).sum())
    for p, v in zip(paths, lw):
        pr = np.exp(v - ll)
        gamma[np.arange(T), p] += pr
        for t in range(1, T):
            counts[p[t] - p[t - 1], p[t - 1]] += pr
    return ll, gamma, counts, paths[int(lw.argmax())], lw.max()


PAIRS = [(6, 4), (4, 4), (7, 5), (5, 1), (1, 1), (3, 5), (7, 3), (2, 3)]     # (T_b, S_b); (3, 5) needs skips


def small_batch(skips, seed, weights=True):
    rng = np.random.default_rng(seed)
    B, T, Smax, C = len(PAIRS), 7, 5, 4
    lp = rng.standard_normal((B, T, C)).astype(np.float32) - 1
    ids = rng.integers(0, C, (B, Smax)).astype(np.int32)
    il = np.array([p[0] for p in PAIRS])
    sl = np.array([p[1] for p in PAIRS])
    w = [(0.5 * rng.standard_normal((B, Smax)) - 0.5).astype(np.float32) for _ in range(3)] if weights else [None] * 3
    if not skips:
        w[2] = None
    return lp, ids, il, sl, w[0], w[1], w[2]


@pytest.mark.parametrize("skips", [False, True])
@pytest.mark.parametrize("weights", [False, True])
def test_restatement_equals_enumeration(skips, weights):
    case = small_batch(skips, 5 + skips, weights)
    lp, ids, il, sl, ws, wn, wk = case
    B, T, C = lp.shape
    A, ll = fz.alpha(*case, dtype=np.float64)
    gamma, grad, gs, gn, gk = fz.occupancy(*case)
    path, score, dur = fz.viterbi(*case)
    W = fz.weights_of(5, B, ws, wn, wk, np.float64)
    feasible = 0
    for b in range(B):
        Tb, Sb = int(il[b]), int(sl[b])
        e = fz.emissions(lp, ids, b, Sb, np.float64)[:Tb]
        want_ll, want_gamma, want_counts, want_path, want_score = enumerate_lattice(
            e, W[0][b], W[1][b], W[2][b], skips and wk is not None)
        if want_path is None:
            assert np.isneginf(ll[b]) and np.isneginf(score[b])
            assert (path[b] == -1).all() and (dur[b] == 0).all()
            assert (gamma[b] == 0).all() and (grad[b] == 0).all()
            assert (gs[b] == 0).all() and (gn[b] == 0).all() and (gk[b] == 0).all()
            continue
        feasible += 1
        assert abs(ll[b] - want_ll) <= 1e-12 * max(1.0, abs(want_ll))
        assert np.abs(gamma[b, :Tb, :Sb] - want_gamma).max() <= 1e-12
        assert (gamma[b, Tb:] == 0).all() and (gamma[b, :, Sb:] == 0).all()
        for got, want in zip((gs, gn, gk), want_counts):
            assert np.abs(got[b, :Sb] - want).max() <= 1e-12 and (got[b, Sb:] == 0).all()
        # the best path: a valid path whose own weight is the enumeration's maximum (positions of
        # one class tie exactly, so the path itself is compared only where the maximum is unique)
        p = path[b, :Tb].astype(np.int64)
        assert (path[b, Tb:] == -1).all() and p[0] == 0 and p[-1] == Sb - 1
        steps = np.diff(p)
        assert (steps >= 0).all() and (steps <= (2 if skips and wk is not None else 1)).all()
        own = e[np.arange(Tb), p].sum() + sum(W[dd][b, s] for s, dd in zip(p[:-1], steps))
        tol = 4 * Tb * fz.EPS24 * max(1.0, abs(want_score))
        assert abs(own - want_score) <= tol and abs(float(score[b]) - want_score) <= tol
        if len({int(x) for x in ids[b, :Sb]}) == Sb:
            assert np.array_equal(p, want_path)
        assert np.array_equal(dur[b, :Sb], np.bincount(p, minlength=Sb)) and (dur[b, Sb:] == 0).all()
        # the invariants of a feasible pair
        assert np.abs(grad[b, :Tb].sum(1) - 1).max() <= 1e-12 and (grad[b, Tb:] == 0).all()
        assert abs(gs[b].sum() + gn[b].sum() + gk[b].sum() - (Tb - 1)) <= 1e-12 * max(1, Tb)
    assert feasible == (len(PAIRS) if skips and wk is not None else len(PAIRS) - 2)
    assert np.isneginf(ll[PAIRS.index((2, 3))]) or (skips and wk is not None)


def test_beta_closes_the_lattice_and_fp32_stays_in_bound():
    """alpha + beta sums to loglik in every frame; the fp32 restatement obeys the step bound."""
    case = small_batch(True, 9)
    lp, ids, il, sl = case[:4]
    B, T, _ = lp.shape
    A, ll = fz.alpha(*case, dtype=np.float64)
    Bt = fz.beta(*case, dtype=np.float64)
    for b in range(B):
        if not np.isfinite(ll[b]):
            continue
        for t in range(int(il[b])):
            with np.errstate(all="ignore"):
                tot = A[b, t] + Bt[b, t]
            tot = tot[np.isfinite(tot)]
            assert abs(tot.max() + np.log(np.exp(tot - tot.max()).sum()) - ll[b]) <= 1e-12 * max(1, abs(ll[b]))
    A32, ll32 = fz.alpha(*case)
    assert A32.dtype == np.float32
    assert fz.step_bound_excess(A32, A, fz.alpha_steps(T, B)) <= 1
    assert fz.step_bound_excess(fz.beta(*case), Bt, fz.beta_steps(T, il)) <= 1
    assert fz.step_bound_excess(ll32, ll, il) <= 1


def test_ids_outside_the_classes_and_neginf_inputs():
    lp, ids, il, sl, ws, wn, wk = small_batch(True, 3)
    ids = ids.copy()
    ids[0, 1] = 99          # the only way from 0 to 2 is then the skip
    ids[1, 1] = ids[1, 2] = -4   # neither the step nor the skip out of position 0 can emit: no path
    lp = lp.copy()
    lp[2, 3, :] = -np.inf   # a frame no class can emit
    wn = wn.copy()
    wn[6, 0] = -np.inf      # (7, 3): leave position 0 by the skip alone
    case = (lp, ids, il, sl, ws, wn, wk)
    A, ll = fz.alpha(*case, dtype=np.float64)
    gamma, grad, gs, gn, gk = fz.occupancy(*case)
    path, score, dur = fz.viterbi(*case)
    assert np.isfinite(ll[0]) and (gamma[0, :, 1] == 0).all() and 1 not in path[0]
    assert np.isneginf(ll[1]) and np.isneginf(ll[2]) and (path[1] == -1).all() and (grad[2] == 0).all()
    assert np.isfinite(ll[6]) and gn[6, 0] == 0 and abs(gk[6, 0] - 1) <= 1e-12 and dur[6, 1] == 0
    assert not np.isnan(gamma).any() and not np.isnan(grad).any()


def test_identity_ids_are_the_columns():
    rng = np.random.default_rng(1)
    value = rng.standard_normal((2, 6, 4)).astype(np.float32)
    il, sl = np.array([6, 5]), np.array([4, 3])
    ids = np.tile(np.arange(4, dtype=np.int32), (2, 1))
    for fn in (fz.alpha, fz.viterbi):
        for a, b in zip(fn(value, None, il, sl), fn(value, ids, il, sl)):
            assert np.array_equal(a, b)


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
SYMBOLS = ("hmm355_forced_workspace_bytes", "hmm355_forced_f32", "hmm355_forced_grad_f32")


def fwd(L, lp=FAKE, ids=FAKE, il=FAKE, sl=FAKE, ws=None, wn=None, wk=None, B=2, T=20, C=5, Smax=4, flags=7,
        alpha=FAKE, beta=FAKE, loglik=FAKE, path=FAKE, score=FAKE, dur=FAKE, wsp=FAKE, nbytes=BIG):
    return L.hmm355_forced_f32(lp, ids, il, sl, ws, wn, wk, B, T, C, Smax, flags, alpha, beta, loglik, path, score,
                               dur, wsp, nbytes, None)


def grd(L, alpha=FAKE, beta=FAKE, loglik=FAKE, ids=FAKE, il=FAKE, sl=FAKE, ws=None, wn=None, wk=None, B=2,
        T=20, C=5, Smax=4, gamma=None, grad=FAKE, gs=None, gn=None, gk=None, wsp=FAKE, nbytes=BIG):
    return L.hmm355_forced_grad_f32(alpha, beta, loglik, ids, il, sl, ws, wn, wk, B, T, C, Smax, gamma, grad, gs, gn,
                                    gk, wsp, nbytes, None)


def test_header_exports_and_version(L, d):
    from pytorch_hmm_amd import _native as nat
    from pytorch_hmm_amd import build_native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hmm355_[a-z0-9_]+)\s*\(", src))
    for name in SYMBOLS:
        assert name in declared and name in nat.EXPORTS and hasattr(L, name)
    assert declared == set(nat.EXPORTS)
    assert L.hmm355_version() >= 8
    assert (d["HMM355_FORCED_ALPHA"], d["HMM355_FORCED_BETA"], d["HMM355_FORCED_VITERBI"]) == \
        (nat.FORCED_ALPHA, nat.FORCED_BETA, nat.FORCED_VITERBI) == (1, 2, 4)
    assert d["HMM355_FORCED_GRAD"] == nat.FORCED_GRAD == 8
    assert d["HMM355_FORCED_MAX_POSITIONS"] == nat.FORCED_MAX_POSITIONS == 4096
    assert "forced.hip" in build_native.SOURCES
    assert "forced" in L.hmm355_strerror(d["HMM355_E_STATES"]).decode()
    src = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "forced.hip")).read()
    threads = int(re.search(r"constexpr int kForcedThreads = (\d+);", src).group(1))
    wide = int(re.search(r"constexpr int kForcedPosWide = (\d+);", src).group(1))
    assert threads * wide >= nat.FORCED_MAX_POSITIONS     # the widest form covers the ABI's limit


@pytest.mark.parametrize("call", [fwd, grd])
def test_argument_checks(L, d, call):
    ARG, STATES, SHAPE = d["HMM355_E_ARG"], d["HMM355_E_STATES"], d["HMM355_E_SHAPE"]
    for dim in ("T", "B", "C"):
        assert call(L, **{dim: 0}) == ARG and call(L, **{dim: -3}) == ARG
    assert call(L, Smax=0) == STATES and call(L, Smax=4097) == STATES and call(L, Smax=-1) == STATES
    for ptr in ("il", "sl", "loglik"):
        assert call(L, **{ptr: None}) == ARG
    assert call(L, ids=None, C=3, Smax=4) == ARG           # the identity chain needs C >= Smax
    assert call(L, T=1 << 30, B=1 << 30) == SHAPE


def test_forward_argument_checks(L, d):
    ARG = d["HMM355_E_ARG"]
    assert fwd(L, lp=None) == ARG
    assert fwd(L, flags=8) == ARG                          # HMM355_FORCED_GRAD belongs to the size query
    assert fwd(L, flags=16) == ARG
    assert fwd(L, alpha=None) == ARG                       # each flag needs its outputs
    for out in ("beta", "path", "score", "dur"):
        assert fwd(L, **{out: None}) == ARG
    assert fwd(L, wsp=None) == ARG and fwd(L, wsp=ctypes.c_void_p(0x1004)) == ARG
    need = L.hmm355_forced_workspace_bytes(2, 20, 4, 7)
    assert fwd(L, nbytes=need - 1) == d["HMM355_E_WORKSPACE"]
    assert fwd(L, nbytes=16, flags=0) == d["HMM355_E_WORKSPACE"]


def test_gradient_argument_checks(L, d):
    for ptr in ("alpha", "beta"):
        assert grd(L, **{ptr: None}) == d["HMM355_E_ARG"]
    assert grd(L, grad=None) == d["HMM355_E_ARG"]          # no output at all
    # the transition gradients alone need the workspace
    need = L.hmm355_forced_workspace_bytes(2, 20, 4, d["HMM355_FORCED_GRAD"])
    for out in ("gs", "gn", "gk"):
        assert grd(L, **{out: FAKE}, wsp=None) == d["HMM355_E_ARG"]
        assert grd(L, **{out: FAKE}, wsp=ctypes.c_void_p(0x1004)) == d["HMM355_E_ARG"]
        assert grd(L, **{out: FAKE}, nbytes=need - 1) == d["HMM355_E_WORKSPACE"]


def test_workspace_sizes(L):
    B, T, S = 3, 100, 81
    value_only = L.hmm355_forced_workspace_bytes(B, T, S, 0)
    tables = L.hmm355_forced_workspace_bytes(B, T, S, 3)
    with_path = L.hmm355_forced_workspace_bytes(B, T, S, 7)
    assert 0 < value_only == tables < B * T           # alpha / beta are outputs; no table in the workspace
    assert with_path >= value_only + B * T * S // 4   # 2 bits per cell
    assert L.hmm355_forced_workspace_bytes(B, T, 4096, 4) > 0
    # the gradient call's per-tile transition sums: three fp64 rows per sequence and tile of frames
    grad = L.hmm355_forced_workspace_bytes(B, T, S, 8)
    assert grad >= B * 3 * S * 8 * (T // 64) and grad > value_only
    assert L.hmm355_forced_workspace_bytes(B, T, S, 8 | 4) == max(grad, with_path)
    for bad in ((0, T, S, 0), (B, 0, S, 0), (B, T, 0, 0), (B, T, 4097, 0), (-1, T, S, 0), (B, T, S, 16),
                (1 << 30, 1 << 30, S, 4)):
        assert L.hmm355_forced_workspace_bytes(*bad) == 0


# ------------------------------------------------------------------------------- Python
NAMES = ("ForcedAligner", "forced_align", "forced_alignment_loglik", "forced_alignment_posteriors",
         "monotonic_alignment_search")


def test_import_surface():
    import pytorch_hmm_amd
    import pytorch_hmm_amd.alignment as al
    for name in NAMES:
        assert hasattr(al, name) and name in al.__all__
        assert getattr(pytorch_hmm_amd, name) is getattr(al, name) and name in pytorch_hmm_amd.__all__
    for op in ("forced", "forced_grad"):
        assert hasattr(torch.ops.hmm355, op)
    from pytorch_hmm_amd.autograd import ForcedLogLik
    assert "log_stay" in ForcedLogLik.__doc__


def test_cpu_tensors_are_refused_by_name():
    import pytorch_hmm_amd.alignment as al
    from pytorch_hmm_amd import ops
    from pytorch_hmm_amd.autograd import ForcedLogLik
    lp = torch.zeros(2, 6, 4)
    ids = torch.tensor([[0, 1, 2], [3, 3, 0]])
    il, sl = torch.tensor([6, 4]), torch.tensor([3, 2])
    tab = torch.zeros(2, 6, 3)
    aligner = al.ForcedAligner(4)
    for call in (lambda: al.forced_align(lp, ids, il, sl), lambda: al.forced_alignment_loglik(lp, ids, il, sl),
                 lambda: al.forced_alignment_loglik(lp.clone().requires_grad_(), ids, il, sl),
                 lambda: al.forced_alignment_posteriors(lp, ids, il, sl),
                 lambda: al.monotonic_alignment_search(lp, il, sl), lambda: aligner(lp, ids, il, sl),
                 lambda: aligner.align(lp, ids, il, sl), lambda: aligner.posteriors(lp, ids, il, sl),
                 lambda: ops.forced(lp, ids, il, sl), lambda: ops.forced_grad(tab, tab, torch.zeros(2), lp, ids, il, sl),
                 lambda: ForcedLogLik.apply(lp, ids, il, sl)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()


def test_host_side_checks_raise_value_error():
    """_forced_args runs before any launch; exercised directly, as a device is not needed for it."""
    from pytorch_hmm_amd import ops
    ids = torch.tensor([[1, 2, 1], [3, 0, 0]])
    ok = dict(shape=(2, 12, 5), ids=ids, il=torch.tensor([12, 7]), sl=torch.tensor([3, 1]), ws=None, wn=None, wk=None)

    def run(**kw):
        a = dict(ok)
        a.update(kw)
        return ops._forced_args(a["shape"], "cpu", a["ids"], a["il"], a["sl"], a["ws"], a["wn"], a["wk"])
    i32, il, sl, ws, wn, wk, Smax = run()
    assert i32.dtype == il.dtype == sl.dtype == torch.int32 and Smax == 3 and ws is wn is wk is None
    w = torch.zeros(2, 3, dtype=torch.float64)
    assert run(ws=w, wk=w)[3].dtype == torch.float32 and run(ws=w, wk=w)[4] is None
    # the identity chain: as wide as log_probs has classes, or as a weight tensor says
    assert run(ids=None, sl=torch.tensor([5, 1]))[6] == 5 and run(ids=None, wn=w)[6] == 3
    # ids are not checked: one outside [0, C) is an emission of -inf
    run(ids=torch.tensor([[1, 99, 1], [-3, 0, 0]]))
    for bad in (dict(il=torch.tensor([13, 7])), dict(il=torch.tensor([12, 0])), dict(sl=torch.tensor([4, 1])),
                dict(sl=torch.tensor([3, 0])), dict(il=torch.tensor([12])), dict(ids=ids.float()), dict(ids=ids[:1]),
                dict(ids=ids[0]), dict(ws=torch.zeros(2, 4)), dict(wk=torch.zeros(3)), dict(shape=(2, 0, 5)),
                dict(ids=torch.zeros(2, 4097, dtype=torch.long)), dict(ids=None, wn=torch.zeros(2, 6)),
                dict(ids=None, sl=torch.tensor([6, 1]))):
        with pytest.raises(ValueError):
            run(**bad)


def test_forced_aligner_expand_and_weights():
    import pytorch_hmm_amd.alignment as al
    m = al.ForcedAligner(6, states_per_token=3, allow_skip=True)
    assert m.num_classes == 18 and isinstance(m.transition_logits, torch.nn.Parameter)
    assert tuple(m.transition_logits.shape) == (18, 3)
    p = torch.softmax(m.transition_logits, 1)
    assert torch.allclose(p[:, 0], torch.full((18,), 0.7)) and torch.allclose(p.sum(1), torch.ones(18))
    tokens = torch.tensor([[4, 0, 5], [2, 2, 77]])
    ids, sl = m.expand(tokens, torch.tensor([3, 2]))
    assert ids.dtype == sl.dtype == torch.int32 and sl.tolist() == [9, 6]
    assert ids[0].tolist() == [12, 13, 14, 0, 1, 2, 15, 16, 17] and ids[1, :6].tolist() == [6, 7, 8, 6, 7, 8]
    ws, wn, wk = m.transition_weights(ids)
    assert ws.shape == wn.shape == wk.shape == (2, 9) and ws.requires_grad
    assert torch.allclose(ws.exp() + wn.exp() + wk.exp(), torch.ones(2, 9))
    for bad_tokens, bad_len in ((tokens, [3, 3]), (tokens, [0, 2]), (tokens, [4, 2]), (tokens.float(), [3, 2]),
                                (torch.tensor([[1, -1, 0], [0, 0, 0]]), [3, 2]), (tokens[0], [3])):
        with pytest.raises(ValueError):
            m.expand(bad_tokens, torch.tensor(bad_len))
    fixed = al.ForcedAligner(4, learnable_transitions=False, self_loop_prob=0.5)
    assert not list(fixed.parameters()) and tuple(fixed.transition_logits.shape) == (4, 2)
    assert fixed.transition_weights(torch.tensor([[0, 3]]))[2] is None
    with pytest.raises(ValueError):
        al.ForcedAligner(0)
    with pytest.raises(ValueError):
        al.ForcedAligner(3, self_loop_prob=1.0)
    with pytest.raises(ValueError):
        fixed._chain(torch.zeros(1, 5, 3), torch.tensor([[0, 3]]), torch.tensor([2]))
