"""CPU: the sparse-transition HMM (include/hmm355.h hmm355_sparse_*, csrc/sparse.hip,
pytorch_hmm_amd/sparse.py) as far as it can be checked without a device.

  * SparseTransitions: host validation, the two sorted orders and their permutations, the
    from_dense / to_dense round trip; sparse_transition_m_step against numpy.
  * The six entry points are declared, exported and reject bad arguments with the documented
    status codes before anything is launched or dereferenced (fake device pointers, real host
    row-pointer arrays).
  * The three ops have shape-only fakes.
  * tests/sparse_numpy.py (the GPU tests' model) equals the dense model on the densified matrix;
    the tie cases of the GPU tests really tie; at least half of the reference counts of the GPU
    tests' cases lie at or above the floor of their relative bound.
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
import sparse_numpy as sn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")
NEG = -np.inf
NAMES = ("hmm355_sparse_viterbi_workspace_bytes", "hmm355_sparse_viterbi_f32",
         "hmm355_sparse_forward_backward_workspace_bytes", "hmm355_sparse_forward_backward_f32",
         "hmm355_sparse_arc_counts_workspace_bytes", "hmm355_sparse_arc_counts_f32")


# ---------------------------------------------------------------------- SparseTransitions
def test_validation():
    from pytorch_hmm_amd import SparseTransitions
    from pytorch_hmm_amd import sparse
    w = torch.zeros(3)
    SparseTransitions([0, 1, 1], [1, 1, 0], w, 2)                       # self-loops are fine
    SparseTransitions([0], [0], torch.tensor([NEG]), 1)                 # so is -inf, and a single arc
    with pytest.raises(ValueError, match="more than once"):
        SparseTransitions([0, 1, 0], [1, 1, 1], w, 2)
    for src, dst in (([0, 1, 2], [0, 0, 0]), ([0, -1, 1], [0, 0, 0]), ([0, 1, 0], [0, 0, 2])):
        with pytest.raises(ValueError, match=r"\[0, 2\)"):
            SparseTransitions(src, dst, w, 2)
    with pytest.raises(ValueError, match="one entry per arc"):
        SparseTransitions([0, 1], [1, 1, 0], w, 2)
    with pytest.raises(ValueError, match="one entry per arc"):
        SparseTransitions([0, 1, 1], [1, 1, 0], torch.zeros(2), 2)
    with pytest.raises(ValueError, match="integers"):
        SparseTransitions(torch.tensor([0.0, 1.0, 1.0]), [1, 1, 0], w, 2)
    for N in (0, -1, sparse.MAX_STATES + 1):
        with pytest.raises(ValueError, match="num_states"):
            SparseTransitions([0], [0], torch.zeros(1), N)
    SparseTransitions([0], [sparse.MAX_STATES - 1], torch.zeros(1), sparse.MAX_STATES)
    with pytest.raises(ValueError, match="number of arcs"):
        SparseTransitions([], [], torch.zeros(0), 2)
    n = sparse.MAX_ARCS + 1
    ids = torch.arange(n)
    with pytest.raises(ValueError, match="number of arcs"):
        SparseTransitions(ids // 2048, ids % 2048, torch.zeros(n), 2048)
    assert sparse.MAX_STATES == 8192 and sparse.MAX_ARCS == 1 << 20


def test_sort_and_permutations():
    from pytorch_hmm_amd import SparseTransitions
    rng = np.random.default_rng(3)
    for N in (1, 2, 7, 65):
        src, dst = sn.random_graph(N, rng, max_in=5)
        E = src.size
        w = torch.arange(E, dtype=torch.float32)
        tr = SparseTransitions(src, dst, w, N)
        perm_in, in_ptr, perm_out, out_ptr = sn.sort_arcs(src, dst, N)
        assert np.array_equal(tr.perm_in.numpy(), perm_in) and np.array_equal(tr.perm_out.numpy(), perm_out)
        assert np.array_equal(tr.in_ptr_host.numpy(), in_ptr) and np.array_equal(tr.out_ptr_host.numpy(), out_ptr)
        assert tr.in_ptr_host.dtype == torch.int32 and tr.in_src.dtype == torch.int32
        # destination order: dst non-decreasing, src ascending within a destination; and the reverse
        s, d = tr.in_src.numpy().astype(np.int64), tr.in_dst.numpy().astype(np.int64)
        assert np.all(np.diff(d * N + s) > 0)
        s, d = tr.out_src.numpy().astype(np.int64), tr.out_dst.numpy().astype(np.int64)
        assert np.all(np.diff(s * N + d) > 0)
        for j in range(N):
            assert np.all(tr.in_dst.numpy()[in_ptr[j]:in_ptr[j + 1]] == j)
            assert np.all(tr.out_src.numpy()[out_ptr[j]:out_ptr[j + 1]] == j)
        # the permutations lead back to the caller's order
        assert np.array_equal(tr.in_src.numpy(), src[tr.perm_in.numpy()])
        assert torch.equal(w[tr.perm_in][tr.inv_in], w) and torch.equal(w[tr.perm_out][tr.inv_out], w)
        assert tr.max_in_degree() == int(np.diff(in_ptr).max())
        assert tr.max_out_degree() == int(np.diff(out_ptr).max())
        assert np.array_equal(tr.to("cpu").in_src.numpy(), tr.in_src.numpy())


def test_dense_round_trip():
    from pytorch_hmm_amd import SparseHMM, SparseTransitions
    rng = np.random.default_rng(4)
    P = rng.standard_normal((9, 9)).astype(np.float32)
    P[rng.random((9, 9)) < 0.6] = NEG
    P[0, 0] = 0.5
    tr = SparseTransitions.from_dense(torch.from_numpy(P))
    assert tr.num_arcs == int(np.isfinite(P).sum())
    assert np.array_equal(tr.to_dense().numpy(), P)
    assert np.array_equal(sn.densify(tr.src.numpy(), tr.dst.numpy(), tr.log_w.numpy(), 9, np.float32), P)
    # other weights on the same graph, and the module's view
    w2 = torch.arange(tr.num_arcs, dtype=torch.float32)
    D = tr.to_dense(w2)
    assert torch.equal(D[tr.src.long(), tr.dst.long()], w2) and int(torch.isfinite(D).sum()) == tr.num_arcs
    hmm = SparseHMM.from_dense(torch.from_numpy(P))
    assert np.array_equal(hmm.to_dense().detach().numpy(), P)
    assert isinstance(hmm.log_w, torch.nn.Parameter) and hmm.log_p0.shape == (9,)
    frozen = SparseHMM(tr, torch.zeros(9), trainable=False)
    assert not list(frozen.parameters()) and "log_w" in dict(frozen.named_buffers())
    with pytest.raises(ValueError):
        SparseTransitions.from_dense(torch.zeros(3, 4))
    with pytest.raises(ValueError, match="log_p0"):
        SparseHMM(tr, torch.zeros(8))


def test_m_step_against_numpy():
    from pytorch_hmm_amd import sparse_transition_m_step
    rng = np.random.default_rng(5)
    N = 12
    src, dst = sn.random_graph(N, rng, max_in=6)
    E = src.size
    xi = rng.random(E)
    xi[rng.random(E) < 0.2] = 0.0
    starved = int(src[0])
    xi[src == starved] = 1e-9            # a source below min_occupancy keeps its weights
    old = rng.standard_normal(E).astype(np.float32)
    got = sparse_transition_m_step(torch.from_numpy(xi), torch.from_numpy(src), torch.from_numpy(old), N, 1e-6)
    tot = np.bincount(src, weights=xi, minlength=N)[src]
    with np.errstate(divide="ignore"):
        want = np.where(tot >= 1e-6, np.log(xi / np.where(tot >= 1e-6, tot, 1.0)), old.astype(np.float64))
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy(), want.astype(np.float32))
    assert np.array_equal(got.numpy()[src == starved], old[src == starved])
    zero = (xi == 0) & (tot >= 1e-6)
    assert zero.any() and np.all(got.numpy()[zero] == NEG)          # exact zeros stay exact
    p = np.bincount(src, weights=np.exp(got.numpy().astype(np.float64)), minlength=N)
    fed = np.bincount(src, weights=xi, minlength=N) >= 1e-6
    assert np.allclose(p[fed], 1.0, atol=1e-6)


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
GOOD = "good"


def host_ptr(N, E, kind=GOOD):
    """A host row-pointer array of N + 1 ints: good (non-decreasing from 0 to E) or broken."""
    p = np.minimum(np.arange(N + 1, dtype=np.int64) * ((E + N - 1) // N), E).astype(np.int32)
    p[N] = E
    if kind == "start":
        p[0] = 1
    elif kind == "end":
        p[N] = E - 1
    elif kind == "order" and N >= 2:
        p[1] = E
        p[2 if N > 2 else 1] = 0 if N > 2 else E + 1
    return p


def vit(L, obs=FAKE, ptr=GOOD, dptr=FAKE, src=FAKE, w=FAKE, init=FAKE, lengths=FAKE, B=2, T=10, N=70, E=200,
        states=FAKE, delta=FAKE, final=FAKE, wsp=FAKE, ws=BIG):
    hp = None if ptr is None else host_ptr(max(N, 1), max(E, 1), ptr).ctypes.data_as(ctypes.c_void_p)
    return L.hmm355_sparse_viterbi_f32(obs, hp, dptr, src, w, init, lengths, B, T, N, E, states, delta, final, wsp, ws,
                                       None)


def fb(L, obs=FAKE, iptr=GOOD, dip=FAKE, isrc=FAKE, iw=FAKE, optr=GOOD, dop=FAKE, odst=FAKE, ow=FAKE, p0=FAKE,
       lengths=FAKE, B=2, T=10, N=70, E=200, loglik=FAKE, post=FAKE, wsp=FAKE, ws=BIG):
    hi = None if iptr is None else host_ptr(max(N, 1), max(E, 1), iptr).ctypes.data_as(ctypes.c_void_p)
    ho = None if optr is None else host_ptr(max(N, 1), max(E, 1), optr).ctypes.data_as(ctypes.c_void_p)
    return L.hmm355_sparse_forward_backward_f32(obs, hi, dip, isrc, iw, ho, dop, odst, ow, p0, lengths, B, T, N, E,
                                                loglik, post, wsp, ws, None)


def cnt(L, obs=FAKE, src=FAKE, dst=FAKE, w=FAKE, weight=FAKE, lengths=FAKE, B=2, T=10, N=70, E=200, fbw=FAKE,
        fbs=BIG, xi=FAKE, wsp=FAKE, ws=BIG):
    return L.hmm355_sparse_arc_counts_f32(obs, src, dst, w, weight, lengths, B, T, N, E, fbw, fbs, xi, wsp, ws, None)


def test_declared_exported_and_version_bumped(L):
    from pytorch_hmm_amd import _native as nat
    from pytorch_hmm_amd import build_native
    header = open(HEADER).read()
    for name in NAMES:
        assert name in nat.EXPORTS and re.search(rf"\b{name}\(", header), name
        assert getattr(L, name).argtypes
    assert L.hmm355_version() >= 14
    assert "sparse.hip" in build_native.SOURCES


def test_limits_match_header(d):
    from pytorch_hmm_amd import _native as nat
    assert d["HMM355_SPARSE_MAX_STATES"] == nat.SPARSE_MAX_STATES == 8192
    assert d["HMM355_SPARSE_MAX_ARCS"] == nat.SPARSE_MAX_ARCS == 1 << 20
    assert "8192" in open(HEADER).read().split("#define HMM355_E_STATES")[1].split("\n")[0]


@pytest.mark.parametrize("call", [vit, fb, cnt], ids=["viterbi", "forward_backward", "arc_counts"])
def test_shape_status_codes(L, d, call):
    assert call(L, B=0) == 0
    for N in (0, -1, 8193):
        assert call(L, N=N) == d["HMM355_E_STATES"], N
    assert call(L, N=8192, E=1 << 20, ws=0) == d["HMM355_E_WORKSPACE"]      # the limits themselves are in range
    for E in (0, -1, (1 << 20) + 1):
        assert call(L, E=E) == d["HMM355_E_SHAPE"], E
    assert call(L, T=0) == d["HMM355_E_SHAPE"]
    assert call(L, B=1 << 30, T=1 << 30) == d["HMM355_E_SHAPE"]
    assert call(L, B=1 << 20, T=1 << 20, N=8192) == d["HMM355_E_SHAPE"]
    assert call(L, B=-1) == d["HMM355_E_ARG"]
    assert call(L, N=0, T=0) == d["HMM355_E_STATES"]     # the states are checked first
    assert call(L, ws=0) == d["HMM355_E_WORKSPACE"]


def test_viterbi_pointer_status_codes(L, d):
    for name in ("obs", "ptr", "dptr", "src", "w", "init", "states", "delta", "wsp"):
        assert vit(L, **{name: None}) == d["HMM355_E_ARG"], name
    for kind in ("start", "end", "order"):
        assert vit(L, ptr=kind) == d["HMM355_E_ARG"], kind
    # lengths and final_score are optional: with them NULL the next check (the workspace) is reached
    assert vit(L, lengths=None, final=None, ws=0) == d["HMM355_E_WORKSPACE"]
    assert vit(L, B=0, obs=None, ptr=None, states=None, wsp=None, ws=0) == 0
    q = L.hmm355_sparse_viterbi_workspace_bytes
    for N in (1, 8, 9, 70, 8192):
        need = q(3, 11, N, 200)
        stride = (N + 7) // 8 * 8
        assert 3 * 11 * stride * 2 <= need < 3 * 11 * stride * 2 + 256     # uint16 pointers: linear
        assert vit(L, B=3, T=11, N=N, ws=need - 1) == d["HMM355_E_WORKSPACE"]


def test_forward_backward_pointer_status_codes(L, d):
    for name in ("obs", "iptr", "dip", "isrc", "iw", "optr", "dop", "odst", "ow", "p0", "loglik", "wsp"):
        assert fb(L, **{name: None}) == d["HMM355_E_ARG"], name
    for kind in ("start", "end", "order"):
        assert fb(L, iptr=kind) == d["HMM355_E_ARG"], kind
        assert fb(L, optr=kind) == d["HMM355_E_ARG"], kind
    assert fb(L, lengths=None, post=None, ws=0) == d["HMM355_E_WORKSPACE"]
    q = L.hmm355_sparse_forward_backward_workspace_bytes
    need = q(3, 11, 70, 200)
    assert need >= 2 * 3 * 11 * 70 * 4 + 4 * 3 * 11 * 4 + 2 * 200 * 4     # U, V, four per-frame rows, A twice
    assert fb(L, B=3, T=11, ws=need - 1) == d["HMM355_E_WORKSPACE"]


def test_arc_counts_pointer_status_codes(L, d):
    for name in ("obs", "src", "dst", "w", "fbw", "xi", "wsp"):
        assert cnt(L, **{name: None}) == d["HMM355_E_ARG"], name
    assert cnt(L, weight=None, lengths=None, ws=0) == d["HMM355_E_WORKSPACE"]
    assert cnt(L, fbs=0) == d["HMM355_E_WORKSPACE"]                         # the forward-backward rows
    need = L.hmm355_sparse_arc_counts_workspace_bytes(2, 10, 70, 200)
    assert need >= 200 * 8 and cnt(L, ws=need - 1) == d["HMM355_E_WORKSPACE"]


def test_size_queries_reject(L):
    for name in NAMES[0::2]:
        q = getattr(L, name)
        assert q(2, 10, 70, 200) > 0
        for bad in ((2, 10, 0, 200), (2, 10, 8193, 200), (2, 10, 70, 0), (2, 10, 70, (1 << 20) + 1), (2, 0, 70, 200),
                    (-1, 10, 70, 200), (1 << 30, 1 << 30, 70, 200)):
            assert q(*bad) == 0, (name, bad)


# --------------------------------------------------------------------------------- ops
def test_fake_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from pytorch_hmm_amd import _native as nat
    from pytorch_hmm_amd import ops  # noqa: F401  (registers the ops)
    B, T, N, E = 3, 9, 70, 200
    need = nat.lib().hmm355_sparse_forward_backward_workspace_bytes(B, T, N, E)
    with FakeTensorMode():
        i32 = dict(dtype=torch.int32)
        ptr, ids = torch.empty(N + 1, **i32), torch.empty(E, **i32)
        # the real ops convert fp64 / fp16 inputs and always allocate these dtypes
        for dtype in (torch.float32, torch.float64, torch.float16):
            for lens in (None, torch.empty(B, dtype=torch.int64)):
                obs, w, p0 = torch.empty(B, T, N, dtype=dtype), torch.empty(E, dtype=dtype), torch.empty(N, dtype=dtype)
                states, delta, final = torch.ops.hmm355.sparse_viterbi(obs, ptr, ptr, ids, w, p0, lens)
                assert states.shape == (B, T) and states.dtype == torch.int64
                assert delta.shape == (B, T, N) and delta.dtype == torch.float32
                assert final.shape == (B,) and final.dtype == torch.float32
                for want in (True, False):
                    ll, post, ws = torch.ops.hmm355.sparse_forward_backward(obs, ptr, ptr, ids, w, ptr, ptr, ids, w,
                                                                            p0, want, lens)
                    assert ll.shape == (B,) and ll.dtype == torch.float32
                    assert post.shape == ((B, T, N) if want else (0,)) and post.dtype == torch.float32
                    assert ws.shape == (need,) and ws.dtype == torch.uint8
                xi = torch.ops.hmm355.sparse_arc_counts(obs, ids, ids, w, ws, torch.empty(B, dtype=dtype), lens)
                assert xi.shape == (E,) and xi.dtype == torch.float64


def test_ops_are_registered_inside_a_function_and_documented():
    from pytorch_hmm_amd import ops
    for name in ("sparse_viterbi", "sparse_forward_backward", "sparse_arc_counts"):
        assert not isinstance(getattr(ops, name), torch.library.CustomOpDef)
        assert name in ops.__doc__ and hasattr(torch.ops.hmm355, name)
    s, dl, f = ops._sparse_viterbi_outputs(torch.empty, 2, 7, 4)
    assert s.shape == (2, 7) and dl.shape == (2, 7, 4) and f.shape == (2,)


def test_host_value_errors_and_cpu_refusal():
    import pytorch_hmm_amd as ph
    src, dst = sn.lr_skip(7)
    hmm = ph.SparseHMM(ph.SparseTransitions(src, dst, torch.zeros(src.size), 7))
    obs = torch.zeros(2, 5, 7)
    with pytest.raises(ValueError, match=r"\[1, 5\]"):
        hmm.viterbi_decode(obs, lengths=[1, 6])
    with pytest.raises(ValueError, match="log_obs has 8"):
        hmm.viterbi_decode(torch.zeros(2, 5, 8))
    for fn in (hmm.viterbi_decode, hmm.forward_backward, hmm.posteriors, hmm.log_likelihood, hmm.e_step,
               hmm.reestimate):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(obs)
    # lengths above 256 states are not refused here (ops.ragged_lengths is called without N)
    big = ph.SparseHMM(ph.SparseTransitions(*sn.lr_skip(300), torch.zeros(3 * 300 - 3), 300))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        big.viterbi_decode(torch.zeros(2, 5, 300), lengths=[5, 2])


# --------------------------------------------------------------------------- the model
def small_cases():
    return [c for c in sn.viterbi_cases() if c["N"] <= 65 and c["T"] <= 70]


def test_model_equals_dense_model():
    """The arc model against the dense model already in tests/ on the densified matrix: Viterbi
    bit for bit in fp32 (the oracle's restatement of the reference), the likelihood and the
    posterior against the fp64 C oracle and a plain log-sum-exp recursion."""
    n = 0
    for c in small_cases():
        if c["N"] > 64 and not c["name"].startswith(("complete", "ties-complete")):
            continue
        lens = np.full(c["B"], c["T"]) if c["lengths"] is None else c["lengths"]
        P32 = sn.densify(c["src"], c["dst"], c["log_w"], c["N"], np.float32)
        v = sn.viterbi(*sn.model_args(c))
        obs = np.nan_to_num(c["log_obs"], nan=0.0, neginf=NEG)
        states, delta, final = rm.viterbi_from_log(obs, P32, c["log_p0"], lens)
        assert np.array_equal(v["states"], states.numpy()), c["name"]
        assert np.array_equal(v["log_delta"], delta.numpy()), c["name"]
        assert np.array_equal(v["final_score"], final.numpy()), c["name"]
        if sn.is_tie_case(c):
            continue
        s = sn.sums(*sn.model_args(c), weight=c["weight"])
        ll = sn.dense_loglik(obs, P32.astype(np.float64), c["log_p0"], lens)
        fin = np.isfinite(ll)
        assert np.array_equal(fin, np.isfinite(s["loglik"])), c["name"]
        assert np.allclose(s["loglik"][fin], ll[fin], rtol=1e-10, atol=1e-9), c["name"]
        for b in range(c["B"]):
            if fin[b] and np.isfinite(obs[b, :lens[b]]).all() and np.isfinite(c["log_p0"]).all():
                _, _, post, l64 = rm.fb64(obs[b:b + 1], P32, c["log_p0"], lens[b:b + 1])
                assert np.allclose(s["gamma"][b], post[0], atol=1e-9), c["name"]
                assert abs(l64[0] - s["loglik"][b]) < 1e-8 * max(1.0, abs(l64[0]))
                n += 1
    assert n >= 10


def test_model_counts_and_identities():
    """xi of the model is the dense model's pair posterior on the arcs (brute force at tiny N),
    every valid frame's gamma sums to 1, the counts sum to sum_b g_b (len_b - 1) over the feasible
    sequences, and an infeasible sequence gives -inf and zeros."""
    rng = np.random.default_rng(11)
    N, T, B = 4, 5, 3
    src, dst = sn.random_graph(N, rng, max_in=3)
    c = sn._case("tiny", N, T, B, (src, dst), rng)       # lengths 5, 1, 3
    g = c["weight"].astype(np.float64)
    s = sn.sums(*sn.model_args(c), weight=g)
    P = sn.densify(src, dst, c["log_w"], N)
    want = np.zeros(src.size)
    for b in range(B):
        Lb = int(c["lengths"][b])
        tot, acc = 0.0, np.zeros(src.size)
        for path in np.ndindex(*([N] * Lb)):
            lp = float(c["log_p0"][path[0]]) + float(c["log_obs"][b, 0, path[0]])
            for t in range(1, Lb):
                lp += P[path[t - 1], path[t]] + float(c["log_obs"][b, t, path[t]])
            p = np.exp(lp)
            tot += p
            for t in range(1, Lb):
                acc[(src == path[t - 1]) & (dst == path[t])] += p
        want += g[b] * acc / tot
        assert abs(np.log(tot) - s["loglik"][b]) < 1e-10
    assert np.allclose(s["xi"], want, atol=1e-12)
    for c in sn.sum_cases():
        if c["N"] > 65:
            continue
        s = sn.sums(*sn.model_args(c), weight=c["weight"])
        lens = np.full(c["B"], c["T"]) if c["lengths"] is None else c["lengths"]
        fin = np.isfinite(s["loglik"])
        for b in range(c["B"]):
            rows = s["gamma"][b, :lens[b]].sum(1)
            assert np.allclose(rows, 1.0 if fin[b] else 0.0, atol=1e-12), c["name"]
            assert np.all(s["gamma"][b, lens[b]:] == 0)
        assert abs(s["xi"].sum() - (c["weight"] * (lens - 1))[fin].sum()) < 1e-9, c["name"]
        assert np.all(s["xi"][~np.isfinite(c["log_w"])] == 0)


def test_cases_cover_what_they_claim():
    names = [c["name"] for c in sn.viterbi_cases()]
    assert len(names) == len(set(names))
    cases = list(sn.sum_cases())
    assert {c["N"] for c in cases} >= set(sn.SIZES) and {c["B"] for c in cases} == {1, 3}
    assert {c["T"] for c in cases} >= {1, 2, 3, 70} and all(c["T"] <= 4 for c in cases if c["N"] == 8192)
    deg = lambda c: int(np.bincount(c["dst"], minlength=c["N"]).max())
    odeg = lambda c: int(np.bincount(c["src"], minlength=c["N"]).max())
    assert all(deg(c) <= 4 and odeg(c) <= 4 for c in cases if c["name"].startswith("lr-"))        # arcs in registers
    assert any(4 < deg(c) <= 64 for c in cases if c["name"].startswith("rand-"))                   # streamed
    hub = [c for c in cases if c["name"].startswith("hub-")]
    assert hub and all(c["N"] == 320 and deg(c) == 300 and odeg(c) == 300 for c in hub)
    assert any(c["name"].startswith("complete-N65") and deg(c) == 65 for c in cases)
    rand = [c for c in cases if c["name"].startswith("rand-") and c["N"] > 2]
    assert all(np.bincount(c["dst"], minlength=c["N"]).min() == 0 for c in rand)                   # no in-arcs
    assert all(np.bincount(c["src"], minlength=c["N"])[-1] == 0 for c in rand)                     # no out-arcs
    assert any(np.isneginf(c["log_w"]).any() for c in rand) and any(np.isneginf(c["log_p0"]).any() for c in rand)
    assert any(np.isneginf(c["log_obs"][2, 1]).all() for c in rand if c["T"] >= 3)
    assert any(c["lengths"] is not None and 1 in c["lengths"] for c in cases)
    one = [c for c in cases if c["N"] == 1]
    assert one and all(c["src"].size == 1 for c in one)


def test_tie_cases_really_tie():
    n = 0
    for c in sn.viterbi_cases():
        if not sn.is_tie_case(c) or c["N"] > 1000:
            continue
        v = sn.viterbi(*sn.model_args(c))
        n += 1
        if np.bincount(c["dst"]).max() < 2:
            continue                       # one candidate per destination: nothing can tie
        assert v["ties"] > 0, c["name"]
        # a destination whose candidates are all -inf takes pointer 0: such destinations exist
    assert n >= 12
    c = next(c for c in sn.viterbi_cases() if c["name"] == "ties-rand-N65-T70-B3")
    assert np.bincount(c["dst"], minlength=65).min() == 0


def test_half_of_the_counts_lie_above_the_floor():
    above = total = 0
    for c in sn.sum_cases():
        xi = sn.sums(*sn.model_args(c), weight=c["weight"])["xi"]
        above += int((xi >= sn.COUNT_FLOOR).sum())
        total += xi.size
    assert above * 2 >= total, (above, total)
