"""GPU parity of dynamic time warping (csrc/dtw.hip; ops.dtw / ops.soft_dtw / autograd.SoftDTW;
pytorch_hmm_amd.alignment).

Contracts:
  * Hard DTW: cost matrix, total and path bit-identical to the reference's (fixtures written by
    tests/golden/make_golden_dtw.py, and the numpy restatement of tests/dtw_numpy.py -- which
    test_dtw_cpu.py holds to the fixtures -- on shapes that cross the kernel's own boundaries:
    its rows-per-pass, the 4-column block, more than one pass).
  * Soft-DTW total: relative error against the fixture's fp64 value <= 4 (N+M) 2^-24: each of the
    <= N+M-1 cells on a path adds one rounding of the add and a few of the shifted log-sum-exp.
  * Soft-DTW gradient: max |E_gpu - E_fp64| <= 8 x max |grad_ref32 - E_fp64|, the error of the
    reference's own fp32 autograd on the same fixture and gamma (entries lie in [0,1]).
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtw_numpy as dn  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "dtw.hip")).read()
ROWS = int(re.search(r"constexpr int kDtwRows = (\d+);", _SRC).group(1))          # rows per thread
THREADS = int(re.search(r"constexpr int kDtwThreads = (\d+);", _SRC).group(1))    # threads per workgroup
assert re.search(r"constexpr int kDtwStrip = kDtwRows \* kDtwThreads;", _SRC)
STRIP = ROWS * THREADS                                                             # rows per pass
EPS24 = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _native():
    import pytorch_hmm_amd._native as nat
    nat.lib()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()


def ops():
    from pytorch_hmm_amd import ops as o
    return o


def t(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(DEV, dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def run_hard(dist, pattern, **kw):
    """ops.dtw on one (N,M) matrix -> numpy (cost, total, path_i, path_j)."""
    o = ops()
    cost, total, pi, pj, pl = o.dtw(t(dist)[None], o.dtw_pattern(pattern), **kw)
    n = int(pl[0])
    assert (pi[0, n:] == -1).all() and (pj[0, n:] == -1).all()
    return cost[0].cpu().numpy(), total[0].cpu().numpy(), pi[0, :n].cpu().numpy(), pj[0, :n].cpu().numpy()


# ------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("pattern", dn.PATTERNS)
@pytest.mark.parametrize("name", dn.FIXTURES)
def test_hard_dtw_reproduces_fixture(gold, name, pattern):
    g = gold("dtw_" + name)
    cost, total, pi, pj = run_hard(g["dist"], pattern)
    assert np.array_equal(bits(cost), bits(g["cost_" + pattern]))
    assert np.array_equal(bits(total), bits(g["total_" + pattern]))
    assert np.array_equal(pi, g["path_i_" + pattern]) and np.array_equal(pj, g["path_j_" + pattern])


# --------------------------------------------------------- the kernel's own boundaries
@functools.lru_cache(maxsize=None)
def boundary_case(N, M, integer):
    rng = np.random.default_rng(N * 4099 + M)
    if integer:
        dist = rng.integers(0, 4, (N, M)).astype(np.float32)
    else:
        dist = rng.random((N, M), dtype=np.float32)
    return dist, {p: dn.hard_dtw(dist, p) for p in dn.PATTERNS}


BOUNDARY = [(n, m, False) for n in (STRIP - 1, STRIP, STRIP + 1) for m in (5, 70)]
BOUNDARY += [(m, n, i) for n, m, i in BOUNDARY] + [(300, 257, True)]


@pytest.mark.parametrize("N,M,integer", BOUNDARY)
def test_hard_dtw_across_kernel_boundaries(N, M, integer):
    dist, want = boundary_case(N, M, integer)
    for p in dn.PATTERNS:
        C, wi, wj = want[p]
        cost, total, pi, pj = run_hard(dist, p)
        assert np.array_equal(bits(cost), bits(C)), p
        assert np.array_equal(bits(total), bits(C[-1, -1])), p
        assert np.array_equal(pi, wi) and np.array_equal(pj, wj), p


# -------------------------------------------------------------------------- ragged batch
LENS = ((13, 9), (1, 7), (20, 20))


def test_ragged_batch_equals_single_calls():
    o = ops()
    rng = np.random.default_rng(5)
    dist = t(rng.random((3, 20, 20), dtype=np.float32))
    n_len = torch.tensor([l[0] for l in LENS], dtype=torch.int32, device=DEV)
    m_len = torch.tensor([l[1] for l in LENS], dtype=torch.int32, device=DEV)
    for pattern in (o.DTW_SYMMETRIC, o.DTW_RABINER_JUANG):
        cost, total, pi, pj, pl = o.dtw(dist, pattern, n_len, m_len)
        for b, (n, m) in enumerate(LENS):
            c1, t1, i1, j1, l1 = o.dtw(dist[b:b + 1, :n, :m].contiguous(), pattern)
            assert torch.equal(cost[b, :n, :m], c1[0]) and torch.equal(total[b], t1[0])
            assert torch.isposinf(cost[b, n:, :]).all() and torch.isposinf(cost[b, :, m:]).all()
            L = int(l1[0])
            assert int(pl[b]) == L and 1 <= L <= n + m - 1
            assert torch.equal(pi[b, :L], i1[0, :L]) and torch.equal(pj[b, :L], j1[0, :L])
            assert (pi[b, L:] == -1).all() and (pj[b, L:] == -1).all()
    # soft-DTW and its gradient on the same corners
    R, total = o.soft_dtw(dist, 0.1, n_len, m_len)
    E = o.soft_dtw_grad(dist, R, 0.1, n_len, m_len)
    for b, (n, m) in enumerate(LENS):
        d1 = dist[b:b + 1, :n, :m].contiguous()
        R1, t1 = o.soft_dtw(d1, 0.1)
        assert torch.equal(R[b, :n + 1, :m + 1], R1[0]) and torch.equal(total[b], t1[0])
        assert torch.isposinf(R[b, n + 1:, :]).all() and torch.isposinf(R[b, :, m + 1:]).all()
        assert torch.equal(E[b, :n, :m], o.soft_dtw_grad(d1, R1, 0.1)[0])
        assert (E[b, n:, :] == 0).all() and (E[b, :, m:] == 0).all()


def test_value_only_call_gives_the_same_totals():
    o = ops()
    rng = np.random.default_rng(6)
    dist = t(rng.random((4, 37, 53), dtype=np.float32))
    for pattern in (o.DTW_SYMMETRIC, o.DTW_ASYMMETRIC, o.DTW_RABINER_JUANG):
        full = o.dtw(dist, pattern)
        cost, total, pi, pj, pl = o.dtw(dist, pattern, None, None, False, False)
        assert torch.equal(total, full[1])
        assert cost.numel() == 0 and pi.numel() == 0 and pj.numel() == 0 and pl.numel() == 0
    empty = o.dtw(dist[:0], o.DTW_SYMMETRIC)
    assert empty[0].shape == (0, 37, 53) and empty[1].shape == (0,)


# ------------------------------------------------------------------------------ soft-DTW
@pytest.mark.parametrize("tag,gamma", dn.GAMMAS)
@pytest.mark.parametrize("name", dn.SOFT_FIXTURES)
def test_soft_dtw_total_vs_fp64(gold, name, tag, gamma):
    g = gold("dtw_" + name)
    N, M = g["dist"].shape
    R, total = ops().soft_dtw(t(g["dist"])[None], gamma)
    want = float(g["soft_total64_" + tag])
    got = float(total[0])
    rel = abs(got - want) / abs(want)
    ref_rel = abs(float(g["soft_total32_" + tag]) - want) / abs(want)
    print(f"soft total {name} gamma={gamma}: rel err {rel:.3e} (reference fp32 {ref_rel:.3e}), "
          f"bound {4 * (N + M) * EPS24:.3e}")
    assert rel <= 4 * (N + M) * EPS24
    assert float(R[0, N, M]) == got and float(R[0, 0, 0]) == 0.0
    assert torch.isposinf(R[0, 0, 1:]).all() and torch.isposinf(R[0, 1:, 0]).all()


@pytest.mark.parametrize("tag,gamma", dn.GAMMAS)
@pytest.mark.parametrize("name", dn.SOFT_FIXTURES)
def test_soft_dtw_gradient_vs_fp64(gold, name, tag, gamma):
    o = ops()
    g = gold("dtw_" + name)
    d = t(g["dist"])[None]
    R, _ = o.soft_dtw(d, gamma)
    E = o.soft_dtw_grad(d, R, gamma)[0].cpu().numpy().astype(np.float64)
    err = np.abs(E - g["soft_grad64_" + tag]).max()
    ref = np.abs(g["grad_ref32_" + tag].astype(np.float64) - g["soft_grad64_" + tag]).max()
    print(f"soft grad {name} gamma={gamma}: max|E_gpu - E_fp64| {err:.3e}, reference fp32 {ref:.3e}")
    assert err <= 8 * ref


def test_soft_dtw_across_passes():
    """More rows than one pass, both kernels, against the fp64 restatement.  The total's bound is the
    one above.  The gradient has no reference fp32 run at this size: its yardstick is the same
    closed form evaluated in numpy fp32, and the bound 8 x that error plus 8 roundings of an entry
    near 1."""
    o = ops()
    N, M, gamma = STRIP + 6, 3, 1.0
    rng = np.random.default_rng(9)
    dist = rng.random((N, M), dtype=np.float32)
    R64 = dn.soft_forward(dist, gamma)
    E64 = dn.soft_grad(dist, R64, gamma)
    R32 = dn.soft_forward(dist, gamma, np.float32)
    E32 = dn.soft_grad(dist, R32, gamma, np.float32)
    d = t(dist)[None]
    R, total = o.soft_dtw(d, gamma)
    rel = abs(float(total[0]) - R64[N, M]) / R64[N, M]
    print(f"soft total {N}x{M}: rel err {rel:.3e}, bound {4 * (N + M) * EPS24:.3e}")
    assert rel <= 4 * (N + M) * EPS24
    E = o.soft_dtw_grad(d, R, gamma)[0].cpu().numpy().astype(np.float64)
    err, ref = np.abs(E - E64).max(), np.abs(E32.astype(np.float64) - E64).max()
    print(f"soft grad {N}x{M}: max|E_gpu - E_fp64| {err:.3e}, numpy fp32 {ref:.3e}")
    assert err <= 8 * ref + 8 * EPS24


@pytest.mark.parametrize("tag,gamma", dn.GAMMAS)
def test_soft_dtw_autograd_reaches_x_and_y(gold, tag, gamma):
    from pytorch_hmm_amd.alignment import compute_distance_matrix
    from pytorch_hmm_amd.autograd import SoftDTW
    g = gold("dtw_xgrad")
    x, y = t(g["x"]).requires_grad_(), t(g["y"]).requires_grad_()
    assert x.shape == (9, 4) and y.shape == (13, 4)
    total = SoftDTW.apply(compute_distance_matrix(x, y)[None], gamma, None, None)
    (2.0 * total.sum()).backward()
    for name, got in (("x", x.grad), ("y", y.grad)):
        want = g[f"{name}grad64_{tag}"]
        err = np.abs(got.cpu().numpy().astype(np.float64) / 2.0 - want).max()
        ref = np.abs(g[f"{name}grad_ref32_{tag}"].astype(np.float64) - want).max()
        print(f"soft d/d{name} gamma={gamma}: max err {err:.3e}, reference fp32 {ref:.3e}")
        assert err <= 8 * ref
    rel = abs(float(total[0].detach()) - float(g["total64_" + tag])) / abs(float(g["total64_" + tag]))
    assert rel <= 4 * (9 + 13) * EPS24 + 4 * 2.0 ** -23     # + the distances' own last bit


# ------------------------------------------------------------------------------- classes
def judged_path(pi, pj, dist, want_total, pattern="symmetric"):
    """A path formed from GPU-side distances may differ where the last bit decides: it is a valid
    step path whose fp64 cost over the fixture's dist is within 1e-4 of the fixture's total."""
    pi, pj = pi.cpu().numpy(), pj.cpu().numpy()
    assert pi.dtype == np.int64 and pj.dtype == np.int64
    assert dn.path_is_valid(pi, pj, *dist.shape)
    assert abs(dn.path_cost(dist, pi, pj, pattern) - float(want_total)) <= 1e-4


def test_compute_distance_matrix_on_device(gold):
    from pytorch_hmm_amd.alignment import compute_distance_matrix
    for name in dn.FIXTURES:
        g = gold("dtw_" + name)
        tol = g["x"].shape[1] * 2.0 ** -23
        for fn in ("euclidean", "cosine", "manhattan"):
            got = compute_distance_matrix(t(g["x"]), t(g["y"]), fn).cpu().numpy()
            ref = g["dist_" + fn]
            assert np.all(np.abs(got - ref) <= tol * np.abs(ref) + (tol if fn == "cosine" else 0.0)), (name, fn)


def test_functions_on_integer_fixture_are_exact(gold):
    import pytorch_hmm_amd.alignment as al
    g = gold("dtw_ties")
    x, y = t(g["x"]), t(g["y"])
    for p in dn.PATTERNS:
        pi, pj, cost = al.compute_dtw_path(t(g["dist"]), p)
        assert pi.dtype == torch.int64 and cost.shape == g["dist"].shape and cost.dtype == torch.float32
        assert np.array_equal(bits(cost.cpu().numpy()), bits(g["cost_" + p]))
        assert np.array_equal(pi.cpu().numpy(), g["path_i_" + p]) and np.array_equal(pj.cpu().numpy(), g["path_j_" + p])
        pi, pj, total = al.dtw_alignment(x, y, "manhattan", p)
        assert np.array_equal(pi.cpu().numpy(), g["path_i_" + p]) and np.array_equal(pj.cpu().numpy(), g["path_j_" + p])
        assert total.dim() == 0 and float(total) == float(g["total_" + p])
        assert float(al.dtw_distance(x, y, "manhattan", p)) == float(g["total_" + p])


def test_functions_on_plain_fixture(gold):
    import pytorch_hmm_amd.alignment as al
    g = gold("dtw_40x40")
    x, y = t(g["x"]), t(g["y"])
    pi, pj, total = al.dtw_alignment(x, y)
    judged_path(pi, pj, g["dist"], g["total_symmetric"])
    assert abs(float(total) - float(g["total_symmetric"])) <= 1e-4
    assert abs(float(al.dtw_distance(x, y)) - float(g["total_symmetric"])) <= 1e-4


def test_dtw_aligner_2d_and_3d(gold):
    from pytorch_hmm_amd import ConstrainedDTWAligner, DTWAligner
    g = gold("dtw_ties")
    x, y = t(g["x"]), t(g["y"])
    hard = DTWAligner(distance_fn="manhattan")
    pi, pj, cost = hard(x, y)
    assert np.array_equal(pi.cpu().numpy(), g["path_i_symmetric"]) and np.array_equal(pj.cpu().numpy(), g["path_j_symmetric"])
    assert float(cost) == float(g["total_symmetric"])
    # 3-D: two lists and the stacked costs; the second pair is the first one reversed in time
    xb, yb = torch.stack([x, x.flip(0)]), torch.stack([y, y.flip(0)])
    li, lj, costs = hard(xb, yb)
    assert isinstance(li, list) and isinstance(lj, list) and len(li) == 2 and costs.shape == (2,)
    assert np.array_equal(li[0].cpu().numpy(), g["path_i_symmetric"]) and np.array_equal(lj[0].cpu().numpy(), g["path_j_symmetric"])
    C, wi, wj = dn.hard_dtw(g["dist"][::-1, ::-1], "symmetric")
    assert np.array_equal(li[1].cpu().numpy(), wi) and np.array_equal(lj[1].cpu().numpy(), wj)
    assert float(costs[0]) == float(g["total_symmetric"]) and float(costs[1]) == float(C[-1, -1])
    # plain features: judged as paths
    b1, b2 = gold("dtw_band"), gold("dtw_noend")
    xb, yb = torch.stack([t(b1["x"]), t(b2["x"])]), torch.stack([t(b1["y"]), t(b2["y"])])
    li, lj, costs = DTWAligner()(xb, yb)
    ci, cj, ccosts = ConstrainedDTWAligner(bandwidth=3)(xb, yb)
    for b, f in enumerate((b1, b2)):
        want = dn.hard_cost(f["dist_euclidean"], "symmetric")[-1, -1]
        judged_path(li[b], lj[b], f["dist_euclidean"], want)
        assert abs(float(costs[b]) - float(want)) <= 1e-4
        # the constrained aligner's results are the unconstrained ones (the reference discards its mask)
        assert torch.equal(ci[b], li[b]) and torch.equal(cj[b], lj[b])
    assert torch.equal(ccosts, costs)
    c2 = ConstrainedDTWAligner(soft_dtw=True, distance_fn="manhattan")(x, y)
    assert torch.equal(c2[0], pi) and torch.equal(c2[1], pj) and torch.equal(c2[2], cost)


def test_dtw_aligner_soft(gold):
    from pytorch_hmm_amd import DTWAligner
    g = gold("dtw_ties")
    N, M = g["dist"].shape
    x, y = t(g["x"]).requires_grad_(), t(g["y"])
    soft = DTWAligner(distance_fn="manhattan", soft_dtw=True, gamma=0.1)
    pi, pj, total = soft(x, y)
    want = float(g["soft_total64_0p1"])
    assert total.dim() == 0 and abs(float(total) - want) <= 4 * (N + M) * EPS24 * abs(want)
    assert torch.equal(pi.cpu(), torch.arange(N))
    assert torch.equal(pj.cpu(), torch.round(torch.linspace(0, M - 1, N)).long())
    total.backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    li, lj, totals = soft(torch.stack([x.detach(), x.detach()]), torch.stack([y, y]))
    assert len(li) == 2 and totals.shape == (2,) and torch.equal(totals[0], totals[1])
    assert torch.equal(totals[0], total.detach()) and torch.equal(li[1], pi) and torch.equal(lj[1], pj)


def test_phoneme_audio_alignment_and_durations(gold):
    import pytorch_hmm_amd.alignment as al
    g = gold("dtw_phoneme")
    alignment, boundaries = al.phoneme_audio_alignment(t(g["phoneme_features"]), t(g["audio_features"]))
    assert alignment.dtype == torch.int64 and alignment.device.type == "cuda"
    assert np.array_equal(alignment.cpu().numpy(), g["alignment"])
    assert np.array_equal(boundaries.cpu().numpy(), g["boundaries"])
    dur = al.extract_phoneme_durations(alignment, len(g["durations"]))
    assert np.array_equal(dur.cpu().numpy(), g["durations"])


# -------------------------------------------------------------------------- stream order
def test_side_stream_matches_default_stream():
    """The launch and the workspace follow the current stream: the same calls on a side stream,
    queued behind a large matrix product there, give the default stream's results."""
    o = ops()
    rng = np.random.default_rng(11)
    dist = t(rng.random((3, 150, 130), dtype=np.float32))

    def run():
        hard = o.dtw(dist, o.DTW_RABINER_JUANG)
        R, total = o.soft_dtw(dist, 0.1)
        return hard + (R, total, o.soft_dtw_grad(dist, R, 0.1))

    want = run()
    big = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _ = big @ big
        got = run()
    side.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
