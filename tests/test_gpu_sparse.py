"""GPU: the sparse-transition HMM (csrc/sparse.hip; ops.sparse_viterbi, ops.sparse_forward_backward,
ops.sparse_arc_counts, autograd.SparseLogLik, pytorch_hmm_amd/sparse.py) against the numpy model
over arcs (tests/sparse_numpy.py) and against the library's dense paths on the densified matrix.

Viterbi is compared bit for bit: with ops.viterbi (N <= 256), ops.viterbi_ragged (with lengths) and
ops.viterbi(wide=True) (N = 257, 1000), and with the fp32 model at every size.  The cases (shared
with tests/test_sparse_cpu.py and the tolerance tool) are the smallest at which the kernel can go
wrong: N in {1, 2, 63, 64, 65, 257, 1000, 8192} (one wave, a wave's edge, several waves, more than
one state per thread), T in {1, 2, 3, 70} (T <= 4 at 8192), B in {1, 3} with ragged lengths
including 1; arcs in registers (left-to-right-skip), streamed arcs (random in-degree 0 .. 40),
hubs taken by a whole wave (in- and out-degree 300 at N = 320, the complete graph at N = 65),
-inf arcs, initial scores and emission rows, states without in- or out-arcs, sequences without a
path, and integer-valued scores that force exact ties.

Allowances of the sums.  The model was run in float32 against float64 over exactly these cases
(tools/measure_sparse_tolerance.py; CPU only) and the largest error per quantity taken; the GPU is
allowed 8x that, for its different summation order and the 1-2 ulp of the hardware exp / log
against numpy's.  Both the absolute and the relative bound of a quantity must hold.  Relative
errors of counts are taken over counts >= COUNT_FLOOR = 1e-8 (a count is a sum of positive
products, so its relative error holds that far down; tests/test_sparse_cpu.py asserts that at
least half of the reference counts lie above the floor).

    quantity, 69 cases                               fp32 model, largest                    allowance (8x)
    loglik       absolute                            4.534e-06  (hub-N320-T70-B3)           3.63e-05
    loglik       relative to max(|.|, 1)             3.410e-06  (hub-N320-T70-B3)           2.73e-05
    gamma        absolute                            3.351e-07  (hub-N320-T70-B3)           2.68e-06
    xi           absolute                            2.684e-06  (hub-N320-T70-B3)           2.15e-05
    xi           relative (>= 1e-08)                 3.763e-06  (hub-N320-T70-B3)           3.01e-05
    gradient, relative to its max-norm               9.786e-07  (lr-N1000-T70-B1)           7.83e-06
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sparse_numpy as sn  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 8.0
MEASURED = dict(loglik_abs=4.534e-06, loglik_rel=3.410e-06, gamma_abs=3.351e-07, xi_abs=2.684e-06, xi_rel=3.763e-06, grad_rel=9.786e-07)
ALLOW = {k: FACTOR * v for k, v in MEASURED.items()}
DEV = "cuda"

SUM_CASES = {c["name"]: c for c in sn.sum_cases()}
VIT_CASES = {c["name"]: c for c in sn.viterbi_cases()}


@functools.lru_cache(maxsize=None)
def ref_sums(name):
    c = SUM_CASES[name]
    return sn.sums(*sn.model_args(c), weight=c["weight"])


@functools.lru_cache(maxsize=None)
def ref_viterbi(name):
    return sn.viterbi(*sn.model_args(VIT_CASES[name]))


def on_gpu(c):
    import pytorch_hmm_amd as ph
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    tr = ph.SparseTransitions(c["src"], c["dst"], t(c["log_w"]), c["N"])
    lens = None if c["lengths"] is None else torch.from_numpy(c["lengths"])
    return tr, t(c["log_obs"]), t(c["log_p0"]), lens, t(c["weight"])


def lens_of(c):
    return np.full(c["B"], c["T"], np.int64) if c["lengths"] is None else c["lengths"]


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=False)


# ------------------------------------------------------------------------------ Viterbi
@pytest.mark.parametrize("name", list(VIT_CASES))
def test_viterbi_bit_exact(name):
    from pytorch_hmm_amd import ops, sparse
    c = VIT_CASES[name]
    tr, obs, p0, lens, _ = on_gpu(c)
    states, delta, final = sparse.sparse_viterbi(tr, obs, p0, lengths=lens)
    m = ref_viterbi(name)
    assert states.dtype == torch.int64 and delta.dtype == torch.float32
    assert same(states.cpu().numpy(), m["states"]), name
    assert same(delta.cpu().numpy(), m["log_delta"]), name
    assert same(final.cpu().numpy(), m["final_score"]), name
    n = lens_of(c)
    for b in range(c["B"]):                                      # padded frames: -1 and -inf
        assert bool((states[b, n[b]:] == -1).all()) and bool((delta[b, n[b]:] == -np.inf).all())
    # the library's dense paths on the densified matrix
    N = c["N"]
    if N > 1000:
        return
    P = tr.to_dense()
    if N <= 256 and lens is None:
        s2, d2, f2 = ops.viterbi(obs, P, p0, ops.OBS_LOG)
    elif N <= 256:
        s2, d2, f2 = ops.viterbi_ragged(obs, P, p0, ops.OBS_LOG, lens)
    else:
        s2, d2, f2 = ops.viterbi(obs, P, p0, ops.OBS_LOG, wide=True)
    if N <= 256 or lens is None:
        assert torch.equal(states, s2) and torch.equal(delta, d2) and torch.equal(final, f2), name
    else:
        # the wide form has no lengths: the valid prefix of the trellis, and everything of a
        # sequence that has the full length
        for b in range(c["B"]):
            assert torch.equal(delta[b, :n[b]], d2[b, :n[b]]), name
            if n[b] == c["T"]:
                assert torch.equal(states[b], s2[b]) and torch.equal(final[b], f2[b]), name


def test_first_index_rule_and_pointer_zero():
    """Every score equal: each destination's first (lowest) source wins, the final state is the
    first argmax, and a destination whose candidates are all -inf points to 0."""
    import pytorch_hmm_amd as ph
    N, T = 70, 6
    src, dst = sn.complete_graph(N)
    keep = (dst != 5) & ~((dst == 9) & (src < 3))     # state 5 has no in-arcs; 9 starts at source 3
    src, dst = src[keep], dst[keep]
    w = np.zeros(src.size, np.float32)
    w[dst == 11] = -np.inf                             # state 11: every candidate -inf
    hmm = ph.SparseHMM(ph.SparseTransitions(src, dst, torch.from_numpy(w), N), torch.zeros(N)).to(DEV)
    obs = torch.zeros(2, T, N, device=DEV)
    obs[1, -1, :4] = -1.0                              # the last row's first maximum is state 4
    states, score = hmm.viterbi_decode(obs)
    assert states[0].tolist() == [0] * T and states[1].tolist() == [0] * (T - 1) + [4]
    assert score.tolist() == [0.0, 0.0]
    m = sn.viterbi(obs.cpu().numpy(), src, dst, w, np.zeros(N, np.float32))
    assert same(states.cpu().numpy(), m["states"]) and m["ties"] > 0
    _, delta, _ = ph.sparse.sparse_viterbi(hmm.transitions, obs, hmm.log_p0.detach())
    assert bool((delta[:, 1:, 5] == -np.inf).all()) and bool((delta[:, 1:, 11] == -np.inf).all())
    # a frame that nothing can emit: every candidate after it is -inf, every pointer 0
    obs2 = torch.zeros(1, 4, N, device=DEV)
    obs2[0, 1] = -np.inf
    s2, sc2 = hmm.viterbi_decode(obs2)
    assert s2[0].tolist() == [0, 0, 0, 0] and sc2[0].item() == -np.inf


# -------------------------------------------------------------------------------- sums
def run_sums(c):
    from pytorch_hmm_amd import sparse
    tr, obs, p0, lens, g = on_gpu(c)
    loglik, gamma, xi = sparse.sparse_e_step(tr, obs, p0, lengths=lens, weight=g)
    return tr, obs, p0, lens, g, loglik, gamma, xi


def check_allowances(err, name):
    for k, v in err.items():
        print(f"{name}: {k} = {v:.3e} (allowed {ALLOW[k]:.3e})")
    for k, v in err.items():
        assert v <= ALLOW[k], (name, k, v, ALLOW[k])


@pytest.mark.parametrize("name", list(SUM_CASES))
def test_sums_against_fp64_model(name):
    c = SUM_CASES[name]
    ref = ref_sums(name)
    tr, obs, p0, lens, g, loglik, gamma, xi = run_sums(c)
    assert loglik.dtype == torch.float32 and gamma.dtype == torch.float32 and xi.dtype == torch.float64
    ll, ga, x = loglik.cpu().numpy(), gamma.cpu().numpy(), xi.cpu().numpy()
    fin = np.isfinite(ref["loglik"])
    assert same(np.isfinite(ll), fin) and np.all(ll[~fin] == -np.inf), name      # no path: -inf, not NaN
    g0 = (ga[:, 0].astype(np.float64) * c["weight"].astype(np.float64)[:, None]).sum(0)
    check_allowances(sn.errors(dict(loglik=ll, gamma=ga, xi=x, gamma0=g0), ref, c), name)
    # identities
    n = lens_of(c)
    rows = ga.astype(np.float64).sum(2)
    tol = ALLOW["gamma_abs"] * c["N"] ** 0.5 + 1e-5
    for b in range(c["B"]):
        assert np.all(ga[b, n[b]:] == 0), name                                   # padded frames: exact zeros
        if fin[b]:
            assert np.all(np.abs(rows[b, :n[b]] - 1.0) <= tol), name
        else:
            assert np.all(ga[b] == 0), name                                      # no path: exact zeros
    want = float((c["weight"].astype(np.float64) * (n - 1))[fin].sum())
    assert abs(x.sum() - want) <= max(want, 1.0) * ALLOW["xi_rel"] * 4 + 1e-6, (name, x.sum(), want)
    assert np.all(x[~np.isfinite(c["log_w"])] == 0), name                        # a -inf arc counts exactly 0
    assert np.all(x >= 0) and np.all(np.isfinite(x))
    if not fin.any():
        assert np.all(x == 0)


@pytest.mark.parametrize("name", ["rand-N65-T70-B3", "hub-N320-T70-B3", "lr-N8192-T4-B1", "rand-N8192-T3-B3",
                                  "nopath-N1000-T70-B3"])
def test_two_calls_give_equal_bits(name):
    c = SUM_CASES[name]
    a = run_sums(c)[5:]
    b = run_sums(c)[5:]
    for x, y in zip(a, b):
        assert torch.equal(x, y), name


def test_infeasible_sequence_alone():
    """A batch whose only sequence has no path: loglik -inf, gamma and every count exactly 0."""
    c = SUM_CASES["nopath-N64-T3-B1"]
    *_, loglik, gamma, xi = run_sums(c)
    assert loglik.tolist() == [-np.inf]
    assert bool((gamma == 0).all()) and bool((xi == 0).all())


# --------------------------------------------------------------------------- gradients
def dense_loglik_torch(obs, log_w, p0, src, dst, N, lens):
    """loglik (B) in fp64 on the CPU through a dense log-sum-exp recursion (torch autograd)."""
    P = torch.full((N, N), -float("inf"), dtype=torch.float64).index_put((src, dst), log_w)
    out = []
    for b in range(obs.shape[0]):
        a = p0 + obs[b, 0]
        for t in range(1, int(lens[b])):
            a = torch.logsumexp(a[:, None] + P, 0) + obs[b, t]
        out.append(torch.logsumexp(a, 0))
    return torch.stack(out)


GRAD_CASES = ["lr-N1-T70-B1", "lr-N2-T3-B1", "lr-N63-T70-B1", "lr-N64-T2-B1", "lr-N65-T70-B1", "lr-N64-T1-B1",
              "complete-N65-T70-B3"]


@pytest.mark.parametrize("name", GRAD_CASES)
@pytest.mark.parametrize("only_w", [False, True])
def test_gradients_against_torch_autograd(name, only_w):
    from pytorch_hmm_amd.autograd import SparseLogLik
    c = SUM_CASES[name]
    tr, obs, p0, lens, g = on_gpu(c)
    if c["B"] == 1:
        g = torch.tensor([0.75], device=DEV)
    w = tr.log_w.clone().requires_grad_(True)
    obs_g, p0_g = obs.clone().requires_grad_(not only_w), p0.clone().requires_grad_(not only_w)
    host = None if lens is None else lens.to(torch.int64)
    ll = SparseLogLik.apply(obs_g, w, p0_g, tr, host)
    (ll * g).sum().backward()                      # a non-uniform incoming gradient (B = 3: 1, 0.5, 2)
    o64 = torch.from_numpy(np.nan_to_num(c["log_obs"], nan=0.0)).double().requires_grad_(True)
    w64 = torch.from_numpy(c["log_w"]).double().requires_grad_(True)
    q64 = torch.from_numpy(c["log_p0"]).double().requires_grad_(True)
    ref = dense_loglik_torch(o64, w64, q64, torch.from_numpy(c["src"]), torch.from_numpy(c["dst"]), c["N"], lens_of(c))
    (ref * g.cpu().double()).sum().backward()
    assert np.abs(ll.detach().cpu().numpy() - ref.detach().numpy()).max() <= ALLOW["loglik_abs"]
    pairs = [(w.grad, w64.grad)]
    if only_w:
        assert obs_g.grad is None and p0_g.grad is None
    else:
        pairs += [(obs_g.grad, o64.grad), (p0_g.grad, q64.grad)]
    for got, want in pairs:
        # torch leaves the gradient of an input that no frame uses (log_w at T = 1) unset: zeros
        got, want = got.cpu().double().numpy(), np.zeros(got.shape) if want is None else want.numpy()
        top = np.abs(want).max()
        err = np.abs(got - want).max() / top if top > 0 else np.abs(got).max()
        print(f"{name}: gradient error relative to its max-norm {err:.3e} (allowed {ALLOW['grad_rel']:.3e})")
        assert err <= ALLOW["grad_rel"], (name, err)
    if c["lengths"] is not None and not only_w:
        n = lens_of(c)
        for b in range(c["B"]):
            assert bool((obs_g.grad[b, n[b]:] == 0).all())


@pytest.mark.parametrize("name", ["rand-N257-T70-B3", "lr-N1000-T70-B1", "rand-N1000-T3-B3", "lr-N8192-T4-B1",
                                  "rand-N8192-T4-B3", "hub-N320-T70-B3"])
def test_gradients_against_the_model(name):
    """Above 65 states: (g gamma, xi, sum_b g_b gamma_0) of the fp64 model, through the module."""
    import pytorch_hmm_amd as ph
    c = SUM_CASES[name]
    ref = ref_sums(name)
    tr, obs, p0, lens, g = on_gpu(c)
    hmm = ph.SparseHMM(tr, p0).to(DEV)
    obs = obs.clone().requires_grad_(True)
    (hmm.log_likelihood(obs, lengths=lens) * g).nan_to_num(neginf=0.0).sum().backward()
    n = lens_of(c)
    valid = (np.arange(c["T"])[None, :] < n[:, None])[..., None]
    want_obs = np.where(valid, ref["gamma"], 0.0) * c["weight"].astype(np.float64)[:, None, None]
    for got, want in ((obs.grad, want_obs), (hmm.log_w.grad, ref["xi"]), (hmm.log_p0.grad, ref["gamma0"])):
        got = got.cpu().double().numpy()
        top = np.abs(want).max()
        err = np.abs(got - want).max() / top if top > 0 else np.abs(got).max()
        print(f"{name}: gradient error relative to its max-norm {err:.3e} (allowed {ALLOW['grad_rel']:.3e})")
        assert err <= ALLOW["grad_rel"], (name, err)
        assert np.all(np.isfinite(got))


# ------------------------------------------------------------------------------ module
def test_reestimate_does_not_lower_the_likelihood():
    import pytorch_hmm_amd as ph
    rng = np.random.default_rng(77)
    N, T, B = 40, 50, 6
    src, dst = sn.lr_skip(N)
    hmm = ph.SparseHMM(ph.SparseTransitions(src, dst, torch.from_numpy(sn.normalised_log_w(src, N, rng)), N)).to(DEV)
    obs = torch.from_numpy((rng.standard_normal((B, T, N)) * 1.5).astype(np.float32)).to(DEV)
    lens = [50, 20, 1, 35, 50, 7]
    totals = []
    for _ in range(4):
        totals.append(float(hmm.reestimate(obs, lengths=lens).double().sum()))
    totals.append(float(hmm.log_likelihood(obs, lengths=lens).detach().double().sum()))
    for a, b in zip(totals, totals[1:]):
        assert b >= a - 1e-5 * max(1.0, abs(a)), totals
    assert totals[-1] > totals[0]
    # the update is a distribution over each source's arcs and over the initial states
    p = torch.zeros(N, dtype=torch.float64, device=DEV).index_add_(0, hmm._src.long(), hmm.log_w.detach().double().exp())
    assert torch.allclose(p, torch.ones_like(p), atol=1e-5)
    assert abs(float(hmm.log_p0.detach().double().exp().sum()) - 1.0) < 1e-5
    loglik, gamma, xi, g0 = hmm.e_step(obs, lengths=lens)
    assert xi.shape == (hmm.num_arcs,) and xi.dtype == torch.float64 and g0.shape == (N,)
    assert abs(float(xi.sum()) - sum(n - 1 for n in lens)) < 1e-2 and abs(float(g0.sum()) - B) < 1e-3


def test_from_dense_agrees_with_hmmpytorch():
    import pytorch_hmm_amd as ph
    rng = np.random.default_rng(12)
    N, T, B = 12, 40, 3
    P = ph.create_left_to_right_matrix(N)
    P = P if isinstance(P, torch.Tensor) else torch.from_numpy(np.asarray(P, np.float32))
    ref = ph.HMMPyTorch(P.float(), device=DEV)
    log_P, log_p0, _ = ref._device_params(torch.device(DEV, torch.cuda.current_device()))
    hmm = ph.SparseHMM.from_dense(log_P, log_p0, trainable=False)
    x = torch.from_numpy(rng.random((B, T, N), dtype=np.float32)).to(DEV)
    log_obs = torch.log((x + 1e-8).double()).float()     # the correctly rounded log the dense kernels take
    for lens in (None, [40, 1, 17]):
        s1, d1 = ref.viterbi_decode(x, lengths=lens)
        s2, score = hmm.viterbi_decode(log_obs, lengths=lens)
        assert torch.equal(s1, s2)
        last = [T - 1] * B if lens is None else [n - 1 for n in lens]
        want = torch.stack([d1[b, last[b]].max() for b in range(B)])
        assert torch.allclose(score, want, rtol=1e-6, atol=1e-5)
        post = hmm.posteriors(log_obs, lengths=lens)
        assert torch.allclose(post, ref.posteriors(x, lengths=lens), atol=ALLOW["gamma_abs"] + 1e-5)
    one, sc = hmm.viterbi_decode(log_obs[0])              # a (T,N) sequence is a batch of one
    assert one.shape == (T,) and sc.shape == ()
