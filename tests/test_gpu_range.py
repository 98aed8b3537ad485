"""GPU: the scaled forward-backward paths at and past the fp32 range, against the float64
log-space reference (tests/logspace_numpy.py) over the cases of tests/range_cases.py.

Class A (in range: a realistic emission spread of hundreds of nats over floored tables, and over
exact-zero tables along a feasible path) runs through every sum-product path -- the dense chain,
the banded chains, the pair kernel, the ragged, wide, time-varying and sparse forms, em.e_step, the
likelihood gradients, posterior sampling -- at the tolerances each path's own tests use against
their fp64 models: gamma 2e-5 absolute, loglik 2e-6 relative, forward / backward 1e-4 relative
where fp32 can hold them, xi and gamma0 as test_gpu_em.py, gradients within 1e-4 of their
largest entry.  Every other fp64 yardstick of these paths is the same scaled recursion in fp64;
this one is not.

The sparse sums.  test_gpu_sparse.py's ALLOW table does not hold at this spread: it was measured
on log-likelihoods of a few hundred nats, and here they reach -12000, where one ulp of the fp32
loglik the kernel stores is 1e-3 (on the MI355X the absolute loglik error reached 4.63e-4 against
that table's 3.63e-5; every other quantity stayed inside it).  As that file did, the fp32 numpy
model over arcs (sparse_numpy.sums) was measured against the reference -- here the log-space one --
over exactly the class A cases (tools/measure_range_tolerance.py; CPU only), and the GPU is allowed
8x the largest error per quantity; both the absolute and the relative bound of a quantity must hold:

    quantity, 34 cases                               fp32 model, largest                     allowance (8x)   MI355X, largest
    loglik       absolute                            4.626e-04  (A-floor-l2r-N200-T230)      3.70e-03         4.626e-04
    loglik       relative to max(|.|, 1)             4.758e-08  (A-floor-jumpy-N256-T70)     3.81e-07         4.758e-08
    gamma        absolute                            5.201e-07  (A-zeros-skip-N200-T230)     4.16e-06         3.795e-07
    xi           absolute                            1.561e-05  (A-zeros-skip-N200-T230)     1.25e-04         1.135e-05
    xi           relative (>= 1e-08)                 8.877e-07  (A-zeros-skip-N200-T230)     7.10e-06         6.377e-07
    gradient, relative to its max-norm               5.201e-07  (A-zeros-skip-N200-T230)     4.16e-06         3.795e-07

Class B (out of range: exact zeros in the table and a row leader no path reaches) runs through
the guarded entry points (pytorch_hmm_amd/range_guard.py; GUARD below: set it to False and these
tests fail), which must equal the reference at the same tolerances, and through the raw ops, which
are documented as in-range only (include/hmm355.h) and must still fail cleanly: no NaN, loglik
finite or -inf, every gamma row a distribution or all zero, neighbouring sequences untouched.

tests/test_range_cpu.py holds the conditions on the cases themselves (class A not one-hot and in
range for the fp32 model, class B wrong in it, the detector's fuzz).
"""
import functools
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import logspace_numpy as lsn  # noqa: E402
import range_cases as rc  # noqa: E402
import sparse_numpy as sn  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = True            # the guarded entry points' range_guard: False makes the class B tests fail

CASES = {c["name"]: c for c in rc.range_cases()}
A_NARROW = [n for n, c in CASES.items() if c["cls"] == "A" and c["N"] <= 256]
A_FULL = [n for n in A_NARROW if CASES[n]["lengths"] is None]          # no lengths: the plain ops
A_RAGGED = [n for n in A_NARROW if CASES[n]["lengths"] is not None]
A_WIDE = [n for n, c in CASES.items() if c["cls"] == "A" and c["N"] > 256]
B_NAMES = [n for n, c in CASES.items() if c["cls"] == "B"]
ALL3 = 7                # FB_POSTERIOR | FB_FORWARD | FB_BACKWARD
SPARSE_MEASURED = dict(loglik_abs=4.626e-04, loglik_rel=4.758e-08, gamma_abs=5.201e-07, xi_abs=1.561e-05,
                       xi_rel=8.877e-07, grad_rel=5.201e-07)
ALLOW = {k: 8.0 * v for k, v in SPARSE_MEASURED.items()}


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASES[name]
    return lsn.forward_backward(c["log_obs"], c["log_P"], c["log_p0"], c["lengths"])


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def gpu(c):
    lens = None if c["lengths"] is None else torch.from_numpy(c["lengths"])
    return dev(c["log_obs"]), dev(c["log_P"]), dev(c["log_p0"]), lens


def valid_mask(c):
    lens = np.full(c["B"], c["T"]) if c["lengths"] is None else c["lengths"]
    return np.arange(c["T"])[None, :] < np.asarray(lens)[:, None]


def check_loglik(tag, got, want):
    got = got.cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), (tag, got, want)
    assert np.all(got[~fin] == -np.inf), (tag, got)
    err = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
    print(f"{tag}: loglik rel err {err.max() if err.size else 0.0:.2e} (allowed 2e-6)")
    assert np.all(err <= 2e-6), (tag, got, want)


def check_gamma(tag, got, ref, c):
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), tag
    valid = valid_mask(c)
    err = float(np.abs(got - ref["gamma"])[valid].max())
    print(f"{tag}: gamma abs err {err:.2e} (allowed 2e-5)")
    assert err <= 2e-5, (tag, err)
    assert np.all(got[~valid] == 0), tag                                 # padded frames: exact zeros
    assert np.all(got[~np.isfinite(ref["loglik"])] == 0), tag             # no path: exact zeros


def check_exp(tag, got, log_want, c):
    """forward / backward = exp(log alpha / beta) wherever fp32 holds the value as a normal number;
    below that the kernel may give a denormal or 0, never more than the smallest normal."""
    got = got.cpu().numpy().astype(np.float64)
    valid = valid_mask(c)[..., None] & np.ones_like(got, bool)
    rep = valid & (log_want > np.log(2.0 ** -120))
    with np.errstate(over="ignore"):
        want = np.exp(log_want)
    n = int(rep.sum())
    if n:
        err = float((np.abs(got - want)[rep] / want[rep]).max())
        print(f"{tag}: {n} representable entries, rel err {err:.2e} (allowed 1e-4)")
        assert err <= 1e-4, (tag, err)
    low = valid & (log_want < np.log(2.0 ** -140))
    assert np.all(got[low] <= 2.0 ** -126), tag
    assert np.isfinite(got).all(), tag


def check_fb_outputs(tag, outs, c, ref, want_exp=True):
    post, fwd, bwd, loglik, _ = outs
    check_loglik(tag, loglik, ref["loglik"])
    check_gamma(tag, post, ref, c)
    if want_exp:
        check_exp(tag + " forward", fwd, ref["log_alpha"], c)
        check_exp(tag + " backward", bwd, ref["log_beta"], c)


def check_counts(tag, xi, gamma0, ref, log_P):
    xi = xi.cpu().numpy().astype(np.float64)
    g0 = gamma0.cpu().numpy().astype(np.float64)
    ex = float(np.abs(xi - ref["xi"]).max() / max(ref["xi"].sum(), 1e-30))
    eg = float(np.abs(g0 - ref["gamma0"]).max() / max(ref["gamma0"].sum(), 1e-30))
    print(f"{tag}: xi err / sum {ex:.2e}, gamma0 err / sum {eg:.2e} (allowed 2e-5)")
    assert ex <= 2e-5 and eg <= 2e-5, (tag, ex, eg)
    assert np.all(xi[np.isinf(log_P)] == 0), tag


# =========================================================================== class A
@pytest.mark.parametrize("form", ["chain", "plan", "pair", "dense-plan"])
@pytest.mark.parametrize("name", A_FULL)
def test_a_forward_backward(name, form):
    from pytorch_hmm_amd import ops
    c, ref = CASES[name], reference(name)
    obs, lP, l0, _ = gpu(c)
    plan = None if form == "chain" else ops.make_plan(lP, dense=form == "dense-plan")
    outs = ops.forward_backward(obs, lP, l0, ops.OBS_LOG, ALL3, plan, True if form == "pair" else None)
    check_fb_outputs(f"{name} {form}", outs, c, ref)


@pytest.mark.parametrize("name", A_RAGGED)
def test_a_ragged(name):
    from pytorch_hmm_amd import ops
    c, ref = CASES[name], reference(name)
    obs, lP, l0, lens = gpu(c)
    outs = ops.forward_backward_ragged(obs, lP, l0, ops.OBS_LOG, lens, ALL3)
    check_fb_outputs(f"{name} ragged", outs, c, ref)


@pytest.mark.parametrize("name", A_WIDE)
def test_a_wide(name):
    from pytorch_hmm_amd import ops
    c, ref = CASES[name], reference(name)
    obs, lP, l0, _ = gpu(c)
    outs = ops.forward_backward(obs, lP, l0, ops.OBS_LOG, ALL3)
    check_fb_outputs(f"{name} wide", outs, c, ref)


@pytest.mark.parametrize("matrix", ["static", "per-step"])
@pytest.mark.parametrize("name", A_FULL)
def test_a_time_varying(name, matrix):
    from pytorch_hmm_amd import ops
    c, ref = CASES[name], reference(name)
    obs, lP, l0, _ = gpu(c)
    A = lP.expand(c["B"], c["T"], c["N"], c["N"])                          # zero strides: never materialised
    if matrix == "per-step":
        A = A.contiguous()
    outs = ops.tv_forward_backward(obs, A, l0, ALL3)
    check_fb_outputs(f"{name} tv {matrix}", outs, c, ref)


def sparse_on_gpu(c):
    import pytorch_hmm_amd as ph
    tr = ph.SparseTransitions(c["src"], c["dst"], dev(c["log_w"]), c["N"])
    return tr


def arc_form(c):
    ind = np.bincount(c["dst"], minlength=c["N"])
    outd = np.bincount(c["src"], minlength=c["N"])
    top = max(ind.max(), outd.max())
    return "registers" if top <= 4 else ("streamed" if top <= 64 else "streamed+hub")


def check_sparse(tag, c, ref, loglik, gamma, xi):
    ll, ga, x = loglik.cpu().numpy(), gamma.cpu().numpy(), xi.cpu().numpy()
    fin = np.isfinite(ref["loglik"])
    assert np.array_equal(np.isfinite(ll), fin) and np.all(ll[~fin] == -np.inf), tag
    assert np.isfinite(ga).all() and np.isfinite(x).all(), tag
    case = dict(c, weight=np.ones(c["B"], np.float32))
    want = dict(loglik=ref["loglik"], gamma=ref["gamma"], xi=ref["xi"][c["src"], c["dst"]], gamma0=ref["gamma0"])
    err = sn.errors(dict(loglik=ll, gamma=ga, xi=x, gamma0=ga[:, 0].astype(np.float64).sum(0)), want, case)
    for k, v in err.items():
        print(f"{tag}: {k} = {v:.3e} (allowed {ALLOW[k]:.3e})")
    for k, v in err.items():
        assert v <= ALLOW[k], (tag, k, v, ALLOW[k])
    assert np.all(ga[~valid_mask(c)] == 0), tag


@pytest.mark.parametrize("name", A_NARROW)
def test_a_sparse(name):
    """Every arc form the cases' degrees reach: arcs in registers (zeros-skip), streamed arcs
    (the floored tables up to 64 states, the random graph), hubs (the floored tables above 64
    states, where every state has more than a wave's worth of arcs, and the rand-hub graph, where
    one state has)."""
    from pytorch_hmm_amd import sparse
    c, ref = CASES[name], reference(name)
    obs, _, l0, lens = gpu(c)
    loglik, gamma, xi = sparse.sparse_e_step(sparse_on_gpu(c), obs, l0, lengths=lens, range_guard=False)
    check_sparse(f"{name} sparse ({arc_form(c)})", c, ref, loglik, gamma, xi)


def test_a_sparse_reaches_every_arc_form():
    assert {arc_form(CASES[n]) for n in A_NARROW} == {"registers", "streamed", "streamed+hub"}


@pytest.mark.parametrize("name", A_NARROW)
def test_a_e_step(name):
    """em.e_step without (the kernels alone) and with the guard: in range nothing is flagged, so
    the guarded call returns the same bits."""
    from pytorch_hmm_amd import em
    c, ref = CASES[name], reference(name)
    obs, lP, l0, lens = gpu(c)
    raw = em.e_step(obs, lP, l0, lens, range_guard=False)
    tag = f"{name} e_step"
    check_loglik(tag, raw.loglik, ref["loglik"])
    check_gamma(tag, raw.gamma, ref, c)
    check_counts(tag, raw.xi, raw.gamma0, ref, c["log_P"])
    if c["T"] == 1:
        assert bool((raw.xi == 0).all())
    guarded = em.e_step(obs, lP, l0, lens)
    for a, b in ((raw.loglik, guarded.loglik), (raw.gamma, guarded.gamma), (raw.xi, guarded.xi),
                 (raw.gamma0, guarded.gamma0)):
        assert torch.equal(a, b), tag


@pytest.mark.parametrize("name", A_NARROW)
def test_a_nothing_flagged_in_the_sparse_guard(name):
    from pytorch_hmm_amd import sparse
    c = CASES[name]
    obs, _, l0, lens = gpu(c)
    tr = sparse_on_gpu(c)
    raw = sparse.sparse_e_step(tr, obs, l0, lengths=lens, range_guard=False)
    guarded = sparse.sparse_e_step(tr, obs, l0, lengths=lens)
    for a, b in zip(raw, guarded):
        assert torch.equal(a, b), name


# ------------------------------------------------------------------------- gradients
def lse_t(x, dim):
    """log sum exp with the `m == -inf ? 0 : m` shift, differentiable with zero (not NaN)
    gradients where every term is -inf."""
    m = x.detach().amax(dim, keepdim=True)
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    s = torch.exp(x - m0).sum(dim)
    pos = s > 0
    out = m0.squeeze(dim) + torch.log(torch.where(pos, s, torch.ones_like(s)))
    return torch.where(pos, out, torch.full_like(out, -float("inf")))


def grad_or_zero(t):
    """t.grad, with autograd's None (T = 1: no transition is ever used) as the zero it stands for."""
    return torch.zeros_like(t) if t.grad is None else t.grad


def autograd_reference(c, weight):
    """(loglik, d sum(weight loglik) / d log_obs, log_P, log_p0) by float64 torch autograd through a
    log-space loop on the host."""
    f64 = torch.float64
    obs = torch.tensor(np.nan_to_num(c["log_obs"], nan=0.0, neginf=-np.inf), dtype=f64, requires_grad=True)
    lP = torch.tensor(c["log_P"], dtype=f64, requires_grad=True)
    l0 = torch.tensor(c["log_p0"], dtype=f64, requires_grad=True)
    lens = np.full(c["B"], c["T"]) if c["lengths"] is None else c["lengths"]
    lls = []
    for b in range(c["B"]):
        a = l0 + obs[b, 0]
        for t in range(1, int(lens[b])):
            a = lse_t(a[:, None] + lP, 0) + obs[b, t]
        lls.append(lse_t(a, 0))
    ll = torch.stack(lls)
    (ll * torch.tensor(weight, dtype=f64)).sum().backward()
    return ll.detach().numpy(), obs.grad.numpy(), grad_or_zero(lP).numpy(), l0.grad.numpy()


def close(tag, a, b, rel=1e-4):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max()
    print(f"{tag}: err / largest entry {err / scale:.2e} (allowed {rel:.0e})")
    assert np.isfinite(a).all() and err <= rel * scale, (tag, err, scale)


GRAD_CASES = A_NARROW


def run_sequence_loglik(c, weight, guard):
    from pytorch_hmm_amd import ops
    from pytorch_hmm_amd.autograd import SequenceLogLik
    obs, lP, l0, lens = gpu(c)
    for t in (obs, lP, l0):
        t.requires_grad_(True)
    host = None if lens is None else ops.active_lengths(lens, c["B"], c["T"], c["N"])
    ll = SequenceLogLik.apply(obs, lP, l0, ops.OBS_LOG, "exact", None, host, guard)
    (ll * dev(weight)).sum().backward()
    return ll.detach(), obs.grad, grad_or_zero(lP), l0.grad


def run_sparse_loglik(c, weight, guard):
    from pytorch_hmm_amd import ops
    from pytorch_hmm_amd.autograd import SparseLogLik
    obs, _, l0, lens = gpu(c)
    tr = sparse_on_gpu(c)
    w = tr.log_w.clone()
    for t in (obs, w, l0):
        t.requires_grad_(True)
    host = None if lens is None else ops.ragged_lengths(lens, c["B"], c["T"])
    ll = SparseLogLik.apply(obs, w, l0, tr, host, guard)
    (ll * dev(weight)).sum().backward()
    return ll.detach(), obs.grad, grad_or_zero(w), l0.grad


def check_gradients(tag, c, got, want, arcs):
    ll, g_obs, g_P, g_0 = got
    wll, wobs, wP, w0 = want
    check_loglik(tag, ll, wll)
    valid = valid_mask(c)[..., None]
    close(tag + " d/d log_obs", np.where(valid, g_obs.cpu().numpy(), 0.0), np.where(valid, wobs, 0.0))
    assert bool((g_obs.cpu()[~torch.from_numpy(valid_mask(c))] == 0).all()), tag
    close(tag + " d/d log_P", g_P.cpu().numpy(), wP[c["src"], c["dst"]] if arcs else wP)
    close(tag + " d/d log_p0", g_0.cpu().numpy(), w0)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_a_sequence_loglik_gradients(name):
    c = CASES[name]
    weight = np.linspace(0.5, 2.0, c["B"])
    want = autograd_reference(c, weight)
    check_gradients(f"{name} SequenceLogLik", c, run_sequence_loglik(c, weight, False), want, arcs=False)
    check_gradients(f"{name} SparseLogLik", c, run_sparse_loglik(c, weight, False), want, arcs=True)


def test_a_posterior_sample_stays_on_the_graph():
    """Every sampled transition is an arc and every sampled state can emit its frame."""
    from pytorch_hmm_amd import ops
    for name in ("A-zeros-skip-N65-T70", "A-zeros-skip-N200-T230", "A-zeros-skip-N65-T70-ragged"):
        c = CASES[name]
        obs, lP, l0, lens = gpu(c)
        gen = torch.Generator(device=DEV).manual_seed(5)
        states, loglik = ops.posterior_sample(obs, lP, l0, ops.OBS_LOG, 16, lengths=lens, generator=gen)
        check_loglik(name + " posterior_sample", loglik, reference(name)["loglik"])
        z = states.cpu().numpy()                                          # (B,K,T)
        n = np.full(c["B"], c["T"]) if c["lengths"] is None else c["lengths"]
        for b in range(c["B"]):
            zb = z[b, :, :n[b]]
            assert (zb >= 0).all() and (z[b, :, n[b]:] == -1).all(), name
            assert np.isfinite(c["log_P"][zb[:, :-1], zb[:, 1:]]).all(), name
            assert np.isfinite(c["log_obs"][b][np.arange(n[b])[None, :], zb]).all(), name
            assert np.isfinite(c["log_p0"][zb[:, 0]]).all(), name


# =========================================================================== class B
def feasible(name):
    return np.isfinite(reference(name)["loglik"])


@pytest.mark.parametrize("name", B_NAMES)
def test_b_e_step_guarded(name):
    from pytorch_hmm_amd import em
    c, ref = CASES[name], reference(name)
    obs, lP, l0, lens = gpu(c)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    es = em.e_step(obs, lP, l0, lens, range_guard=GUARD)
    torch.cuda.synchronize()
    print(f"{name}: guarded e_step took {(time.perf_counter() - t0) * 1e3:.1f} ms")
    tag = f"{name} e_step guarded"
    check_loglik(tag, es.loglik, ref["loglik"])
    check_gamma(tag, es.gamma, ref, c)
    check_counts(tag, es.xi, es.gamma0, ref, c["log_P"])


@pytest.mark.parametrize("name", B_NAMES)
def test_b_e_step_guarded_with_a_plan(name):
    """The detector over the rows of the banded chains (make_plan) and of the dense chains a dense
    plan selects: the same results as without a plan."""
    from pytorch_hmm_amd import em, ops
    c, ref = CASES[name], reference(name)
    obs, lP, l0, _ = gpu(c)
    for dense in (False, True):
        es = em.e_step(obs, lP, l0, None, ops.make_plan(lP, dense=dense), range_guard=GUARD)
        tag = f"{name} e_step guarded, {'dense' if dense else 'banded'} plan"
        check_loglik(tag, es.loglik, ref["loglik"])
        check_gamma(tag, es.gamma, ref, c)
        check_counts(tag, es.xi, es.gamma0, ref, c["log_P"])


@pytest.mark.parametrize("name", [n for n in A_FULL if CASES[n]["T"] >= 33])
def test_a_e_step_with_a_plan_flags_nothing(name):
    from pytorch_hmm_amd import em, ops
    c = CASES[name]
    obs, lP, l0, _ = gpu(c)
    plan = ops.make_plan(lP)
    raw, guarded = em.e_step(obs, lP, l0, None, plan, range_guard=False), em.e_step(obs, lP, l0, None, plan)
    check_gamma(f"{name} e_step with a plan", raw.gamma, reference(name), c)
    assert torch.equal(raw.loglik, guarded.loglik) and torch.equal(raw.gamma, guarded.gamma), name
    assert torch.equal(raw.xi, guarded.xi), name


def test_b_mixture_layer_log_likelihood_guarded():
    """MixtureGaussianHMMLayer.log_likelihood on a fixed left-to-right transition_matrix (exact
    zeros) with one outlier frame: the frame lies on state 0's mean after the path has left state 0
    by three frames of 112 nats each, so the row's leader holds no fp32 mass and the states that do
    are flushed.  Guarded, the layer gives the log-space value; unguarded it does not."""
    import pytorch_hmm_amd as ph
    S, D, C, T = 8, 2, 2, 24
    rng = np.random.default_rng(20260405)
    layer = ph.MixtureGaussianHMMLayer(S, D, C, learnable_transitions=False).to(DEV)
    with torch.no_grad():
        layer.means.copy_(dev(15.0 * np.arange(S)[:, None, None] + 0.5 * rng.standard_normal((S, C, D))))
    path = np.minimum(S - 1, 1 + np.arange(T) // 3)
    x = 15.0 * path[None, :, None] + rng.standard_normal((3, T, D))
    x[1, 4] = 0.3 * rng.standard_normal(D)                               # the outlier, on state 0's mean
    lens = np.array([T, T, T - 5])
    xd = dev(x)
    with torch.no_grad():
        log_P, log_p0, log_w = layer._em_model(xd.device)
        lp = ph.ops.gmm_diag_logprob(xd, layer.means.detach(), layer._component_log_vars().detach(), log_w, 1)
    for lengths in (None, lens):
        ref = lsn.forward_backward(lp.cpu().numpy(), log_P.cpu().numpy(), log_p0.cpu().numpy(), lengths)["loglik"]
        assert np.isfinite(ref).all()
        check_loglik("mixture layer log_likelihood guarded", layer.log_likelihood(xd, lengths, range_guard=GUARD), ref)
        raw = layer.log_likelihood(xd, lengths, range_guard=False).cpu().numpy().astype(np.float64)
        print(f"mixture layer: reference {ref}, unguarded {raw}")
        assert not np.isfinite(raw[1]) or abs(raw[1] - ref[1]) > 1.0       # the case is the hazard
        assert np.abs(raw[[0, 2]] - ref[[0, 2]]).max() <= 2e-6 * np.abs(ref).max()


@pytest.mark.parametrize("name", B_NAMES)
def test_b_sparse_e_step_guarded(name):
    import pytorch_hmm_amd as ph
    from pytorch_hmm_amd import sparse
    c, ref = CASES[name], reference(name)
    obs, _, l0, lens = gpu(c)
    tr = sparse_on_gpu(c)
    loglik, gamma, xi = sparse.sparse_e_step(tr, obs, l0, lengths=lens, range_guard=GUARD)
    check_sparse(f"{name} sparse guarded", c, ref, loglik, gamma, xi)
    if GUARD:
        # the module's methods are guarded by default
        hmm = ph.SparseHMM(tr, l0).to(DEV)
        ll2, g2, xi2, _ = hmm.e_step(obs, lens)
        assert torch.equal(ll2, loglik) and torch.equal(g2, gamma) and torch.equal(xi2, xi)
        check_loglik(f"{name} SparseHMM.log_likelihood", hmm.log_likelihood(obs, lens).detach(), ref["loglik"])


@pytest.mark.parametrize("name", B_NAMES)
def test_b_loglik_gradients_guarded(name):
    c = CASES[name]
    weight = np.linspace(0.5, 2.0, c["B"])
    want = autograd_reference(c, weight)
    check_gradients(f"{name} SequenceLogLik guarded", c, run_sequence_loglik(c, weight, GUARD), want, arcs=False)
    check_gradients(f"{name} SparseLogLik guarded", c, run_sparse_loglik(c, weight, GUARD), want, arcs=True)


def test_b_batch_neighbours_keep_their_bits():
    """The in-range sequences of B-batch come out as from a call without the other two; the
    infeasible sequence gives -inf and exact zeros."""
    from pytorch_hmm_amd import em, sparse
    c = CASES["B-batch"]
    obs, lP, l0, _ = gpu(c)
    keep = list(rc.BATCH_IN_RANGE)
    whole = em.e_step(obs, lP, l0, range_guard=GUARD)
    alone = em.e_step(obs[keep], lP, l0, range_guard=GUARD)
    assert torch.equal(whole.loglik[keep], alone.loglik) and torch.equal(whole.gamma[keep], alone.gamma)
    assert float(whole.loglik[rc.BATCH_INFEASIBLE]) == -np.inf
    assert bool((whole.gamma[rc.BATCH_INFEASIBLE] == 0).all())
    tr = sparse_on_gpu(c)
    ll, g, _ = sparse.sparse_e_step(tr, obs, l0, range_guard=GUARD)
    ll1, g1, _ = sparse.sparse_e_step(tr, obs[keep], l0, range_guard=GUARD)
    assert torch.equal(ll[keep], ll1) and torch.equal(g[keep], g1)
    assert float(ll[rc.BATCH_INFEASIBLE]) == -np.inf and bool((g[rc.BATCH_INFEASIBLE] == 0).all())


# ----------------------------------------------------------------- class B, raw ops
def check_clean(tag, loglik, post, others=()):
    ll = loglik.cpu().numpy()
    ga = post.cpu().numpy().astype(np.float64)
    rows = ga.sum(-1)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(rows - 1.0) <= 1e-4) | (np.abs(ga).max(-1) == 0)
    nan_others = [bool(torch.isnan(o).any()) for o in others]
    print(f"{tag}: raw loglik {ll}, gamma NaN {int(np.isnan(ga).sum())} inf {int(np.isinf(ga).sum())}, "
          f"rows neither 1 nor 0: {int((~ok).sum())}, NaN in the other outputs {nan_others}")
    assert not np.isnan(ll).any() and np.all((ll == -np.inf) | np.isfinite(ll)), (tag, ll)
    assert np.isfinite(ga).all(), tag
    assert ok.all(), (tag, rows[~ok])
    assert not any(nan_others), tag


def two_lengths(c):
    """The case's sequences twice, the copies one frame shorter: unequal lengths, so the ragged
    kernels run (equal lengths dispatch to the plain chains)."""
    obs = np.concatenate([c["log_obs"], c["log_obs"]])
    lens = np.concatenate([np.full(c["B"], c["T"]), np.full(c["B"], c["T"] - 1)]).astype(np.int64)
    return dev(obs), torch.from_numpy(lens)


RAW_PATHS = ("chain", "plan", "pair", "dense-plan", "wide", "ragged", "tv", "sparse")


@pytest.mark.parametrize("path", RAW_PATHS)
@pytest.mark.parametrize("name", B_NAMES)
def test_b_raw_ops_fail_cleanly(name, path):
    """The raw ops are in-range only, but out of range they must still fail cleanly: no NaN, loglik
    finite or -inf, every gamma row a distribution or all zero.

    Before the row passes were repaired 29 of these 36 cases failed on the MI355X: the dense, banded
    and tv chains gave NaN loglik, NaN gamma rows and NaN forward / backward once the forward row
    died (B-outlier, B-deadend, B-survivor, both bad sequences of B-batch); every path gave NaN and
    inf gamma entries on B-latewinner / B-earlywinner (and NaN arc counts in the sparse form), the
    sparse form also on B-survivor.  The device keeps fp32 denormals, so `s > 0 ? 1 / s : 0` let
    1 / denormal = inf through, and the library is built with -fno-honor-nans, under which a float
    compare does not reliably stop a NaN.  The row passes, the chains' exp flush, the arc counts and
    the loglik stores now test the bits (csrc/common.h rcp_normal, row_value, clean_loglik)."""
    from pytorch_hmm_amd import ops, sparse
    c = CASES[name]
    obs, lP, l0, _ = gpu(c)
    tag = f"{name} raw {path}"
    if path in ("chain", "plan", "pair", "dense-plan", "wide"):
        # (pair: both chains in one workgroup where the table is banded -- every class B table but
        # B-deadend's is; wide: the batch-tiled form of more than 256 states, forced at this size)
        plan = None if path in ("chain", "wide") else ops.make_plan(lP, dense=path == "dense-plan")
        post, fwd, bwd, loglik, _ = ops.forward_backward(obs, lP, l0, ops.OBS_LOG, ALL3, plan,
                                                         True if path == "pair" else None, None,
                                                         True if path == "wide" else None)
        check_clean(tag, loglik, post, (fwd, bwd))
    elif path == "ragged":
        obs2, lens2 = two_lengths(c)
        post, fwd, bwd, loglik, _ = ops.forward_backward_ragged(obs2, lP, l0, ops.OBS_LOG, lens2, ALL3)
        check_clean(tag, loglik, post, (fwd, bwd))
    elif path == "tv":
        post, fwd, bwd, loglik, _ = ops.tv_forward_backward(obs, lP, l0, ALL3)
        check_clean(tag, loglik, post, (fwd, bwd))
    else:
        obs2, lens2 = two_lengths(c)
        loglik, post, xi = sparse.sparse_e_step(sparse_on_gpu(c), obs2, l0, lengths=lens2, range_guard=False)
        check_clean(tag, loglik, post, (xi,))


def test_b_raw_neighbours_unaffected():
    from pytorch_hmm_amd import ops, sparse
    c = CASES["B-batch"]
    obs, lP, l0, _ = gpu(c)
    keep = list(rc.BATCH_IN_RANGE)
    whole = ops.forward_backward(obs, lP, l0, ops.OBS_LOG, ALL3)
    alone = ops.forward_backward(obs[keep], lP, l0, ops.OBS_LOG, ALL3)
    for a, b in zip(whole, alone):
        assert torch.equal(a[keep], b)
    ref = reference("B-batch")
    check_loglik("B-batch raw, in-range sequences", whole[3][keep], ref["loglik"][keep])
    for form in ("pair", "wide", "tv"):
        if form == "tv":
            whole, alone = ops.tv_forward_backward(obs, lP, l0, ALL3), ops.tv_forward_backward(obs[keep], lP, l0, ALL3)
        else:
            plan = ops.make_plan(lP) if form == "pair" else None
            kw = dict(pair=True) if form == "pair" else dict(wide=True)
            whole = ops.forward_backward(obs, lP, l0, ops.OBS_LOG, ALL3, plan, **kw)
            alone = ops.forward_backward(obs[keep], lP, l0, ops.OBS_LOG, ALL3, plan, **kw)
        for a, b in zip(whole, alone):
            assert torch.equal(a[keep], b), form
        check_loglik(f"B-batch raw {form}, in-range sequences", whole[3][keep], ref["loglik"][keep])
    lens = torch.tensor([c["T"], c["T"], c["T"] - 3, c["T"]])
    whole = ops.forward_backward_ragged(obs, lP, l0, ops.OBS_LOG, lens, ALL3)
    alone = ops.forward_backward_ragged(obs[keep], lP, l0, ops.OBS_LOG, lens[keep], ALL3)
    for a, b in zip(whole, alone):
        assert torch.equal(a[keep], b)
    tr = sparse_on_gpu(c)
    ll, g, _ = sparse.sparse_e_step(tr, obs, l0, range_guard=False)
    ll1, g1, _ = sparse.sparse_e_step(tr, obs[keep], l0, range_guard=False)
    assert torch.equal(ll[keep], ll1) and torch.equal(g[keep], g1)
