"""GPU: ops.hsmm_forward_backward (csrc/hsmm_fb.hip), autograd.HsmmLogLik and the HSMMLayer methods
built on them, every output against the fp64 numpy model (tests/hsmm_fb_numpy.py).

Allowances.  The model was run in float32 against float64 over exactly the cases of this file
(tools/measure_hsmm_fb_tolerance.py; CPU only) and the largest error per quantity taken; the GPU
is allowed 8x that, for its different summation order and the 1-2 ulp of the hardware exp / log
against numpy's.  Both the absolute and the relative bound of a quantity must hold.  Relative
errors of counts are taken over counts >= COUNT_FLOOR: below it a count is a rounding-sized share
of a segment and only its absolute error says anything.

    quantity                                fp32 model, largest of 585 calls    allowance (8x)
    loglik       absolute                   3.945e-04  (large-emissions)        3.16e-03
    loglik       relative to max(|.|, 1)    2.611e-06  (dead-end-leader)        2.09e-05
    gamma        absolute                   1.445e-04  (S5-D64-T197)            1.16e-03
    init_post    absolute                   6.322e-05  (S5-D64-T197)            5.06e-04
    dur_counts   absolute                   1.653e-03  (S5-D64-T197)            1.32e-02
    dur_counts   relative (>= floor)        1.070e-04  (S5-D64-T197)            8.56e-04
    trans_counts absolute                   1.200e-03  (S2-D65-T200)            9.60e-03
    trans_counts relative (>= floor)        8.160e-05  (S63-D65-T200)           6.53e-04
    layer gradients, relative to the gradient's max-norm   2.568e-06            2.05e-05

The absolute errors of the counts are those of counts in the tens (a two-state model changes
state a hundred times in 200 frames); their relative errors are the 1e-4 of an fp32 exponent of
magnitude 1e3.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import hsmm_fb_numpy as M  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR = 8.0
LL_ABS = FACTOR * 3.945e-04
LL_REL = FACTOR * 2.611e-06
GAMMA_ABS = FACTOR * 1.445e-04
INIT_ABS = FACTOR * 6.322e-05
DUR_ABS = FACTOR * 1.653e-03
DUR_REL = FACTOR * 1.070e-04
TRANS_ABS = FACTOR * 1.200e-03
TRANS_REL = FACTOR * 8.160e-05
LAYER_GRAD_REL = FACTOR * 2.568e-06
COUNT_FLOOR = 1e-3

GOLDEN = os.path.join(HERE, "golden")
FIXTURES = ("hsmm_s2", "hsmm_s5", "hsmm_s8", "hsmm_d96")
OUTPUTS = ("loglik", "gamma", "dur_counts", "trans_counts", "init_post")
STATES = (1, 2, 5, 63, 64, 65, 256)
DURATIONS = (1, 2, 40, 64, 65, 128)
MAX_CELLS = 16384
# The chain kernel has one body and three placements of its tables, chosen by size
# (csrc/hsmm_fb.hip, placement() below): log_T and dur_lp both in LDS beside the ring, log_T in LDS
# and dur_lp read from memory, log_T read from memory and dur_lp in LDS.  Both sides of each switch:
# at S = 128 dur_lp leaves LDS between Dmax = 90 and 91; at S = 160 log_T leaves it (and dur_lp
# returns) between Dmax = 88 and 89; (128, 128) and (160, 102) are the largest rings of each.
PLACEMENT_PAIRS = [(128, 90), (128, 91), (128, 128), (160, 88), (160, 89), (160, 102)]
PAIRS = [(S, Dm) for S in STATES for Dm in DURATIONS if S * Dm <= MAX_CELLS] + PLACEMENT_PAIRS


def placement(S, Dm, budget=159 * 1024):
    """(log_T in LDS, dur_lp in LDS) as hmm355_hsmm_fb_f32 chooses them: the lanes per state, then
    the ring and the step rows, log_T at row stride S + lanes if it fits, dur_lp if it still fits."""
    sub = 64
    while sub > 1 and S * sub > 1024:
        sub >>= 1
    while sub > 1 and (sub >> 1) >= max(S, Dm):
        sub >>= 1
    lds = (S * Dm + 2 * S) * 4
    lt = lds + S * (S + sub) * 4 <= budget
    if lt:
        lds += S * (S + sub) * 4
    return lt, lds + S * Dm * 4 <= budget


# ------------------------------------------------------------------------------------ cases
# (everything below this line down to "the GPU side" runs without a GPU: the tolerance tool
# imports it)
def lengths(Dm):
    """T in {1, 2, Dmax-1, Dmax, Dmax+1, 3 Dmax+5}, capped at 200, T >= 1, without repeats"""
    return sorted({min(200, t) for t in (1, 2, Dm - 1, Dm, Dm + 1, 3 * Dm + 5) if t >= 1})


def random_tables(B, T, S, Dm, seed):
    rng = np.random.default_rng(seed)
    lp = rng.normal(-5.0, 3.0, (B, T, S)).astype(np.float32)
    du = np.log(rng.random((S, Dm)) + 1e-3).astype(np.float32)
    lt = np.log(rng.random((S, S)) + 1e-3).astype(np.float32)
    li = np.log(rng.random(S) + 1e-3).astype(np.float32)
    return lp, du, lt, li


def boundary_cases(S, Dm):
    """The calls of one (S, Dmax) pair: at every length a batch of three with log_init given and
    its first sequence alone with log_init None; at T = Dmax + 1 the other two combinations."""
    out = []
    for T in lengths(Dm):
        lp, du, lt, li = random_tables(3, T, S, Dm, 1000 * S + 10 * Dm + T)
        out.append((f"S{S}-D{Dm}-T{T}-B3-init", lp, du, lt, li))
        out.append((f"S{S}-D{Dm}-T{T}-B1", lp[:1], du, lt, None))
        if T == min(200, Dm + 1):
            out.append((f"S{S}-D{Dm}-T{T}-B3", lp, du, lt, None))
            out.append((f"S{S}-D{Dm}-T{T}-B1-init", lp[:1], du, lt, li))
    return out


def fixture_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=True)
    return (name, z["log_probs"], z["dur_log_probs"], z["log_T"], None)


def case_min_duration():
    lp, du, lt, li = random_tables(3, 40, 5, 8, 11)
    du[:, :2] = -np.inf   # no segment shorter than 3 frames
    return ("min-duration", lp, du, lt, li)


def case_left_to_right():
    lp, du, _, _ = random_tables(3, 30, 6, 10, 12)
    lt = np.full((6, 6), -np.inf, np.float32)
    lt[np.arange(5), np.arange(1, 6)] = np.log(np.float32(0.9))
    return ("left-to-right", lp, du, lt, None)


def case_scattered():
    lp, du, lt, li = random_tables(3, 40, 5, 7, 13)
    hole = np.random.default_rng(14).random(lp.shape) < 0.12
    hole[..., 0] = False  # state 0 is always allowed: no frame loses every state
    lp[hole] = -np.inf
    return ("scattered", lp, du, lt, li)


def case_infeasible_middle():
    lp, du, lt, li = random_tables(3, 25, 4, 6, 15)
    lp[1, 9, :] = -np.inf   # no state can take frame 9 of the middle sequence
    return ("infeasible-middle", lp, du, lt, li)


def case_dead_end_leader():
    """State 0 leads by 200 nats per frame in the first two frames and has no way out; it cannot
    span the six frames (Dmax = 2), so every segmentation avoids it there.  A per-step maximum
    shared by all target states would be state 0's and flush the others' 200 nats below it."""
    lp, du, lt, _ = random_tables(2, 6, 3, 2, 16)
    lp[:, :2, 0] = 200.0
    lt[0, :] = -np.inf
    return ("dead-end-leader", lp, du, lt, None)


def case_large_emissions():
    rng = np.random.default_rng(17)
    _, du, lt, li = random_tables(2, 64, 8, 10, 17)
    lp = rng.normal(-300.0, 30.0, (2, 64, 8)).astype(np.float32)
    return ("large-emissions", lp, du, lt, li)


def case_gradient():
    lp, du, lt, li = random_tables(3, 23, 5, 7, 18)
    return ("gradient", lp, du, lt, li)


SPECIAL = (case_min_duration, case_left_to_right, case_scattered, case_infeasible_middle, case_dead_end_leader,
           case_large_emissions, case_gradient)

_REF = {}


def reference(case):
    """the fp64 model of a case, computed once"""
    name, lp, du, lt, li = case
    if name not in _REF:
        _REF[name] = M.hsmm_fb(lp, du, lt, li)
    return _REF[name]


def errors(got, ref):
    """The error figures of one call: got and ref are dicts of the five outputs."""
    r = {k: np.asarray(ref[k], np.float64) for k in OUTPUTS}
    g = {k: np.asarray(got[k], np.float64) for k in OUTPUTS}
    fin = np.isfinite(r["loglik"])
    e = {"ll_abs": 0.0, "ll_rel": 0.0}
    if fin.any():
        d = np.abs(g["loglik"][fin] - r["loglik"][fin])
        e["ll_abs"] = float(d.max())
        e["ll_rel"] = float((d / np.maximum(np.abs(r["loglik"][fin]), 1.0)).max())
    e["ll_inf_ok"] = bool(np.array_equal(g["loglik"][~fin], r["loglik"][~fin]))
    e["gamma_abs"] = float(np.abs(g["gamma"] - r["gamma"]).max())
    e["init_abs"] = float(np.abs(g["init_post"] - r["init_post"]).max())
    for k, n in (("dur_counts", "dur"), ("trans_counts", "trans")):
        d = np.abs(g[k] - r[k])
        e[n + "_abs"] = float(d.max())
        big = r[k] >= COUNT_FLOOR
        e[n + "_rel"] = float((d[big] / r[k][big]).max()) if big.any() else 0.0
    return e


LIMITS = {"ll_abs": LL_ABS, "ll_rel": LL_REL, "gamma_abs": GAMMA_ABS, "init_abs": INIT_ABS, "dur_abs": DUR_ABS,
          "dur_rel": DUR_REL, "trans_abs": TRANS_ABS, "trans_rel": TRANS_REL}


def layer_tables64(p, x, Dm, eps=1e-8):
    """HSMMLayer's tables (gamma durations, min_duration 1) restated in float64 torch."""
    S, D = p["observation_means"].shape
    lv = p["observation_log_vars"]
    diff = x[:, :, None, :] - p["observation_means"][None, None]
    lp = -0.5 * (D * np.log(2 * np.pi) + lv.sum(-1)[None, None] + (diff * diff / lv.exp()[None, None]).sum(-1))
    d = torch.arange(1, Dm + 1, dtype=torch.float64)[None]
    shape = torch.nn.functional.softplus(p["duration_shape"])[:, None]
    rate = torch.nn.functional.softplus(p["duration_rate"])[:, None]
    dl = (shape - 1) * torch.log(d + eps) - rate * d - torch.lgamma(shape) + shape * torch.log(rate + eps)
    dur_lp = torch.log(torch.exp(dl) + eps)
    logits = p["transition_logits"].masked_fill(torch.eye(S, dtype=torch.bool), float("-inf"))
    log_T = torch.log(torch.softmax(logits, -1) + eps)
    return lp, dur_lp, log_T


def layer_loss64(lp, dur_lp, log_T):
    """-mean loglik by the forward recursion in log space (float64 torch loops; autograd through it
    is the reference gradient).  Finite tables only."""
    B, T, S = lp.shape
    Dm = dur_lp.shape[1]
    off = torch.zeros(S, S, dtype=torch.float64).masked_fill(torch.eye(S, dtype=torch.bool), float("-inf"))
    cs = torch.cat([torch.zeros(B, 1, S, dtype=torch.float64), lp.cumsum(1)], 1)
    begin = [torch.zeros(B, S, dtype=torch.float64)]
    F = []
    for t in range(T):
        cand = [begin[t - d + 1] + (cs[:, t + 1] - cs[:, t - d + 1]) + dur_lp[None, :, d - 1]
                for d in range(1, min(Dm, t + 1) + 1)]
        F.append(torch.logsumexp(torch.stack(cand, 0), 0))
        begin.append(torch.logsumexp(F[t][:, :, None] + (log_T + off)[None], 1))
    return -torch.logsumexp(F[T - 1], 1).mean()


def layer_params64(z):
    return {k: torch.tensor(np.asarray(z[k], np.float64), requires_grad=True)
            for k in ("observation_means", "observation_log_vars", "transition_logits", "duration_shape",
                      "duration_rate")}


# ------------------------------------------------------------------------------ the GPU side
DEV = torch.device("cuda", 0)


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def run_op(case, **kw):
    from pytorch_hmm_amd import ops
    _, lp, du, lt, li = case
    want = dict(want_gamma=True, want_dur=True, want_trans=True, want_init=True)
    want.update(kw)
    res = ops.hsmm_forward_backward(t(lp), t(du), t(lt), t(li), **want)
    return dict(zip(OUTPUTS, (r.cpu().numpy() for r in res)))


def check(case):
    got, ref = run_op(case), reference(case)
    for k in OUTPUTS:
        assert got[k].shape == np.asarray(ref[k]).shape, (case[0], k)
        assert not np.isnan(got[k]).any(), (case[0], k)
    e = errors(got, ref)
    print(case[0], " ".join(f"{k}={v:.3e}" for k, v in e.items() if k != "ll_inf_ok"))
    assert e["ll_inf_ok"], case[0]
    for k, lim in LIMITS.items():
        assert e[k] <= lim, (case[0], k, e[k], lim)
    return got, ref


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_tables(name):
    got, _ = check(fixture_case(name))
    np.testing.assert_allclose(got["gamma"].sum(-1), 1.0, atol=2 * GAMMA_ABS)


@pytest.mark.parametrize("S,Dm", PAIRS)
def test_random_tables_at_the_shape_boundaries(S, Dm):
    """One kernel body serves every size, with three placements of log_T and dur_lp (LDS or
    memory).  The issue's pairs take two of them (everything up to S = 65 holds both tables in
    LDS, S = 256 reads log_T from memory); PLACEMENT_PAIRS add the third and both sides of each
    switch (tests/test_hsmm_fb_cpu.py checks that against the host code's arithmetic)."""
    for case in boundary_cases(S, Dm):
        check(case)


@pytest.mark.parametrize("make", [case_min_duration, case_left_to_right, case_scattered])
def test_neg_inf_entries(make):
    got, ref = check(make())
    assert np.isfinite(ref["loglik"]).all()


def test_infeasible_sequence_in_a_batch():
    got, ref = check(case_infeasible_middle())
    assert got["loglik"][1] == -np.inf and np.isfinite(got["loglik"][[0, 2]]).all()
    for k in OUTPUTS[1:]:
        assert (got[k][1] == 0).all(), k
    # its neighbours are what they are alone
    _, lp, du, lt, li = case_infeasible_middle()
    alone = run_op(("alone", lp[[0, 2]], du, lt, li))
    for k in OUTPUTS:
        assert np.array_equal(alone[k], got[k][[0, 2]]), k


def test_dead_end_leader():
    got, ref = check(case_dead_end_leader())
    # state 0 can only be a segmentation's last segment (frames 4..5): nowhere before
    assert np.isfinite(got["loglik"]).all() and (got["gamma"][:, :4, 0] == 0).all()


def test_large_emissions():
    check(case_large_emissions())


@pytest.mark.parametrize("case", [fixture_case(n) for n in FIXTURES] + [case_gradient(), case_large_emissions()],
                         ids=lambda c: c[0])
def test_viterbi_score_bounds_the_likelihood(case):
    from pytorch_hmm_amd import ops
    _, lp, du, lt, _ = case
    best = ops.hsmm_viterbi(t(lp), t(du), t(lt))[1].cpu().numpy().astype(np.float64)
    ll = run_op((case[0], lp, du, lt, None), want_gamma=False, want_dur=False, want_trans=False,
                want_init=False)["loglik"].astype(np.float64)
    assert (best <= ll + np.minimum(LL_ABS, LL_REL * np.maximum(np.abs(ll), 1.0))).all(), (best, ll)


def test_semimarkov_forward_agrees():
    """With additive scores (seg_const None) SemiMarkovHMM's forward sums the same segmentations.
    Each kernel is within its own tolerance of the truth: this op's allowance plus the 2e-6
    relative that tests/test_gpu_semimarkov.py holds semimarkov_forward to."""
    from pytorch_hmm_amd import ops
    _, lp, du, lt, li = case_gradient()
    ours = run_op(("smk", lp, du, lt, li))["loglik"].astype(np.float64)
    theirs = ops.semimarkov_forward(t(lp), None, t(li), t(lt), t(du), False)[0].cpu().numpy().astype(np.float64)
    scale = np.maximum(np.abs(ours), 1.0)
    assert (np.abs(ours - theirs) <= np.minimum(LL_ABS, LL_REL * scale) + 2e-6 * scale).all(), (ours, theirs)


def test_two_calls_are_bit_identical():
    """There is one kernel form (HMM355_FORM_GENERAL is accepted and selects the same code), so
    the comparison is call against call and flag against no flag."""
    from pytorch_hmm_amd import ops
    for case in (case_gradient(), boundary_cases(65, 128)[-1], case_scattered()):
        a, b, c = run_op(case), run_op(case), run_op(case, flags=ops.FORM_GENERAL)
        for k in OUTPUTS:
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), (case[0], k)
        lik = run_op(case, want_gamma=False, want_dur=False, want_trans=False, want_init=False)
        assert np.array_equal(lik["loglik"], a["loglik"]) and lik["gamma"].shape == (0,)


@pytest.mark.parametrize("make", [case_gradient, case_min_duration])
def test_gradients(make):
    from pytorch_hmm_amd.autograd import HsmmLogLik
    case = make()
    _, lp, du, lt, li = case
    ref = reference(case)
    g = np.array([0.7, -1.3, 2.1], np.float32)
    ins = [t(a).requires_grad_() for a in (lp, du, lt, li)]
    ll = HsmmLogLik.apply(*ins)
    assert np.abs(ll.detach().cpu().numpy() - ref["loglik"]).max() <= LL_ABS
    (ll * t(g)).sum().backward()
    g1 = float(np.abs(g).sum())
    want = (g[:, None, None] * ref["gamma"], np.einsum("b,bsd->sd", g, ref["dur_counts"]),
            np.einsum("b,bij->ij", g, ref["trans_counts"]), np.einsum("b,bs->s", g, ref["init_post"]))
    tol = (np.abs(g).max() * GAMMA_ABS, g1 * DUR_ABS, g1 * TRANS_ABS, g1 * INIT_ABS)
    full = [x.grad.cpu().numpy() for x in ins]
    for name, got, w, tl in zip(("lp", "dur_lp", "log_T", "log_init"), full, want, tol):
        err = np.abs(got - w).max()
        print(case[0], name, f"{err:.3e}", f"{tl:.3e}")
        assert err <= tl, (name, err, tl)
    # only the inputs that need a gradient get one, and it is the same
    for subset in ((1,), (0, 3), (2,)):
        ins = [t(a).requires_grad_(i in subset) for i, a in enumerate((lp, du, lt, li))]
        (HsmmLogLik.apply(*ins) * t(g)).sum().backward()
        for i, x in enumerate(ins):
            assert (x.grad is not None) == (i in subset)
            if i in subset:
                assert np.array_equal(x.grad.cpu().numpy(), full[i]), (subset, i)
    # log_init None
    ins = [t(a).requires_grad_() for a in (lp, du, lt)]
    HsmmLogLik.apply(*ins, None).sum().backward()
    assert all(x.grad is not None for x in ins)


def test_layer():
    import pytorch_hmm_amd as ph
    z = np.load(os.path.join(GOLDEN, "hsmm_s5.npz"), allow_pickle=True)
    S, D, Dm = 5, 30, 20
    layer = ph.HSMMLayer(S, D, max_duration=Dm).to(DEV)
    names = ("observation_means", "observation_log_vars", "transition_logits", "duration_shape", "duration_rate")
    with torch.no_grad():
        for k in names:
            getattr(layer, k).copy_(t(z[k]))
    x = t(z["x"]).requires_grad_()
    ref = reference(fixture_case("hsmm_s5"))
    ll = layer.log_likelihood(x)
    d = np.abs(ll.detach().cpu().numpy() - ref["loglik"])
    print("layer loglik", d.max(), (d / np.abs(ref["loglik"])).max())
    assert d.max() <= LL_ABS and (d / np.abs(ref["loglik"])).max() <= LL_REL
    loss = layer.compute_loss(x)
    loss.backward()
    # the same layer in float64 on the CPU
    p = layer_params64(z)
    x64 = torch.tensor(np.asarray(z["x"], np.float64), requires_grad=True)
    loss64 = layer_loss64(*layer_tables64(p, x64, Dm))
    loss64.backward()
    assert abs(float(loss) - float(loss64)) <= LL_REL * abs(float(loss64))
    for k in names + ("x",):
        got = (x.grad if k == "x" else getattr(layer, k).grad)
        assert got is not None, k
        want = (x64.grad if k == "x" else p[k].grad).numpy()
        err = np.abs(got.cpu().numpy() - want).max() / np.abs(want).max()
        print("layer grad", k, f"{err:.3e}")
        assert err <= LAYER_GRAD_REL, (k, err)
    post = layer.state_posteriors(x.detach())
    assert post.shape == (2, 30, S) and not post.requires_grad
    np.testing.assert_allclose(post.sum(-1).cpu().numpy(), 1.0, atol=2 * GAMMA_ABS)
    np.testing.assert_allclose(post.cpu().numpy(), ref["gamma"], atol=GAMMA_ABS)
    states, _ = layer(x.detach())
    assert np.array_equal(states.cpu().numpy(), z["states"])
