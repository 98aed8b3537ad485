"""GPU: the banded chains (csrc/band.h, recur.h band_chain / rec_band, fbpair.h, the followers
of follow.h) on every window form they are instantiated for, with one floor for all rows and
with a floor per row.

The matrices come from oracle/band_model.py: the six Toeplitz offset ranges, a Toeplitz range
with a floor-valued slot, ranges outside the instantiated codes, general windows 2 / 4 / 8 wide
(and 9: dense), a ragged band, a permutation, tables banded in one direction only, all-floor
tables and rows, band entries one ulp above the floor, a row whose minimum is one isolated
entry, and random dense tables of 8 and 9 states.  `classify` (the host model of
band_prep_kernel) says which chain each selects; every case first asserts that this is the
chain it is built for, so none can drift onto the dense path unnoticed
(tests/test_band_model_cpu.py checks the model and the cases without a GPU).

Contracts (tests/test_gpu_band.py): Viterbi states and trellis bit-identical to the
C oracle through every path; forward-backward against the fp64 oracle with posterior atol 2e-5,
log-likelihood rtol 2e-6, forward / backward rtol 1e-4 where the oracle's value exceeds 1e-30.
A plan made with dense=True runs the dense chains on the same inputs: the control."""
import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

B, T = 2, 150            # ten 16-step blocks (the last ragged), three 64-step chunks (the last partial)
BASE_NS = (40, 100, 128, 200)          # NP = 64, 128 with padding, 128 exactly, 256
SMALL_NS = (1, 2, 3, 8, 9, 129)        # below the padded window widths; 8 | 9; NP = 256 mostly padding
SMALL_CASES = (M.TRI, "ragged", "rand_dense")
FLOORS = ("uniform", "per_row", "grid")
MIXED = ("mixed_col", "mixed_row")

CASE_NS = [(name, N) for name in M.CASES
           for N in BASE_NS + (SMALL_NS if name in SMALL_CASES else ()) if M.case_exists(name, N)]


def t(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def ops():
    from pytorch_hmm_amd import ops as o
    return o


def case_rng(name, N, floors):
    return np.random.default_rng([M.CASES.index(name), N, FLOORS.index(floors)])


def guarded_case(name, N, floors):
    """The case's table, its rng and its classification -- after the coverage guard: the chains
    the host model selects at this NP are the ones the case is built to hit."""
    rng = case_rng(name, N, floors)
    L = M.band_case(name, N, floors, rng)
    c = M.classify(L)
    assert (c["col_chain"], c["row_chain"]) == M.expected_chains(name, N), (name, N, floors, c)
    u = M.expected_uniform(name, N, floors)
    assert u is None or c["uniform_floor"] == int(u), (name, N, floors, c)
    return L, rng, c


def log_p0(N, rng, grid=False):
    if grid:
        return (-0.25 * rng.integers(0, 5, N)).astype(np.float32)
    p = rng.random(N) + 0.1
    return np.log(p / p.sum()).astype(np.float32)


# ------------------------------------------------------------------------ band_prep_kernel
@pytest.mark.parametrize("name", M.CASES)
def test_plan_header_matches_model(name):
    """make_plan's header (hulls through LDS atomics, the dense short-cut, empty hulls, N below
    64 lanes) equals the host model field for field."""
    o = ops()
    ns = [N for n, N in CASE_NS if n == name]
    assert ns
    for N in ns:
        for floors in FLOORS:
            L, _, c = guarded_case(name, N, floors)
            plan = o.make_plan(t(L))
            info = o.plan_info(plan)
            assert {k: info[k] for k in M.HEADER_KEYS} == {k: c[k] for k in M.HEADER_KEYS}, (name, N, floors)
            assert plan._hmm355_banded == c["banded"] == (c["wc"] <= 8 and c["wr"] <= 8), (name, N, floors)
            # a dense-forced plan keeps the measured tables and selects the dense chains
            forced = o.plan_info(o.make_plan(t(L), dense=True))
            assert (forced["forward"], forced["backward"], forced["viterbi"]) == ("dense",) * 3


# --------------------------------------------------------------------------------- Viterbi
def viterbi_paths(o, L):
    """(label, plan, follow): no plan (structure detected per call); a plan with the work beside
    the chain (banded: log leaders + decode follower, else the psi followers); the same plan
    with the passes after the chain (vit_psi_kernel / psi_band_rows + vit_backtrace_kernel);
    the dense chains."""
    plan = o.make_plan(t(L))
    return (("no plan", None, None), ("plan", plan, None), ("plan, follow=False", plan, False),
            ("dense plan", o.make_plan(t(L), dense=True), None))


@pytest.mark.parametrize("name,N", CASE_NS)
def test_viterbi_structures_bitexact(name, N):
    o = ops()
    for floors in FLOORS:
        L, rng, c = guarded_case(name, N, floors)
        grid = floors == "grid"
        if grid:   # emissions on the 0.25 grid too: floor and window candidates tie, first index decides
            lo = (-0.25 * rng.integers(0, 9, (B, T, N))).astype(np.float32)
        else:
            lo = np.log(rng.random((B, T, N), dtype=np.float32) + np.float32(1e-8)).astype(np.float32)
        init = log_p0(N, rng, grid)
        cs, cd, _ = O.c_viterbi(lo, L, init)
        for label, plan, follow in viterbi_paths(o, L):
            states, delta, final = o.viterbi(t(lo), t(L), t(init), o.OBS_LOG, plan, follow)
            msg = f"{name} N={N} {floors}: {label} ({c['col_chain']})"
            assert np.array_equal(delta.cpu().numpy(), cd), msg
            assert np.array_equal(states.cpu().numpy(), cs), msg
            assert np.array_equal(final.cpu().numpy(), cd[:, -1].max(-1)), msg


@pytest.mark.parametrize("Tn", [1, 17])
def test_viterbi_per_row_tridiagonal_short(Tn):
    """T = 1 (no step at all) and 17 (one step into the second block), per-row floors."""
    o = ops()
    for N in (100, 200):
        L, rng, c = guarded_case(M.TRI, N, "per_row")
        lo = np.log(rng.random((B, Tn, N), dtype=np.float32) + np.float32(1e-8)).astype(np.float32)
        init = log_p0(N, rng)
        cs, cd, _ = O.c_viterbi(lo, L, init)
        for label, plan, follow in viterbi_paths(o, L):
            states, delta, _ = o.viterbi(t(lo), t(L), t(init), o.OBS_LOG, plan, follow)
            assert np.array_equal(delta.cpu().numpy(), cd), (N, label)
            assert np.array_equal(states.cpu().numpy(), cs), (N, label)


def test_viterbi_prob_input_per_row_floor():
    """OBS_PROB through the banded plan: the log leaders feed a chain with per-row floors.
    Tolerances of test_viterbi_end_to_end_prob_input: states exact, delta rtol 2e-6 (a 1-ulp
    difference of an emission's log is the only source)."""
    o = ops()
    N = 128
    L, rng, c = guarded_case(M.TRI, N, "per_row")
    assert c["col_chain"] == "tw3 d0=-1" and c["banded"]
    obs = rng.random((B, T, N), dtype=np.float32)
    init = log_p0(N, rng)
    lo = np.log((obs + np.float32(1e-8)).astype(np.float64)).astype(np.float32)   # fp32 sum, rounded log
    cs, cd, _ = O.c_viterbi(lo, L, init)
    plan = o.make_plan(t(L))
    assert plan._hmm355_banded
    states, delta, _ = o.viterbi(t(obs), t(L), t(init), o.OBS_PROB, plan)
    assert np.array_equal(states.cpu().numpy(), cs)
    np.testing.assert_allclose(delta.cpu().numpy(), cd, rtol=2e-6, atol=1e-5)


# ------------------------------------------------------------------------ forward-backward
def check_fb(out, ref, msg):
    post, fwd, bwd, loglik, _ = (x.cpu().numpy() for x in out)
    la, lb, post64, ll64 = ref
    np.testing.assert_allclose(post, post64, atol=2e-5, rtol=0, err_msg=msg + " posterior")
    np.testing.assert_allclose(loglik, ll64, rtol=2e-6, err_msg=msg + " loglik")
    for got, lg, what in ((fwd, la, " forward"), (bwd, lb, " backward")):
        want = np.exp(lg)
        big = want > 1e-30
        np.testing.assert_allclose(got[big], want[big], rtol=1e-4, err_msg=msg + what)


@pytest.mark.parametrize("name,N", CASE_NS)
def test_fb_structures_vs_fp64(name, N):
    """(No case needed its eps range changed: the dense control holds the tolerances on all.)"""
    o = ops()
    for floors in ("uniform", "per_row"):
        L, rng, c = guarded_case(name, N, floors)
        obs = rng.random((B, T, N), dtype=np.float32)
        lp0 = log_p0(N, rng)
        ref = O.c_fb64(np.log(obs + np.float32(1e-8)), L, lp0)
        plan = o.make_plan(t(L))
        assert plan._hmm355_banded == c["banded"]
        # the control first: a case the dense chains miss is outside the contract
        runs = [("dense plan", o.make_plan(t(L), dense=True), None), ("no plan", None, None)]
        if c["banded"]:
            runs.append(("plan + followers", plan, False))
            if N <= 128:
                runs.append(("pair", plan, True))
        elif name in MIXED:
            # one recursion banded, the other dense: the pair kernel with the banded attribute
            # forced finds a dense chain on the device and falls back (fbpair.h), as in
            # test_pair_wrong_hint_falls_back_to_dense
            wrong = plan.clone()
            wrong._hmm355_banded = True
            runs.append(("pair, forced hint", wrong, True))
        for label, p, pair in runs:
            out = o.forward_backward(t(obs), t(L), t(lp0), o.OBS_PROB, 7, p, pair=pair)
            check_fb(out, ref, f"{name} N={N} {floors}: {label} ({c['col_chain']} / {c['row_chain']})")


@pytest.mark.parametrize("Tn", [1, 17])
def test_fb_per_row_tridiagonal_short(Tn):
    o = ops()
    for N in (100, 200):
        L, rng, c = guarded_case(M.TRI, N, "per_row")
        obs = rng.random((B, Tn, N), dtype=np.float32)
        lp0 = log_p0(N, rng)
        ref = O.c_fb64(np.log(obs + np.float32(1e-8)), L, lp0)
        plan = o.make_plan(t(L))
        runs = [("dense plan", o.make_plan(t(L), dense=True), None), ("no plan", None, None),
                ("plan + followers", plan, False)] + ([("pair", plan, True)] if N <= 128 else [])
        for label, p, pair in runs:
            out = o.forward_backward(t(obs), t(L), t(lp0), o.OBS_PROB, 7, p, pair=pair)
            check_fb(out, ref, f"N={N} T={Tn}: {label}")


def test_loglik_gradient_per_row_floor():
    """The adjoint runs the banded beta chain from a terminal vector (binit) with a floor per
    row (non-uniform afl); fp64 autograd through the reference loop, 1e-4 of the largest entry
    (test_gpu_autograd.py's comparison)."""
    from test_gpu_autograd import close, oracle_grads
    from pytorch_hmm_amd.autograd import SequenceLogLik
    o = ops()
    Bn, Tn, N = 2, 30, 70
    L, rng, c = guarded_case(M.TRI, N, "per_row")
    assert c["row_chain"] == "tw3 d0=-1" and c["uniform_floor"] == 0
    lP, lp0 = torch.from_numpy(L), torch.from_numpy(log_p0(N, rng))
    obs = torch.from_numpy(rng.random((Bn, Tn, N), dtype=np.float32) * 0.9 + 0.1)
    for kind in ("exact", "ref"):
        ll_ref, g_obs, g_lP, g_lp0, w = oracle_grads(obs, lP, lp0, kind)
        for use_plan in (False, True):
            ob = obs.to(DEV).requires_grad_(True)
            P_ = lP.to(DEV).requires_grad_(True)
            p0 = lp0.to(DEV).requires_grad_(True)
            plan = o.make_plan(P_.detach()) if use_plan else None
            ll = SequenceLogLik.apply(ob, P_, p0, o.OBS_PROB, kind, plan)
            (ll * w.float().to(DEV)).sum().backward()
            np.testing.assert_allclose(ll.detach().cpu().numpy(), ll_ref.numpy(), rtol=2e-5, atol=2e-5)
            close(ob.grad.cpu(), g_obs)
            close(P_.grad.cpu(), g_lP)
            close(p0.grad.cpu(), g_lp0)
