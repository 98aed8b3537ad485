"""CPU: the conditions that keep tests/test_gpu_range.py honest, checked on the float64 log-space
reference (tests/logspace_numpy.py), the fp32 model of the kernels (tests/range_cases.py
scaled_model) and the range detector (pytorch_hmm_amd/range_guard.py) alone.

  - the reference equals brute-force enumeration of all paths on tiny models, -inf arcs, -inf
    emissions and an infeasible sequence included;
  - class A is in range: not one-hot (at least 10 % of the frames have max gamma < 0.9; the one
    exception is A-zeros-skip at T = 1, whose only frame is one-hot by its initial distribution),
    the fp32 model agrees with the reference, nothing flagged;
  - class B is the hazard: the fp32 model is wrong by more than a nat or not finite, all flagged;
  - fuzz: over 2000 small exact-zero models no sequence is both unflagged and wrong;
  - the torch fallback (range_guard.logspace_forward_backward) equals the numpy reference.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logspace_numpy as lsn  # noqa: E402
import range_cases as rc  # noqa: E402
import sparse_numpy as sn  # noqa: E402

from pytorch_hmm_amd import range_guard as rg  # noqa: E402

CASES = {c["name"]: c for c in rc.range_cases()}
A_NAMES = [n for n, c in CASES.items() if c["cls"] == "A"]
B_NAMES = [n for n, c in CASES.items() if c["cls"] == "B"]


def args(c):
    return c["log_obs"], c["log_P"], c["log_p0"], c["lengths"]


@functools.lru_cache(maxsize=None)
def reference(name):
    return lsn.forward_backward(*args(CASES[name]))


@functools.lru_cache(maxsize=None)
def model32(name):
    return rc.scaled_model(*args(CASES[name]), dtype=np.float32)


def detect(m, lengths):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    lens = None if lengths is None else torch.as_tensor(np.asarray(lengths))
    return rg.out_of_range(t(m["U"]), t(m["V"]), t(m["CA"]), lens, E=t(m["E"])).numpy()


def valid_mask(c):
    lens = np.full(c["B"], c["T"]) if c["lengths"] is None else c["lengths"]
    return np.arange(c["T"])[None, :] < np.asarray(lens)[:, None]


# ------------------------------------------------------------- the reference itself
def tiny_models():
    rng = np.random.default_rng(7)
    for k in range(12):
        N, T, B = int(rng.integers(1, 5)), int(rng.integers(1, 7)), 2
        log_P = np.log(rng.dirichlet(np.ones(N), N))
        log_P[rng.random((N, N)) < 0.3] = -np.inf                     # forbidden arcs
        log_p0 = np.log(rng.dirichlet(np.ones(N)))
        if N > 1:
            log_p0[rng.integers(0, N)] = -np.inf
        obs = rng.normal(size=(B, T, N)) * 3 - 2
        obs[rng.random((B, T, N)) < 0.15] = -np.inf                   # impossible emissions
        lengths = None if k % 2 else np.array([T, max(1, T // 2)])
        yield obs, log_P, log_p0, lengths
    # a sequence that no path explains beside one that has paths
    log_P = np.log(np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.0, 0.0, 1.0]]) + 0.0)
    obs = rng.normal(size=(2, 4, 3))
    obs[0, 1, :2] = -np.inf                                           # frame 1 needs state 2: too early
    yield obs, log_P, np.log(np.array([1.0, 0.0, 0.0])), None


def test_reference_equals_brute_force():
    seen_infeasible = seen_feasible = 0
    with np.errstate(divide="ignore"):
        for obs, log_P, log_p0, lengths in tiny_models():
            ref = lsn.forward_backward(obs, log_P, log_p0, lengths)
            bf = lsn.brute_force(obs, log_P, log_p0, lengths)
            fin = np.isfinite(bf["loglik"])
            assert np.array_equal(np.isfinite(ref["loglik"]), fin)
            assert np.all(ref["loglik"][~fin] == -np.inf)
            assert np.allclose(ref["loglik"][fin], bf["loglik"][fin], rtol=1e-12, atol=1e-12)
            for k in ("gamma", "xi", "gamma0"):
                assert np.isfinite(ref[k]).all()
                assert np.abs(ref[k] - bf[k]).max() <= 1e-12, k
            assert np.all(ref["gamma"][~fin] == 0)
            seen_infeasible += int((~fin).sum())
            seen_feasible += int(fin.sum())
    assert seen_infeasible >= 1 and seen_feasible >= 10


def test_arc_wrapper_equals_dense():
    c = CASES["A-zeros-skip-N5-T33"]
    ref = reference(c["name"])
    arcs = lsn.forward_backward_arcs(c["log_obs"], c["src"], c["dst"], c["log_w"], c["log_p0"], c["lengths"])
    assert np.array_equal(arcs["loglik"], ref["loglik"]) and np.array_equal(arcs["gamma"], ref["gamma"])
    assert np.array_equal(arcs["xi"], ref["xi"][c["src"], c["dst"]])
    assert ref["xi"].sum() == pytest.approx(arcs["xi"].sum())


def test_case_set_is_complete():
    for kind in rc.A_KINDS:
        for N, T in rc.A_SHAPES:
            assert f"A-{kind}-N{N}-T{T}" in CASES
        assert f"A-{kind}-N65-T70-ragged" in CASES
    for name in ("A-floor-l2r-N300-T40", "A-floor-jumpy-N300-T40", "A-rand-hub-N65-T70", "B-outlier", "B-deadend",
                 "B-latewinner", "B-earlywinner", "B-survivor", "B-batch"):
        assert name in CASES
    hub = CASES["A-rand-hub-N65-T70"]
    indeg = np.bincount(hub["dst"], minlength=65)
    assert indeg.max() > 64 and np.median(indeg) <= 11
    for c in CASES.values():
        assert np.array_equal(sn.densify(c["src"], c["dst"], c["log_w"], c["N"], np.float32), c["log_P"])
        if c["cls"] == "B":
            assert np.isinf(c["log_P"]).any()                         # exact zeros in every B table


# ------------------------------------------------------------------------ class A
@pytest.mark.parametrize("name", A_NAMES)
def test_class_a_is_in_range(name):
    c, ref, m = CASES[name], reference(name), model32(name)
    assert np.isfinite(ref["loglik"]).all()
    valid = valid_mask(c)
    top = ref["gamma"].max(-1)[valid]
    soft = float((top < 0.9).mean())
    rows = ref["gamma"].sum(-1)[valid]
    assert np.abs(rows - 1).max() <= 1e-9
    dg = float(np.abs(m["gamma"].astype(np.float64) - ref["gamma"])[valid].max())
    dl = float((np.abs(m["loglik"] - ref["loglik"]) / np.maximum(np.abs(ref["loglik"]), 1.0)).max())
    print(f"{name}: soft frames {soft:.2f}, fp32 model gamma err {dg:.2e}, loglik rel err {dl:.2e}")
    if c["T"] == 1 and np.isinf(c["log_p0"]).any():
        # one frame and an initial distribution on state 0 alone: gamma_0 is one-hot by construction,
        # the one A case that cannot meet the condition below
        assert soft == 0.0 and np.all(ref["gamma"][:, 0, 0] == 1.0)
    else:
        assert soft >= 0.10                                           # the posteriors are not one-hot
    assert dg <= 2e-5 and dl <= 2e-6                                  # the GPU tests' bounds hold for the model
    assert not detect(m, c["lengths"]).any()


def test_model32_matches_the_sparse_model():
    """scaled_model is sparse_numpy.sums on a dense matrix: the same recursion, another summation order."""
    c = CASES["A-zeros-skip-N65-T70-ragged"]
    m = model32(c["name"])
    s = sn.sums(c["log_obs"], c["src"], c["dst"], c["log_w"], c["log_p0"], c["lengths"], dtype=np.float32)
    assert np.abs(m["gamma"] - s["gamma"])[valid_mask(c)].max() <= 2e-6
    assert np.abs(m["loglik"] - s["loglik"]).max() <= 2e-6 * np.abs(s["loglik"]).max()


# ------------------------------------------------------------------------ class B
@pytest.mark.parametrize("name", B_NAMES)
def test_class_b_is_the_hazard(name):
    c, ref, m = CASES[name], reference(name), model32(name)
    feasible = np.ones(c["B"], bool)
    hazard = np.ones(c["B"], bool)
    if name == "B-batch":
        feasible[rc.BATCH_INFEASIBLE] = False
        hazard[:] = False
        hazard[rc.BATCH_OUT] = True
    assert np.array_equal(np.isfinite(ref["loglik"]), feasible)
    wrong = ~np.isfinite(m["loglik"]) | ~np.isfinite(m["gamma"]).all((1, 2))
    with np.errstate(invalid="ignore"):
        wrong |= np.abs(m["loglik"] - ref["loglik"]) > 1.0
    print(f"{name}: reference {ref['loglik']}, fp32 model {m['loglik']}")
    assert wrong[hazard].all()
    flag = detect(m, c["lengths"])
    assert flag[hazard].all()
    if name == "B-batch":
        assert not flag[list(rc.BATCH_IN_RANGE)].any() and not wrong[list(rc.BATCH_IN_RANGE)].any()
        assert ref["loglik"][rc.BATCH_INFEASIBLE] == -np.inf and m["loglik"][rc.BATCH_INFEASIBLE] == -np.inf


# --------------------------------------------------------------------------- fuzz
def test_fuzz_no_sequence_is_unflagged_and_wrong():
    rng = np.random.default_rng(20260404)
    feasible = wrong_n = flagged_n = missed = 0
    for _ in range(2000):
        obs, log_P, log_p0 = rc.fuzz_model(rng)
        ref = lsn.forward_backward(obs, log_P, log_p0)
        m = rc.scaled_model(obs, log_P, log_p0, dtype=np.float32)
        flag = detect(m, None)
        ll = ref["loglik"]
        fin = np.isfinite(ll)
        with np.errstate(invalid="ignore"):
            bad_ll = ~(np.abs(m["loglik"] - ll) <= 2e-6 * np.maximum(1.0, np.abs(ll)) + 1e-4)
            bad_g = ~(np.abs(m["gamma"].astype(np.float64) - ref["gamma"]).max((1, 2)) <= 2e-5)
        wrong = fin & (bad_ll | bad_g)
        feasible += int(fin.sum())
        wrong_n += int(wrong.sum())
        flagged_n += int((flag & fin).sum())
        missed += int((wrong & ~flag).sum())
    print(f"fuzz: {feasible} feasible sequences, {wrong_n} wrong in the fp32 model, {flagged_n} flagged, "
          f"{missed} wrong and unflagged")
    assert feasible >= 1000 and wrong_n >= 100                        # the fuzz does reach the hazard
    assert missed == 0


# ------------------------------------------------------------------- the fallback
@pytest.mark.parametrize("name", ["A-zeros-skip-N65-T70-ragged", "A-floor-rand-N5-T33", "B-outlier", "B-deadend",
                                  "B-latewinner", "B-earlywinner", "B-survivor", "B-batch"])
def test_torch_fallback_equals_reference(name):
    c, ref = CASES[name], reference(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    lens = None if c["lengths"] is None else t(c["lengths"])
    w = torch.linspace(0.5, 2.0, c["B"], dtype=torch.float64)
    ll, g, xi = rg.logspace_forward_backward(t(c["log_obs"]), t(c["log_p0"]), t(c["log_P"]), lengths=lens, weight=w)
    ll2, g2, xa = rg.logspace_forward_backward(t(c["log_obs"]), t(c["log_p0"]), src=t(c["src"]), dst=t(c["dst"]),
                                               log_w=t(c["log_w"]), lengths=lens, weight=w)
    fin = np.isfinite(ref["loglik"])
    for got_ll, got_g in ((ll, g), (ll2, g2)):
        assert np.array_equal(np.isfinite(got_ll.numpy()), fin)
        assert np.allclose(got_ll.numpy()[fin], ref["loglik"][fin], rtol=1e-12, atol=1e-9)
        assert np.abs(got_g.numpy() - ref["gamma"]).max() <= 1e-10
        assert np.all(got_g.numpy()[~fin] == 0)
    want = (ref["xi_seq"] * w.numpy()[:, None, None]).sum(0)
    assert np.abs(xi.numpy() - want).max() <= 1e-9
    assert np.abs(xa.numpy() - want[c["src"], c["dst"]]).max() <= 1e-9
