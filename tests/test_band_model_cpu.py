"""CPU: the host model of the banded classification (oracle/band_model.py) against the chain
every structured case is built to select, the factory matrices against DESIGN §4, and the
oracle against itself on the tie-heavy grid cases.

The GPU tests of tests/test_gpu_band_structures.py draw their matrices from the same builder and
guard their coverage with the same `classify`; this file is what keeps those cases on the
chains they are named for (a case that drifted onto the dense path would pass every parity
check there without running a banded kernel)."""
import numpy as np
import pytest
import torch

from oracle import band_model as M
from oracle import hmm_oracle as O

NS = (3, 40, 100, 128, 200)
FLOORS = ("uniform", "per_row", "grid")


def case_rng(name, N, floors):
    return np.random.default_rng([M.CASES.index(name), N, FLOORS.index(floors)])


@pytest.mark.parametrize("name", M.CASES)
def test_cases_classify_as_named(name):
    ran = 0
    for N in NS:
        if not M.case_exists(name, N):
            continue
        for floors in FLOORS:
            L = M.band_case(name, N, floors, case_rng(name, N, floors))
            assert L.dtype == np.float32 and L.shape == (N, N) and np.isfinite(L).all()
            for NP in sorted({M.pad_states(N), 256 if N >= 16 else M.pad_states(N)}):
                c = M.classify(L, NP)
                want = M.expected_chains(name, N, NP)
                assert (c["col_chain"], c["row_chain"]) == want, (name, N, floors, NP, c)
                assert c["banded"] == ("dense" not in want)
            u = M.expected_uniform(name, N, floors)
            assert u is None or c["uniform_floor"] == int(u), (name, N, floors, c)
            if floors != "grid" and name not in ("allfloor",):
                # rows that hold band entries are stochastic to within their eps (<= 0.3): the
                # band shares 1 - eps and the floor entries add back eps * (their count) / N
                s = np.exp(L.astype(np.float64)).sum(axis=1)[(L != L.min(axis=1, keepdims=True)).any(axis=1)]
                assert s.max() < 1 + 1e-6 and s.min() > 1 - min(0.3, 0.02 * N) - 1e-6, (name, N, floors)
            ran += 1
    assert ran > 0


def test_every_chain_form_is_covered():
    """All six Toeplitz codes and the three general widths, for the column windows (Viterbi,
    alpha) and the row windows (beta), at NP = 64 and NP = 128; the general widths at NP = 256;
    with one floor and with a floor per row."""
    toep = {f"tw{w} d0={d}" for w, d in M.TOEPLITZ_CODES}
    gen = {"w2", "w4", "w8"}
    for N, forms in ((40, toep | gen), (100, toep | gen), (128, toep | gen), (200, gen)):
        for floors in ("uniform", "per_row"):
            col, row = set(), set()
            for name in M.CASES:
                if M.case_exists(name, N):
                    c = M.classify(M.band_case(name, N, floors, case_rng(name, N, floors)))
                    assert c["uniform_floor"] == int(M.expected_uniform(name, N, floors))
                    col.add(c["col_chain"])
                    row.add(c["row_chain"])
            assert forms <= col and forms <= row, (N, floors, forms - col, forms - row)
            assert "dense" in col and "dense" in row


def test_header_fields_of_known_tables():
    """The raw header on tables small enough to work out by hand."""
    # tridiagonal on a floor: hull width 3, offsets -1..1 both ways
    c = M.classify(M.band_case(M.TRI, 40, "per_row", np.random.default_rng(0)))
    assert [c[k] for k in M.HEADER_KEYS] == [3, 3, 4, 4, -1, 3, -1, 3, 0]
    # all-floor: empty hulls count 1 and any offset range fits (band.h:141-142,160-161)
    c = M.classify(np.zeros((5, 5), np.float32))
    assert [c[k] for k in M.HEADER_KEYS] == [1, 1, 2, 2, 0, 1, 0, 1, 1]
    # width 8 against 9 (kBandMax)
    c8 = M.classify(M.band_case("gen{-4..3}", 40, "uniform", np.random.default_rng(0)))
    c9 = M.classify(M.band_case("gen{-4..4}", 40, "uniform", np.random.default_rng(0)))
    assert (c8["wc"], c8["wr"], c8["wcp"], c8["banded"]) == (8, 8, 8, True)
    assert (c9["wc"], c9["wr"], c9["banded"]) == (M.K_BAND_N, M.K_BAND_N, False)
    # one row with a second entry far away: the columns stay 1 wide, the rows do not
    c = M.classify(M.band_case("mixed_col", 40, "per_row", np.random.default_rng(0)))
    assert c["wc"] == 1 and c["wr"] > M.K_BAND_MAX and not c["banded"]
    c = M.classify(M.band_case("mixed_row", 40, "per_row", np.random.default_rng(0)))
    assert c["wr"] == 1 and c["wc"] > M.K_BAND_MAX and not c["banded"]
    # a random dense table: 8 states fit the widest window, 9 do not
    assert M.classify(M.band_case("rand_dense", 8, "per_row", np.random.default_rng(0)))["col_chain"] == "w8"
    assert M.classify(M.band_case("rand_dense", 9, "per_row", np.random.default_rng(0)))["col_chain"] == "dense"
    rng = np.random.default_rng(1)
    for N, want in ((3, True), (5, True), (9, False), (10, False)):
        lP, _ = O.hmm_params(torch.from_numpy(rng.random((N, N), dtype=np.float32)))
        assert M.classify(lP.numpy())["banded"] == want, N


@pytest.mark.parametrize("N", [40, 128, 200])
def test_factory_matrices_classify_as_designed(N):
    """DESIGN §4 'Banded chain': left-to-right window 2, skip 3, the factory's ergodic matrix 1
    (a constant off-diagonal floor plus the diagonal), circular dense (its wrap-around entry
    makes one hull N wide).  hmm_params' log(P + 1e-8) gives every row the same floor."""
    NP = M.pad_states(N)
    small = NP <= 128
    for kind, col, row in (("left_to_right", "tw2 d0=-1", "tw2 d0=0"), ("left_to_right_skip", "tw3 d0=-2", "tw3 d0=0"),
                           ("ergodic", "tw1 d0=0", "tw1 d0=0"), ("circular", "dense", "dense")):
        lP, _ = O.hmm_params(O.transition_matrix(N, kind))
        c = M.classify(lP.numpy())
        if not small and col != "dense":
            col, row = f"w{c['wcp']}", f"w{c['wrp']}"
            assert (c["wcp"], c["wrp"]) == {"left_to_right": (2, 2), "left_to_right_skip": (4, 4), "ergodic": (2, 2)}[kind]
        assert (c["col_chain"], c["row_chain"]) == (col, row), (kind, c)
        # (the ergodic rows are renormalised by fp32 row sums that may differ in the last bit)
        assert c["uniform_floor"] == 1 or kind == "ergodic"
    lP, _ = O.hmm_params(O.left_to_right_matrix(N, 0.7))
    assert M.classify(lP.numpy(), 128)["col_chain"] == "tw2 d0=-1"


@pytest.mark.parametrize("name", [M.TRI, "toep{0,1,2}", "gen{-2..2}", "ragged", "perm", "near_floor", "rand_dense"])
def test_oracle_agrees_with_itself_on_grid_cases(name):
    """Floors, band entries and emissions on multiples of 0.25: every sum is exact and floor
    candidates tie with window candidates; the C oracle and the torch restatement of the
    reference loop must pick the same first index everywhere."""
    N, B, T = (8 if name == "rand_dense" else 40), 2, 150
    rng = case_rng(name, N, "grid")
    L = M.band_case(name, N, "grid", rng)
    lo = (-0.25 * rng.integers(0, 9, (B, T, N))).astype(np.float32)
    init = (-0.25 * rng.integers(0, 5, N)).astype(np.float32)
    cs, cd, _ = O.c_viterbi(lo, L, init)
    ts, td = O.viterbi_from_log(torch.from_numpy(lo), torch.from_numpy(L), torch.from_numpy(init))
    assert np.array_equal(cd, td.numpy())
    assert np.array_equal(cs, ts.numpy())
    # the ties are really there: many steps have more than one maximising predecessor
    cand = cd[:, :-1, :, None] + L[None, None]
    ties = (cand == cand.max(axis=2, keepdims=True)).sum(axis=2) > 1
    assert ties.mean() > 0.05
