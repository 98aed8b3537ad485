"""TEST INFRASTRUCTURE ONLY -- host model of the banded classification and a builder of
structured transition tables.

`classify` restates in numpy the rule band_prep_kernel applies on the device
(pytorch_hmm_amd/csrc/band.h:72-170) and the chain choice of rec_band_code
(pytorch_hmm_amd/csrc/recur.h:1841-1861).  `band_case` builds a log-domain table for every
window form the chains are instantiated for, with one floor for all rows or a floor per row;
`expected_chains` is the chain each named case is built to select, worked out from its
construction alone (not through `classify`), so the tests can hold the two against each other.
The product (pytorch_hmm_amd) never imports this module.
"""
import numpy as np

K_BAND_MAX = 8      # band.h:33 kBandMax
K_BAND_N = 256      # band.h:34 kBandN
BIG = 1 << 20       # band.h:86-87, the initial value of every hull minimum

# rec_band_code's instantiated Toeplitz windows (recur.h:1852-1858), as (width, first offset)
TOEPLITZ_CODES = {(1, 0), (2, -1), (2, 0), (3, -2), (3, -1), (3, 0)}

HEADER_KEYS = ("wc", "wr", "wcp", "wrp", "tcd0", "tcw", "trd0", "trw", "uniform_floor")


def pad_states(N):
    """common.h:295."""
    return 64 if N <= 64 else (128 if N <= 128 else 256)


def band_pad(w):
    """band.h:70."""
    return 2 if w <= 2 else (4 if w <= 4 else 8)


def _hulls(nf):
    """Per line of a boolean (lines, positions) array: hull width (an empty hull counts 1,
    band.h:141-142) and the range of (position - line index) over all non-empty lines."""
    n = nf.shape[0]
    wmax, d0, d1 = 0, BIG, -BIG
    for j in range(n):
        idx = np.flatnonzero(nf[j])
        if idx.size == 0:
            wmax = max(wmax, 1)
            continue
        lo, hi = int(idx[0]), int(idx[-1])
        wmax = max(wmax, hi - lo + 1)
        d0, d1 = min(d0, lo - j), max(d1, hi - j)
    return wmax, d0, d1


def _toeplitz(d0, d1):
    """band.h:159-163: an all-floor table fits any range; a Toeplitz window is an offset
    range of width <= 3 inside [-2, 2]."""
    if d1 < d0:
        d0 = d1 = 0
    w = d1 - d0 + 1
    return d0, (w if (w <= 3 and d0 >= -2 and d1 <= 2) else 0)


def chain_name(w, wp, tw, td0, NP):
    """recur.h:1845-1861 rec_band_code, as a name: 'dense', 'tw<W> d0=<D>' (Toeplitz register
    windows, NP <= 128 only) or 'w2' / 'w4' / 'w8' (general windows of the padded width)."""
    if w > K_BAND_MAX:
        return "dense"
    if NP <= 128 and tw > 0 and (tw, td0) in TOEPLITZ_CODES:
        return f"tw{tw} d0={td0}"
    return f"w{wp}"


def classify(L, NP=None):
    """The BandDesc header band_prep_kernel writes for the (N, N) float32 table L, plus the
    chains rec_band_code selects at the padded state count NP (default: pad_states(N)):
    'col_chain' serves Viterbi and alpha (column windows), 'row_chain' serves beta."""
    L = np.asarray(L, np.float32)
    N = L.shape[0]
    assert L.shape == (N, N) and 1 <= N <= K_BAND_N
    NP = pad_states(N) if NP is None else NP
    rfl = L.min(axis=1)                                  # band.h:106-110 row floor = row minimum
    nf = L != rfl[:, None]                               # band.h:117,126 non-floor entries
    cnt = nf.sum(axis=1)
    dense = bool((cnt > K_BAND_MAX).any())               # band.h:119-122
    nf = nf & (cnt <= K_BAND_MAX)[:, None]               # (such a row's hull updates are skipped)
    wr, rd0, rd1 = _hulls(nf)                            # row i: columns o, offsets o - i
    wc, cd0, cd1 = _hulls(nf.T)                          # column o: rows i, offsets i - o
    if dense:
        wc = wr = K_BAND_N                               # band.h:157
    tcd0, tcw = _toeplitz(cd0, cd1)
    trd0, trw = _toeplitz(rd0, rd1)
    out = {"wc": wc, "wr": wr, "wcp": band_pad(wc), "wrp": band_pad(wr),
           "tcd0": tcd0, "tcw": tcw, "trd0": trd0, "trw": trw,
           "uniform_floor": int(bool((rfl == rfl[0]).all()))}   # band.h:167-169
    out["col_chain"] = chain_name(wc, out["wcp"], tcw, tcd0, NP)
    out["row_chain"] = chain_name(wr, out["wrp"], trw, trd0, NP)
    out["banded"] = wc <= K_BAND_MAX and wr <= K_BAND_MAX       # fb.hip hmm355_plan_banded
    return out


# ------------------------------------------------------------------------ case builder
# Offset sets are i - o of the non-floor entries of column o (row i, column o).
_OFFSETS = {
    "toep{0}": (0,), "toep{-1,0}": (-1, 0), "toep{0,1}": (0, 1),
    "toep{-2,-1,0}": (-2, -1, 0), "toep{-1,0,1}": (-1, 0, 1), "toep{0,1,2}": (0, 1, 2),
    "hole{-2,0}": (-2, 0),
    "off{1,2}": (1, 2), "off{-2,-1}": (-2, -1), "off{2}": (2,), "off{-3}": (-3,),
    "gen{-1..2}": (-1, 0, 1, 2), "gen{-2..2}": (-2, -1, 0, 1, 2),
    "gen{-4..3}": tuple(range(-4, 4)), "gen{-4..4}": tuple(range(-4, 5)),
}
_OTHER = ("ragged", "perm", "mixed_col", "mixed_row", "allfloor", "tri_floor_rows", "near_floor",
          "inverted", "rand_dense")
CASES = tuple(_OFFSETS) + _OTHER
TRI = "toep{-1,0,1}"


def _min_n(name):
    """Smallest N at which the case has the structure it is named for (every row keeps at least
    one floor entry and both ends of its offset range occur)."""
    if name in _OFFSETS:
        offs = _OFFSETS[name]
        return 1 if name == TRI else max(len(offs) + 1, max(abs(d) for d in offs) + 1)
    return {"ragged": 16, "perm": 12, "mixed_col": 24, "mixed_row": 24, "allfloor": 1,
            "tri_floor_rows": 8, "near_floor": 4, "inverted": 10, "rand_dense": 1}[name]


def case_exists(name, N):
    return N >= _min_n(name)


def _general(w, NP):
    return "dense" if w > K_BAND_MAX else f"w{band_pad(w)}"


def _toep_or_general(d0, d1, NP):
    w = d1 - d0 + 1
    if NP <= 128 and (w, d0) in TOEPLITZ_CODES:
        return f"tw{w} d0={d0}"
    return _general(w, NP)


def expected_chains(name, N, NP=None):
    """(col_chain, row_chain) the named case is built to select at N states, from its
    construction: the offset set of its columns, mirrored for its rows."""
    NP = pad_states(N) if NP is None else NP
    assert case_exists(name, N), (name, N)
    none = _toep_or_general(0, 0, NP)       # all-floor: width 1, any range fits
    if name == TRI and N <= 2:
        # N = 1: the single entry is its row's floor.  N = 2: the dominant diagonal is the only
        # non-floor entry of either row.
        return none, none
    if name in _OFFSETS:
        offs = _OFFSETS[name]
        if len(offs) > K_BAND_MAX:
            return "dense", "dense"
        return _toep_or_general(min(offs), max(offs), NP), _toep_or_general(-max(offs), -min(offs), NP)
    if name in ("tri_floor_rows", "near_floor"):
        return _toep_or_general(-1, 1, NP), _toep_or_general(-1, 1, NP)
    if name == "ragged":
        return "w8", "w8"
    if name == "perm":
        return "w2", "w2"
    if name == "mixed_col":     # every column holds one entry, one row holds two far apart
        return "w2", "dense"
    if name == "mixed_row":
        return "dense", "w2"
    if name == "allfloor":
        return none, none
    if name == "inverted":
        return "dense", "dense"
    if name == "rand_dense":
        # row i's minimum sits in column (i + 1) % N: every other entry is a band entry, and for
        # N >= 3 some column's hull spans all N rows
        if N <= 2:
            return none, none
        return _general(N, NP), _general(N, NP)
    raise KeyError(name)


def expected_uniform(name, N, floors):
    """The uniform-floor flag the case is built to have (None: not fixed by the construction --
    a handful of random grid floors may coincide)."""
    if N == 1:
        return True
    if floors == "grid":
        return None if N < 8 else False
    if name == "inverted":
        return False
    if name == TRI and N <= 3:
        return False     # a row full of band values: its floor is whichever of them is smallest
    return floors == "uniform"


def _eps(N, floors, rng):
    """eps_i: the mass a row spreads over its floor (floor value log(eps_i / N))."""
    hi = min(0.3, 0.02 * N)      # keeps eps_i / N below the smallest band share (0.7 * 0.5 / 8.5)
    if floors == "uniform":
        return np.full(N, 1e-4)
    e = np.logspace(-6, np.log10(hi), N) if N > 1 else np.array([1e-3])
    return rng.permutation(e)


def _mask(name, N, rng):
    i, o = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    if name in _OFFSETS:
        return np.isin(i - o, _OFFSETS[name])
    if name in ("tri_floor_rows", "near_floor", "inverted"):
        M = np.isin(i - o, (-1, 0, 1))
        if name == "tri_floor_rows":
            M[[2, N // 2, N - 1], :] = False
        return M
    if name == "ragged":
        # column o's hull: a random width 1..8 at a random place inside rows o-4 .. o+3, its ends
        # set and its interior random; eight columns in the middle take the whole range, which
        # makes one column hull and one row hull exactly 8 wide
        M = np.zeros((N, N), bool)
        mid = N // 2
        for c in range(N):
            w = int(rng.integers(1, 9))
            s = c - 4 + int(rng.integers(0, 9 - w))
            full = mid - 3 <= c <= mid + 4
            if full:
                w, s = 8, c - 4
            rows = np.arange(s, s + w)
            keep = (rng.random(w) < 0.6) | full
            keep[0] = keep[-1] = True
            rows = rows[keep]
            M[rows[(rows >= 0) & (rows < N)], c] = True
        return M
    if name in ("perm", "mixed_col", "mixed_row"):
        p = rng.permutation(N)
        p[[0, int(np.flatnonzero(p == N - 1)[0])]] = N - 1, p[0]   # row 0 -> the last column
        M = np.zeros((N, N), bool)
        M[np.arange(N), p] = True
        if name != "perm":
            i0 = N // 2
            far = (int(p[i0]) + N // 2) % N      # >= 12 columns from row i0's own entry
            M[:, far] = False                    # clear the column's own entry ...
            M[i0, far] = True                    # ... and give it to row i0 as a second entry
            if name == "mixed_row":
                M = M.T.copy()
        return M
    if name == "allfloor":
        return np.zeros((N, N), bool)
    if name == "rand_dense":
        return (o != (i + 1) % N) | (N == 1)
    raise KeyError(name)


def band_case(name, N, floors, rng):
    """log_P (N, N) float32 of the named structure, built in the log domain.  Row i's floor is
    log(eps_i / N) and its band entries share 1 - eps_i with random weights (rows that hold band
    entries are stochastic to within N * eps_i / N; an all-floor row sums to eps_i).
    floors: 'uniform' (one eps), 'per_row' (eps_i over 1e-6 .. 0.3, shuffled) or 'grid' (floors
    and band entries on multiples of 0.25, a floor per row: exact sums, frequent ties)."""
    assert floors in ("uniform", "per_row", "grid") and case_exists(name, N), (name, N, floors)
    M = _mask(name, N, rng)
    L = np.empty((N, N), np.float32)
    tri = name in (TRI, "tri_floor_rows", "near_floor", "inverted")
    if floors == "grid":
        r = -0.25 * rng.integers(8, 15, N)               # floors -2 .. -3.5
        B = -0.25 * rng.integers(0, 8, (N, N))           # band entries 0 .. -1.75
        if tri:                                          # a dominant diagonal: 0 .. -0.5 over -0.75 ..
            B = np.where(np.eye(N, dtype=bool), -0.25 * rng.integers(0, 3, (N, N)), -0.25 * rng.integers(3, 8, (N, N)))
        L[:] = np.where(M, B, r[:, None])
    else:
        eps = _eps(N, floors, rng)
        if name == "allfloor":                           # constant rows: stochastic, or a spread
            eps = np.ones(N) if floors == "uniform" else rng.permutation(np.linspace(0.05, 1.0, N))
        W = np.where(M, rng.random((N, N)) * 0.5 + 0.5, 0.0)
        if tri:
            W[np.arange(N), np.arange(N)] *= 3.0         # a dominant diagonal
        if name == "near_floor":
            W *= np.eye(N)                               # (its off-diagonals are set below)
        tot = np.maximum(W.sum(axis=1, keepdims=True), 1e-300)
        with np.errstate(divide="ignore"):
            Lb = np.log((1.0 - eps)[:, None] * W / tot)
        r = np.log(eps / N)
        L[:] = np.where(M, Lb, r[:, None])
    r32 = r.astype(np.float32)
    if name == "near_floor":                             # off-diagonals one ulp above the floor
        off = M & ~np.eye(N, dtype=bool)
        L[:] = np.where(off, np.nextafter(r32, np.float32(np.inf))[:, None], L)
    # every band entry lies strictly above the floor value of its row
    assert (np.where(M, L, np.inf) > r32[:, None]).all(), (name, N, floors)
    if name == "inverted":
        # one row whose bulk lies above a single isolated minimum: N - 1 non-floor entries
        i0, lo_col = N // 3, (N // 3 + N // 2) % N
        L[i0, :] = np.float32(np.log(0.999 / (N - 1))) if floors != "grid" else np.float32(-1.0)
        L[i0, lo_col] = np.float32(np.log(1e-3)) if floors != "grid" else np.float32(-3.0)
    return L
