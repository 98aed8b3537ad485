"""numpy restatements of the reference's DTW (pytorch_hmm/alignment/dtw.py), shared by
test_dtw_cpu.py (which checks them against the fixtures the reference wrote) and test_gpu_dtw.py
(which uses them as the oracle on shapes the fixtures do not cover).  Not a test module.

  hard_cost      the cost matrix by anti-diagonals in fp32: one add (rabiner_juang: 2*d exact, then
                 one add per candidate) of exact minima, the reference's bits
  backtrace      from (n-1, m-1) to (0,0) to the predecessor of smallest raw cost, order diagonal,
                 up, left with a strict <
  soft_forward   R (n+1, m+1) in fp64
  soft_grad      Cuturi & Blondel's Algorithm 2 (the closed-form E recursion) in fp64
"""
import numpy as np

PATTERNS = ("symmetric", "asymmetric", "rabiner_juang")
FIXTURES = ("1x1", "1x7", "7x1", "13x9", "40x40", "ties", "band", "noend")
SOFT_FIXTURES = ("1x1", "1x7", "7x1", "13x9", "40x40", "ties")
GAMMAS = (("1", 1.0), ("0p1", 0.1), ("0p01", 0.01))


def hard_cost(dist, pattern):
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    N, M = dist.shape
    inf = np.float32(np.inf)
    C = np.full((N, M), inf, np.float32)
    C[0, 0] = dist[0, 0]
    with np.errstate(invalid="ignore"):
        for s in range(1, N + M - 1):
            i = np.arange(max(0, s - M + 1), min(N - 1, s) + 1)
            j = s - i
            im, jm = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            dg = np.where((i > 0) & (j > 0), C[im, jm], inf)
            up = np.where(i > 0, C[im, j], inf)
            lf = np.where(j > 0, C[i, jm], inf)
            d = dist[i, j]
            if pattern == "rabiner_juang":
                C[i, j] = np.minimum(np.minimum(dg + np.float32(2) * d, up + d), lf + d)
            else:
                C[i, j] = d + np.minimum(np.minimum(dg, up), lf)
    return C


def backtrace(C):
    i, j = C.shape[0] - 1, C.shape[1] - 1
    pi, pj = [], []
    while i > 0 or j > 0:
        pi.append(i)
        pj.append(j)
        best, step = None, None
        for ok, ni, nj in ((i > 0 and j > 0, i - 1, j - 1), (i > 0, i - 1, j), (j > 0, i, j - 1)):
            if ok and (best is None or C[ni, nj] < best):
                best, step = C[ni, nj], (ni, nj)
        i, j = step
    pi.append(0)
    pj.append(0)
    return np.array(pi[::-1], np.int64), np.array(pj[::-1], np.int64)


def hard_dtw(dist, pattern):
    C = hard_cost(dist, pattern)
    pi, pj = backtrace(C)
    return C, pi, pj


def _softmin(c, gamma):
    m = c.min()
    if not np.isfinite(m):
        return c.dtype.type(np.inf)
    return m - gamma * np.log(np.exp(-(c - m) / gamma).sum())


def soft_forward(dist, gamma, dtype=np.float64):
    """R (n+1, m+1), every operation in `dtype`."""
    D = np.asarray(dist, dtype)
    gamma = dtype(gamma)
    n, m = D.shape
    R = np.full((n + 1, m + 1), np.inf, dtype)
    R[0, 0] = 0.0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            R[i, j] = D[i - 1, j - 1] + _softmin(np.array([R[i - 1, j - 1], R[i - 1, j], R[i, j - 1]], dtype), gamma)
    return R


def soft_grad(dist, R, gamma, dtype=np.float64):
    """E[1..n, 1..m] with R[:, m+1] = R[n+1, :] = -inf, R[n+1, m+1] = R[n, m], E[n+1, m+1] = 1 and D,
    E padded with 0; every operation in `dtype`."""
    D = np.asarray(dist, dtype)
    gamma = dtype(gamma)
    n, m = D.shape
    Dp = np.zeros((n + 2, m + 2), dtype)
    Dp[1:n + 1, 1:m + 1] = D
    Rp = np.full((n + 2, m + 2), -np.inf, dtype)
    Rp[:n + 1, :m + 1] = R
    Rp[n + 1, m + 1] = R[n, m]
    E = np.zeros((n + 2, m + 2), dtype)
    E[n + 1, m + 1] = 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n, 0, -1):
            for j in range(m, 0, -1):
                if not np.isfinite(Rp[i, j]):
                    continue
                v = dtype(0.0)
                for a, b in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
                    if E[a, b] != 0.0:
                        v += E[a, b] * np.exp((Rp[a, b] - Rp[i, j] - Dp[a, b]) / gamma)
                E[i, j] = v
    return E[1:n + 1, 1:m + 1]


def path_is_valid(pi, pj, N, M):
    """A step path from (0,0) to (N-1,M-1): every step one of (1,1), (1,0), (0,1)."""
    pi, pj = np.asarray(pi), np.asarray(pj)
    if len(pi) != len(pj) or len(pi) == 0 or (pi[0], pj[0]) != (0, 0) or (pi[-1], pj[-1]) != (N - 1, M - 1):
        return False
    di, dj = np.diff(pi), np.diff(pj)
    return bool(np.all((di >= 0) & (dj >= 0) & (di <= 1) & (dj <= 1) & (di + dj >= 1)))


def path_cost(dist, pi, pj, pattern):
    """fp64 cost of a path over dist under the pattern's step weights."""
    D = np.asarray(dist, np.float64)
    w = np.ones(len(pi))
    if pattern == "rabiner_juang":
        w[1:][(np.diff(pi) == 1) & (np.diff(pj) == 1)] = 2.0
    return float((w * D[np.asarray(pi), np.asarray(pj)]).sum())
