"""The HMM over an arc list in numpy: the model of csrc/sparse.hip and pytorch_hmm_amd/sparse.py.

N states, arcs (src[e], dst[e], log_w[e]), initial scores log_p0 (N), log-emissions (B,T,N),
optional lengths: exactly the dense model whose log_P is -inf off the arcs (`densify`).

`viterbi(..., dtype=np.float32)` reproduces the kernel's arithmetic bit for bit: candidates
fl(delta[src] + log_w) in ascending source with strict >, pointer 0 for a destination whose
maximum is -inf, the first argmax at the end.  It also counts the exact ties it met.

`sums(..., dtype)` is the scaled probability-domain recursion with the deferred normaliser, the
tables kept the way the kernel keeps them (U, V, the step normalisers, e = exp(obs - rowmax)):
float64 is the reference, float32 the stand-in whose error against float64 sets the GPU tests'
allowances (tools/measure_sparse_tolerance.py).  The log-scales are summed in float64 in both.

The cases of tests/test_gpu_sparse.py live here too (`viterbi_cases`, `sum_cases`), so that the CPU
tests and the tolerance tool run over exactly the same inputs.
"""
import numpy as np

NEG = -np.inf


# ------------------------------------------------------------------------------ the model
def densify(src, dst, log_w, N, dtype=np.float64):
    """(N,N) log matrix: log_w on the arcs, -inf elsewhere."""
    P = np.full((N, N), NEG, dtype=dtype)
    P[np.asarray(src), np.asarray(dst)] = np.asarray(log_w, dtype=dtype)
    return P


def sort_arcs(src, dst, N):
    """(perm_in, in_ptr, perm_out, out_ptr): the arcs by (dst, src) and by (src, dst)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    perm_in = np.argsort(dst * N + src, kind="stable")
    perm_out = np.argsort(src * N + dst, kind="stable")
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=N))]).astype(np.int32)
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=N))]).astype(np.int32)
    return perm_in, in_ptr, perm_out, out_ptr


def _lens(lengths, B, T):
    return np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)


def viterbi(log_obs, src, dst, log_w, log_p0, lengths=None, dtype=np.float32):
    """dict(states (B,T) int64, log_delta (B,T,N), final_score (B), ties): ties counts the
    destinations (and final rows) whose finite maximum was reached by more than one candidate."""
    obs = np.asarray(log_obs, dtype)
    B, T, N = obs.shape
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    perm = np.argsort(dst * N + src, kind="stable")
    s, d, w = src[perm], dst[perm], np.asarray(log_w, dtype)[perm]
    E = s.size
    pos = np.arange(E)
    lens = _lens(lengths, B, T)
    states = np.full((B, T), -1, np.int64)
    delta = np.full((B, T, N), NEG, dtype)
    final = np.zeros(B, dtype)
    ties = 0
    p0 = np.asarray(log_p0, dtype)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            L = int(lens[b])
            bp = np.zeros((L, N), np.int64)
            delta[b, 0] = p0 + obs[b, 0]
            for t in range(1, L):
                cand = delta[b, t - 1][s] + w
                best = np.full(N, NEG, dtype)
                np.maximum.at(best, d, cand)
                hit = (cand == best[d]) & (cand > NEG)
                first = np.full(N, E, np.int64)
                np.minimum.at(first, d, np.where(hit, pos, E))
                bp[t] = np.where(first < E, s[np.minimum(first, E - 1)], 0)
                ties += int((np.bincount(d[hit], minlength=N) > 1).sum())
                delta[b, t] = best + obs[b, t]
            last = delta[b, L - 1]
            z = int(np.argmax(last))
            ties += int(last[z] > NEG and (last == last[z]).sum() > 1)
            final[b] = last[z]
            for t in range(L - 1, -1, -1):
                states[b, t] = z
                z = int(bp[t, z])
    return dict(states=states, log_delta=delta, final_score=final, ties=ties)


def _gather_sum(idx_out, vals, N, dtype):
    if dtype == np.float64:
        return np.bincount(idx_out, weights=vals, minlength=N)
    acc = np.zeros(N, dtype)
    np.add.at(acc, idx_out, vals)   # in arc order, in dtype: the kernel's order within a state
    return acc


def sums(log_obs, src, dst, log_w, log_p0, lengths=None, weight=None, dtype=np.float64):
    """dict(loglik (B) float64, gamma (B,T,N), xi (E) float64 in the given arc order, gamma0 (N)):
    xi and gamma0 carry the per-sequence weight (default 1)."""
    obs = np.asarray(log_obs, dtype)
    B, T, N = obs.shape
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    E = src.size
    pin = np.argsort(dst * N + src, kind="stable")
    pout = np.argsort(src * N + dst, kind="stable")
    with np.errstate(divide="ignore", over="ignore"):
        A = np.exp(np.asarray(log_w, dtype))
        p0 = np.exp(np.asarray(log_p0, dtype))
    lens = _lens(lengths, B, T)
    g = np.ones(B) if weight is None else np.asarray(weight, np.float64)
    loglik = np.zeros(B)
    gamma = np.zeros((B, T, N), dtype)
    xi = np.zeros(E)
    one, zero = dtype(1), dtype(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            L = int(lens[b])
            M = obs[b, :L].max(1)
            M = np.where(np.isfinite(M), M, zero).astype(dtype)
            e = np.exp(obs[b, :L] - M[:, None])
            U = np.zeros((L, N), dtype)
            V = np.zeros((L, N), dtype)
            CA = np.ones(L, dtype)
            U[0] = p0 * e[0]
            for t in range(1, L):
                sx = U[t - 1].sum(dtype=dtype)
                CA[t - 1] = sx
                inv = one / sx if sx > 0 else zero
                acc = _gather_sum(dst[pin], U[t - 1][src[pin]] * A[pin], N, dtype)
                U[t] = (acc * e[t]) * inv
            V[L - 1] = one
            for t in range(L - 2, -1, -1):
                x = e[t + 1] * V[t + 1]
                sx = x.sum(dtype=dtype)
                inv = one / sx if sx > 0 else zero
                V[t] = _gather_sum(src[pout], x[dst[pout]] * A[pout], N, dtype) * inv
            last = float(U[L - 1].astype(np.float64).sum())
            loglik[b] = float(M.astype(np.float64).sum()) + float(np.log(CA[:L - 1].astype(np.float64)).sum()) + \
                (np.log(last) if last > 0 else NEG)
            mu, mv = U.max(1), V.max(1)
            iu = np.where(mu > 0, one / np.where(mu > 0, mu, one), zero).astype(dtype)
            iv = np.where(mv > 0, one / np.where(mv > 0, mv, one), zero).astype(dtype)
            prod = (U * iu[:, None]) * (V * iv[:, None])
            s = prod.sum(1, dtype=dtype)
            is_ = np.where(s > 0, one / np.where(s > 0, s, one), zero).astype(dtype)
            gamma[b, :L] = prod * is_[:, None]
            for t in range(1, L):
                ica = one / CA[t - 1] if CA[t - 1] > 0 else zero
                left = (U[t - 1][src] * ica) * A
                right = (e[t][dst] * V[t][dst]) * iv[t]
                xi += ((left * right) * (iu[t] * is_[t])).astype(np.float64) * g[b]
    xi[A == 0] = 0.0
    if dtype != np.float64:
        loglik = loglik.astype(dtype).astype(np.float64)   # the kernel's loglik is stored in fp32
    gamma0 = (gamma[:, 0].astype(np.float64) * g[:, None]).sum(0)
    return dict(loglik=loglik, gamma=gamma, xi=xi, gamma0=gamma0)


def dense_loglik(log_obs, log_P, log_p0, lengths=None):
    """loglik (B) of the dense model by a plain float64 log-sum-exp recursion."""
    obs = np.asarray(log_obs, np.float64)
    B, T, N = obs.shape
    lens = _lens(lengths, B, T)
    out = np.zeros(B)

    def lse(x, axis):
        m = x.max(axis)
        m0 = np.where(np.isfinite(m), m, 0.0)
        with np.errstate(divide="ignore"):
            return m0 + np.log(np.exp(x - np.expand_dims(m0, axis)).sum(axis))
    for b in range(B):
        a = np.asarray(log_p0, np.float64) + obs[b, 0]
        for t in range(1, int(lens[b])):
            a = lse(a[:, None] + log_P, 0) + obs[b, t]
        out[b] = lse(a, 0)
    return out


# -------------------------------------------------------------------------------- graphs
def lr_skip(N):
    """Left-to-right with a skip: i -> i, i + 1, i + 2."""
    i = np.arange(N)
    src = np.concatenate([i, i[:-1], i[:-2]]) if N > 2 else np.concatenate([i, i[:-1]])
    dst = np.concatenate([i, i[1:], i[2:]]) if N > 2 else np.concatenate([i, i[1:]])
    return src.astype(np.int64), dst.astype(np.int64)


def random_graph(N, rng, max_in=40):
    """Ragged in-degree 0 .. max_in; state 1 (N > 2) has no in-arcs and the last state no
    out-arcs (N > 1); N = 1 is the single self-loop."""
    if N == 1:
        return np.zeros(1, np.int64), np.zeros(1, np.int64)
    srcs, dsts = [], []
    pool = np.arange(N - 1)   # the last state is never a source
    for j in range(N):
        deg = int(rng.integers(0, min(max_in, pool.size) + 1))
        if j == 0:
            deg = max(deg, 1)
        if j == 1 and N > 2:
            deg = 0
        srcs.append(rng.choice(pool, size=deg, replace=False))
        dsts.append(np.full(deg, j))
    src, dst = np.concatenate(srcs).astype(np.int64), np.concatenate(dsts).astype(np.int64)
    perm = rng.permutation(src.size)   # the caller's order is arbitrary
    return src[perm], dst[perm]


def hub_graph(N=320, deg=300):
    """The left-to-right-skip graph plus a hub: state 7 has in-degree `deg` and state 5 has
    out-degree `deg` (more than a wave's worth in both arc orders)."""
    src, dst = lr_skip(N)
    have = set(zip(src.tolist(), dst.tolist()))
    es, ed = [], []
    for i in range(N):
        if len([1 for s, d in have if d == 7]) + len(es) >= deg:
            break
        if (i, 7) not in have:
            es.append(i)
            ed.append(7)
    have |= set(zip(es, ed))
    fs, fd = [], []
    n5 = len([1 for s, d in have if s == 5])
    for j in range(N):
        if n5 + len(fs) >= deg:
            break
        if (5, j) not in have:
            fs.append(5)
            fd.append(j)
    return (np.concatenate([src, es, fs]).astype(np.int64), np.concatenate([dst, ed, fd]).astype(np.int64))


def complete_graph(N):
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return i.ravel().astype(np.int64), j.ravel().astype(np.int64)


def normalised_log_w(src, N, rng):
    """Random weights normalised over the arcs of a source."""
    w = rng.uniform(0.1, 1.0, size=src.size)
    tot = np.bincount(src, weights=w, minlength=N)
    return np.log(w / tot[src]).astype(np.float32)


# --------------------------------------------------------------------------------- cases
SIZES = (1, 2, 63, 64, 65, 257, 1000, 8192)
WEIGHT = (1.0, 0.5, 2.0)   # the per-sequence weight of the counts and the incoming gradient


def frames(N):
    return (1, 2, 3, 4) if N == 8192 else (1, 2, 3, 70)


def ragged(B, T):
    """Lengths of a B = 3 batch: the full length, length 1 and one in between."""
    return None if B == 1 else np.array([T, 1, max(1, (T + 1) // 2)], np.int64)


def _case(name, N, T, B, graph, rng, integer=False, neg_arcs=False, neg_p0=False, neg_rows=False, no_path=False):
    src, dst = graph
    E = src.size
    if integer:
        log_w = rng.integers(-3, 1, size=E).astype(np.float32)
        log_p0 = rng.integers(-3, 1, size=N).astype(np.float32)
        obs = rng.integers(-3, 1, size=(B, T, N)).astype(np.float32)
    else:
        log_w = normalised_log_w(src, N, rng)
        log_p0 = np.log(rng.dirichlet(np.ones(N)) + 1e-12).astype(np.float32)
        obs = (rng.standard_normal((B, T, N)) * 1.5 - 1.0).astype(np.float32)
    if neg_arcs and E > 2:
        log_w[rng.random(E) < 0.1] = NEG
    if neg_p0 and N > 1:
        log_p0[rng.random(N) < 0.1] = NEG
        log_p0[0] = 0.0 if integer else log_p0[0] if np.isfinite(log_p0[0]) else -1.0
    lengths = ragged(B, T)
    if neg_rows and B == 3 and T >= 3:
        obs[2, 1, :] = NEG      # a whole emission row: sequence 2 (length >= 2) has no path
    if no_path and T >= 2:
        log_p0[:] = NEG         # everything starts in state 0, whose successors cannot emit frame 1
        log_p0[0] = 0.0
        obs[0, 1, dst[src == 0]] = NEG
    if lengths is not None:
        for b in range(B):
            obs[b, int(lengths[b]):] = np.nan   # padded frames are never read
    return dict(name=name, N=N, T=T, B=B, src=src, dst=dst, log_w=log_w, log_p0=log_p0, log_obs=obs,
                lengths=lengths, weight=np.asarray(WEIGHT[:B], np.float32))


def _graphs(N, rng):
    yield "lr", 1, lr_skip(N)
    yield "rand", 3, random_graph(N, rng)


def sum_cases():
    """The cases of the sums, counts and gradients: every size, frame count and batch; the
    left-to-right-skip graph (arcs in registers) with B = 1 and the random graph (streamed arcs,
    -inf arcs, -inf initial scores, a -inf emission row) with B = 3 and ragged lengths; the hub, the
    complete graph and a sequence that no path explains."""
    rng = np.random.default_rng(20260355)
    for N in SIZES:
        for T in frames(N):
            for gname, B, graph in _graphs(N, rng):
                r = gname == "rand"
                yield _case(f"{gname}-N{N}-T{T}-B{B}", N, T, B, graph, rng, neg_arcs=r, neg_p0=r, neg_rows=r)
    for T in (3, 70):
        yield _case(f"hub-N320-T{T}-B3", 320, T, 3, hub_graph(), rng)
    yield _case("complete-N65-T70-B3", 65, 70, 3, complete_graph(65), rng)
    yield _case("nopath-N64-T3-B1", 64, 3, 1, lr_skip(64), rng, no_path=True)
    yield _case("nopath-N1000-T70-B3", 1000, 70, 3, lr_skip(1000), rng, no_path=True)


def viterbi_cases():
    """The cases of sum_cases with real-valued scores, and the same graphs with integer-valued
    weights and emissions, which force exact ties."""
    yield from sum_cases()
    rng = np.random.default_rng(355)
    for N in SIZES:
        T = 3 if N == 8192 else 70
        for gname, B, graph in _graphs(N, rng):
            r = gname == "rand"
            yield _case(f"ties-{gname}-N{N}-T{T}-B{B}", N, T, B, graph, rng, integer=True, neg_arcs=r, neg_p0=r)
    yield _case("ties-hub-N320-T70-B3", 320, 70, 3, hub_graph(), rng, integer=True)
    yield _case("ties-complete-N65-T70-B3", 65, 70, 3, complete_graph(65), rng, integer=True)


def is_tie_case(case):
    return case["name"].startswith("ties-")


def model_args(case):
    return (case["log_obs"], case["src"], case["dst"], case["log_w"], case["log_p0"], case["lengths"])


# ------------------------------------------------------------------------------ allowances
COUNT_FLOOR = 1e-8   # counts are sums of positive products: their relative error holds down to here


def errors(got, ref, case):
    """The error figures of one case: got / ref are dicts with loglik, gamma, xi, gamma0 (numpy).
    The gradient of sum_b weight[b] loglik[b] is (weight gamma, xi, gamma0): its error is taken
    relative to its max-norm."""
    out = {}
    fin = np.isfinite(ref["loglik"])
    dl = np.abs(np.asarray(got["loglik"], np.float64)[fin] - ref["loglik"][fin])
    out["loglik_abs"] = float(dl.max()) if dl.size else 0.0
    out["loglik_rel"] = float((dl / np.maximum(np.abs(ref["loglik"][fin]), 1.0)).max()) if dl.size else 0.0
    lens = _lens(case["lengths"], case["B"], case["T"])
    valid = np.arange(case["T"])[None, :] < lens[:, None]
    dg = np.abs(np.asarray(got["gamma"], np.float64) - ref["gamma"])[valid]
    out["gamma_abs"] = float(dg.max())
    dx = np.abs(np.asarray(got["xi"], np.float64) - ref["xi"])
    out["xi_abs"] = float(dx.max())
    big = np.abs(ref["xi"]) >= COUNT_FLOOR
    out["xi_rel"] = float((dx[big] / np.abs(ref["xi"][big])).max()) if big.any() else 0.0
    w = np.asarray(case["weight"], np.float64)[:, None, None]
    grads = [(np.where(valid[..., None], np.asarray(got["gamma"], np.float64), 0.0) * w,
              np.where(valid[..., None], ref["gamma"], 0.0) * w),
             (np.asarray(got["xi"], np.float64), ref["xi"]),
             (np.asarray(got["gamma0"], np.float64), ref["gamma0"])]
    rel = 0.0
    for a, b in grads:
        top = np.abs(b).max()
        if top > 0:
            rel = max(rel, float(np.abs(a - b).max() / top))
    out["grad_rel"] = rel
    return out
