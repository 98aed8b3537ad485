"""Inputs that probe the fp32 range of the scaled forward-backward paths, and the fp32 model of them.

The sum-product kernels keep state probabilities in fp32 and rescale a row by one factor; the
log-emissions are shifted by the row maximum over all states, so a state more than about 87 nats
behind its row's leader is exactly 0.  `range_cases()` returns two classes of named cases:

  A  in range: emissions with a realistic spread (per frame the path state and its two neighbours
     at -50 + 2 randn, every other state at -300 + 30 randn) over floored tables, and over
     exact-zero tables along a feasible path.  The kernels must match the log-space reference here.
  B  out of range, all with exact zeros in the table: the row leader is a state no path reaches
     (or that leads nowhere), so every reachable state is flushed.  The raw kernels are documented
     as wrong here; the guarded entry points (pytorch_hmm_amd/range_guard.py) must be right.

Each case is a dict: name, cls ('A' / 'B'), log_obs (B,T,N), log_P (N,N), log_p0 (N) in float32,
lengths (B) int64 or None (padded frames hold NaN), src / dst / log_w of the same matrix (its
entries above -inf, row-major), N, T, B.  Seeds are fixed.

`scaled_model` is the dense form of tests/sparse_numpy.py `sums`: the kernels' scaled recursion
in a chosen dtype, returning also the rows (U, V, CA, E) that the range detector reads.
"""
import numpy as np

NEG = -np.inf
f32 = lambda a: np.asarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------ tables
def l2r(N, stay=0.7):
    """Left-to-right: stay / next, the last state absorbing."""
    P = np.zeros((N, N))
    for i in range(N):
        if i + 1 < N:
            P[i, i], P[i, i + 1] = stay, 1.0 - stay
        else:
            P[i, i] = 1.0
    return P


def l2r_skip(rng, N):
    """Exact-zero left-to-right with skips (test_gpu_em.py left_to_right)."""
    P = np.zeros((N, N))
    for i in range(N):
        hi = min(N, i + 3)
        P[i, i:hi] = rng.dirichlet(np.ones(hi - i) * 2)
    return P


def log0(P):
    with np.errstate(divide="ignore"):
        return f32(np.log(P))


def arcs_of(log_P):
    s, d = np.nonzero(log_P > NEG)
    return s.astype(np.int64), d.astype(np.int64), f32(log_P[s, d])


# ---------------------------------------------------------------------------- emissions
def emissions(rng, path, N):
    """(T,N): the path state and its two neighbours at -50 + 2 randn, the rest at -300 + 30 randn."""
    T = len(path)
    obs = -300.0 + 30.0 * rng.standard_normal((T, N))
    for t, z in enumerate(path):
        for j in (z - 1, z, z + 1):
            if 0 <= j < N:
                obs[t, j] = -50.0 + 2.0 * rng.standard_normal()
    return obs


def monotone_path(rng, N, T, steps):
    z = [0]
    for _ in range(T - 1):
        z.append(min(N - 1, z[-1] + int(rng.choice(steps))))
    return z


def graph_walk(rng, P, T, start=0):
    z = [start]
    for _ in range(T - 1):
        nxt = np.nonzero(P[z[-1]] > 0)[0]
        z.append(int(rng.choice(nxt)))
    return z


def _finish(name, cls, obs, log_P, log_p0, lengths=None):
    obs = f32(obs)
    B, T, N = obs.shape
    if lengths is not None:
        lengths = np.asarray(lengths, np.int64)
        for b in range(B):
            obs[b, int(lengths[b]):] = np.nan          # padded frames are never read
    src, dst, log_w = arcs_of(log_P)
    return dict(name=name, cls=cls, log_obs=obs, log_P=f32(log_P), log_p0=f32(log_p0), lengths=lengths,
                src=src, dst=dst, log_w=log_w, N=N, T=T, B=B)


A_SHAPES = ((5, 33), (64, 70), (65, 70), (200, 230), (256, 70), (65, 1), (65, 2))
A_KINDS = ("floor-l2r", "floor-jumpy", "floor-rand", "zeros-skip")


def _a_case(kind, N, T, rng, B=2, lengths=None, tag=""):
    uniform = np.full(N, -np.log(N))
    if kind in ("floor-l2r", "floor-jumpy"):
        log_P = np.log(l2r(N) + 1e-8)
        log_p0 = uniform
        paths = [monotone_path(rng, N, T, (0, 1)) if kind == "floor-l2r" else list(rng.integers(0, N, T))
                 for _ in range(B)]
    elif kind == "floor-rand":
        keep = rng.random((N, N)) < 0.3
        keep[np.arange(N), np.arange(N)] = True
        P = rng.dirichlet(np.ones(N), N) * keep
        log_P = np.log(P / P.sum(1, keepdims=True) + 1e-8)
        log_p0 = uniform
        paths = [list(rng.integers(0, N, T)) for _ in range(B)]
    elif kind == "zeros-skip":
        log_P = log0(l2r_skip(rng, N))
        log_p0 = np.full(N, NEG)
        log_p0[0] = 0.0
        paths = [monotone_path(rng, N, T, (0, 1, 2)) for _ in range(B)]
    elif kind == "rand-hub":
        # a sparse random graph with exact zeros: in-degree at most 11 (streamed arcs), except
        # state 7, which every state reaches (in-degree N > 64: taken by a whole wave)
        P = np.zeros((N, N))
        for j in range(N):
            P[rng.choice(N, size=int(rng.integers(1, 9)), replace=False), j] = 1.0
        i = np.arange(N)
        P[i, i] = P[i, (i + 1) % N] = P[i, (i - 1) % N] = 1.0         # the path state's neighbours are reachable
        P[:, 7] = 1.0
        P = P * rng.uniform(0.1, 1.0, (N, N))
        P /= P.sum(1, keepdims=True)
        log_P = log0(P)
        log_p0 = uniform
        paths = [graph_walk(rng, P, T, int(rng.integers(0, N))) for _ in range(B)]
    else:
        raise ValueError(kind)
    obs = np.stack([emissions(rng, p, N) for p in paths])
    return _finish(f"A-{kind}-N{N}-T{T}{tag}", "A", obs, log_P, log_p0, lengths)


def a_cases():
    rng = np.random.default_rng(20260401)
    for N, T in A_SHAPES:
        for kind in A_KINDS:
            yield _a_case(kind, N, T, rng)
    for kind in A_KINDS:
        yield _a_case(kind, 65, 70, rng, B=3, lengths=(70, 1, 35), tag="-ragged")
    yield _a_case("rand-hub", 65, 70, rng, B=3, lengths=(70, 1, 35), tag="-ragged")
    yield _a_case("rand-hub", 65, 70, rng)


def wide_cases():
    """The in-range cases of the batch-tiled form (N > 256; no lengths, no arcs needed)."""
    rng = np.random.default_rng(20260402)
    for kind in ("floor-l2r", "floor-jumpy"):
        yield _a_case(kind, 300, 40, rng)


# ------------------------------------------------------------------------ out of range
def _outlier_parts(rng, N=8, T=24):
    """Exact-zero stay / next chain from state 0; frame 3 favours the last state, which no path
    reaches before frame N - 1, by 150 nats over the path state."""
    log_P = log0(l2r(N))
    log_p0 = np.full(N, NEG)
    log_p0[0] = 0.0
    path = monotone_path(rng, N, T, (0, 1))
    obs = emissions(rng, path, N)
    obs[3] -= 150.0
    obs[3, N - 1] = -50.0
    return obs, log_P, log_p0


def b_cases():
    rng = np.random.default_rng(20260403)
    obs, log_P, log_p0 = _outlier_parts(rng)
    yield _finish("B-outlier", "B", obs[None], log_P, log_p0)

    # state 1 has no out-arcs and frame 1 favours it by 150
    P = np.array([[0.4, 0.3, 0.3], [0.0, 0.0, 0.0], [0.5, 0.0, 0.5]])
    obs = -1.0 + 0.3 * rng.standard_normal((1, 4, 3))
    obs[0, 1] = (-150.0, 0.0, -151.0)
    yield _finish("B-deadend", "B", obs, log0(P), np.log(np.full(3, 1 / 3)))

    # two disconnected 2-state branches; branch B starts 120 behind and gains 10 a frame
    P = np.zeros((4, 4))
    P[:2, :2] = 0.5
    P[2:, 2:] = 0.5
    T = 17
    late = np.zeros((1, T, 4))
    late[0, 0, 2:] = -120.0
    late[0, 1:, :2] = -10.0
    yield _finish("B-latewinner", "B", late, log0(P), np.log(np.full(4, 0.25)))
    yield _finish("B-earlywinner", "B", late[:, ::-1].copy(), log0(P), np.log(np.full(4, 0.25)))

    # the row maximum (state 3: no in-arcs, no initial mass) is unreachable; the reachable states
    # sit 95, 99 and 300 below it
    P = np.zeros((4, 4))
    P[:3, :3] = rng.dirichlet(np.ones(3) * 2, 3)
    P[3, 3] = 1.0
    obs = -2.0 + 0.5 * rng.standard_normal((1, 5, 4))
    obs[0, 2] = (-95.0, -99.0, -300.0, 0.0)
    p0 = np.array([0.5, 0.3, 0.2, 0.0])
    yield _finish("B-survivor", "B", obs, log0(P), log0(p0))

    # a feasible out-of-range sequence between two in-range ones, and one with no path at all
    # (frame 3 can only be emitted by the last state)
    o1, log_P, log_p0 = _outlier_parts(rng)
    N, T = o1.shape[1], o1.shape[0]
    o0 = emissions(rng, monotone_path(rng, N, T, (0, 1)), N)
    o2 = emissions(rng, monotone_path(rng, N, T, (0, 1)), N)
    o3 = emissions(rng, monotone_path(rng, N, T, (0, 1)), N)
    o3[3, :N - 1] = NEG
    yield _finish("B-batch", "B", np.stack([o0, o1, o2, o3]), log_P, log_p0)


BATCH_IN_RANGE = (0, 2)     # B-batch: the in-range sequences
BATCH_OUT = 1               # the feasible out-of-range one
BATCH_INFEASIBLE = 3        # the one without a path


def range_cases():
    return list(a_cases()) + list(wide_cases()) + list(b_cases())


# ----------------------------------------------------------------------------- fuzz
FUZZ_LEVELS = (0.0, -20.0, -60.0, -95.0, -110.0, -200.0)


def fuzz_model(rng):
    """One small exact-zero model: N 3-7, T 2-13, B 1-3, a sparse random table and initial vector,
    emissions drawn from FUZZ_LEVELS + randn."""
    N, T, B = int(rng.integers(3, 8)), int(rng.integers(2, 14)), int(rng.integers(1, 4))
    keep = rng.random((N, N)) < rng.uniform(0.2, 0.6)
    P = rng.uniform(0.1, 1.0, (N, N)) * keep
    rows = P.sum(1, keepdims=True)
    P = np.where(rows > 0, P / np.where(rows > 0, rows, 1.0), 0.0)
    p0 = rng.uniform(0.1, 1.0, N) * (rng.random(N) < 0.6)
    if p0.sum() == 0:
        p0[0] = 1.0
    obs = rng.choice(FUZZ_LEVELS, size=(B, T, N)) + rng.standard_normal((B, T, N))
    return f32(obs), log0(P), log0(p0 / p0.sum())


# ------------------------------------------------------------------- the scaled model
def scaled_model(log_obs, log_P, log_p0, lengths=None, dtype=np.float32):
    """The kernels' recursion in `dtype` (sparse_numpy.sums on a dense matrix):
        e_t = exp(obs_t - M_t),  U_0 = p0 e_0,  U_t = (U_{t-1} A) e_t / CA_{t-1},  CA_t = sum U_t,
        V_{L-1} = 1,  V_t = A (e_{t+1} V_{t+1}) / sum(e_{t+1} V_{t+1}),
        gamma = (U / max U)(V / max V) / their sum,  loglik = sum M + sum log CA + log sum U_{L-1}
    with every 1/s taken as `s > 0 ? 1/s : 0`.  Returns dict(loglik (B) float64, gamma, U, V, E
    (B,T,N), CA (B,T)); padded frames: zero rows, CA = 1 (also at L - 1)."""
    obs = np.asarray(log_obs, dtype)
    B, T, N = obs.shape
    lens = np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)
    one, zero = dtype(1), dtype(0)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
        A = np.exp(np.asarray(log_P, dtype))
        p0 = np.exp(np.asarray(log_p0, dtype))
        U = np.zeros((B, T, N), dtype)
        V = np.zeros((B, T, N), dtype)
        E = np.zeros((B, T, N), dtype)
        CA = np.ones((B, T), dtype)
        gamma = np.zeros((B, T, N), dtype)
        loglik = np.zeros(B)
        for b in range(B):
            L = int(lens[b])
            M = obs[b, :L].max(1)
            M = np.where(np.isfinite(M), M, zero).astype(dtype)
            e = np.exp(obs[b, :L] - M[:, None]).astype(dtype)
            E[b, :L] = e
            u = U[b]
            v = V[b]
            u[0] = p0 * e[0]
            for t in range(1, L):
                sx = u[t - 1].sum(dtype=dtype)
                CA[b, t - 1] = sx
                inv = one / sx if sx > 0 else zero
                u[t] = ((u[t - 1] @ A).astype(dtype) * e[t]) * inv
            v[L - 1] = one
            for t in range(L - 2, -1, -1):
                x = e[t + 1] * v[t + 1]
                sx = x.sum(dtype=dtype)
                inv = one / sx if sx > 0 else zero
                v[t] = (A @ x).astype(dtype) * inv
            last = float(u[L - 1].astype(np.float64).sum())
            loglik[b] = float(M.astype(np.float64).sum()) + float(np.log(CA[b, :L - 1].astype(np.float64)).sum()) + \
                (np.log(last) if last > 0 else NEG)
            mu, mv = u[:L].max(1), v[:L].max(1)
            iu = np.where(mu > 0, one / np.where(mu > 0, mu, one), zero).astype(dtype)
            iv = np.where(mv > 0, one / np.where(mv > 0, mv, one), zero).astype(dtype)
            prod = (u[:L] * iu[:, None]) * (v[:L] * iv[:, None])
            s = prod.sum(1, dtype=dtype)
            is_ = np.where(s > 0, one / np.where(s > 0, s, one), zero).astype(dtype)
            gamma[b, :L] = prod * is_[:, None]
    if dtype != np.float64:
        loglik = loglik.astype(dtype).astype(np.float64)
    return dict(loglik=loglik, gamma=gamma, U=U, V=V, E=E, CA=CA)
