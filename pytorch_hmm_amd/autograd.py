"""Autograd for the forward-backward path (HMMLayer.compute_loss / training).

The reference differentiates through its Python loops with plain autograd
(hmm.py:89-101 via hmm_layer.py:144-173; test_hmm.py:189-208 trains HMMLayer through
compute_loss).  Here the gradient is the analytic adjoint of the forward recursion, run by
the same HIP kernels:

For a loss L(log alpha_{T-1}) with g = dL/d log alpha_{T-1} and G = sum_j g_j, the adjoint
lambda_t = dL/d log alpha_t satisfies lambda_t = alpha_t * mu_t where mu is the BACKWARD
recursion started from mu_{T-1} = g / alpha_{T-1} (hmm355_forward_backward_ex_f32 with
log_beta_T = log mu_{T-1}); sum_j lambda_t(j) = G at every t, so
    dL/d log_obs_t = G * posterior'_t          (posterior' = u v / sum(u v) of that pass)
    dL/d log_p0    = sum_b G_b posterior'_{b,0}
    dL/d log_P     = exp(log_P) * sum_{b,t} G_b X_t (x) Y_t,
        X_t = u_{t-1} / (c_{t-1} * sum_k u_t v_t),  Y_t = e_t * v_t,  c_{t-1} = sum u_{t-1}
(u, v: the scaled rows the chains store; every factor is O(1), no exp of log-scales).  The
last contraction is a plain batched GEMM (torch.einsum -> hipBLASLt).

Losses: 'ref'   = the reference's compute_likelihood value LSE_j log(exp(log alpha_{T-1,j}) + 1e-8)
                  (its gradient underflows to 0 exactly where the reference's does);
        'exact' = log sum_j alpha_{T-1,j}  (HMMPyTorch.log_likelihood).
Back-propagating THROUGH the posteriors / forward / backward outputs (HMMLayer training,
the supervised cross-entropy of compute_loss) is ForwardBackwardFn: the adjoint of both
recursions with per-step sources, on hmm355_fb_adjoint_f32 (csrc/adjoint.hip); with one
transition matrix per step (NeuralHMM) TvForwardBackwardFn on hmm355_tv_fb_adjoint_f32
(csrc/tv.hip).
"""
import math

import torch

from . import _native as nat
from . import ops
from . import range_guard as rg


def needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _pad(N):
    return 64 if N <= 64 else (128 if N <= 128 else 256)


FB_PIECES = ("U", "V", "LA", "LB", "band", "binit", "bscale", "rmax", "CA", "CB")


def fb_layout(B, T, N):
    """{piece: byte offset} of the forward-backward workspace (hmm355_fb_workspace_layout)."""
    import ctypes
    out = (ctypes.c_size_t * len(FB_PIECES))()
    nat.check(nat.lib().hmm355_fb_workspace_layout(B, T, N, out))
    return dict(zip(FB_PIECES, out))


def _require_narrow(N, what):
    """The adjoints read the scaled rows and step factors of the one-workgroup-per-sequence
    chains (fb_layout); the batch-tiled form above 256 states keeps another layout and takes no
    terminal backward vector, so gradients stop at 256 states."""
    if N > nat.NARROW_MAX_STATES:
        raise NotImplementedError(
            f"{what} is implemented for at most {nat.NARROW_MAX_STATES} states (got {N}): above that the "
            "forward-backward runs without autograd support (call it under torch.no_grad() / on detached inputs)")


def _fb_outputs(dev, B, T, N, mask):
    """((posterior, forward, backward, loglik, lik_ref), their five pointers for the entry point): the
    ops' forward-backward outputs (ops._fb_outputs), with None for one the mask leaves out."""
    outs = ops._fb_outputs(ops._on(dev), B, T, N, mask)
    wanted = (o if mask & bit else None for o, bit in zip(outs, (nat.FB_POSTERIOR, nat.FB_FORWARD, nat.FB_BACKWARD)))
    return (*wanted, outs[3], outs[4]), ops._fb_ptrs(outs, mask)


def _run_fb(obs, log_P, log_p0, obs_mode, log_beta_T=None, posterior=False, out_mask=None, plan=None, lengths=None):
    """One hmm355_forward_backward_plan_f32 call; returns (posterior|None, loglik, lik_ref, U, V,
    LA, LB), or with `out_mask` ((posterior, forward, backward) per the mask, loglik, lik_ref, U,
    V, LA, LB).  With `lengths` (host int64 (B), checked by ops.ragged_lengths) the call is
    hmm355_forward_backward_ragged_f32: the same workspace pieces, zero rows and unit normalisers
    in the padded frames (hmm355.h)."""
    B, T, N = obs.shape
    NP = _pad(N)
    dev = obs.device
    L = nat.lib()
    mask = out_mask if out_mask is not None else (nat.FB_POSTERIOR if posterior else 0)
    (post, fwd, bwd, loglik, lik_ref), ptrs = _fb_outputs(dev, B, T, N, mask)
    model = (nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(log_p0))
    nbytes = L.hmm355_fb_workspace_bytes(B, T, N)
    if lengths is not None:
        lens = lengths.to(torch.int32).to(dev)
        ws = ops._call(dev, L.hmm355_forward_backward_ragged_f32, *model, nat.ptr(log_beta_T), nat.ptr(lens),
                       B, T, N, mask, *ptrs, ws=nbytes)
    else:
        ws = ops._call(dev, L.hmm355_forward_backward_plan_f32, *model, nat.ptr(plan), nat.ptr(log_beta_T),
                       B, T, N, mask, *ptrs, ws=nbytes)
    rows = B * T
    # the workspace pieces, at the offsets the library reports (hmm355_fb_workspace_layout); they are
    # views of ws, which lives as long as they do
    o = fb_layout(B, T, N)
    fl = ws.view(torch.float32)
    piece = lambda name, n: fl[o[name] // 4: o[name] // 4 + n]
    U = piece("U", rows * NP).view(B, T, NP)[..., :N]
    V = piece("V", rows * NP).view(B, T, NP)[..., :N]
    LA = piece("LA", rows).view(B, T)
    LB = piece("LB", rows).view(B, T)
    CA = piece("CA", rows).view(B, T)
    CB = piece("CB", rows).view(B, T)
    if out_mask is not None:
        return (post, fwd, bwd), loglik, lik_ref, U, V, LA, LB, CA, CB
    return post, loglik, lik_ref, U, V, LA, LB, CA, CB


def valid_frames(lengths, T, dev):
    """(B,T) bool: frame t of sequence b is one of its lengths[b] frames (None without lengths)."""
    if lengths is None:
        return None
    return torch.arange(T, device=dev)[None, :] < lengths.to(dev)[:, None]


def _staged_emissions(obs, obs_mode, valid=None):
    """The emissions the chains multiply by: obs + 1e-8 (OBS_PROB, hmm.py:86) or exp(obs - M_t)
    with M_t the row maximum (OBS_LOG; 0 for a row without a finite maximum, hmm355.h).  With
    `valid` (B,T) the padded frames are exactly 0 (selected, not multiplied: a NaN pad stays out)."""
    if valid is not None:
        obs = torch.where(valid[..., None], obs, torch.zeros_like(obs))
    if obs_mode == nat.OBS_PROB:
        e = obs + 1e-8
    else:
        m = obs.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        e = torch.exp(obs - m)
    return e if valid is None else torch.where(valid[..., None], e, torch.zeros_like(e))


def _terminal_adjoint(a_last, kind):
    """g = dL/d log alpha of the last frame (B,N) for the 'ref' / 'exact' likelihood, and
    log(g / alpha): the terminal backward vector of the adjoint pass (module docstring)."""
    if kind == "ref":
        f = torch.exp(a_last)                                 # the reference's forward[:, -1]
        z = torch.log(f + 1e-8)
        w = torch.softmax(z, dim=-1)
        g = w * f / (f + 1e-8)                                # dL/d log alpha_{T-1}
        log_mu = torch.log(w) - z                             # log(g / alpha_{T-1})
    else:
        g = torch.softmax(a_last, dim=-1)
        log_mu = torch.zeros_like(a_last)
    return g, log_mu


def _guard_replace(grads, bad, gout, obs, lP, l0, lengths):
    """(grad_obs, grad_lP, grad_l0) with the flagged sequences' share -- which the callers zeroed
    -- taken from the log-space loop: d loglik_b / d log_obs = gamma_b, d / d log_P = xi_b,
    d / d log_p0 = gamma_b[0], times the incoming gradient."""
    grad_obs, grad_lP, grad_l0 = grads
    g = gout[bad].to(torch.float64)
    lens = None if lengths is None else lengths.to(obs.device)[bad]
    _, gam, xi = rg.logspace_forward_backward(obs[bad], l0, lP, lengths=lens, weight=g, want_xi=grad_lP is not None)
    gam = gam * g[:, None, None]
    grad_obs = grad_obs.index_copy(0, bad, gam.to(grad_obs.dtype))
    grad_l0 = grad_l0 + gam[:, 0].sum(0).to(grad_l0.dtype)
    if grad_lP is not None:
        grad_lP = grad_lP + xi.to(grad_lP.dtype)
    return grad_obs, grad_lP, grad_l0


class SequenceLogLik(torch.autograd.Function):
    """(B,) log-likelihood of each sequence ('ref' or 'exact'), differentiable in obs,
    log_P and log_p0.

    range_guard (default on; 'exact' with OBS_LOG only): a sequence that left the kernels' fp32
    range (range_guard.out_of_range; possible only with exact zeros in log_P) takes its value and,
    in the backward, its gradients from the float64 log-space loop
    (range_guard.logspace_forward_backward), the others keep the kernels' bits.  One host read of a
    flag per forward; skipped while a CUDA graph is being captured."""

    @staticmethod
    def forward(ctx, obs, log_P, log_p0, obs_mode, kind, plan=None, lengths=None, range_guard=True):
        """lengths: host int64 (B) from ops.ragged_lengths, or None.  With it sequence b is
        obs[b, :lengths[b]] (the ragged entry point); the gradients are those of the per-sequence
        computations, grad_obs exactly 0 in the padded frames."""
        _require_narrow(obs.shape[-1], "the gradient of the sequence log-likelihood")
        nat.require_gpu(obs, log_P, log_p0)
        obs_c, lP, l0 = (t.detach().to(torch.float32).contiguous() for t in (obs, log_P, log_p0))
        _, loglik, lik_ref, U, V, _, _, CA, CB = _run_fb(obs_c, lP, l0, obs_mode, plan=plan, lengths=lengths)
        bad = None
        if range_guard and kind == "exact" and obs_mode == nat.OBS_LOG:
            valid = valid_frames(lengths, obs_c.shape[1], obs_c.device)
            bad = rg.flagged(U, V, CA, lengths, E=_staged_emissions(obs_c, obs_mode, valid), CB=CB)
            if bad is not None:
                lens = None if lengths is None else lengths.to(obs_c.device)[bad]
                ll, _, _ = rg.logspace_forward_backward(obs_c[bad], l0, lP, lengths=lens, want_xi=False)
                loglik = loglik.index_copy(0, bad, ll.to(loglik.dtype))
        ctx.save_for_backward(obs_c, lP, l0)
        ctx.obs_mode, ctx.kind, ctx.plan, ctx.lengths, ctx.bad = obs_mode, kind, plan, lengths, bad
        return lik_ref if kind == "ref" else loglik

    @staticmethod
    def backward(ctx, gout):
        obs, lP, l0 = ctx.saved_tensors
        B, T, N = obs.shape
        if ctx.lengths is not None:
            return SequenceLogLik._backward_ragged(ctx, gout)
        _, _, _, U, _, LA, _, _, _ = _run_fb(obs, lP, l0, ctx.obs_mode, plan=ctx.plan)
        a_last = torch.log(U[:, -1]) + LA[:, -1:]                 # log alpha_{T-1}  (B,N)
        g, log_mu = _terminal_adjoint(a_last, ctx.kind)
        G = g.sum(-1) * gout                                      # (B,)
        post, _, _, U, V, _, _, CA, _ = _run_fb(obs, lP, l0, ctx.obs_mode, log_beta_T=log_mu.contiguous(),
                                                posterior=True, plan=ctx.plan)
        bad = ctx.bad
        if bad is not None:
            # the flagged sequences' rows may hold anything (NaN included): out of every factor
            G, post, U, V = (x.index_fill(0, bad, 0.0) for x in (G, post, U, V))
            CA = CA.index_fill(0, bad, 1.0)
        grad_lo = G[:, None, None] * post
        if ctx.obs_mode == nat.OBS_PROB:
            grad_obs = grad_lo / (obs + 1e-8)
            e = obs + 1e-8
        else:
            grad_obs = grad_lo
            # the kernels' shifted emissions e_t = exp(lo_t - M_t) (hmm355.h, OBS_LOG): the
            # shift cancels in X_t (x) Y_t, and unshifted exp(lo) would underflow
            m = obs.amax(-1, keepdim=True)
            m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
            e = torch.exp(obs - m)
        grad_l0 = (G[:, None] * post[:, 0]).sum(0)
        grad_lP = None
        if T > 1 and ctx.needs_input_grad[1]:
            c = CA                                                # U_{t+1} = A^T U_t e_{t+1} / c_t
            S = (U * V).sum(-1)                                   # (B,T)
            X = U[:, :-1] / (c[:, :-1] * S[:, 1:]).unsqueeze(-1) * G[:, None, None]
            if bad is not None:
                X = X.index_fill(0, bad, 0.0)                     # 0 / (1 * 0) above
            Y = e[:, 1:] * V[:, 1:]
            M = torch.einsum("bti,btj->ij", X, Y)
            grad_lP = torch.exp(lP) * M
        if bad is not None:
            grad_obs, grad_lP, grad_l0 = _guard_replace((grad_obs, grad_lP, grad_l0), bad, gout, obs, lP, l0, None)
        return grad_obs, grad_lP, grad_l0, None, None, None, None, None

    @staticmethod
    def _backward_ragged(ctx, gout):
        """backward() with per-sequence lengths: log alpha is taken at frame len_b - 1, the
        emissions and every factor of the padded frames are selected to exactly 0 (torch.where: a
        NaN pad stays out), and the transition pairs (t, t + 1) stop at len_b - 1."""
        obs, lP, l0 = ctx.saved_tensors
        B, T, N = obs.shape
        lengths = ctx.lengths
        dev = obs.device
        valid = valid_frames(lengths, T, dev)                    # (B,T)
        last = (lengths.to(dev) - 1)
        rows = torch.arange(B, device=dev)
        _, _, _, U, _, LA, _, _, _ = _run_fb(obs, lP, l0, ctx.obs_mode, lengths=lengths)
        a_last = torch.log(U[rows, last]) + LA[rows, last][:, None]   # log alpha_{len-1}  (B,N)
        g, log_mu = _terminal_adjoint(a_last, ctx.kind)
        G = g.sum(-1) * gout
        post, _, _, U, V, _, _, CA, _ = _run_fb(obs, lP, l0, ctx.obs_mode, log_beta_T=log_mu.contiguous(),
                                                posterior=True, lengths=lengths)
        bad = ctx.bad
        if bad is not None:
            G, post, U, V = (x.index_fill(0, bad, 0.0) for x in (G, post, U, V))
            CA = CA.index_fill(0, bad, 1.0)
        grad_lo = G[:, None, None] * post                         # post is 0 in the padded frames
        e = _staged_emissions(obs, ctx.obs_mode, valid)
        if ctx.obs_mode == nat.OBS_PROB:
            grad_obs = torch.where(valid[..., None], grad_lo / (obs + 1e-8), torch.zeros_like(grad_lo))
        else:
            grad_obs = grad_lo
        grad_l0 = (G[:, None] * post[:, 0]).sum(0)
        grad_lP = None
        if T > 1 and ctx.needs_input_grad[1]:
            pair = valid[:, 1:, None]                             # frames t and t + 1 both valid
            S = (U * V).sum(-1)
            den = (CA[:, :-1] * S[:, 1:]).unsqueeze(-1)
            X = torch.where(pair, U[:, :-1] / torch.where(pair, den, torch.ones_like(den)), torch.zeros_like(U[:, :-1]))
            X = X * G[:, None, None]
            if bad is not None:
                X = X.index_fill(0, bad, 0.0)
            Y = e[:, 1:] * V[:, 1:]
            grad_lP = torch.exp(lP) * torch.einsum("bti,btj->ij", X, Y)
        if bad is not None:
            grad_obs, grad_lP, grad_l0 = _guard_replace((grad_obs, grad_lP, grad_l0), bad, gout, obs, lP, l0, lengths)
        return grad_obs, grad_lP, grad_l0, None, None, None, None, None


def _run_tv_fb(log_obs, A, sb, st, log_p0, log_beta_T=None, posterior=False, out_mask=None):
    """One hmm355_tv_forward_backward_ex_f32 call; returns (posterior|None, loglik, lik_ref, U, V, E, LA),
    with `out_mask` the first item is the (posterior, forward, backward) tuple per the mask."""
    B, T, N = log_obs.shape
    NP = _pad(N)
    dev = log_obs.device
    L = nat.lib()
    mask = out_mask if out_mask is not None else (nat.FB_POSTERIOR if posterior else 0)
    (post, fwd, bwd, loglik, lik_ref), ptrs = _fb_outputs(dev, B, T, N, mask)
    ws = ops._call(dev, L.hmm355_tv_forward_backward_ex_f32, nat.ptr(log_obs), nat.ptr(A), sb, st, nat.ptr(log_p0),
                   nat.ptr(log_beta_T), B, T, N, mask, *ptrs, ws=L.hmm355_tv_fb_workspace_bytes(B, T, N))
    if out_mask is not None:
        post = (post, fwd, bwd)
    rows = B * T
    al = lambda n: ((n + 255) // 256) * 256
    fl = ws.view(torch.float32)
    U = fl[: rows * NP].view(B, T, NP)[..., :N]
    V = fl[rows * NP: 2 * rows * NP].view(B, T, NP)[..., :N]
    off = al(2 * rows * NP * 4) + al(2 * rows * 4)          # after U|V and LA|LB (hmm355.h)
    E = fl[off // 4: off // 4 + rows * NP].view(B, T, NP)[..., :N]
    offL = al(2 * rows * NP * 4) // 4
    LA = fl[offL: offL + rows].view(B, T)
    return post, loglik, lik_ref, U, V, E, LA


class TvSequenceLogLik(torch.autograd.Function):
    """(B,) log-likelihood of each sequence under per-step transition matrices
    (NeuralHMM.compute_likelihood, neural.py:513-519), differentiable in log_obs, log_A
    ((N,N) or (B,T,N,N)) and log_p0.  The adjoint of module docstring with the shifted
    emissions E_t = exp(log_obs_t - M_t) the tv kernels use: dL/d log_A_k = G exp(log_A_k)
    (X_{k+1} (x) Y_{k+1}) for the matrix k between steps k and k+1."""

    @staticmethod
    def forward(ctx, log_obs, log_A, log_p0, kind):
        from .ops import _tv_matrix
        nat.require_gpu(log_obs, log_A, log_p0)
        lo = log_obs.detach().to(torch.float32).contiguous()
        l0 = log_p0.detach().to(torch.float32).contiguous()
        B, T, N = lo.shape
        A, sb, st = _tv_matrix(log_A.detach(), B, T, N)
        _, loglik, lik_ref, _, _, _, _ = _run_tv_fb(lo, A, sb, st, l0)
        ctx.save_for_backward(lo, A, l0)
        ctx.sb, ctx.st, ctx.kind, ctx.static = sb, st, kind, log_A.dim() == 2
        return lik_ref if kind == "ref" else loglik

    @staticmethod
    def backward(ctx, gout):
        lo, A, l0 = ctx.saved_tensors
        B, T, N = lo.shape
        _, _, _, U, _, _, LA = _run_tv_fb(lo, A, ctx.sb, ctx.st, l0)
        a_last = torch.log(U[:, -1]) + LA[:, -1:]
        if ctx.kind == "ref":
            f = torch.exp(a_last)
            z = torch.log(f + 1e-8)
            w = torch.softmax(z, dim=-1)
            g = w * f / (f + 1e-8)
            log_mu = torch.log(w) - z
        else:
            g = torch.softmax(a_last, dim=-1)
            log_mu = torch.zeros_like(a_last)
        G = g.sum(-1) * gout
        post, _, _, U, V, E, _ = _run_tv_fb(lo, A, ctx.sb, ctx.st, l0, log_beta_T=log_mu.contiguous(), posterior=True)
        grad_lo = G[:, None, None] * post
        grad_l0 = (G[:, None] * post[:, 0]).sum(0)
        grad_A = None
        if ctx.needs_input_grad[1]:
            c = U.sum(-1)
            S = (U * V).sum(-1)
            X = U[:, :-1] / (c[:, :-1] * S[:, 1:]).unsqueeze(-1) * G[:, None, None]   # (B,T-1,N)
            Y = E[:, 1:] * V[:, 1:]                                                   # (B,T-1,N)
            if ctx.static:
                grad_A = torch.exp(A) * torch.einsum("bti,btj->ij", X, Y)
            else:
                Af = A if A.stride(1) != 0 else A.expand(B, T, N, N)
                grad_A = torch.zeros(B, T, N, N, device=lo.device)
                if T > 1:
                    grad_A[:, :-1] = torch.exp(Af[:, :-1]) * X.unsqueeze(-1) * Y.unsqueeze(-2)
        return grad_lo, grad_A, grad_l0, None


def _adjoint_sources(U, V, E, post, fwd, bwd, gp, gf, gb, CA=None, CB=None):
    """Per-step sources and scales of the two adjoint chains (ForwardBackwardFn's docstring):
    srcW = v (Gp - <gamma, Gp>) / sum(u v) + Gf exp(LA), srcZ = u (Gp - <gamma, Gp>) / sum(u v)
    + Gb exp(LB) (Gf exp(LA) = Gf forward / u), Fw_t = 1 / sum u_t, Fz_t = 1 / sum v_t E_t
    (t >= 1).  Formed in fp64 from the stored fp32 rows, returned as contiguous fp32.  The step
    factors are the chains' own normalisers CA / CB (hmm355.h; the dense chain's rows do not sum
    to 1, so they are not the row sums there)."""
    B, T, N = U.shape
    U64, V64 = U.double(), V.double()
    Suv = (U64 * V64).sum(-1, keepdim=True)
    srcW = torch.zeros(B, T, N, dtype=torch.float64, device=U.device)
    srcZ = torch.zeros_like(srcW)
    if gp is not None:
        g64 = gp.double()
        q = (g64 - (post.double() * g64).sum(-1, keepdim=True)) / torch.where(Suv > 0, Suv, torch.ones_like(Suv))
        q = torch.where(Suv > 0, q, torch.zeros_like(q))
        srcW += V64 * q
        srcZ += U64 * q
    if gf is not None:
        srcW += torch.where(U64 > 0, gf.double() * fwd.double() / torch.where(U64 > 0, U64, torch.ones_like(U64)),
                            torch.zeros_like(U64))
    if gb is not None:
        srcZ += torch.where(V64 > 0, gb.double() * bwd.double() / torch.where(V64 > 0, V64, torch.ones_like(V64)),
                            torch.zeros_like(V64))
    Fw = torch.zeros(B, T, device=U.device)                                    # 1/c_t (t <= T-2)
    Fz = torch.zeros(B, T, device=U.device)                                    # 1/c'_{t-1} (t >= 1)
    if T > 1:
        # (CA / CB None: chains that normalise every step exactly, c_t = sum u_t -- csrc/tv.hip)
        ca = CA[:, :-1].double() if CA is not None else U64[:, :-1].sum(-1)
        cb = CB[:, 1:].double() if CB is not None else (V64[:, 1:] * E[:, 1:].double()).sum(-1)
        Fw[:, :-1] = (1.0 / ca).float()
        Fz[:, 1:] = (1.0 / cb).float()
    return srcW.float().contiguous(), Fw, srcZ.float().contiguous(), Fz


class ForwardBackwardFn(torch.autograd.Function):
    """HMMPyTorch.forward_backward outputs (posterior, forward, backward) per `out_mask`,
    differentiable in obs, log_P and log_p0 — the reference back-propagates through its
    log-space loops (hmm.py:89-130; HMMLayer training mode hmm_layer.py:119-121, supervised
    compute_loss :159-165).  Forward: the gfx950 chains, keeping their scaled rows
    (alpha_t = U_t exp(LA_t), beta_t = V_t exp(LB_t)).  Backward: the analytic adjoint.

    With a = log alpha, b = log beta, gamma = exp(a + b - LSE(a + b)) and output gradients
    Gp, Gf, Gb, the direct adjoints are
        h_t = gamma_t (Gp_t - <gamma_t, Gp_t>) + Gf_t exp(a_t)     (of a_t)
        k_t = gamma_t (Gp_t - <gamma_t, Gp_t>) + Gb_t exp(b_t)     (of b_t).
    The total adjoint of a_t is alpha_t * W_t e^{-LA_t}, W the forward recursion's adjoint in
    alpha's scaling, and that of b_t is beta_t * Z_t e^{-LB_t}:
        W_{t-1} = h_{t-1} / u_{t-1} + (1/c_{t-1}) A (E_t W_t),          c_t = CA_t
        Z_{t+1} = k_{t+1} / v_{t+1} + (1/c'_t) E_{t+1} (A^T Z_t),       c'_t = CB_{t+1}
    with c, c' the chains' step normalisers (u_{t+1} = A^T u_t E_{t+1} / c_t, v_t = A E_{t+1}
    v_{t+1} / c'_t; hmm355.h workspace CA / CB)
    (hmm355_fb_adjoint_f32), where h/u = v (Gp - <.,.>) / sum(u v) + Gf exp(LA) and
    k/v = u (Gp - <.,.>) / sum(u v) + Gb exp(LB) are O(1) (no division by a vanishing u or v).
    Then, with P = Z - k/v the propagated part of Z,
        dL/d log_obs_t = u_t W_t + v_t P_t
        dL/d log_p0    = sum_b u_0 W_0
        dL/d log_P     = exp(log_P) * sum_{b,t} [ (u_{t-1}/c_{t-1}) (x) (E_t W_t)
                                                 + Z_t (x) (E_{t+1} v_{t+1} / c'_t) ]
    (two GEMMs over the frames, hipBLASLt through torch)."""

    @staticmethod
    def forward(ctx, obs, log_P, log_p0, obs_mode, out_mask, plan=None, lengths=None):
        """lengths: host int64 (B) from ops.ragged_lengths, or None.  With it the rows come from
        the ragged entry point: U = V = 0 and unit normalisers in the padded frames, so the W chain
        of hmm355_fb_adjoint_f32 stays 0 down to frame len_b - 1, where it equals its source, and
        the Z chain propagates zeros past it."""
        nat.require_gpu(obs, log_P, log_p0)
        obs_c, lP, l0 = (t.detach().to(torch.float32).contiguous() for t in (obs, log_P, log_p0))
        outs, _, _, U, V, _, _, CA, CB = _run_fb(obs_c, lP, l0, obs_mode, out_mask=out_mask | nat.FB_POSTERIOR,
                                                 plan=plan, lengths=lengths)
        post, fwd, bwd = outs
        ctx.save_for_backward(obs_c, lP, l0, U, V, post, fwd, bwd, CA, CB)
        ctx.obs_mode, ctx.out_mask, ctx.lengths = obs_mode, out_mask, lengths
        ctx.set_materialize_grads(False)   # outputs the loss does not use arrive as None
        res = tuple(o for bit, o in ((nat.FB_POSTERIOR, post), (nat.FB_FORWARD, fwd), (nat.FB_BACKWARD, bwd))
                    if out_mask & bit)
        return res

    @staticmethod
    def backward(ctx, *grads):
        obs, lP, l0, U, V, post, fwd, bwd, CA, CB = ctx.saved_tensors
        B, T, N = obs.shape
        returned = [k for bit, k in ((nat.FB_POSTERIOR, "p"), (nat.FB_FORWARD, "f"), (nat.FB_BACKWARD, "b"))
                    if ctx.out_mask & bit]
        got = dict(zip(returned, grads))
        gp, gf, gb = got.get("p"), got.get("f"), got.get("b")
        valid = valid_frames(ctx.lengths, T, obs.device)
        if valid is not None:
            # sources are 0 in the padded frames whatever the incoming gradient holds there
            gp, gf, gb = (None if g is None else torch.where(valid[..., None], g, torch.zeros_like(g))
                          for g in (gp, gf, gb))
        E = _staged_emissions(obs, ctx.obs_mode, valid).contiguous()
        srcW, Fw, srcZ, Fz = _adjoint_sources(U, V, E, post, fwd, bwd, gp, gf, gb, CA, CB)
        W = torch.empty(B, T, N, device=obs.device)
        P = torch.empty(B, T, N, device=obs.device)
        ops._call(obs.device, nat.lib().hmm355_fb_adjoint_f32, nat.ptr(E), nat.ptr(lP), nat.ptr(srcW), nat.ptr(Fw),
                  nat.ptr(srcZ), nat.ptr(Fz), B, T, N, nat.ptr(W), nat.ptr(P))
        grad_lo = U * W + V * P
        grad_obs = grad_lo / (obs + 1e-8) if ctx.obs_mode == nat.OBS_PROB else grad_lo
        if valid is not None:
            grad_obs = torch.where(valid[..., None], grad_obs, torch.zeros_like(grad_obs))
        grad_l0 = (U[:, 0] * W[:, 0]).sum(0)
        grad_lP = None
        if ctx.needs_input_grad[1]:
            M = torch.zeros(N, N, device=obs.device)
            if T > 1:
                X1 = U[:, :-1] * Fw[:, :-1, None]
                Y1 = E[:, 1:] * W[:, 1:]
                Z = srcZ + P
                Y2 = E[:, 1:] * V[:, 1:] * Fz[:, 1:, None]
                M = torch.einsum("bti,btj->ij", X1, Y1) + torch.einsum("bti,btj->ij", Z[:, :-1], Y2)
            grad_lP = torch.exp(lP) * M
        return grad_obs, grad_lP, grad_l0, None, None, None, None


class TvForwardBackwardFn(torch.autograd.Function):
    """NeuralHMM.forward outputs (posterior, forward, backward) per `out_mask` under per-step
    transition matrices, differentiable in log_obs, log_A ((N,N) or (B,T,N,N)) and log_p0 —
    the reference back-propagates through its per-step logsumexp loops (neural.py:391-461).
    Forward: csrc/tv.hip's chains (log-emissions staged as E_t = exp(lo_t - M_t)).  Backward:
    ForwardBackwardFn's adjoint with the step's own matrix: hmm355_tv_fb_adjoint_f32 runs the
    W / Z chains streaming A_k = exp(log_A_k) as the forward does, then
        dL/d log_obs_t = u_t W_t + v_t P_t,   dL/d log_p0 = sum_b u_0 W_0,
        dL/d log_A_k   = exp(log_A_k) * [ (u_k / c_k) (x) (E_{k+1} W_{k+1})
                                          + Z_k (x) (E_{k+1} v_{k+1} / c'_k) ]   (k <= T-2; 0 at k = T-1)
    (summed over (b, k) for one static matrix)."""

    @staticmethod
    def forward(ctx, log_obs, log_A, log_p0, out_mask):
        from .ops import _tv_matrix
        nat.require_gpu(log_obs, log_A, log_p0)
        lo = log_obs.detach().to(torch.float32).contiguous()
        l0 = log_p0.detach().to(torch.float32).contiguous()
        B, T, N = lo.shape
        A, sb, st = _tv_matrix(log_A.detach(), B, T, N)
        outs, _, _, U, V, E, _ = _run_tv_fb(lo, A, sb, st, l0, out_mask=out_mask | nat.FB_POSTERIOR)
        post, fwd, bwd = outs
        ctx.save_for_backward(lo, A, l0, U, V, E, post, fwd, bwd)
        ctx.sb, ctx.st, ctx.static, ctx.out_mask = sb, st, log_A.dim() == 2, out_mask
        ctx.a_shape = tuple(log_A.shape)
        ctx.set_materialize_grads(False)
        return tuple(o for bit, o in ((nat.FB_POSTERIOR, post), (nat.FB_FORWARD, fwd), (nat.FB_BACKWARD, bwd))
                     if out_mask & bit)

    @staticmethod
    def backward(ctx, *grads):
        lo, A, l0, U, V, E, post, fwd, bwd = ctx.saved_tensors
        B, T, N = lo.shape
        returned = [k for bit, k in ((nat.FB_POSTERIOR, "p"), (nat.FB_FORWARD, "f"), (nat.FB_BACKWARD, "b"))
                    if ctx.out_mask & bit]
        got = dict(zip(returned, grads))
        E = E.contiguous()
        srcW, Fw, srcZ, Fz = _adjoint_sources(U, V, E, post, fwd, bwd, got.get("p"), got.get("f"), got.get("b"))
        W = torch.empty(B, T, N, device=lo.device)
        P = torch.empty(B, T, N, device=lo.device)
        ops._call(lo.device, nat.lib().hmm355_tv_fb_adjoint_f32, nat.ptr(E), nat.ptr(A), ctx.sb, ctx.st, nat.ptr(srcW),
                  nat.ptr(Fw), nat.ptr(srcZ), nat.ptr(Fz), B, T, N, nat.ptr(W), nat.ptr(P))
        grad_lo = U * W + V * P
        grad_l0 = (U[:, 0] * W[:, 0]).sum(0)
        grad_A = None
        if ctx.needs_input_grad[1]:
            if ctx.static:
                M = torch.zeros(N, N, device=lo.device)
                if T > 1:
                    X1 = U[:, :-1] * Fw[:, :-1, None]
                    Y1 = E[:, 1:] * W[:, 1:]
                    Y2 = E[:, 1:] * V[:, 1:] * Fz[:, 1:, None]
                    M = torch.einsum("bti,btj->ij", X1, Y1) + torch.einsum("bti,btj->ij", (srcZ + P)[:, :-1], Y2)
                grad_A = torch.exp(A) * M
            else:
                # matrices k = 0 .. T-2 are used; any further ones (log_A may carry T or more
                # steps, neural.py:377-381) get a zero gradient
                grad_A = torch.zeros(ctx.a_shape, device=lo.device)
                if T > 1:
                    # both outer products of a step as one K = 2 batched GEMM, then * exp(log_A_k)
                    Lf = torch.stack([U[:, :-1] * Fw[:, :-1, None], (srcZ + P)[:, :-1]], -1)        # (B,T-1,N,2)
                    Rf = torch.stack([E[:, 1:] * W[:, 1:], E[:, 1:] * V[:, 1:] * Fz[:, 1:, None]], -2)  # (B,T-1,2,N)
                    g = torch.matmul(Lf, Rf)
                    g.mul_(torch.exp(A.expand(ctx.a_shape)[:, :T - 1]))
                    grad_A[:, :T - 1] = g
        return grad_lo, grad_A, grad_l0, None


def tv_forward_backward_with_grad(log_obs, log_A, log_p0, out_mask):
    """Differentiable NeuralHMM forward-backward outputs (tuple per out_mask)."""
    return TvForwardBackwardFn.apply(log_obs, log_A, log_p0, out_mask)


def forward_backward_with_grad(obs, log_P, log_p0, obs_mode, out_mask, plan=None, lengths=None):
    """Differentiable forward-backward outputs (tuple per out_mask: posterior, forward, backward).
    lengths: host int64 (B) from ops.ragged_lengths, or None."""
    _require_narrow(obs.shape[-1], "the gradient of the forward-backward outputs")
    return ForwardBackwardFn.apply(obs, log_P, log_p0, obs_mode, out_mask, plan, lengths)


class GmmLogProb(torch.autograd.Function):
    """Diagonal-Gaussian (mixture) emission log-probabilities: forward by the gfx950 scorer
    (ops.gmm_diag_logprob), backward analytic.  With comp[b,t,s,c] the component log-density
    plus log_w and r = d lp / d comp (softmax over c of the reference's clamped LSE,
    mixture_gaussian.py:141-155; r = 1 when mix_lse == 0):
        d/d means   = r g (x - mu) / var          d/d log_vars = r g ((x - mu)^2 / var - 1) / 2
        d/d x       = -sum_{s,c} r g (x - mu) / var                d/d log_w = r g
    expanded into GEMMs over the frames (torch.matmul), T-chunked.

    Precision.  The expansion x^2 iv - 2 x (mu iv) + sum mu^2 iv and the moments
    gx2 - 2 mu gx1 + mu^2 gsum cancel: with features that are not centred (x, mu ~ off, spread xs)
    the terms are (off / xs)^2 times the result, and in fp32 that lost 2-3 digits against fp32
    autograd of the direct (x - mu)^2 / var form (tests/test_gpu_gmm.py: 41 to 4490 x its error
    on the cases with off != 0).  The component scores, the GEMMs and the moment algebra
    therefore run in float64, like the forward scorer's quadratic form (csrc/gmm.hip); the
    gradients are rounded to the inputs' dtypes once, at the end.  Each product pair shares one
    GEMM ([x^2, x] against stacked tables) and the responsibilities are one fused softmax: the
    passes over the (frames, S*C) temporaries, not the fp64 GEMMs, set the time."""

    # bytes of one (frames, S*C) temporary of the backward's T-chunks
    _CHUNK_BYTES = 16 << 20

    @staticmethod
    def forward(ctx, x, means, log_vars, log_w, mix_lse):
        from . import ops
        lp = ops.gmm_diag_logprob(x.detach(), means.detach(), log_vars.detach(), log_w.detach(), mix_lse)
        ctx.save_for_backward(x, means, log_vars, log_w)
        ctx.mix_lse = mix_lse
        return lp

    @staticmethod
    def backward(ctx, g):
        x, means, log_vars, log_w = ctx.saved_tensors
        B, T, D = x.shape
        S, C, _ = means.shape
        f64 = torch.float64
        mu = means.detach().to(f64).reshape(S * C, D)
        lv = log_vars.detach().to(f64).reshape(S * C, D)
        iv = torch.exp(-lv)                                   # 1 / var
        miv = mu * iv
        if ctx.mix_lse:
            # comp = [x^2, x] @ wcat + bias, one GEMM: -0.5 (x^2 iv - 2 x mu iv + sum mu^2 iv + K) + log_w
            lw = log_w.detach().to(f64)
            # a state whose components all have log_w = -inf: the reference's m = -inf -> 0 and
            # clamp(min=1e-8) leave it a zero slope; its log_w is cleared so the softmax stays finite
            alive = ~torch.isneginf(lw).all(-1)               # (S)
            lw = torch.where(alive[:, None], lw, torch.zeros_like(lw)).reshape(S * C)
            bias = lw - 0.5 * ((mu * miv).sum(-1) + lv.sum(-1) + D * math.log(2 * math.pi))
            wcat = torch.cat([-0.5 * iv, miv], 1).t()         # (2D, SC)
        xcat = torch.cat([miv, iv], 1)                        # (SC, 2D): grad_x's two products
        gxx = torch.zeros(S * C, 2 * D, device=x.device, dtype=f64)    # sum gc [x^2, x]
        gsum = torch.zeros(S * C, device=x.device, dtype=f64)
        grad_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        # frames-of-T per chunk: the (frames, S*C) float64 temporaries stay at _CHUNK_BYTES each
        step = max(1, GmmLogProb._CHUNK_BYTES // (mu.element_size() * max(1, B * S * C)))
        for t0 in range(0, T, step):
            xc = x.detach()[:, t0:t0 + step].reshape(-1, D).to(f64)     # (F, D)
            gl = g[:, t0:t0 + step].reshape(-1, S).to(f64)              # (F, S)
            xx = torch.cat([xc * xc, xc], 1)                            # (F, 2D)
            if ctx.mix_lse:
                r = torch.softmax(torch.addmm(bias, xx, wcat).view(-1, S, C), -1)
                gc = r.mul_((gl * alive).unsqueeze(-1)).view(-1, S * C)
            else:
                gc = gl
            gsum += gc.sum(0)
            gxx += gc.t() @ xx
            if grad_x is not None:
                o = gc @ xcat
                grad_x[:, t0:t0 + step] = torch.addcmul(o[:, :D], xc, o[:, D:], value=-1.0).view(B, -1, D)
        gx2, gx1 = gxx[:, :D], gxx[:, D:]
        grad_means = (gx1 - mu * gsum[:, None]) * iv
        grad_lv = 0.5 * ((gx2 - 2 * mu * gx1 + mu * mu * gsum[:, None]) * iv - gsum[:, None])
        return (grad_x, grad_means.view(S, C, D).to(means.dtype), grad_lv.view(S, C, D).to(log_vars.dtype),
                gsum.view(S, C).to(log_w.dtype), None)


class ViterbiScore(torch.autograd.Function):
    """(states, max_j delta_{T-1}[j]) of the Viterbi recursion (ops.viterbi, OBS_LOG), with the
    gradient of the score: the reference's max-plus recursion (mixture_gaussian.py:290-338)
    routes it along the decoded path only — d/d lp[b,t,s_t] = g_b, d/d log_T[s_{t-1},s_t] += g_b."""

    @staticmethod
    def forward(ctx, lp, log_T, init, plan=None, lengths=None):
        """lengths: per-sequence lengths (ops.viterbi_ragged) or None.  With them the score is
        max_j delta[len_b - 1][j], states is -1 in the padded frames and the gradient follows the
        decoded path over the valid frames only."""
        from . import ops
        if lengths is None:
            states, _, final = ops.viterbi(lp.detach(), log_T.detach(), init.detach(), ops.OBS_LOG, plan)
        else:
            states, _, final = ops.viterbi_ragged(lp.detach(), log_T.detach(), init.detach(), ops.OBS_LOG, lengths)
        ctx.save_for_backward(states)
        ctx.shapes = (lp.shape, log_T.shape)
        ctx.ragged = lengths is not None
        ctx.mark_non_differentiable(states)
        return states, final

    @staticmethod
    def backward(ctx, g_states, g):
        (states,) = ctx.saved_tensors
        (B, T, S), _ = ctx.shapes
        if ctx.ragged:
            # a padded frame (state -1) routes a zero to state 0
            on = states >= 0
            gt = g.view(B, 1) * on
            path = states.clamp(min=0)
            grad_lp = torch.zeros(B, T, S, device=g.device).scatter_(2, path.unsqueeze(-1), gt.unsqueeze(-1))
            grad_T = torch.zeros(S * S, device=g.device)
            if T > 1:
                grad_T.index_add_(0, (path[:, :-1] * S + path[:, 1:]).reshape(-1), gt[:, 1:].reshape(-1))
            grad_init = torch.zeros(S, device=g.device).index_add_(0, path[:, 0], g)
            return grad_lp, grad_T.view(S, S), grad_init, None, None
        grad_lp = torch.zeros(B, T, S, device=g.device)
        grad_lp.scatter_(2, states.unsqueeze(-1), g.view(B, 1, 1).expand(B, T, 1).contiguous())
        grad_T = torch.zeros(S * S, device=g.device)
        if T > 1:
            idx = (states[:, :-1] * S + states[:, 1:]).reshape(-1)
            grad_T.index_add_(0, idx, g.view(B, 1).expand(B, T - 1).reshape(-1))
        grad_init = torch.zeros(S, device=g.device).index_add_(0, states[:, 0], g)
        return grad_lp, grad_T.view(S, S), grad_init, None, None


class SoftDTW(torch.autograd.Function):
    """total (B) = soft-DTW of the distance matrices dist (B,N,M) (ops.soft_dtw), differentiable in
    dist: the backward is the reverse wavefront of Cuturi & Blondel's Algorithm 2 over the saved
    dist and R (ops.soft_dtw_grad), E * grad_total.  Replaces the reference's autograd through the
    per-cell loop of DTWAligner._soft_dtw_align (alignment/dtw.py:277-299); the gradient reaches
    the sequences through the distance matrix by plain torch autograd.

        total = SoftDTW.apply(dist, gamma, n_len, m_len)      # n_len / m_len (B) or None
    """

    @staticmethod
    def forward(ctx, dist, gamma, n_len=None, m_len=None):
        from . import ops
        d = dist.detach()
        R, total = ops.soft_dtw(d, float(gamma), n_len, m_len)
        ctx.save_for_backward(d, R)
        ctx.gamma, ctx.lens = float(gamma), (n_len, m_len)
        return total

    @staticmethod
    def backward(ctx, grad_total):
        from . import ops
        d, R = ctx.saved_tensors
        E = ops.soft_dtw_grad(d, R, ctx.gamma, *ctx.lens)
        return E * grad_total.to(E.dtype)[:, None, None], None, None, None


class CTCLogLik(torch.autograd.Function):
    """loglik (B) = the log-probability CTC gives the targets (ops.ctc, csrc/ctc.hip),
    differentiable in log_probs (T,B,C).  The forward keeps alpha and beta; the backward is the
    occupancy kernel (ops.ctc_grad): d loglik[b] / d log_probs[t,b,c] = the sum of
    gamma[b,t,s] = exp(alpha + beta - loglik) over the positions s of class c, times grad_loglik.
    Replaces autograd through the per-cell loop of ctc_forward_algorithm (alignment/ctc.py:32-121).

    This is the true gradient of loglik with respect to log_probs taken as free variables,
    +sum gamma (each frame's row sums to 1 for a feasible pair).  torch's ctc_loss backward does
    NOT return that: it returns exp(log_probs) - sum gamma at log_probs, i.e. the gradient of the
    loss with log_softmax's Jacobian already folded in (its rows sum to 0, not -1).  The two
    conventions agree only once both are taken back through a log_softmax to the logits, where
    d(-loglik)/d logits = softmax - sum gamma either way; compare them there.

        loglik = CTCLogLik.apply(log_probs, targets, input_lengths, target_lengths, blank)
    """

    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank=0):
        from . import ops
        loglik, alpha, beta, _, _ = ops.ctc(log_probs.detach(), targets, input_lengths, target_lengths, int(blank),
                                            alpha=True, beta=True)
        ctx.save_for_backward(alpha, beta, loglik, targets, torch.as_tensor(input_lengths),
                              torch.as_tensor(target_lengths))
        ctx.blank, ctx.classes, ctx.dtype = int(blank), log_probs.shape[2], log_probs.dtype
        return loglik

    @staticmethod
    def backward(ctx, grad_loglik):
        from . import ops
        alpha, beta, loglik, targets, il, tl = ctx.saved_tensors
        grad, _ = ops.ctc_grad(alpha, beta, loglik, targets, il, tl, ctx.classes, ctx.blank)
        grad = grad * grad_loglik.to(grad.dtype)[None, :, None]
        return grad.to(ctx.dtype), None, None, None, None


class ForcedLogLik(torch.autograd.Function):
    """loglik (B) = the log of the sum over every path of an utterance through its own
    left-to-right chain (ops.forced, csrc/forced.hip), differentiable in log_probs (B,T,C) and in
    whichever of log_stay / log_next / log_skip (B,Smax) are given.  The forward keeps alpha and
    beta; the backward is one launch of the occupancy kernel (ops.forced_grad):

        d loglik[b] / d log_probs[b,t,c] = sum of gamma[b,t,s] over the positions s of class c
        d loglik[b] / d log_stay[b,s]    = the expected number of stays in s, likewise next, skip

    each times grad_loglik[b].  For a pair with a path every frame's log_probs gradient sums to 1
    and the three transition gradients together to T_b - 1; a pair with no path (loglik = -inf)
    contributes exact zeros, not NaN, and so do frames and positions past either length.

        loglik = ForcedLogLik.apply(log_probs, state_ids, input_lengths, state_lengths,
                                    log_stay, log_next, log_skip)
    """

    @staticmethod
    def forward(ctx, log_probs, state_ids, input_lengths, state_lengths, log_stay=None, log_next=None, log_skip=None):
        from . import ops
        det = [None if t is None else t.detach() for t in (log_probs, log_stay, log_next, log_skip)]
        loglik, alpha, beta, _, _, _ = ops.forced(det[0], state_ids, input_lengths, state_lengths, det[1], det[2],
                                                  det[3], alpha=True, beta=True)
        ctx.save_for_backward(alpha, beta, loglik, det[0], state_ids, torch.as_tensor(input_lengths),
                              torch.as_tensor(state_lengths), det[1], det[2], det[3])
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (log_probs, log_stay, log_next, log_skip))
        return loglik

    @staticmethod
    def backward(ctx, grad_loglik):
        from . import ops
        alpha, beta, loglik, lp, ids, il, sl, ws, wn, wk = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = (need[0], ws is not None and need[4], wn is not None and need[5], wk is not None and need[6])
        if not any(want):
            return (None,) * 7
        _, g_lp, g_s, g_n, g_k = ops.forced_grad(alpha, beta, loglik, lp, ids, il, sl, ws, wn, wk, want_gamma=False,
                                                 want_grad=want[0], want_stay=want[1], want_next=want[2],
                                                 want_skip=want[3])
        g = grad_loglik.to(torch.float32)
        out = []
        for w, t, dt in zip(want, (g_lp, g_s, g_n, g_k), ctx.dtypes):
            out.append((t * g.reshape((-1,) + (1,) * (t.dim() - 1))).to(dt) if w else None)
        return out[0], None, None, None, out[1], out[2], out[3]


class DurForcedLogLik(torch.autograd.Function):
    """loglik (B) = the log of the sum over every segmentation of an utterance along its own
    transcript chain with explicit per-position duration scores (ops.durforced,
    csrc/durforced.hip), differentiable in log_probs (B,T,C) and dur_lp (B,Lmax,Dmax).  The
    forward keeps the four tables; the backward is one ops.durforced_grad call that forms only
    the gradients needs_input_grad asks for:

        d loglik[b] / d log_probs[b,t,c] = sum of gamma[b,t,l] over the positions l of class c
        d loglik[b] / d dur_lp[b,l,d-1]  = the expected number of "position l lasts d frames"

    each times grad_loglik[b].  For a feasible pair every used frame's log_probs gradient and every
    used position's dur_lp gradient sum to 1; an infeasible pair (loglik = -inf) contributes exact
    zeros, not NaN, and so do frames and positions past either length.

        loglik = DurForcedLogLik.apply(log_probs, state_ids, input_lengths, state_lengths, dur_lp)
    """

    @staticmethod
    def forward(ctx, log_probs, state_ids, input_lengths, state_lengths, dur_lp):
        from . import ops
        lp, du = log_probs.detach(), dur_lp.detach()
        loglik, begin, F, Bend, Bbeg, shift, lls, _, _, _ = ops.durforced(lp, state_ids, input_lengths, state_lengths,
                                                                          du, tables=True)
        ctx.save_for_backward(begin, F, Bend, Bbeg, shift, lls, lp, state_ids, torch.as_tensor(input_lengths),
                              torch.as_tensor(state_lengths), du)
        ctx.dtypes = (log_probs.dtype, dur_lp.dtype)
        return loglik

    @staticmethod
    def backward(ctx, grad_loglik):
        from . import ops
        need = ctx.needs_input_grad
        want = (need[0], need[4])
        if not any(want):
            return (None,) * 5
        _, g_lp, g_du = ops.durforced_grad(*ctx.saved_tensors, want_gamma=False, want_grad=want[0], want_dur=want[1])
        g = grad_loglik.to(torch.float32)
        out = [(t * g.reshape(-1, 1, 1)).to(dt) if w else None for w, t, dt in zip(want, (g_lp, g_du), ctx.dtypes)]
        return out[0], None, None, None, out[1]


class HsmmLogLik(torch.autograd.Function):
    """loglik (B) = log of the sum over segmentations of the explicit-duration model
    (ops.hsmm_forward_backward, csrc/hsmm_fb.hip), differentiable in lp (B,T,S), dur_lp (S,Dmax),
    log_T (S,S) and log_init (S) or None.  The forward is the forward sum alone; the backward is
    one forward-backward call that forms only the posteriors and counts of the inputs that need a
    gradient, weighted per sequence by the incoming gradient:

        grad_lp = g_b gamma_b            grad_dur_lp   = sum_b g_b dur_counts_b
        grad_log_T = sum_b g_b trans_counts_b          grad_log_init = sum_b g_b init_post_b

    log_T's diagonal is never used by the model, so its gradient is zero there.
    The backward's call runs the forward sum again beside the backward one: no (B,T,S) table is
    kept alive between forward and backward.

        loglik = HsmmLogLik.apply(lp, dur_lp, log_T, log_init)
    """

    @staticmethod
    def forward(ctx, lp, dur_lp, log_T, log_init=None):
        from . import ops
        saved = [t.detach() for t in (lp, dur_lp, log_T)]
        saved.append(None if log_init is None else log_init.detach())
        loglik = ops.hsmm_forward_backward(*saved)[0]
        ctx.save_for_backward(*saved)
        ctx.dtypes = tuple(None if t is None else t.dtype for t in (lp, dur_lp, log_T, log_init))
        return loglik

    @staticmethod
    def backward(ctx, g):
        from . import ops
        lp, dur_lp, log_T, log_init = ctx.saved_tensors
        need = list(ctx.needs_input_grad[:4])
        need[3] = need[3] and log_init is not None
        if not any(need):
            return None, None, None, None
        _, gamma, dur_c, trans_c, init_p = ops.hsmm_forward_backward(
            lp, dur_lp, log_T, log_init, want_gamma=need[0], want_dur=need[1], want_trans=need[2],
            want_init=need[3])
        g = g.to(torch.float32)
        grads = [gamma * g[:, None, None] if need[0] else None,
                 torch.einsum("b,bsd->sd", g, dur_c) if need[1] else None,
                 torch.einsum("b,bij->ij", g, trans_c) if need[2] else None,
                 torch.einsum("b,bs->s", g, init_p) if need[3] else None]
        return tuple(None if x is None else x.to(dt) for x, dt in zip(grads, ctx.dtypes))


class SparseLogLik(torch.autograd.Function):
    """loglik (B) of a padded batch under an HMM whose transitions are an arc list
    (sparse.SparseTransitions; ops.sparse_forward_backward, csrc/sparse.hip), differentiable in

        log_obs (B,T,N)   d loglik[b] / d log_obs[b,t,j] = gamma[b,t,j]
        log_w   (E)       d sum_b g_b loglik[b] / d log_w[e] = xi[e], the expected number of times
                          arc e is taken, in the caller's arc order (ops.sparse_arc_counts with g)
        log_p0  (N)       d loglik[b] / d log_p0[j] = gamma[b,0,j]

    The forward asks for the posterior only when log_obs or log_p0 needs a gradient and keeps the
    workspace only when log_w does; the backward forms xi in one call with the incoming gradient as
    the per-sequence weight.  A sequence with no path (loglik = -inf) and padded frames contribute
    exact zeros.  This is the gradient of more than 256 states that SequenceLogLik refuses.

        loglik = SparseLogLik.apply(log_obs, log_w, log_p0, transitions, lengths)

    lengths: host int64 (B) from ops.ragged_lengths, or None.  range_guard (default on): a sequence
    that left the kernels' fp32 range (range_guard.out_of_range) takes its value, posterior and arc
    counts -- so its gradients -- from the float64 log-space loop; the others keep the kernels' bits.
    One host read of a flag per forward; skipped while a CUDA graph is being captured."""

    @staticmethod
    def forward(ctx, log_obs, log_w, log_p0, transitions, lengths=None, range_guard=True):
        tr = transitions
        nat.require_gpu(log_obs, log_w, log_p0)
        obs = log_obs.detach().to(torch.float32).contiguous()
        w = log_w.detach().to(torch.float32)
        need = ctx.needs_input_grad
        want_post = bool(need[0] or need[2])
        loglik, post, ws = ops.sparse_forward_backward(
            obs, tr.in_ptr_host, tr.in_ptr, tr.in_src, w[tr.perm_in].contiguous(), tr.out_ptr_host, tr.out_ptr,
            tr.out_dst, w[tr.perm_out].contiguous(), log_p0.detach(), want_post, lengths)
        bad = rg.sparse_flagged(ws, obs, lengths) if range_guard and obs.shape[0] else None
        if bad is not None:
            lens = None if lengths is None else lengths.to(obs.device)[bad]
            ll, g, _ = rg.logspace_forward_backward(obs[bad], log_p0, src=tr.src, dst=tr.dst, log_w=w, lengths=lens,
                                                    want_xi=False)
            loglik = loglik.index_copy(0, bad, ll.to(loglik.dtype))
            if want_post:
                post = post.index_copy(0, bad, g.to(post.dtype))
        ctx.transitions, ctx.lengths, ctx.bad = tr, lengths, bad
        ctx.dtypes = (log_obs.dtype, log_w.dtype, log_p0.dtype)
        # (log_p0: the backward's log-space counts of the flagged sequences need it)
        ctx.save_for_backward(post if want_post else None, *((obs, w, ws) if need[1] else (None, None, None)),
                              log_p0.detach() if bad is not None and need[1] else None)
        return loglik

    @staticmethod
    def backward(ctx, grad_loglik):
        post, obs, w, ws, l0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        tr = ctx.transitions
        g = grad_loglik.to(torch.float32).contiguous()
        g_obs = g_w = g_p0 = None
        if need[0]:
            g_obs = (post * g[:, None, None]).to(ctx.dtypes[0])
        if need[2]:
            g_p0 = (post[:, 0] * g[:, None]).sum(0).to(ctx.dtypes[2])
        if need[1]:
            g_w = ops.sparse_arc_counts(obs, tr.src, tr.dst, w.contiguous(), ws, g, ctx.lengths)
            bad = ctx.bad
            if bad is not None:
                # the forward neutralised the flagged sequences' rows: their counts come from the loop
                lens = None if ctx.lengths is None else ctx.lengths.to(obs.device)[bad]
                g_w = g_w + rg.logspace_forward_backward(obs[bad], l0, src=tr.src, dst=tr.dst, log_w=w,
                                                         lengths=lens, weight=g[bad])[2]
            g_w = g_w.to(ctx.dtypes[1])
        return g_obs, g_w, g_p0, None, None, None
