"""PyTorch-ROCm custom ops over the hmm355 C ABI (namespace ``hmm355``).

Each op allocates its outputs (and the C ABI's workspace) through the torch caching
allocator on the input's device and launches on the current HIP stream.  The ops are
registered with torch.library so they are visible to torch.compile / export and have
shape-only fake implementations; their only real implementation is the HIP library.
An op's outputs are written once, in its `_<op>_outputs` spec, which the op and its fake both
call; every native call goes through `_call` (workspace, stream, device, error check) and every
lengths argument through `_lengths`.

  torch.ops.hmm355.forward_backward(obs, log_P, log_p0, obs_mode, out_mask)
      -> (posterior, forward, backward, loglik, lik_ref)
  torch.ops.hmm355.viterbi(obs, log_P, init, obs_mode) -> (states, log_delta, final_score)
  torch.ops.hmm355.forward_backward_ragged(obs, log_P, log_p0, obs_mode, lengths, out_mask, log_beta_T)
      -> (posterior, forward, backward, loglik, lik_ref)     sequence b = obs[b, :lengths[b]]
  torch.ops.hmm355.viterbi_ragged(obs, log_P, init, obs_mode, lengths) -> (states, log_delta, final_score)
  torch.ops.hmm355.gmm_diag_logprob(x, means, log_vars, log_w, mix_lse) -> log_probs
  torch.ops.hmm355.hsmm_viterbi(lp, dur_lp, log_T) -> (states, scores)
  torch.ops.hmm355.hsmm_forward_backward(lp, dur_lp, log_T, log_init, want_gamma=, want_dur=,
                                         want_trans=, want_init=, flags=)
      -> (loglik, gamma, dur_counts, trans_counts, init_post)
  torch.ops.hmm355.tv_forward_backward(log_obs, log_A, log_p0, out_mask)
      -> (posterior, forward, backward, loglik, lik_ref)
  torch.ops.hmm355.tv_viterbi(log_obs, log_A, init) -> (states, log_delta)
  torch.ops.hmm355.dtw(dist, pattern, n_len, m_len, want_cost, want_path)
      -> (cost_matrix, total, path_i, path_j, path_len)
  torch.ops.hmm355.soft_dtw(dist, gamma, n_len, m_len) -> (R, total)
  torch.ops.hmm355.soft_dtw_grad(dist, R, gamma, n_len, m_len) -> E
  torch.ops.hmm355.ctc(log_probs, targets, input_lengths, target_lengths, blank, alpha, beta, viterbi)
      -> (loglik, alpha, beta, path, score)
  torch.ops.hmm355.ctc_grad(alpha, beta, loglik, targets, input_lengths, target_lengths, num_classes,
                            blank, want_gamma) -> (grad, gamma)
  torch.ops.hmm355.duration_constrained_viterbi(emission_log_probs, log_transitions, min_duration,
                                                max_duration, penalty_weight, per_sequence, want_trellis)
      -> (states, final_score, log_delta, durations)
  torch.ops.hmm355.forced(log_probs, state_ids, input_lengths, state_lengths, log_stay, log_next, log_skip,
                          alpha, beta, viterbi) -> (loglik, alpha, beta, path, score, durations)
  torch.ops.hmm355.forced_grad(alpha, beta, loglik, log_probs, state_ids, input_lengths, state_lengths,
                               log_stay, log_next, log_skip, want_gamma, want_grad, want_stay, want_next,
                               want_skip) -> (gamma, grad_log_probs, grad_stay, grad_next, grad_skip)
  torch.ops.hmm355.durforced(log_probs, state_ids, input_lengths, state_lengths, dur_lp, tables=, viterbi=)
      -> (loglik, begin, F, Bend, Bbeg, frame_shift, loglik_shifted, path, score, durations)
  torch.ops.hmm355.durforced_grad(begin, F, Bend, Bbeg, frame_shift, loglik_shifted, log_probs, state_ids,
                                  input_lengths, state_lengths, dur_lp, want_gamma=, want_grad=, want_dur=)
      -> (gamma, grad_log_probs, grad_dur_lp)
  torch.ops.hmm355.ffbs(fwd, log_P, uniforms, lengths) -> states (B,K,T)     posterior path samples
  torch.ops.hmm355.gmm_stats(x, weight, means, log_vars, log_w, mix_lse, lengths) -> (occ, sx, sxx)
  torch.ops.hmm355.viterbi_nbest(obs, log_P, init, obs_mode, num_paths, lengths)
      -> (paths (B,K,T), scores (B,K), count (B))     the K best state paths, in order
  torch.ops.hmm355.sparse_viterbi(obs, in_ptr_host, in_ptr, in_src, in_log_w, init, lengths)
      -> (states, log_delta, final_score)             Viterbi over an arc list, N <= 8192
  torch.ops.hmm355.sparse_forward_backward(obs, in_ptr_host, in_ptr, in_src, in_log_w, out_ptr_host, out_ptr,
                                           out_dst, out_log_w, log_p0, want_posterior, lengths)
      -> (loglik (B), posterior (B,T,N), workspace)   the sums over an arc list
  torch.ops.hmm355.sparse_arc_counts(obs, src, dst, log_w, workspace, weight, lengths) -> xi (E) fp64
"""
import functools
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _native as nat

OBS_PROB = nat.OBS_PROB
OBS_LOG = nat.OBS_LOG
FB_POSTERIOR = nat.FB_POSTERIOR
FB_PAIR = nat.FB_PAIR
FB_PLAN_BANDED = nat.FB_PLAN_BANDED
# test / A-B switches of the followers' end rows, passed in forward_backward's out_mask
FB_NO_END_ROWS = nat.FB_NO_END_ROWS
FB_END_ROWS_ODD_LEFT = nat.FB_END_ROWS_ODD_LEFT
VIT_PLAN_BANDED = nat.VIT_PLAN_BANDED
VIT_PLAN_DENSE = nat.VIT_PLAN_DENSE
FORM_GENERAL = nat.FORM_GENERAL
FORM_SERIAL_WALK = nat.FORM_SERIAL_WALK
FB_FORWARD = nat.FB_FORWARD
FB_BACKWARD = nat.FB_BACKWARD
NARROW_MAX_STATES = nat.NARROW_MAX_STATES
WIDE_MAX_STATES = nat.WIDE_MAX_STATES

_EMPTY = (0,)
_F32, _I64, _I32 = torch.float32, torch.int64, torch.int32


def _f32c(t):
    return t.to(torch.float32).contiguous()


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


# A spec `_<op>_outputs(mk, sizes..., wants...)` allocates each output with mk(shape, dtype=...): the op
# passes _on(device), its fake x.new_empty.  It states every dtype (new_empty would inherit the
# input's) and gives an output that is not wanted the empty shape _EMPTY (0 for the 1-D ones).
def _on(device):
    return functools.partial(torch.empty, device=device)


def _scores_output(mk, B, T, S):
    """The single fp32 (B,T,S) output of gmm_diag_logprob, semimarkov_quad and soft_dtw_grad."""
    return mk((B, T, S), dtype=_F32)


def _opt(t, want):
    """Pointer of an optional output: NULL unless it is wanted."""
    return nat.ptr(t) if want else None


def _call(dev, fn, *args, ws=None):
    """One native call on `dev`'s current stream, raised through nat.check: fn(*args, stream), or with
    `ws` fn(*args, workspace, its bytes, stream).  ws is the workspace's size in bytes, allocated here,
    or a workspace tensor to use again; the tensor is returned (callers that read it keep it)."""
    if ws is None:
        tail = ()
    else:
        if not isinstance(ws, Tensor):
            ws = _workspace(ws, dev)
        tail = (nat.ptr(ws), ws.numel())
    with torch.cuda.device(dev):
        nat.check(fn(*args, *tail, nat.stream_of(dev)))
    return ws


def _lengths(lengths, name, count, lo, hi, dev=None, integers=None):
    """One lengths argument (a tensor on any device, a list or a numpy array) checked on the host
    (ValueError): `count` values in [lo, hi].  integers: None takes any dtype (whole numbers in a
    float tensor pass); "first" / "last" refuse a floating, complex or boolean one before / after
    the count is checked (the order each caller has always had).  Returns (CPU int64 tensor, int32
    tensor on `dev` or None without one).  Reading the values is one synchronisation."""
    t = torch.as_tensor(lengths)
    refused = integers is not None and (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)
    if refused and integers == "first":
        raise ValueError(f"{name} must hold integers; got {t.dtype}")
    if t.numel() != count:
        raise ValueError(f"{name} must hold one length per sequence ({count}); got {tuple(t.shape)}")
    if refused:
        raise ValueError(f"{name} must hold integers; got {t.dtype}")
    host = t.detach().reshape(count).to("cpu", torch.int64)
    if count and (int(host.min()) < lo or int(host.max()) > hi):
        raise ValueError(f"{name} must lie in [{lo}, {hi}]; got {host.tolist()}")
    return host, None if dev is None else host.to(torch.int32).to(dev)


# ------------------------------------------------------------------ forward-backward
def _use_wide(N: int, wide: Optional[bool]) -> bool:
    """The batch-tiled form (csrc/wide.hip, one launch per time step, N <= 4096): above 256 states
    unless the caller says otherwise; wide=True forces it at any N (parity tests)."""
    return N > NARROW_MAX_STATES if wide is None else bool(wide)


def make_plan(log_P: Tensor, read_banded: bool = True, dense: bool = False) -> Optional[Tensor]:
    """Measure log_P's banded structure once (hmm355_plan_ex_f32) into a device byte tensor that
    forward_backward / viterbi accept as `plan` (valid while log_P is unchanged).  dense=True
    (HMM355_PLAN_DENSE) makes a plan that selects the dense chains whatever the structure (the
    parity tests run both chain families on one matrix).

    The kernels read the structure from the plan on the device; the host only needs it to
    choose between launch shapes (the pair kernel, the psi followers), and reading it back is
    one synchronous device -> host copy.  With read_banded=False (a plan re-formed on every
    training step, where log_P changes each call) that read is skipped and the plan's host
    word stays unknown (None): forward_backward takes the two-kernel path, whose chains branch
    on the device-side structure, and viterbi asks for psi followers, which return at once on
    a banded plan (vit_kern.h vit_psi_follow) -- so the call stays asynchronous.

    Above 256 states there is no plan (None, no native call): forward_backward / viterbi take
    the batch-tiled form there, which reads log_P as it is."""
    if log_P.shape[0] > NARROW_MAX_STATES:
        return None
    nat.require_gpu(log_P)
    log_P = _f32c(log_P)
    N = log_P.shape[0]
    L = nat.lib()
    plan = torch.empty(L.hmm355_plan_bytes(N), dtype=torch.uint8, device=log_P.device)
    _call(log_P.device, L.hmm355_plan_ex_f32, nat.ptr(log_P), N, nat.PLAN_DENSE if dense else 0, nat.ptr(plan))
    if not read_banded:
        plan._hmm355_banded = None
        return plan
    # banded in both directions: forward_backward then runs both chains of a sequence in
    # one workgroup (HMM355_FB_PAIR, csrc/fbpair.h).  One synchronous read per plan.
    with torch.cuda.device(log_P.device):
        banded = L.hmm355_plan_banded(nat.ptr(plan), nat.stream_of(log_P.device))
    if banded < 0:
        nat.check(banded)
    plan._hmm355_banded = banded == 1
    return plan


def plan_info(plan: Optional[Tensor]) -> dict:
    """Which chains a plan selects (band.h BandDesc: wc/wr window widths, Toeplitz windows).
    Reads a few ints back to the host."""
    if plan is None:
        return {"forward": "detected per call", "backward": "detected per call", "viterbi": "detected per call"}
    h = plan[: 4 * 7177].cpu().view(torch.int32).tolist()
    wc, wr = h[0], h[1]
    tcd0, tcw, trd0, trw = h[7172:7176]
    band_max = 8   # band.h kBandMax

    def name(w, tw, td0):
        if w > band_max:
            return "dense"
        return f"banded(W={w}, toeplitz {td0}..{td0 + tw - 1})" if tw > 0 else f"banded(W={w})"
    col = name(wc, tcw, tcd0)
    # beside the names, the raw header (BandDesc wc .. wrp, tcd0 .. trw, uafl)
    return {"forward": col, "viterbi": col, "backward": name(wr, trw, trd0),
            "wc": wc, "wr": wr, "wcp": h[2], "wrp": h[3], "tcd0": tcd0, "tcw": tcw, "trd0": trd0, "trw": trw,
            "uniform_floor": h[7176]}


_CUS = {}


# forward_backward's posterior beside the chains (follow=None): measured per round on MI355X
# (DESIGN.md §5); a caller's True / False wins
FB_FOLLOW_DEFAULT = True


def fb_follow_default(follow: Optional[bool]) -> bool:
    return FB_FOLLOW_DEFAULT if follow is None else bool(follow)


def _use_pair(B: int, dev) -> bool:
    """Both chains of a sequence in one workgroup (csrc/fbpair.h, HMM355_FB_PAIR) when the
    batch is larger than half the CUs: the two-kernel path then needs more CU-owning
    workgroups (2B) than the chip has and runs in two rounds, while the pair kernel needs B.
    Measured: B=32 two-kernel 0.24 ms vs pair 0.38 ms; B=256 FB op 0.90 vs 0.51
    ms.  (forward_backward's `pair` argument overrides it.)"""
    key = str(dev)
    if key not in _CUS:
        _CUS[key] = torch.cuda.get_device_properties(dev).multi_processor_count
    return B > _CUS[key] // 2


def _fb_outputs(mk, B, T, N, out_mask):
    """(posterior, forward, backward, loglik, lik_ref) of every forward-backward entry point."""
    rows = (B, T, N)   # (written out, not looped: bench.py's step pays this host time)
    return (mk(rows if out_mask & FB_POSTERIOR else _EMPTY, dtype=_F32),
            mk(rows if out_mask & FB_FORWARD else _EMPTY, dtype=_F32),
            mk(rows if out_mask & FB_BACKWARD else _EMPTY, dtype=_F32), mk(B, dtype=_F32), mk(B, dtype=_F32))


def _fb_ptrs(outs, out_mask):
    """The five output pointers as the forward-backward entry points take them."""
    post, fwd, bwd, loglik, lik_ref = outs
    return (nat.ptr(post) if out_mask & FB_POSTERIOR else None, nat.ptr(fwd) if out_mask & FB_FORWARD else None,
            nat.ptr(bwd) if out_mask & FB_BACKWARD else None, nat.ptr(loglik), nat.ptr(lik_ref))


@torch.library.custom_op("hmm355::forward_backward", mutates_args=())
def forward_backward(obs: Tensor, log_P: Tensor, log_p0: Tensor, obs_mode: int,
                     out_mask: int, plan: Optional[Tensor] = None, pair: Optional[bool] = None,
                     follow: Optional[bool] = None,
                     wide: Optional[bool] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """pair / follow (None = chosen from the batch and the plan): with a host-known banded plan,
    `pair` runs both chains of a sequence in one workgroup (HMM355_FB_PAIR, large batches) and
    otherwise `follow` forms the posterior inside the chains' launch (HMM355_FB_PLAN_BANDED).
    wide (None = N > 256): the batch-tiled form (hmm355_forward_backward_wide_f32, N <= 4096),
    which ignores plan / pair / follow."""
    nat.require_gpu(obs, log_P, log_p0)
    obs, log_P, log_p0 = _f32c(obs), _f32c(log_P), _f32c(log_p0)
    B, T, N = obs.shape
    dev = obs.device
    L = nat.lib()
    outs = _fb_outputs(_on(dev), B, T, N, out_mask)
    if B == 0:
        return outs
    if _use_wide(N, wide):
        _call(dev, L.hmm355_forward_backward_wide_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(log_p0),
              B, T, N, out_mask & 7, *_fb_ptrs(outs, out_mask), ws=L.hmm355_fb_wide_workspace_bytes(B, T, N))
        return outs
    banded = plan is not None and getattr(plan, "_hmm355_banded", False) is True
    use_pair = banded and (_use_pair(B, dev) if pair is None else pair)
    if use_pair:
        out_mask |= FB_PAIR
    elif banded and (out_mask & FB_POSTERIOR) and fb_follow_default(follow):
        out_mask |= FB_PLAN_BANDED
    _call(dev, L.hmm355_forward_backward_plan_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(log_p0),
          nat.ptr(plan), None, B, T, N, out_mask, *_fb_ptrs(outs, out_mask),
          ws=L.hmm355_fb_workspace_bytes(B, T, N))
    return outs


@forward_backward.register_fake
def _(obs, log_P, log_p0, obs_mode, out_mask, plan=None, pair=None, follow=None, wide=None):
    return _fb_outputs(obs.new_empty, *obs.shape, out_mask)


# ---------------------------------------------------------------------------- Viterbi
def _viterbi_outputs(mk, B, T, N):
    """(states, log_delta, final_score) of viterbi and viterbi_ragged."""
    return mk((B, T), dtype=_I64), mk((B, T, N), dtype=_F32), mk(B, dtype=_F32)


@torch.library.custom_op("hmm355::viterbi", mutates_args=())
def viterbi(obs: Tensor, log_P: Tensor, init: Tensor, obs_mode: int,
            plan: Optional[Tensor] = None, follow: Optional[bool] = None,
            wide: Optional[bool] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """follow (None = on): with a plan, the work beside the chain inside its launch -- for a
    host-known banded plan the log leaders and the decode follower (HMM355_VIT_PLAN_BANDED), for a
    dense one the psi followers (HMM355_VIT_PLAN_DENSE).
    wide (None = N > 256): the batch-tiled form (hmm355_viterbi_wide_f32, N <= 4096), which
    ignores plan / follow."""
    nat.require_gpu(obs, log_P, init)
    obs, log_P, init = _f32c(obs), _f32c(log_P), _f32c(init)
    B, T, N = obs.shape
    dev = obs.device
    L = nat.lib()
    states, delta, final = outs = _viterbi_outputs(_on(dev), B, T, N)
    if B == 0:
        return outs
    if _use_wide(N, wide):
        _call(dev, L.hmm355_viterbi_wide_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(init), B, T, N,
              nat.ptr(states), nat.ptr(delta), nat.ptr(final),
              ws=L.hmm355_viterbi_wide_workspace_bytes(B, T, N, obs_mode))
        return outs
    flags = 0
    if plan is not None and follow is not False:
        if getattr(plan, "_hmm355_banded", False) is True:
            flags = VIT_PLAN_BANDED   # the decode beside the banded chain (csrc/follow.h)
        else:
            # a dense plan: the argmax pointers computed beside the chain, on the CUs it leaves
            # (a plan whose structure the host never read,
            # make_plan(read_banded=False), asks for them too: on a banded matrix they return at once)
            flags = VIT_PLAN_DENSE
    _call(dev, L.hmm355_viterbi_plan_ex_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(init), nat.ptr(plan),
          flags, B, T, N, nat.ptr(states), nat.ptr(delta), nat.ptr(final),
          ws=L.hmm355_viterbi_workspace_bytes_ex(B, T, N, obs_mode))
    return outs


@viterbi.register_fake
def _(obs, log_P, init, obs_mode, plan=None, follow=None, wide=None):
    return _viterbi_outputs(obs.new_empty, *obs.shape)


# ------------------------------------------------------- padded batches with lengths
def ragged_lengths(lengths, B: int, T: int, N: Optional[int] = None) -> Tensor:
    """Checks the per-sequence lengths of a padded (B,T,N) batch on the host (ValueError) and
    returns them as a CPU int64 tensor (B).  Accepts a tensor on any device, a list or a numpy
    array; needs exactly B integer values in [1, T].  The lengths are read on the host: the call's
    one synchronisation.  With N given, more than 256 states are rejected: the ragged form is one
    workgroup per sequence (csrc/ragged.hip)."""
    if N is not None and N > NARROW_MAX_STATES:
        raise ValueError(f"per-sequence lengths are supported for at most {NARROW_MAX_STATES} states; got {N}")
    return _lengths(lengths, "lengths", B, 1, T, integers="first")[0]


def active_lengths(lengths, B: int, T: int, N: Optional[int] = None) -> Optional[Tensor]:
    """The checked lengths (ragged_lengths) when they shorten a sequence, None when `lengths` is
    None or every length is T: the callers' `lengths=None` path, bit for bit."""
    if lengths is None:
        return None
    host = ragged_lengths(lengths, B, T, N)
    return None if bool((host == T).all()) else host


def _equal_length(host: Tensor) -> Optional[int]:
    """The common length when every sequence has the same one (B == 1 included), else None."""
    if host.numel() == 0:
        return None
    first = int(host[0])
    return first if bool((host == first).all()) else None


def _pad_frames(x: Tensor, T: int, fill) -> Tensor:
    """x (B,L,...) padded with `fill` to T frames (x itself when L == T)."""
    if x.shape[1] == T:
        return x
    out = x.new_full((x.shape[0], T) + tuple(x.shape[2:]), fill)
    out[:, : x.shape[1]] = x
    return out


@torch.library.custom_op("hmm355::forward_backward_ragged", mutates_args=())
def forward_backward_ragged(obs: Tensor, log_P: Tensor, log_p0: Tensor, obs_mode: int, lengths: Tensor,
                            out_mask: int,
                            log_beta_T: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """forward_backward of a padded batch: sequence b is obs[b, :lengths[b]].  Outputs as
    forward_backward; posterior / forward / backward are 0 in frames >= lengths[b], which are
    never read.  Dispatch is from the input alone: equal lengths (B == 1 included) run the tuned
    chains on obs[:, :L] with today's speed and bits, unequal ones csrc/ragged.hip.  log_beta_T
    (B,N): the terminal backward vector at frame lengths[b] - 1 (always the ragged form)."""
    B, T, N = obs.shape
    host = ragged_lengths(lengths, B, T, N)
    nat.require_gpu(obs, log_P, log_p0, log_beta_T)
    out_mask &= FB_POSTERIOR | FB_FORWARD | FB_BACKWARD
    L0 = _equal_length(host)
    if log_beta_T is None and (B == 0 or L0 is not None):
        post, fwd, bwd, loglik, lik_ref = forward_backward(obs[:, :L0] if B else obs, log_P, log_p0, obs_mode, out_mask)
        pad = lambda x, bit: _pad_frames(x, T, 0.0) if out_mask & bit else x
        return pad(post, FB_POSTERIOR), pad(fwd, FB_FORWARD), pad(bwd, FB_BACKWARD), loglik, lik_ref
    obs, log_P, log_p0 = _f32c(obs), _f32c(log_P), _f32c(log_p0)
    lbt = None if log_beta_T is None else _f32c(log_beta_T)
    dev = obs.device
    lens = host.to(torch.int32).to(dev)
    L = nat.lib()
    outs = _fb_outputs(_on(dev), B, T, N, out_mask)
    _call(dev, L.hmm355_forward_backward_ragged_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(log_p0),
          nat.ptr(lbt), nat.ptr(lens), B, T, N, out_mask, *_fb_ptrs(outs, out_mask),
          ws=L.hmm355_fb_workspace_bytes(B, T, N))
    return outs


@forward_backward_ragged.register_fake
def _(obs, log_P, log_p0, obs_mode, lengths, out_mask, log_beta_T=None):
    return _fb_outputs(obs.new_empty, *obs.shape, out_mask)


@torch.library.custom_op("hmm355::viterbi_ragged", mutates_args=())
def viterbi_ragged(obs: Tensor, log_P: Tensor, init: Tensor, obs_mode: int,
                   lengths: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """viterbi of a padded batch: sequence b is obs[b, :lengths[b]].  (states, log_delta,
    final_score) as viterbi, the valid frames bit-identical to a decode of the slice alone;
    frames >= lengths[b] are never read and get states = -1, log_delta = -inf.  final_score[b] =
    max_j delta[lengths[b] - 1][j].  Equal lengths run the tuned chains on obs[:, :L], unequal
    ones csrc/ragged.hip."""
    B, T, N = obs.shape
    host = ragged_lengths(lengths, B, T, N)
    nat.require_gpu(obs, log_P, init)
    L0 = _equal_length(host)
    if B == 0 or L0 is not None:
        states, delta, final = viterbi(obs[:, :L0] if B else obs, log_P, init, obs_mode)
        return _pad_frames(states, T, -1), _pad_frames(delta, T, float("-inf")), final
    obs, log_P, init = _f32c(obs), _f32c(log_P), _f32c(init)
    dev = obs.device
    lens = host.to(torch.int32).to(dev)
    L = nat.lib()
    states, delta, final = outs = _viterbi_outputs(_on(dev), B, T, N)
    _call(dev, L.hmm355_viterbi_ragged_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(init), nat.ptr(lens),
          B, T, N, nat.ptr(states), nat.ptr(delta), nat.ptr(final),
          ws=L.hmm355_viterbi_ragged_workspace_bytes(B, T, N, obs_mode))
    return outs


@viterbi_ragged.register_fake
def _(obs, log_P, init, obs_mode, lengths):
    return _viterbi_outputs(obs.new_empty, *obs.shape)


# ------------------------------------------------------------------- N-best Viterbi
NBEST_MAX_PATHS = 16


def _viterbi_nbest_outputs(mk, B, T, K):
    """(paths, scores, count) of viterbi_nbest."""
    return mk((B, K, T), dtype=_I64), mk((B, K), dtype=_F32), mk(B, dtype=_I32)


def _viterbi_nbest_op():
    """Registers hmm355::viterbi_nbest and its fake.  The op takes checked arguments (lengths: the
    CPU tensor of ragged_lengths, or None); viterbi_nbest below is its caller."""
    @torch.library.custom_op("hmm355::viterbi_nbest", mutates_args=())
    def op(obs: Tensor, log_P: Tensor, init: Tensor, obs_mode: int, num_paths: int,
           lengths: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        nat.require_gpu(obs, log_P, init)
        obs, log_P, init = _f32c(obs.detach()), _f32c(log_P.detach()), _f32c(init.detach())
        B, T, N = obs.shape
        dev = obs.device
        paths, scores, count = outs = _viterbi_nbest_outputs(_on(dev), B, T, num_paths)
        if B == 0:
            return outs
        lens = None if lengths is None else lengths.to(torch.int32).to(dev)
        L = nat.lib()
        _call(dev, L.hmm355_viterbi_nbest_f32, nat.ptr(obs), obs_mode, nat.ptr(log_P), nat.ptr(init), nat.ptr(lens),
              B, T, N, num_paths, nat.ptr(paths), nat.ptr(scores), nat.ptr(count),
              ws=L.hmm355_viterbi_nbest_workspace_bytes(B, T, N, num_paths, obs_mode))
        return outs

    @op.register_fake
    def _(obs, log_P, init, obs_mode, num_paths, lengths=None):
        return _viterbi_nbest_outputs(obs.new_empty, obs.shape[0], obs.shape[1], num_paths)


_viterbi_nbest_op()


def viterbi_nbest(obs: Tensor, log_P: Tensor, init: Tensor, obs_mode: int, num_paths: int,
                  lengths=None) -> Tuple[Tensor, Tensor, Tensor]:
    """The num_paths = K most probable state paths of every sequence, in order (list Viterbi:
    torch.ops.hmm355.viterbi_nbest over hmm355_viterbi_nbest_f32, csrc/nbest.hip; the recursion and
    its tie order are spelled out in include/hmm355.h).  obs (B,T,N), log_P (N,N), init (N);
    lengths: None or one length per sequence in any form ragged_lengths takes.  Returns
    (paths (B,K,T) int64, scores (B,K) fp32 non-increasing in k, count (B) int32: the ranks with a
    score above -inf).  Rank 0 is the path and final_score of viterbi / viterbi_ragged, bit for
    bit; a rank k >= max(count, 1) does not exist and gets score -inf and states -1; frames
    >= lengths[b] are never read and get state -1.  1 <= N <= 256, 1 <= K <= 16 (ValueError
    beyond, raised here on the host).  No gradients: the inputs are detached."""
    if obs.dim() != 3:
        raise ValueError(f"obs must be (B, T, N); got {tuple(obs.shape)}")
    B, T, N = obs.shape
    K = int(num_paths)
    if K < 1 or K > NBEST_MAX_PATHS:
        raise ValueError(f"num_paths must lie in [1, {NBEST_MAX_PATHS}]; got {num_paths}")
    if N > NARROW_MAX_STATES:
        raise ValueError(f"N-best Viterbi supports at most {NARROW_MAX_STATES} states; got {N}")
    host = None if lengths is None else ragged_lengths(lengths, B, T, N)
    nat.require_gpu(obs, log_P, init)
    return torch.ops.hmm355.viterbi_nbest(obs, log_P, init, obs_mode, K, host)


# ------------------------------------------------------------- sparse transitions (arc list)
SPARSE_MAX_STATES = nat.SPARSE_MAX_STATES
SPARSE_MAX_ARCS = nat.SPARSE_MAX_ARCS


def _sparse_viterbi_outputs(mk, B, T, N):
    """(states, log_delta, final_score) of sparse_viterbi."""
    return mk((B, T), dtype=_I64), mk((B, T, N), dtype=_F32), mk(B, dtype=_F32)


def _sparse_fb_outputs(mk, B, T, N, E, want_posterior):
    """(loglik, posterior, workspace) of sparse_forward_backward; the workspace's size is the
    library's answer (a host function), so the fake gives the same shape."""
    nbytes = nat.lib().hmm355_sparse_forward_backward_workspace_bytes(B, T, N, E) if B else 0
    return (mk(B, dtype=_F32), mk((B, T, N) if want_posterior else _EMPTY, dtype=_F32),
            mk(max(int(nbytes), 1), dtype=torch.uint8))


def _sparse_counts_outputs(mk, E):
    """xi of sparse_arc_counts."""
    return mk(E, dtype=torch.float64)


def _dev_lengths(lengths, dev):
    return None if lengths is None else lengths.to(torch.int32).to(dev)


def _sparse_ops():
    """Registers hmm355::sparse_viterbi, ::sparse_forward_backward and ::sparse_arc_counts with their
    fakes.  The ops take checked arguments: the sorted arc arrays of sparse.SparseTransitions (a
    row-pointer array twice, as a CPU int32 tensor and on the device) and lengths as the CPU tensor
    of ragged_lengths, or None; the functions below are their callers."""
    @torch.library.custom_op("hmm355::sparse_viterbi", mutates_args=())
    def vit(obs: Tensor, in_ptr_host: Tensor, in_ptr: Tensor, in_src: Tensor, in_log_w: Tensor, init: Tensor,
            lengths: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        nat.require_gpu(obs, in_ptr, in_src, in_log_w, init)
        obs, w, init = _f32c(obs.detach()), _f32c(in_log_w.detach()), _f32c(init.detach())
        B, T, N = obs.shape
        E = w.numel()
        dev = obs.device
        states, delta, final = outs = _sparse_viterbi_outputs(_on(dev), B, T, N)
        if B == 0:
            return outs
        lens = _dev_lengths(lengths, dev)
        L = nat.lib()
        _call(dev, L.hmm355_sparse_viterbi_f32, nat.ptr(obs), nat.ptr(in_ptr_host), nat.ptr(in_ptr), nat.ptr(in_src),
              nat.ptr(w), nat.ptr(init), nat.ptr(lens), B, T, N, E, nat.ptr(states), nat.ptr(delta), nat.ptr(final),
              ws=L.hmm355_sparse_viterbi_workspace_bytes(B, T, N, E))
        return outs

    @vit.register_fake
    def _(obs, in_ptr_host, in_ptr, in_src, in_log_w, init, lengths=None):
        return _sparse_viterbi_outputs(obs.new_empty, *obs.shape)

    @torch.library.custom_op("hmm355::sparse_forward_backward", mutates_args=())
    def fb(obs: Tensor, in_ptr_host: Tensor, in_ptr: Tensor, in_src: Tensor, in_log_w: Tensor,
           out_ptr_host: Tensor, out_ptr: Tensor, out_dst: Tensor, out_log_w: Tensor, log_p0: Tensor,
           want_posterior: bool, lengths: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
        nat.require_gpu(obs, in_ptr, in_src, in_log_w, out_ptr, out_dst, out_log_w, log_p0)
        obs, wi, wo, p0 = (_f32c(t.detach()) for t in (obs, in_log_w, out_log_w, log_p0))
        B, T, N = obs.shape
        E = wi.numel()
        dev = obs.device
        loglik, post, ws = outs = _sparse_fb_outputs(_on(dev), B, T, N, E, want_posterior)
        if B == 0:
            return outs
        lens = _dev_lengths(lengths, dev)
        L = nat.lib()
        _call(dev, L.hmm355_sparse_forward_backward_f32, nat.ptr(obs), nat.ptr(in_ptr_host), nat.ptr(in_ptr),
              nat.ptr(in_src), nat.ptr(wi), nat.ptr(out_ptr_host), nat.ptr(out_ptr), nat.ptr(out_dst), nat.ptr(wo),
              nat.ptr(p0), nat.ptr(lens), B, T, N, E, nat.ptr(loglik), _opt(post, want_posterior), ws=ws)
        return outs

    @fb.register_fake
    def _(obs, in_ptr_host, in_ptr, in_src, in_log_w, out_ptr_host, out_ptr, out_dst, out_log_w, log_p0,
          want_posterior, lengths=None):
        return _sparse_fb_outputs(obs.new_empty, *obs.shape, in_log_w.numel(), want_posterior)

    @torch.library.custom_op("hmm355::sparse_arc_counts", mutates_args=())
    def counts(obs: Tensor, src: Tensor, dst: Tensor, log_w: Tensor, workspace: Tensor,
               weight: Optional[Tensor] = None, lengths: Optional[Tensor] = None) -> Tensor:
        nat.require_gpu(obs, src, dst, log_w, workspace, weight)
        obs, w = _f32c(obs.detach()), _f32c(log_w.detach())
        g = None if weight is None else _f32c(weight.detach())
        B, T, N = obs.shape
        E = w.numel()
        dev = obs.device
        if B == 0:
            return torch.zeros(E, dtype=torch.float64, device=dev)
        xi = _sparse_counts_outputs(_on(dev), E)
        lens = _dev_lengths(lengths, dev)
        L = nat.lib()
        _call(dev, L.hmm355_sparse_arc_counts_f32, nat.ptr(obs), nat.ptr(src), nat.ptr(dst), nat.ptr(w), nat.ptr(g),
              nat.ptr(lens), B, T, N, E, nat.ptr(workspace), workspace.numel(), nat.ptr(xi),
              ws=L.hmm355_sparse_arc_counts_workspace_bytes(B, T, N, E))
        return xi

    @counts.register_fake
    def _(obs, src, dst, log_w, workspace, weight=None, lengths=None):
        return _sparse_counts_outputs(obs.new_empty, log_w.numel())


_sparse_ops()


def _sparse_check(obs, ptr_host, N_of, what):
    if obs.dim() != 3:
        raise ValueError(f"log_obs must be (B, T, N); got {tuple(obs.shape)}")
    N = obs.shape[2]
    if N < 1 or N > SPARSE_MAX_STATES:
        raise ValueError(f"{what} supports 1 to {SPARSE_MAX_STATES} states; got {N}")
    if ptr_host.numel() != N + 1 or N_of.numel() != N:
        raise ValueError(f"the transitions have {ptr_host.numel() - 1} states and the initial scores {N_of.numel()}; "
                         f"log_obs has {N}")


def sparse_viterbi(obs: Tensor, in_ptr_host: Tensor, in_ptr: Tensor, in_src: Tensor, in_log_w: Tensor,
                   init: Tensor, lengths=None) -> Tuple[Tensor, Tensor, Tensor]:
    """Viterbi over an arc list (torch.ops.hmm355.sparse_viterbi over hmm355_sparse_viterbi_f32,
    csrc/sparse.hip): obs (B,T,N) log-emissions, the arcs sorted by destination as
    sparse.SparseTransitions keeps them (in_ptr_host: CPU int32 (N+1); in_ptr, in_src, in_log_w on
    the device), init (N).  lengths: None or one length per sequence in any form ragged_lengths
    takes (no 256-state limit here).  Returns (states (B,T) int64, log_delta (B,T,N), final_score
    (B)), bit-identical to viterbi / viterbi_ragged on the dense matrix that is -inf off the arcs;
    padded frames get state -1 and log_delta -inf.  1 <= N <= 8192.  No gradients."""
    _sparse_check(obs, in_ptr_host, init, "sparse Viterbi")
    host = None if lengths is None else ragged_lengths(lengths, obs.shape[0], obs.shape[1])
    nat.require_gpu(obs, in_ptr, in_src, in_log_w, init)
    return torch.ops.hmm355.sparse_viterbi(obs, in_ptr_host, in_ptr, in_src, in_log_w, init, host)


def sparse_forward_backward(obs: Tensor, in_ptr_host: Tensor, in_ptr: Tensor, in_src: Tensor, in_log_w: Tensor,
                            out_ptr_host: Tensor, out_ptr: Tensor, out_dst: Tensor, out_log_w: Tensor,
                            log_p0: Tensor, want_posterior: bool = True,
                            lengths=None) -> Tuple[Tensor, Tensor, Tensor]:
    """The sums over an arc list (hmm355_sparse_forward_backward_f32): (loglik (B), posterior
    (B,T,N) or an empty tensor, workspace).  The workspace (a device byte tensor holding the scaled
    rows) is what sparse_arc_counts reads.  Padded frames have posterior 0; a sequence with no
    path gets loglik -inf and zeros.  Arguments as sparse_viterbi, with the arcs in both orders."""
    _sparse_check(obs, in_ptr_host, log_p0, "sparse forward-backward")
    host = None if lengths is None else ragged_lengths(lengths, obs.shape[0], obs.shape[1])
    nat.require_gpu(obs, in_ptr, in_src, in_log_w, out_ptr, out_dst, out_log_w, log_p0)
    return torch.ops.hmm355.sparse_forward_backward(obs, in_ptr_host, in_ptr, in_src, in_log_w, out_ptr_host,
                                                    out_ptr, out_dst, out_log_w, log_p0, bool(want_posterior), host)


def sparse_arc_counts(obs: Tensor, src: Tensor, dst: Tensor, log_w: Tensor, workspace: Tensor, weight=None,
                      lengths=None) -> Tensor:
    """xi (E) fp64, in the order of src / dst / log_w (int32, int32, fp32 on the device): the
    expected number of times each arc is taken, summed over the batch with the per-sequence
    `weight` (B) or 1 (hmm355_sparse_arc_counts_f32).  workspace: sparse_forward_backward's, from
    the same obs and lengths.  Two calls give the same bits."""
    host = None if lengths is None else ragged_lengths(lengths, obs.shape[0], obs.shape[1])
    nat.require_gpu(obs, src, dst, log_w, workspace)
    return torch.ops.hmm355.sparse_arc_counts(obs, src, dst, log_w, workspace, weight, host)


# ------------------------------------------------------------------- GMM emission
def _gmm_stats_outputs(mk, S, C, D):
    """(occ, sx, sxx)."""
    return mk((S, C), dtype=_F32), mk((S, C, D), dtype=_F32), mk((S, C, D), dtype=_F32)


@torch.library.custom_op("hmm355::gmm_diag_logprob", mutates_args=())
def gmm_diag_logprob(x: Tensor, means: Tensor, log_vars: Tensor, log_w: Tensor, mix_lse: int) -> Tensor:
    nat.require_gpu(x, means, log_vars, log_w)
    x, means, log_vars, log_w = _f32c(x), _f32c(means), _f32c(log_vars), _f32c(log_w)
    B, T, D = x.shape
    S, C, D2 = means.shape
    if D2 != D:
        raise ValueError(f"feature dim mismatch: x has {D}, means have {D2}")
    out = _scores_output(_on(x.device), B, T, S)
    if B * T == 0:
        return out
    L = nat.lib()
    _call(x.device, L.hmm355_gmm_diag_logprob_f32, nat.ptr(x), nat.ptr(means), nat.ptr(log_vars), nat.ptr(log_w),
          B, T, D, S, C, mix_lse, nat.ptr(out), ws=L.hmm355_gmm_workspace_bytes(B, T, D, S, C))
    return out


@gmm_diag_logprob.register_fake
def _(x, means, log_vars, log_w, mix_lse):
    return _scores_output(x.new_empty, x.shape[0], x.shape[1], means.shape[0])


@torch.library.custom_op("hmm355::gmm_stats", mutates_args=())
def gmm_stats(x: Tensor, weight: Tensor, means: Tensor, log_vars: Tensor, log_w: Tensor, mix_lse: int,
              lengths: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Occupancy-weighted sufficient statistics of the diagonal Gaussian (mixture) emissions
    (hmm355_gmm_stats_f32, csrc/emstats.hip; spelled out in include/hmm355.h): with r the component
    responsibilities of the scorer's model and w = weight * r,
        occ (S,C) = sum w,  sx (S,C,D) = sum w (x - mu),  sxx (S,C,D) = sum w (x - mu)^2
    over the frames t < lengths[b] of every sequence.  x (B,T,D), weight (B,T,S) of any sign (the
    E-step passes the state posteriors), means / log_vars (S,C,D), log_w (S,C), mix_lse as
    gmm_diag_logprob (0 needs C == 1: r = 1), lengths (B) or None.  Frames past a length are never
    read.  Bitwise reproducible; no (frames, S*C) temporary."""
    if x.dim() != 3 or weight.dim() != 3 or means.dim() != 3:
        raise ValueError(f"x, weight and means must be (B,T,D), (B,T,S) and (S,C,D); got {tuple(x.shape)}, "
                         f"{tuple(weight.shape)}, {tuple(means.shape)}")
    B, T, D = x.shape
    S, C, D2 = means.shape
    if D2 != D:
        raise ValueError(f"feature dim mismatch: x has {D}, means have {D2}")
    if tuple(weight.shape) != (B, T, S):
        raise ValueError(f"weight must be (B, T, S) = ({B}, {T}, {S}); got {tuple(weight.shape)}")
    if tuple(log_vars.shape) != (S, C, D) or tuple(log_w.shape) != (S, C):
        raise ValueError(f"log_vars must be ({S}, {C}, {D}) and log_w ({S}, {C}); got {tuple(log_vars.shape)}, "
                         f"{tuple(log_w.shape)}")
    if D > nat.GMM_STATS_MAX_DIM:
        raise ValueError(f"gmm_stats supports at most {nat.GMM_STATS_MAX_DIM} feature dims; got {D}")
    if C > 256 or S * C > 65536:
        raise ValueError(f"gmm_stats supports at most 256 components per state and 65536 in all; got S={S}, C={C}")
    if not mix_lse and C != 1:
        raise ValueError(f"mix_lse == 0 needs one component per state; got C={C}")
    host = None if lengths is None else ragged_lengths(lengths, B, T)
    nat.require_gpu(x, weight, means, log_vars, log_w)
    x, weight, means, log_vars, log_w = (_f32c(t.detach()) for t in (x, weight, means, log_vars, log_w))
    dev = x.device
    if B * T == 0:   # no frame: the sums are zero
        return _gmm_stats_outputs(functools.partial(torch.zeros, device=dev), S, C, D)
    occ, sx, sxx = outs = _gmm_stats_outputs(_on(dev), S, C, D)
    lens = None if host is None else host.to(torch.int32).to(dev)
    L = nat.lib()
    _call(dev, L.hmm355_gmm_stats_f32, nat.ptr(x), nat.ptr(weight), nat.ptr(means), nat.ptr(log_vars),
          nat.ptr(log_w), nat.ptr(lens), B, T, D, S, C, int(mix_lse), nat.ptr(occ), nat.ptr(sx), nat.ptr(sxx),
          ws=L.hmm355_gmm_stats_workspace_bytes(B, T, D, S, C))
    return outs


@gmm_stats.register_fake
def _(x, weight, means, log_vars, log_w, mix_lse, lengths=None):
    return _gmm_stats_outputs(x.new_empty, *means.shape)


# ------------------------------------------------------------------------------- HSMM
def _hsmm_viterbi_outputs(mk, B, T):
    """(states, scores)."""
    return mk((B, T), dtype=_I64), mk(B, dtype=_F32)


@torch.library.custom_op("hmm355::hsmm_viterbi", mutates_args=())
def hsmm_viterbi(lp: Tensor, dur_lp: Tensor, log_T: Tensor, flags: int = 0) -> Tuple[Tensor, Tensor]:
    """flags: kernel-form flags (FORM_GENERAL, FORM_SERIAL_WALK; identical results)."""
    nat.require_gpu(lp, dur_lp, log_T)
    lp, dur_lp, log_T = _f32c(lp), _f32c(dur_lp), _f32c(log_T)
    B, T, S = lp.shape
    Dm = dur_lp.shape[1]
    dev = lp.device
    states, scores = outs = _hsmm_viterbi_outputs(_on(dev), B, T)
    if B == 0:
        return outs
    L = nat.lib()
    # The general form (S or Dmax beyond the register-slot kernels) keeps a (B,T,S,Dmax+1) fp32
    # table: checked against the device's free memory up front, and decoded in batch slices
    # that fit when the whole batch does not (sequences are independent).
    wsb = lambda b_, t_, s_, d_: L.hmm355_hsmm_workspace_bytes_ex(b_, t_, s_, d_, flags)
    _call_slices(dev, L.hmm355_hsmm_viterbi_ex_f32, wsb, "HSMM decode", B, T, S, Dm, lambda sl, nb: (
        nat.ptr(lp[sl]), nat.ptr(dur_lp), nat.ptr(log_T), nb, T, S, Dm, flags, nat.ptr(states[sl]),
        nat.ptr(scores[sl])))
    return outs


_HSMM_WS_CHECK_BYTES = 1 << 30  # workspaces above this are checked against free device memory


def _ws_batch(ws_bytes, B, T, S, Dm, dev, what):
    """The batch slice whose workspace fits the device (general-form segment recursions keep a
    (B,T,S,Dmax) fp32 table): B when the whole batch's workspace is small or fits, else the
    largest slice that fits; OutOfMemoryError when not even one sequence does."""
    need = ws_bytes(B, T, S, Dm)
    if need <= _HSMM_WS_CHECK_BYTES:
        return B
    per_seq = ws_bytes(1, T, S, Dm)
    free, _ = torch.cuda.mem_get_info(dev)
    avail = free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if per_seq > 0.9 * avail:
        raise torch.cuda.OutOfMemoryError(
            f"{what} of one sequence (T={T}, S={S}, max_duration={Dm}) needs {per_seq / 2**30:.1f} GiB "
            f"of workspace (about T*S*max_duration*4 bytes), {avail / 2**30:.1f} GiB are available on {dev}")
    return max(1, min(B, int(0.9 * avail) // per_seq))


def _call_slices(dev, fn, ws_bytes, what, B, T, S, Dm, args, cap=None):
    """fn over the batch in slices whose workspace fits the device (_ws_batch; at most `cap`
    sequences each), all in one workspace.  args(sl, nb) gives the call's leading arguments for
    the nb sequences of the slice sl."""
    Bc = _ws_batch(ws_bytes, B, T, S, Dm, dev, what)
    if cap is not None:
        Bc = max(1, min(Bc, cap))
    ws = _workspace(ws_bytes(Bc, T, S, Dm), dev)
    for b0 in range(0, B, Bc):
        sl = slice(b0, min(b0 + Bc, B))
        _call(dev, fn, *args(sl, sl.stop - b0), ws=ws)


@hsmm_viterbi.register_fake
def _(lp, dur_lp, log_T, flags=0):
    return _hsmm_viterbi_outputs(lp.new_empty, lp.shape[0], lp.shape[1])


HSMM_FB_MAX_STATES = nat.HSMM_FB_MAX_STATES
HSMM_FB_MAX_DURATION = nat.HSMM_FB_MAX_DURATION
HSMM_FB_MAX_CELLS = nat.HSMM_FB_MAX_CELLS


def hsmm_fb_supported(S: int, Dm: int) -> bool:
    """The sizes hsmm_forward_backward takes (csrc/hsmm_fb.hip: a sequence's open segments live in
    64 KiB of LDS)."""
    return 1 <= S <= HSMM_FB_MAX_STATES and 1 <= Dm <= HSMM_FB_MAX_DURATION and S * Dm <= HSMM_FB_MAX_CELLS


def _hsmm_fb_outputs(mk, B, T, S, Dm, want_gamma, want_dur, want_trans, want_init):
    """(loglik, gamma, dur_counts, trans_counts, init_post)."""
    return (mk(B, dtype=_F32), mk((B, T, S) if want_gamma else _EMPTY, dtype=_F32),
            mk((B, S, Dm) if want_dur else _EMPTY, dtype=_F32), mk((B, S, S) if want_trans else _EMPTY, dtype=_F32),
            mk((B, S) if want_init else _EMPTY, dtype=_F32))


@torch.library.custom_op("hmm355::hsmm_forward_backward", mutates_args=())
def hsmm_forward_backward(lp: Tensor, dur_lp: Tensor, log_T: Tensor, log_init: Optional[Tensor] = None, *,
                          want_gamma: bool = False, want_dur: bool = False, want_trans: bool = False,
                          want_init: bool = False, flags: int = 0
                          ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The sum over the segmentations hsmm_viterbi maximises over (hmm355_hsmm_fb_f32,
    csrc/hsmm_fb.hip) -> (loglik (B), gamma (B,T,S), dur_counts (B,S,Dmax), trans_counts (B,S,S),
    init_post (B,S)); an output that is not wanted comes back as an empty (0,) tensor.  Each output
    is the derivative of loglik with respect to lp, dur_lp, log_T and log_init.  log_init None:
    all zeros, as in the decoder.  With no output wanted only the forward sum runs."""
    nat.require_gpu(lp, dur_lp, log_T, log_init)
    lp, dur_lp, log_T = _f32c(lp), _f32c(dur_lp), _f32c(log_T)
    if log_init is not None:
        log_init = _f32c(log_init)
    B, T, S = lp.shape
    Dm = dur_lp.shape[1]
    if dur_lp.shape[0] != S or tuple(log_T.shape) != (S, S) or (log_init is not None and log_init.shape != (S,)):
        raise ValueError(f"hsmm_forward_backward: lp {tuple(lp.shape)}, dur_lp {tuple(dur_lp.shape)}, log_T "
                         f"{tuple(log_T.shape)} and log_init do not agree on the number of states")
    dev = lp.device
    wants = (want_gamma, want_dur, want_trans, want_init)
    loglik, *counts = outs = _hsmm_fb_outputs(_on(dev), B, T, S, Dm, *wants)
    L = nat.lib()
    fl = (int(flags) | (nat.HSMM_FB_GAMMA if want_gamma else 0) | (nat.HSMM_FB_DUR if want_dur else 0) |
          (nat.HSMM_FB_TRANS if want_trans else 0) | (nat.HSMM_FB_INIT if want_init else 0))
    if B == 0 or T < 1 or not hsmm_fb_supported(S, Dm):
        # the native call names what is wrong with the shape (nothing is launched)
        nat.check(L.hmm355_hsmm_fb_f32(None, None, None, None, B, T, S, Dm, fl, None, None, None, None, None,
                                       None, 0, None))
        return outs
    wsb = lambda b_, t_, s_, d_: L.hmm355_hsmm_fb_workspace_bytes(b_, t_, s_, d_, fl)
    _call_slices(dev, L.hmm355_hsmm_fb_f32, wsb, "HSMM forward-backward", B, T, S, Dm, lambda sl, nb: (
        nat.ptr(lp[sl]), nat.ptr(dur_lp), nat.ptr(log_T), nat.ptr(log_init), nb, T, S, Dm, fl, nat.ptr(loglik[sl]),
        *[_opt(o[sl], want) for o, want in zip(counts, wants)]),
        cap=min(nat.HSMM_FB_MAX_BATCH, (1 << 31) // T))   # the native call's limits on B and B * T
    return outs


@hsmm_forward_backward.register_fake
def _(lp, dur_lp, log_T, log_init=None, *, want_gamma=False, want_dur=False, want_trans=False, want_init=False,
      flags=0):
    B, T, S = lp.shape
    return _hsmm_fb_outputs(lp.new_empty, B, T, S, dur_lp.shape[1], want_gamma, want_dur, want_trans, want_init)


# ------------------------------------------------- time-varying transitions (NeuralHMM)
def _tv_matrix(log_A: Tensor, B: int, T: int, N: int):
    """(tensor, batch stride, step stride) for the C ABI.  log_A is (N,N) (one matrix for all
    steps) or (B,T,N,N) with contiguous rows — an expand()ed static matrix keeps its zero
    strides, so it is never materialised (neural.py:385 expands one (N,N) over (B,T))."""
    if log_A.dtype != torch.float32:
        log_A = log_A.float()
    if log_A.dim() == 2:
        if tuple(log_A.shape) != (N, N):
            raise ValueError(f"transition matrix shape {tuple(log_A.shape)} != ({N}, {N})")
        return log_A.contiguous(), 0, 0
    if log_A.dim() != 4 or log_A.shape[0] != B or tuple(log_A.shape[2:]) != (N, N):
        raise ValueError(f"log transition tensor shape {tuple(log_A.shape)} != ({B}, {T}, {N}, {N})")
    if log_A.shape[1] < T - 1:  # steps 0..T-2 are read (neural.py:419-458)
        raise IndexError(f"log transition tensor has {log_A.shape[1]} steps, the recursion needs {T - 1}")
    if log_A.stride(3) != 1 or log_A.stride(2) != N or min(log_A.stride(0), log_A.stride(1)) < 0:
        log_A = log_A.contiguous()
    if log_A.stride(0) == 0 and log_A.stride(1) == 0:
        return log_A, 0, 0
    if log_A.stride(1) == 0 or log_A.stride(0) == 0:
        log_A = log_A.contiguous()
    return log_A, log_A.stride(0), log_A.stride(1)


@torch.library.custom_op("hmm355::tv_forward_backward", mutates_args=())
def tv_forward_backward(log_obs: Tensor, log_A: Tensor, log_p0: Tensor,
                        out_mask: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    nat.require_gpu(log_obs, log_A, log_p0)
    log_obs, log_p0 = _f32c(log_obs), _f32c(log_p0)
    B, T, N = log_obs.shape
    dev = log_obs.device
    L = nat.lib()
    outs = _fb_outputs(_on(dev), B, T, N, out_mask)
    if B == 0:
        return outs
    A, sb, st = _tv_matrix(log_A, B, T, N)
    _call(dev, L.hmm355_tv_forward_backward_f32, nat.ptr(log_obs), nat.ptr(A), sb, st, nat.ptr(log_p0), B, T, N,
          out_mask, *_fb_ptrs(outs, out_mask), ws=L.hmm355_tv_fb_workspace_bytes(B, T, N))
    return outs


@tv_forward_backward.register_fake
def _(log_obs, log_A, log_p0, out_mask):
    return _fb_outputs(log_obs.new_empty, *log_obs.shape, out_mask)


def _tv_viterbi_outputs(mk, B, T, N):
    """(states, log_delta)."""
    return mk((B, T), dtype=_I64), mk((B, T, N), dtype=_F32)


@torch.library.custom_op("hmm355::tv_viterbi", mutates_args=())
def tv_viterbi(log_obs: Tensor, log_A: Tensor, init: Tensor) -> Tuple[Tensor, Tensor]:
    nat.require_gpu(log_obs, log_A, init)
    log_obs, init = _f32c(log_obs), _f32c(init)
    B, T, N = log_obs.shape
    dev = log_obs.device
    states, delta = outs = _tv_viterbi_outputs(_on(dev), B, T, N)
    if B == 0:
        return outs
    A, sb, st = _tv_matrix(log_A, B, T, N)
    L = nat.lib()
    _call(dev, L.hmm355_tv_viterbi_f32, nat.ptr(log_obs), nat.ptr(A), sb, st, nat.ptr(init), B, T, N,
          nat.ptr(states), nat.ptr(delta), ws=L.hmm355_tv_viterbi_workspace_bytes(B, T, N))
    return outs


@tv_viterbi.register_fake
def _(log_obs, log_A, init):
    return _tv_viterbi_outputs(log_obs.new_empty, *log_obs.shape)


# ------------------------------------------------------- explicit-duration (semi-Markov)
@torch.library.custom_op("hmm355::semimarkov_quad", mutates_args=())
def semimarkov_quad(x: Tensor, means_t: Tensor, vars_t: Tensor) -> Tensor:
    """(B,T,Df) frames, (Df,S) means / variances -> (B,T,S) sum_k (x-mu)^2/var (k ascending)."""
    nat.require_gpu(x, means_t, vars_t)
    x, means_t, vars_t = _f32c(x), _f32c(means_t), _f32c(vars_t)
    B, T, Df = x.shape
    S = means_t.shape[1]
    if means_t.shape[0] != Df or tuple(vars_t.shape) != tuple(means_t.shape):
        raise ValueError(f"feature dim mismatch: x has {Df}, means {tuple(means_t.shape)}, "
                         f"variances {tuple(vars_t.shape)} (expected ({Df}, S))")
    q = _scores_output(_on(x.device), B, T, S)
    _call(x.device, nat.lib().hmm355_semimarkov_quad_f32, nat.ptr(x), nat.ptr(means_t), nat.ptr(vars_t), B, T, Df, S,
          nat.ptr(q))
    return q


@semimarkov_quad.register_fake
def _(x, means_t, vars_t):
    return _scores_output(x.new_empty, x.shape[0], x.shape[1], means_t.shape[1])


def _smk_args(quad, seg_const, log_init, log_T, dur_lp):
    nat.require_gpu(quad, seg_const, log_init, log_T, dur_lp)
    quad, log_init, log_T, dur_lp = _f32c(quad), _f32c(log_init), _f32c(log_T), _f32c(dur_lp)
    seg_const = None if seg_const is None else _f32c(seg_const)
    B, T, S = quad.shape
    if tuple(log_T.shape) != (S, S) or log_init.shape != (S,) or dur_lp.shape[0] != S:
        raise ValueError(f"parameter shapes {tuple(log_init.shape)}, {tuple(log_T.shape)}, "
                         f"{tuple(dur_lp.shape)} do not match {S} states")
    if seg_const is not None and seg_const.shape != (S,):
        raise ValueError(f"segment constant shape {tuple(seg_const.shape)} != ({S},)")
    return quad, seg_const, log_init, log_T, dur_lp, B, T, S, dur_lp.shape[1]


def _smk_viterbi_outputs(mk, B, T):
    """(seg_states, seg_durs, seg_count, scores); the op zeroes seg_count."""
    return mk((B, T), dtype=_I64), mk((B, T), dtype=_I64), mk(B, dtype=_I32), mk(B, dtype=_F32)


def _smk_forward_outputs(mk, B, T, S, Dm, want_alpha):
    """(log_prob, log_alpha)."""
    return mk(B, dtype=_F32), mk((B, T, S, Dm) if want_alpha else _EMPTY, dtype=_F32)


@torch.library.custom_op("hmm355::semimarkov_viterbi", mutates_args=())
def semimarkov_viterbi(quad: Tensor, seg_const: Optional[Tensor], log_init: Tensor, log_T: Tensor,
                       dur_lp: Tensor, flags: int = 0) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> seg_states (B,T) int64, seg_durs (B,T) int64 (right-aligned: the last seg_count[b] entries
    of row b; the entries in front of them are seg_states = -1, seg_durs = 0), seg_count (B) int32,
    scores (B).  flags: FORM_GENERAL forces the general form (identical results)."""
    quad, seg_const, log_init, log_T, dur_lp, B, T, S, Dm = _smk_args(quad, seg_const, log_init, log_T, dur_lp)
    dev = quad.device
    seg_s, seg_d, cnt, scores = outs = _smk_viterbi_outputs(_on(dev), B, T)
    cnt.zero_()
    if B == 0:
        return outs
    L = nat.lib()
    wsb = lambda b_, t_, s_, d_: L.hmm355_semimarkov_workspace_bytes_ex(b_, t_, s_, d_, flags)
    _call_slices(dev, L.hmm355_semimarkov_viterbi_ex_f32, wsb, "semi-Markov decode", B, T, S, Dm, lambda sl, nb: (
        nat.ptr(quad[sl]), nat.ptr(seg_const), nat.ptr(log_init), nat.ptr(log_T), nat.ptr(dur_lp), nb, T, S, Dm,
        flags, nat.ptr(seg_s[sl]), nat.ptr(seg_d[sl]), nat.ptr(cnt[sl]), nat.ptr(scores[sl])))
    return outs


@semimarkov_viterbi.register_fake
def _(quad, seg_const, log_init, log_T, dur_lp, flags=0):
    return _smk_viterbi_outputs(quad.new_empty, quad.shape[0], quad.shape[1])


@torch.library.custom_op("hmm355::semimarkov_forward", mutates_args=())
def semimarkov_forward(quad: Tensor, seg_const: Optional[Tensor], log_init: Tensor, log_T: Tensor,
                       dur_lp: Tensor, want_alpha: bool, flags: int = 0) -> Tuple[Tensor, Tensor]:
    """-> log_prob (B), log_alpha (B,T,S,Dmax) (empty (0,) unless want_alpha)."""
    quad, seg_const, log_init, log_T, dur_lp, B, T, S, Dm = _smk_args(quad, seg_const, log_init, log_T, dur_lp)
    dev = quad.device
    lp, alpha = outs = _smk_forward_outputs(_on(dev), B, T, S, Dm, want_alpha)
    if B == 0:
        return outs
    L = nat.lib()
    wsb = lambda b_, t_, s_, d_: L.hmm355_semimarkov_workspace_bytes_ex(b_, t_, s_, d_, flags)
    _call_slices(dev, L.hmm355_semimarkov_forward_ex_f32, wsb, "semi-Markov forward", B, T, S, Dm, lambda sl, nb: (
        nat.ptr(quad[sl]), nat.ptr(seg_const), nat.ptr(log_init), nat.ptr(log_T), nat.ptr(dur_lp), nb, T, S, Dm,
        flags, _opt(alpha[sl], want_alpha), nat.ptr(lp[sl])))
    return outs


@semimarkov_forward.register_fake
def _(quad, seg_const, log_init, log_T, dur_lp, want_alpha, flags=0):
    return _smk_forward_outputs(quad.new_empty, *quad.shape, dur_lp.shape[1], want_alpha)


# ------------------------------------------------------------------ streaming decoders
STREAM_SLOTS = 32   # hypothesis slots per stream (max beam width; 16 when N > 128)


def _stream_greedy_outputs(mk, B, T):
    """(states, step scores)."""
    return mk((B, T), dtype=_I64), mk((B, T), dtype=_F32)


@torch.library.custom_op("hmm355::stream_greedy", mutates_args=())
def stream_greedy(emis: Tensor, log_T: Tensor, prev_state: Tensor, log_n: float) -> Tuple[Tensor, Tensor]:
    """(B,T,N) emission log-probs -> greedy chain states (B,T) int64 and step scores (B,T).
    prev_state (B) int32: the stream's last decoded state, or -1 for its first chunk."""
    nat.require_gpu(emis, log_T, prev_state)
    emis, log_T = _f32c(emis), _f32c(log_T)
    prev_state = prev_state.to(torch.int32).contiguous()
    B, T, N = emis.shape
    states, scores = outs = _stream_greedy_outputs(_on(emis.device), B, T)
    _call(emis.device, nat.lib().hmm355_stream_greedy_f32, nat.ptr(emis), nat.ptr(log_T), nat.ptr(prev_state),
          float(log_n), B, T, N, nat.ptr(states), nat.ptr(scores))
    return outs


@stream_greedy.register_fake
def _(emis, log_T, prev_state, log_n):
    return _stream_greedy_outputs(emis.new_empty, emis.shape[0], emis.shape[1])


def stream_beam(emis: Tensor, log_T: Tensor, beam_width: int, hyp_score: Tensor, hyp_last: Tensor,
                hyp_count: Tensor, first: Tensor, live_max: int = STREAM_SLOTS):
    """One chunk of beam search for B streams.  hyp_score (B,32) fp32, hyp_last (B,32) int32
    and hyp_count (B) int32 are the streams' hypotheses (rank order, STREAM_SLOTS slots),
    updated IN PLACE; K = beam_width <= 32 (<= 16 when N > 128), N <= 256;
    first (B) int32 marks streams whose paths are still empty; live_max bounds hyp_count.  Returns (best-path states
    (B,T) int64, parent (B,T,K) int16, state (B,T,K) int16): new hypothesis r at step t came
    from hypothesis parent[t, r] of step t-1 and entered state[t, r]; at a step with fewer than K
    hypotheses (an under-full beam: min(K, live * N) of them) the other ranks get parent = state = -1."""
    nat.require_gpu(emis, log_T, hyp_score, hyp_last, hyp_count, first)
    emis, log_T = _f32c(emis), _f32c(log_T)
    B, T, N = emis.shape
    K = int(beam_width)
    for name, ten, dt in (("hyp_score", hyp_score, torch.float32), ("hyp_last", hyp_last, torch.int32),
                          ("hyp_count", hyp_count, torch.int32), ("first", first, torch.int32)):
        if ten.dtype != dt or not ten.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor")
    if tuple(hyp_score.shape) != (B, STREAM_SLOTS) or tuple(hyp_last.shape) != (B, STREAM_SLOTS):
        raise ValueError(f"hypothesis tensors must be ({B}, {STREAM_SLOTS})")
    dev = emis.device
    states = torch.empty((B, T), dtype=torch.int64, device=dev)
    parent = torch.empty((B, T, K), dtype=torch.int16, device=dev)
    hstate = torch.empty((B, T, K), dtype=torch.int16, device=dev)
    _call(dev, nat.lib().hmm355_stream_beam_f32, nat.ptr(emis), nat.ptr(log_T), B, T, N, K, int(live_max),
          nat.ptr(hyp_score), nat.ptr(hyp_last), nat.ptr(hyp_count), nat.ptr(first), nat.ptr(parent), nat.ptr(hstate),
          nat.ptr(states))
    return states, parent, hstate


# ------------------------------------------------------------------ dynamic time warping
DTW_SYMMETRIC = nat.DTW_SYMMETRIC
DTW_ASYMMETRIC = nat.DTW_ASYMMETRIC
DTW_RABINER_JUANG = nat.DTW_RABINER_JUANG
DTW_PATTERNS = {"symmetric": DTW_SYMMETRIC, "asymmetric": DTW_ASYMMETRIC, "rabiner_juang": DTW_RABINER_JUANG}


def dtw_pattern(step_pattern) -> int:
    """The HMM355_DTW_* constant of a reference step-pattern name (or of the constant itself)."""
    if isinstance(step_pattern, str):
        if step_pattern not in DTW_PATTERNS:
            raise ValueError(f"Unknown step pattern: {step_pattern}")
        return DTW_PATTERNS[step_pattern]
    return int(step_pattern)


def _dtw_lens(dist, n_len, m_len):
    nat.require_gpu(dist, n_len, m_len)
    if dist.dim() != 3:
        raise ValueError(f"dist must be (B, N, M); got {tuple(dist.shape)}")
    B = dist.shape[0]
    out = []
    for name, t in (("n_len", n_len), ("m_len", m_len)):
        if t is not None:
            if t.numel() != B:
                raise ValueError(f"{name} must hold one length per pair ({B}); got {tuple(t.shape)}")
            t = t.to(torch.int32).contiguous()
        out.append(t)
    return out


def _dtw_outputs(mk, B, N, M, want_cost, want_path):
    """(cost_matrix, total, path_i, path_j, path_len)."""
    path = (B, N + M - 1) if want_path else _EMPTY
    return (mk((B, N, M) if want_cost else _EMPTY, dtype=_F32), mk(B, dtype=_F32), mk(path, dtype=_I32),
            mk(path, dtype=_I32), mk(B if want_path else 0, dtype=_I32))


def _soft_dtw_outputs(mk, B, N, M):
    """(R, total)."""
    return mk((B, N + 1, M + 1), dtype=_F32), mk(B, dtype=_F32)


@torch.library.custom_op("hmm355::dtw", mutates_args=())
def dtw(dist: Tensor, pattern: int, n_len: Optional[Tensor] = None, m_len: Optional[Tensor] = None,
        want_cost: bool = True, want_path: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Hard DTW of B distance matrices (B,N,M) in one launch (hmm355_dtw_f32, csrc/dtw.hip).
    pattern: DTW_SYMMETRIC / DTW_ASYMMETRIC / DTW_RABINER_JUANG (dtw_pattern(name)).  n_len / m_len
    (B) restrict pair b to its top-left corner.  Returns (cost_matrix (B,N,M), +inf outside a
    pair's corner; total (B); path_i, path_j (B,N+M-1) int32, -1 past the end; path_len (B) int32);
    want_cost=False / want_path=False return empty tensors in their places (with both off no
    N x M table is written).  A band is +inf entries in dist."""
    n_len, m_len = _dtw_lens(dist, n_len, m_len)
    dist = _f32c(dist)
    B, N, M = dist.shape
    dev = dist.device
    if N < 1 or M < 1:
        raise ValueError(f"dist must have at least one row and one column; got {tuple(dist.shape)}")
    cost, total, path_i, path_j, path_len = outs = _dtw_outputs(_on(dev), B, N, M, want_cost, want_path)
    if B == 0:
        return outs
    L = nat.lib()
    flags = nat.DTW_PATH if want_path else 0
    _call(dev, L.hmm355_dtw_f32, nat.ptr(dist), nat.ptr(n_len), nat.ptr(m_len), B, N, M, int(pattern), flags,
          _opt(cost, want_cost), nat.ptr(total), _opt(path_i, want_path), _opt(path_j, want_path),
          _opt(path_len, want_path), ws=L.hmm355_dtw_workspace_bytes(B, N, M, flags))
    return outs


@dtw.register_fake
def _(dist, pattern, n_len=None, m_len=None, want_cost=True, want_path=True):
    return _dtw_outputs(dist.new_empty, *dist.shape, want_cost, want_path)


@torch.library.custom_op("hmm355::soft_dtw", mutates_args=())
def soft_dtw(dist: Tensor, gamma: float, n_len: Optional[Tensor] = None,
             m_len: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Soft-DTW of B distance matrices (hmm355_softdtw_f32): R (B,N+1,M+1) and total (B) = R[n,m].
    No gradient of its own: autograd.SoftDTW saves R and runs soft_dtw_grad."""
    n_len, m_len = _dtw_lens(dist, n_len, m_len)
    dist = _f32c(dist)
    B, N, M = dist.shape
    dev = dist.device
    if N < 1 or M < 1:
        raise ValueError(f"dist must have at least one row and one column; got {tuple(dist.shape)}")
    R, total = outs = _soft_dtw_outputs(_on(dev), B, N, M)
    _call(dev, nat.lib().hmm355_softdtw_f32, nat.ptr(dist), nat.ptr(n_len), nat.ptr(m_len), B, N, M, float(gamma),
          nat.ptr(R), nat.ptr(total))
    return outs


@soft_dtw.register_fake
def _(dist, gamma, n_len=None, m_len=None):
    return _soft_dtw_outputs(dist.new_empty, *dist.shape)


@torch.library.custom_op("hmm355::soft_dtw_grad", mutates_args=())
def soft_dtw_grad(dist: Tensor, R: Tensor, gamma: float, n_len: Optional[Tensor] = None,
                  m_len: Optional[Tensor] = None) -> Tensor:
    """E (B,N,M) = d total / d dist from dist and the R soft_dtw returned (hmm355_softdtw_grad_f32)."""
    n_len, m_len = _dtw_lens(dist, n_len, m_len)
    nat.require_gpu(R)
    dist, R = _f32c(dist), _f32c(R)
    B, N, M = dist.shape
    if tuple(R.shape) != (B, N + 1, M + 1):
        raise ValueError(f"R must be ({B}, {N + 1}, {M + 1}); got {tuple(R.shape)}")
    dev = dist.device
    E = _scores_output(_on(dev), B, N, M)
    _call(dev, nat.lib().hmm355_softdtw_grad_f32, nat.ptr(dist), nat.ptr(R), nat.ptr(n_len), nat.ptr(m_len), B, N, M,
          float(gamma), nat.ptr(E))
    return E


@soft_dtw_grad.register_fake
def _(dist, R, gamma, n_len=None, m_len=None):
    return _scores_output(dist.new_empty, *dist.shape)


# ------------------------------------------------------------------ CTC lattice
CTC_ALPHA = nat.CTC_ALPHA
CTC_BETA = nat.CTC_BETA
CTC_VITERBI = nat.CTC_VITERBI
CTC_MAX_TARGET = nat.CTC_MAX_TARGET


def _ctc_args(shape, dev, targets, input_lengths, target_lengths, blank):
    """Checks the arguments of a CTC call over log_probs of `shape` = (T,B,C) on the host
    (ValueError) and returns (int32 targets (B, max(Lmax, 1)), int32 input and target lengths, all
    on `dev`, blank, Lmax as the caller gave it): the layout the C ABI takes.  The lengths (B
    values each) are read on the host; that and the label check are the call's two
    synchronisations."""
    T, B, C = shape
    if T < 1 or B < 1 or C < 1:
        raise ValueError(f"log_probs needs at least one frame, sequence and class; got {tuple(shape)}")
    if targets.dim() != 2 or targets.shape[0] != B:
        raise ValueError(f"targets must be (B, Lmax) with B = {B}; got {tuple(targets.shape)}")
    if targets.dtype.is_floating_point or targets.dtype == torch.bool:
        raise ValueError(f"targets must hold integer labels; got {targets.dtype}")
    Lmax = targets.shape[1]
    if Lmax > CTC_MAX_TARGET:
        raise ValueError(f"targets longer than {CTC_MAX_TARGET} labels are not supported; got {Lmax}")
    blank = int(blank)
    if not 0 <= blank < C:
        raise ValueError(f"blank must lie in [0, {C}); got {blank}")
    il = _lengths(input_lengths, "input_lengths", B, 1, T, dev)[1]
    tl = _lengths(target_lengths, "target_lengths", B, 0, Lmax, dev)[1]
    tg = targets.detach().to(device=dev, dtype=torch.int32)
    if Lmax == 0:
        tg = torch.zeros((B, 1), dtype=torch.int32, device=dev)
    else:
        used = torch.arange(Lmax, device=dev)[None, :] < tl[:, None]
        if bool((((tg < 0) | (tg >= C)) & used).any()):
            raise ValueError(f"targets hold labels outside [0, {C})")
    return tg.contiguous(), il, tl, blank, Lmax


def _lattice_outputs(mk, B, T, S, alpha, beta, viterbi):
    """(loglik, alpha, beta, path, score) of a lattice of S positions: ctc's outputs and the first
    five of forced's."""
    return (mk(B, dtype=_F32), mk((B, T, S) if alpha else _EMPTY, dtype=_F32),
            mk((B, T, S) if beta else _EMPTY, dtype=_F32), mk((B, T) if viterbi else _EMPTY, dtype=_I32),
            mk(B if viterbi else 0, dtype=_F32))


@torch.library.custom_op("hmm355::ctc", mutates_args=())
def ctc(log_probs: Tensor, targets: Tensor, input_lengths: Tensor, target_lengths: Tensor, blank: int = 0,
        alpha: bool = False, beta: bool = False, viterbi: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The CTC lattice of B sequences in one launch (hmm355_ctc_f32, csrc/ctc.hip).  log_probs
    (T,B,C), targets (B,Lmax) integer labels, input_lengths / target_lengths (B) on any device.
    Returns (loglik (B); alpha (B,T,2 Lmax+1); beta (B,T,2 Lmax+1), the reference's convention
    without the frame's own emission; path (B,T) int32 expanded positions of the best single
    path, -1 past input_lengths[b] and for a pair with no alignment; score (B) of that path).
    alpha / beta / viterbi select what is computed beyond loglik; the others come back as empty
    tensors, and with none of them no (B,T,S') table is written.  Lengths outside
    [1, T] / [0, Lmax], labels outside [0, C) and a blank outside [0, C) raise ValueError (the
    reference would index row -1)."""
    nat.require_gpu(log_probs, targets)
    if log_probs.dim() != 3:
        raise ValueError(f"log_probs must be (T, B, C); got {tuple(log_probs.shape)}")
    dev = log_probs.device
    tg, il, tl, blank, Lmax = _ctc_args(log_probs.shape, dev, targets, input_lengths, target_lengths, blank)
    lp = _f32c(log_probs.detach())
    T, B, C = lp.shape
    Lk = tg.shape[1]
    loglik, A, Bt, path, score = _lattice_outputs(_on(dev), B, T, 2 * Lk + 1, alpha, beta, viterbi)
    flags = (CTC_ALPHA if alpha else 0) | (CTC_BETA if beta else 0) | (CTC_VITERBI if viterbi else 0)
    L = nat.lib()
    _call(dev, L.hmm355_ctc_f32, nat.ptr(lp), nat.ptr(tg), nat.ptr(il), nat.ptr(tl), T, B, C, Lk, blank, flags,
          _opt(A, alpha), _opt(Bt, beta), nat.ptr(loglik), _opt(path, viterbi), _opt(score, viterbi),
          ws=L.hmm355_ctc_workspace_bytes(B, T, Lk, flags))
    if Lk != Lmax:  # an empty targets matrix: the lattice is the single blank position
        if alpha:
            A = A[:, :, :1].contiguous()
        if beta:
            Bt = Bt[:, :, :1].contiguous()
    return loglik, A, Bt, path, score


@ctc.register_fake
def _(log_probs, targets, input_lengths, target_lengths, blank=0, alpha=False, beta=False, viterbi=False):
    T, B, _ = log_probs.shape
    return _lattice_outputs(log_probs.new_empty, B, T, 2 * targets.shape[1] + 1, alpha, beta, viterbi)


def _ctc_grad_outputs(mk, B, T, C, S, want_gamma):
    """(grad, gamma)."""
    return mk((T, B, C), dtype=_F32), mk((B, T, S) if want_gamma else _EMPTY, dtype=_F32)



@torch.library.custom_op("hmm355::ctc_grad", mutates_args=())
def ctc_grad(alpha: Tensor, beta: Tensor, loglik: Tensor, targets: Tensor, input_lengths: Tensor,
             target_lengths: Tensor, num_classes: int, blank: int = 0,
             want_gamma: bool = False) -> Tuple[Tensor, Tensor]:
    """(grad (T,B,C), gamma (B,T,S') or empty) from the alpha, beta and loglik of one ops.ctc call
    (hmm355_ctc_grad_f32): gamma = exp(alpha + beta - loglik) and grad[t,b,c] =
    d loglik[b] / d log_probs[t,b,c] = the sum of gamma over the positions of class c.  Zero in
    frames past input_lengths[b] and for a pair with no alignment; the same bits on every call."""
    nat.require_gpu(alpha, beta, loglik, targets)
    if alpha.dim() != 3 or alpha.shape != beta.shape:
        raise ValueError(f"alpha and beta must both be (B, T, S'); got {tuple(alpha.shape)} and {tuple(beta.shape)}")
    B, T, S = alpha.shape
    C = int(num_classes)
    if loglik.numel() != B:
        raise ValueError(f"loglik must hold one value per sequence ({B}); got {tuple(loglik.shape)}")
    if targets.dim() != 2 or S != 2 * targets.shape[1] + 1:
        raise ValueError(f"alpha has {S} positions; targets {tuple(targets.shape)} do not expand to that many")
    dev = alpha.device
    tg, il, tl, blank, Lmax = _ctc_args((T, B, C), dev, targets, input_lengths, target_lengths, blank)
    alpha, beta, loglik = _f32c(alpha), _f32c(beta), _f32c(loglik)
    Lk = tg.shape[1]
    if Lk != Lmax:  # an empty targets matrix: widen the single blank column to the kernel's Lmax = 1
        pad = alpha.new_full((B, T, 2), float("-inf"))
        alpha, beta = torch.cat([alpha, pad], 2).contiguous(), torch.cat([beta, pad], 2).contiguous()
    grad, gamma = _ctc_grad_outputs(_on(dev), B, T, C, 2 * Lk + 1, want_gamma)
    _call(dev, nat.lib().hmm355_ctc_grad_f32, nat.ptr(alpha), nat.ptr(beta), nat.ptr(loglik), nat.ptr(tg), nat.ptr(il),
          nat.ptr(tl), T, B, C, Lk, blank, _opt(gamma, want_gamma), nat.ptr(grad))
    if want_gamma and Lk != Lmax:
        gamma = gamma[:, :, :1].contiguous()
    return grad, gamma


@ctc_grad.register_fake
def _(alpha, beta, loglik, targets, input_lengths, target_lengths, num_classes, blank=0, want_gamma=False):
    B, T, S = alpha.shape
    return _ctc_grad_outputs(alpha.new_empty, B, T, num_classes, S, want_gamma)


# ------------------------------------------------------------------ transcript forced alignment
FORCED_ALPHA = nat.FORCED_ALPHA
FORCED_BETA = nat.FORCED_BETA
FORCED_VITERBI = nat.FORCED_VITERBI
FORCED_MAX_POSITIONS = nat.FORCED_MAX_POSITIONS


def _forced_args(shape, dev, state_ids, input_lengths, state_lengths, log_stay=None, log_next=None, log_skip=None):
    """Checks the arguments of a forced-alignment call over log_probs of `shape` = (B,T,C) on the
    host (ValueError) and returns (int32 state_ids (B,Smax) or None, int32 input and state lengths,
    the three fp32 weight tensors (B,Smax) or None, all on `dev`, Smax): the layout the C ABI
    takes.  Without state_ids the chain is the identity over the columns of log_probs (Smax = C,
    or the width of a weight tensor if one is given).  The lengths (B values each) are read on the
    host: the call's one synchronisation.  Ids are not checked: one outside [0, C) counts as an
    emission of -inf."""
    B, T, C = shape
    if T < 1 or B < 1 or C < 1:
        raise ValueError(f"log_probs needs at least one sequence, frame and class; got {tuple(shape)}")
    weights = (("log_stay", log_stay), ("log_next", log_next), ("log_skip", log_skip))
    if state_ids is not None:
        if state_ids.dim() != 2 or state_ids.shape[0] != B:
            raise ValueError(f"state_ids must be (B, Smax) with B = {B}; got {tuple(state_ids.shape)}")
        if state_ids.dtype.is_floating_point or state_ids.dtype == torch.bool:
            raise ValueError(f"state_ids must hold integer class ids; got {state_ids.dtype}")
        Smax = state_ids.shape[1]
    else:
        given = [w.shape[1] for _, w in weights if w is not None and w.dim() == 2]
        Smax = given[0] if given else C
        if Smax > C:
            raise ValueError(f"without state_ids the chain is the columns of log_probs: {Smax} positions need "
                             f"C >= {Smax}; got C = {C}")
    if Smax < 1 or Smax > FORCED_MAX_POSITIONS:
        raise ValueError(f"chains of 1 to {FORCED_MAX_POSITIONS} positions are supported; got {Smax}")
    il = _lengths(input_lengths, "input_lengths", B, 1, T, dev)[1]
    sl = _lengths(state_lengths, "state_lengths", B, 1, Smax, dev)[1]
    ws = []
    for name, w in weights:
        if w is not None:
            if tuple(w.shape) != (B, Smax):
                raise ValueError(f"{name} must be (B, Smax) = ({B}, {Smax}); got {tuple(w.shape)}")
            w = _f32c(w.detach().to(dev))
        ws.append(w)
    ids = None if state_ids is None else state_ids.detach().to(device=dev, dtype=torch.int32).contiguous()
    return ids, il, sl, ws[0], ws[1], ws[2], Smax


def _forced_outputs(mk, B, T, S, alpha, beta, viterbi):
    """(loglik, alpha, beta, path, score, durations)."""
    return (*_lattice_outputs(mk, B, T, S, alpha, beta, viterbi), mk((B, S) if viterbi else _EMPTY, dtype=_I32))


def _forced_grad_outputs(mk, B, T, C, S, want_gamma, want_grad, want_stay, want_next, want_skip):
    """(gamma, grad_log_probs, grad_stay, grad_next, grad_skip)."""
    return tuple(mk(shape if want else _EMPTY, dtype=_F32) for want, shape in (
        (want_gamma, (B, T, S)), (want_grad, (B, T, C)), (want_stay, (B, S)), (want_next, (B, S)), (want_skip, (B, S))))


@torch.library.custom_op("hmm355::forced", mutates_args=())
def forced(log_probs: Tensor, state_ids: Optional[Tensor], input_lengths: Tensor, state_lengths: Tensor,
           log_stay: Optional[Tensor] = None, log_next: Optional[Tensor] = None, log_skip: Optional[Tensor] = None,
           alpha: bool = False, beta: bool = False,
           viterbi: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The forced-alignment lattices of B utterances in one launch (hmm355_forced_f32,
    csrc/forced.hip; the recursion is spelled out in include/hmm355.h).  log_probs (B,T,C);
    state_ids (B,Smax) integer classes of the chain positions, or None for the identity chain
    (monotonic alignment search over log_probs (B,T,S)); input_lengths / state_lengths (B) on any
    device; log_stay / log_next / log_skip (B,Smax) per-position weights of s->s, s->s+1, s->s+2 or
    None (0, 0, -inf: no skips).  Returns (loglik (B); alpha (B,T,Smax); beta (B,T,Smax), its own
    frame's emission left out; path (B,T) int32 position of each frame on the best path, -1 past
    input_lengths[b] and for a pair with no path; score (B) of that path; durations (B,Smax) int32
    frames per position).  alpha / beta / viterbi select what is computed beyond loglik; the others
    come back as empty tensors.  Lengths outside [1, T] / [1, Smax] raise ValueError."""
    nat.require_gpu(log_probs, state_ids, log_stay, log_next, log_skip)
    if log_probs.dim() != 3:
        raise ValueError(f"log_probs must be (B, T, C); got {tuple(log_probs.shape)}")
    dev = log_probs.device
    ids, il, sl, ws, wn, wk, S = _forced_args(log_probs.shape, dev, state_ids, input_lengths, state_lengths,
                                              log_stay, log_next, log_skip)
    lp = _f32c(log_probs.detach())
    B, T, C = lp.shape
    loglik, A, Bt, path, score, dur = outs = _forced_outputs(_on(dev), B, T, S, alpha, beta, viterbi)
    flags = (FORCED_ALPHA if alpha else 0) | (FORCED_BETA if beta else 0) | (FORCED_VITERBI if viterbi else 0)
    L = nat.lib()
    _call(dev, L.hmm355_forced_f32, nat.ptr(lp), nat.ptr(ids), nat.ptr(il), nat.ptr(sl), nat.ptr(ws), nat.ptr(wn),
          nat.ptr(wk), B, T, C, S, flags, _opt(A, alpha), _opt(Bt, beta), nat.ptr(loglik), _opt(path, viterbi),
          _opt(score, viterbi), _opt(dur, viterbi), ws=L.hmm355_forced_workspace_bytes(B, T, S, flags))
    return outs


def _forced_width(log_probs, state_ids, log_stay, log_next, log_skip):
    if state_ids is not None:
        return state_ids.shape[1]
    given = [w.shape[1] for w in (log_stay, log_next, log_skip) if w is not None]
    return given[0] if given else log_probs.shape[2]


@forced.register_fake
def _(log_probs, state_ids, input_lengths, state_lengths, log_stay=None, log_next=None, log_skip=None, alpha=False,
      beta=False, viterbi=False):
    B, T, _ = log_probs.shape
    S = _forced_width(log_probs, state_ids, log_stay, log_next, log_skip)
    return _forced_outputs(log_probs.new_empty, B, T, S, alpha, beta, viterbi)


@torch.library.custom_op("hmm355::forced_grad", mutates_args=())
def forced_grad(alpha: Tensor, beta: Tensor, loglik: Tensor, log_probs: Tensor, state_ids: Optional[Tensor],
                input_lengths: Tensor, state_lengths: Tensor, log_stay: Optional[Tensor] = None,
                log_next: Optional[Tensor] = None, log_skip: Optional[Tensor] = None, want_gamma: bool = False,
                want_grad: bool = True, want_stay: bool = False, want_next: bool = False,
                want_skip: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(gamma (B,T,Smax), grad_log_probs (B,T,C), grad_stay, grad_next, grad_skip (B,Smax)) from the
    alpha, beta and loglik of one ops.forced call on the same inputs (hmm355_forced_grad_f32):
    gamma = exp(alpha + beta - loglik), grad_log_probs[b,t,c] = the sum of gamma over the positions
    of class c, and the expected number of times each stay / next / skip transition is taken.
    Outputs not asked for come back as empty tensors (at least one must be asked for).  Zero past
    either length and for a pair with no path; the same bits on every call.  Of log_probs only
    the shape is used (alpha already holds its emissions)."""
    nat.require_gpu(alpha, beta, loglik, log_probs, state_ids, log_stay, log_next, log_skip)
    if alpha.dim() != 3 or alpha.shape != beta.shape:
        raise ValueError(f"alpha and beta must both be (B, T, Smax); got {tuple(alpha.shape)} and {tuple(beta.shape)}")
    if log_probs.dim() != 3 or log_probs.shape[:2] != alpha.shape[:2]:
        raise ValueError(f"log_probs must be (B, T, C) over alpha's B, T; got {tuple(log_probs.shape)}")
    if not (want_gamma or want_grad or want_stay or want_next or want_skip):
        raise ValueError("forced_grad: no output asked for")
    B, T, S = alpha.shape
    C = log_probs.shape[2]
    if loglik.numel() != B:
        raise ValueError(f"loglik must hold one value per sequence ({B}); got {tuple(loglik.shape)}")
    dev = alpha.device
    ids, il, sl, ws, wn, wk, Sk = _forced_args((B, T, C), dev, state_ids, input_lengths, state_lengths,
                                               log_stay, log_next, log_skip)
    if Sk != S:
        raise ValueError(f"alpha has {S} positions; the chain arguments describe {Sk}")
    alpha, beta, loglik = _f32c(alpha), _f32c(beta), _f32c(loglik)
    wants = (want_gamma, want_grad, want_stay, want_next, want_skip)
    out = _forced_grad_outputs(_on(dev), B, T, C, S, *wants)
    L = nat.lib()
    args = (nat.ptr(alpha), nat.ptr(beta), nat.ptr(loglik), nat.ptr(ids), nat.ptr(il), nat.ptr(sl), nat.ptr(ws),
            nat.ptr(wn), nat.ptr(wk), B, T, C, S, *[_opt(o, w) for o, w in zip(out, wants)])
    if want_stay or want_next or want_skip:     # their per-tile sums live in a workspace
        _call(dev, L.hmm355_forced_grad_f32, *args, ws=L.hmm355_forced_workspace_bytes(B, T, S, nat.FORCED_GRAD))
    else:
        _call(dev, L.hmm355_forced_grad_f32, *args, None, 0)
    return out


@forced_grad.register_fake
def _(alpha, beta, loglik, log_probs, state_ids, input_lengths, state_lengths, log_stay=None, log_next=None,
      log_skip=None, want_gamma=False, want_grad=True, want_stay=False, want_next=False, want_skip=False):
    B, T, S = alpha.shape
    return _forced_grad_outputs(alpha.new_empty, B, T, log_probs.shape[2], S, want_gamma, want_grad, want_stay,
                                want_next, want_skip)


# ------------------------------------------------------------------ explicit-duration forced alignment
DURFORCED_MAX_POSITIONS = nat.DURFORCED_MAX_POSITIONS
DURFORCED_MAX_DURATION = nat.DURFORCED_MAX_DURATION
DURFORCED_MAX_CELLS = nat.DURFORCED_MAX_CELLS
_DURFORCED_TABLES = ("begin", "F", "Bend", "Bbeg")


def durforced_supported(Lmax: int, Dmax: int) -> bool:
    """The sizes durforced takes (csrc/durforced.hip: a sequence's open segments and its dur_lp
    live in one workgroup's LDS)."""
    return (1 <= Lmax <= DURFORCED_MAX_POSITIONS and 1 <= Dmax <= DURFORCED_MAX_DURATION and
            Lmax * Dmax <= DURFORCED_MAX_CELLS)


def _durforced_args(log_probs, dev, state_ids, input_lengths, state_lengths, dur_lp):
    """Checks the arguments of an explicit-duration forced-alignment call on the host, before any
    device call (ValueError; sizes beyond the kernel's limits raise the native library's error,
    which names them), and returns (int32 state_ids (B,Lmax) or None, int32 input and state
    lengths, fp32 dur_lp (B,Lmax,Dmax), all on `dev`, Lmax, Dmax): the layout the C ABI takes.
    The lengths (B values each) are read on the host: the call's one synchronisation.  Ids are
    not checked: one outside [0, C) counts as an emission of -inf."""
    if log_probs.dim() != 3:
        raise ValueError(f"log_probs must be (B, T, C); got {tuple(log_probs.shape)}")
    if not log_probs.dtype.is_floating_point:
        raise ValueError(f"log_probs must be a floating-point tensor; got {log_probs.dtype}")
    B, T, C = log_probs.shape
    if T < 1 or B < 1 or C < 1:
        raise ValueError(f"log_probs needs at least one sequence, frame and class; got {tuple(log_probs.shape)}")
    if dur_lp.dim() != 3 or dur_lp.shape[0] != B:
        raise ValueError(f"dur_lp must be (B, Lmax, Dmax) with B = {B}; got {tuple(dur_lp.shape)}")
    if not dur_lp.dtype.is_floating_point:
        raise ValueError(f"dur_lp must be a floating-point tensor; got {dur_lp.dtype}")
    Lmax, Dmax = dur_lp.shape[1], dur_lp.shape[2]
    if state_ids is not None:
        if state_ids.dim() != 2 or tuple(state_ids.shape) != (B, Lmax):
            raise ValueError(f"state_ids must be (B, Lmax) = ({B}, {Lmax}); got {tuple(state_ids.shape)}")
        if state_ids.dtype.is_floating_point or state_ids.dtype == torch.bool:
            raise ValueError(f"state_ids must hold integer class ids; got {state_ids.dtype}")
    elif Lmax > C:
        raise ValueError(f"without state_ids the chain is the columns of log_probs: {Lmax} positions need "
                         f"C >= {Lmax}; got C = {C}")
    if not durforced_supported(Lmax, Dmax):
        # the native call names what is wrong with the shape (nothing is launched)
        nat.check(nat.lib().hmm355_durforced_f32(None, None, None, None, None, B, T, C, Lmax, Dmax, 0, None, None,
                                                 None, None, None, None, None, None, None, None, None, 0, None))
        raise ValueError(f"dur_lp of {Lmax} positions x {Dmax} durations is outside the supported sizes")
    il = _lengths(input_lengths, "input_lengths", B, 1, T, dev, integers="last")[1]
    sl = _lengths(state_lengths, "state_lengths", B, 1, Lmax, dev, integers="last")[1]
    ids = None if state_ids is None else state_ids.detach().to(device=dev, dtype=torch.int32).contiguous()
    return ids, il, sl, _f32c(dur_lp.detach().to(dev)), Lmax, Dmax


def _durforced_outputs(mk, B, T, Lm, tables, viterbi):
    """(loglik, begin, F, Bend, Bbeg, frame_shift, loglik_shifted, path, score, durations)."""
    return (mk(B, dtype=_F32), *[mk((B, T, Lm) if tables else _EMPTY, dtype=_F32) for _ in _DURFORCED_TABLES],
            mk((B, T) if tables else _EMPTY, dtype=_F32), mk(B if tables else 0, dtype=_F32),
            mk((B, T) if viterbi else _EMPTY, dtype=_I32), mk(B if viterbi else 0, dtype=_F32),
            mk((B, Lm) if viterbi else _EMPTY, dtype=_I32))


def _durforced_grad_outputs(mk, B, T, C, Lm, Dm, want_gamma, want_grad, want_dur):
    """(gamma, grad_log_probs, grad_dur_lp)."""
    return tuple(mk(shape if want else _EMPTY, dtype=_F32) for want, shape in (
        (want_gamma, (B, T, Lm)), (want_grad, (B, T, C)), (want_dur, (B, Lm, Dm))))


@torch.library.custom_op("hmm355::durforced", mutates_args=())
def durforced(log_probs: Tensor, state_ids: Optional[Tensor], input_lengths: Tensor, state_lengths: Tensor,
              dur_lp: Tensor, *, tables: bool = False, viterbi: bool = False
              ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Explicit-duration forced alignment of B utterances in one launch (hmm355_durforced_f32,
    csrc/durforced.hip; the recursions are spelled out in include/hmm355.h).  log_probs (B,T,C);
    state_ids (B,Lmax) integer classes of the chain positions, or None for the identity chain over
    log_probs (B,T,Lmax); input_lengths / state_lengths (B) on any device; dur_lp (B,Lmax,Dmax),
    dur_lp[b,l,d-1] the score of position l lasting d frames (-inf forbids it).  Returns (loglik
    (B); begin, F, Bend, Bbeg (B,T,Lmax), frame_shift (B,T) and loglik_shifted (B): the tables
    ops.durforced_grad takes; path (B,T) int32 position of each frame on the best segmentation, -1
    past input_lengths[b] and for an infeasible pair; score (B); durations (B,Lmax) int32).
    tables / viterbi select what is computed beyond loglik; the others come back as empty
    tensors, and without tables no table is written.  Lengths outside [1, T] / [1, Lmax] raise
    ValueError."""
    nat.require_gpu(log_probs, state_ids, dur_lp)
    dev = log_probs.device
    ids, il, sl, du, Lm, Dm = _durforced_args(log_probs, dev, state_ids, input_lengths, state_lengths, dur_lp)
    lp = _f32c(log_probs.detach())
    B, T, C = lp.shape
    loglik, *tabs, path, score, dur = outs = _durforced_outputs(_on(dev), B, T, Lm, tables, viterbi)
    flags = (nat.DURFORCED_TABLES if tables else 0) | (nat.DURFORCED_VITERBI if viterbi else 0)
    L = nat.lib()
    _call(dev, L.hmm355_durforced_f32, nat.ptr(lp), nat.ptr(ids), nat.ptr(il), nat.ptr(sl), nat.ptr(du), B, T, C, Lm,
          Dm, flags, *[_opt(t, tables) for t in tabs], nat.ptr(loglik), _opt(path, viterbi), _opt(score, viterbi),
          _opt(dur, viterbi), ws=L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, flags))
    return outs


@durforced.register_fake
def _(log_probs, state_ids, input_lengths, state_lengths, dur_lp, *, tables=False, viterbi=False):
    B, T, _ = log_probs.shape
    return _durforced_outputs(log_probs.new_empty, B, T, dur_lp.shape[1], tables, viterbi)


@torch.library.custom_op("hmm355::durforced_grad", mutates_args=())
def durforced_grad(begin: Tensor, F: Tensor, Bend: Tensor, Bbeg: Tensor, frame_shift: Tensor, loglik_shifted: Tensor,
                   log_probs: Tensor, state_ids: Optional[Tensor], input_lengths: Tensor, state_lengths: Tensor,
                   dur_lp: Tensor, *, want_gamma: bool = False, want_grad: bool = True,
                   want_dur: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """(gamma (B,T,Lmax), grad_log_probs (B,T,C), grad_dur_lp (B,Lmax,Dmax)) from the tables of one
    ops.durforced(..., tables=True) call on the same inputs (hmm355_durforced_grad_f32): the
    posterior of position l at frame t, its sum over the positions of each class (d loglik /
    d log_probs) and the expected number of "position l lasts d frames" (d loglik / d dur_lp).
    Outputs not asked for come back as empty tensors (at least one must be asked for).  Zero past
    either length and for an infeasible pair; the same bits on every call."""
    nat.require_gpu(begin, F, Bend, Bbeg, frame_shift, loglik_shifted, log_probs, state_ids, dur_lp)
    if not (want_gamma or want_grad or want_dur):
        raise ValueError("durforced_grad: no output asked for")
    dev = log_probs.device
    ids, il, sl, du, Lm, Dm = _durforced_args(log_probs, dev, state_ids, input_lengths, state_lengths, dur_lp)
    B, T, C = log_probs.shape
    for name, t in zip(_DURFORCED_TABLES, (begin, F, Bend, Bbeg)):
        if tuple(t.shape) != (B, T, Lm):
            raise ValueError(f"{name} must be (B, T, Lmax) = ({B}, {T}, {Lm}); got {tuple(t.shape)}")
    if tuple(frame_shift.shape) != (B, T) or loglik_shifted.numel() != B:
        raise ValueError(f"frame_shift must be ({B}, {T}) and loglik_shifted hold {B} values; got "
                         f"{tuple(frame_shift.shape)} and {tuple(loglik_shifted.shape)}")
    lp = _f32c(log_probs.detach())
    tabs = [_f32c(t) for t in (begin, F, Bend, Bbeg, frame_shift, loglik_shifted)]
    wants = (want_gamma, want_grad, want_dur)
    out = _durforced_grad_outputs(_on(dev), B, T, C, Lm, Dm, *wants)
    L = nat.lib()
    args = (*[nat.ptr(t) for t in tabs], nat.ptr(lp), nat.ptr(ids), nat.ptr(il), nat.ptr(sl), nat.ptr(du), B, T, C,
            Lm, Dm, *[_opt(o, w) for o, w in zip(out, wants)])
    if want_dur or (want_grad and not want_gamma):
        _call(dev, L.hmm355_durforced_grad_f32, *args,
              ws=L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, nat.DURFORCED_GRAD))
    else:
        _call(dev, L.hmm355_durforced_grad_f32, *args, None, 0)
    return out


@durforced_grad.register_fake
def _(begin, F, Bend, Bbeg, frame_shift, loglik_shifted, log_probs, state_ids, input_lengths, state_lengths, dur_lp, *,
      want_gamma=False, want_grad=True, want_dur=False):
    B, T, C = log_probs.shape
    return _durforced_grad_outputs(log_probs.new_empty, B, T, C, dur_lp.shape[1], dur_lp.shape[2], want_gamma,
                                   want_grad, want_dur)


# ------------------------------------------------------------------ duration-constrained Viterbi
def _dchmm_outputs(mk, B, T, S, want_trellis):
    """(states, final_score, log_delta, durations)."""
    trellis = (B, T, S) if want_trellis else _EMPTY
    return mk((B, T), dtype=_I64), mk(B, dtype=_F32), mk(trellis, dtype=_F32), mk(trellis, dtype=_I32)


@torch.library.custom_op("hmm355::duration_constrained_viterbi", mutates_args=())
def duration_constrained_viterbi(emission_log_probs: Tensor, log_transitions: Tensor, min_duration: int,
                                 max_duration: int, penalty_weight: float = 0.1, per_sequence: bool = False,
                                 want_trellis: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """The duration-penalty Viterbi of DurationConstrainedHMM (hmm355_dchmm_viterbi_f32,
    csrc/dchmm.hip; the recursion is spelled out in include/hmm355.h).  emission_log_probs (B,T,S),
    log_transitions (S,S).  Returns (states (B,T) int64; final_score (B) = max_s delta[b,T-1,s];
    log_delta (B,T,S) fp32 and durations (B,T,S) int32, the whole trellis, or two empty tensors
    without want_trellis).  As in the reference the penalties of a step come from the largest and
    smallest run length over the whole batch, so the sequences of a batch are coupled and the
    batch runs in one workgroup: B * S <= 4096.  per_sequence=True gives every sequence its own
    penalties (the reference run on one sequence at a time), one workgroup each and any B.
    1 <= S <= 256.  Sizes outside the limits raise ValueError."""
    nat.require_gpu(emission_log_probs, log_transitions)
    if emission_log_probs.dim() != 3:
        raise ValueError(f"emission_log_probs must be (B, T, S); got {tuple(emission_log_probs.shape)}")
    B, T, S = emission_log_probs.shape
    if tuple(log_transitions.shape) != (S, S):
        raise ValueError(f"log_transitions must be ({S}, {S}); got {tuple(log_transitions.shape)}")
    if B < 1 or T < 1:
        raise ValueError(f"emission_log_probs needs B >= 1 and T >= 1; got {tuple(emission_log_probs.shape)}")
    if not 1 <= S <= nat.DCHMM_MAX_STATES:
        raise ValueError(f"duration_constrained_viterbi supports 1 <= S <= {nat.DCHMM_MAX_STATES} states; got {S}")
    group = 1 if per_sequence else B
    if group * S > nat.DCHMM_MAX_CELLS:
        raise ValueError(
            f"duration_constrained_viterbi couples the batch (the penalties of a step are taken over all B "
            f"sequences), which needs B * S <= {nat.DCHMM_MAX_CELLS}; got B = {B}, S = {S}.  per_sequence=True "
            "decodes each sequence with its own penalties at any B")
    dev = emission_log_probs.device
    e, lT = _f32c(emission_log_probs.detach()), _f32c(log_transitions.detach())
    states, score, delta, dur = outs = _dchmm_outputs(_on(dev), B, T, S, want_trellis)
    L = nat.lib()
    _call(dev, L.hmm355_dchmm_viterbi_f32, nat.ptr(e), nat.ptr(lT), B, T, S, group, int(min_duration),
          int(max_duration), float(penalty_weight), nat.ptr(states), nat.ptr(score), _opt(delta, want_trellis),
          _opt(dur, want_trellis), ws=L.hmm355_dchmm_workspace_bytes(B, T, S))
    return outs


@duration_constrained_viterbi.register_fake
def _(emission_log_probs, log_transitions, min_duration, max_duration, penalty_weight=0.1, per_sequence=False,
      want_trellis=False):
    return _dchmm_outputs(emission_log_probs.new_empty, *emission_log_probs.shape, want_trellis)


# ------------------------------------------------------------------ posterior path sampling
def _row_stride(x: Tensor) -> Optional[int]:
    """ld when the rows of x (B,T,N) are contiguous and row (b,t) starts (b*T + t) * ld floats into
    x with ld >= N (a [..., :N] view of a (B,T,NP) buffer, or a contiguous tensor), else None."""
    B, T, N = x.shape
    if N > 1 and x.stride(2) != 1:
        return None
    ld = x.stride(1) if T > 1 else (x.stride(0) if B > 1 else N)
    if ld < N or (T > 1 and B > 1 and x.stride(0) != T * ld):
        return None
    return ld


def _ffbs_output(mk, B, K, T):
    """states."""
    return mk((B, K, T), dtype=_I64)


@torch.library.custom_op("hmm355::ffbs", mutates_args=())
def ffbs(fwd: Tensor, log_P: Tensor, uniforms: Tensor, lengths: Optional[Tensor] = None) -> Tensor:
    """The backward-sampling pass of forward-filter backward-sample (hmm355_ffbs_f32,
    csrc/ffbs.hip; the draw is spelled out in include/hmm355.h).  fwd (B,T,N): rows proportional
    to alpha_t, non-negative, any positive scale -- the U rows autograd._run_fb returns are the
    intended input.  A strided view with a contiguous last dimension is read in place (its row
    stride is the C ABI's ld); anything else is copied.  log_P (N,N), uniforms (B,K,T) in [0, 1),
    lengths (B) or None.  Returns states (B,K,T) int64, -1 in frames >= lengths[b]; those frames'
    rows and uniforms are never read.  1 <= N <= 256."""
    if fwd.dim() != 3:
        raise ValueError(f"fwd must be (B, T, N); got {tuple(fwd.shape)}")
    B, T, N = fwd.shape
    if N > NARROW_MAX_STATES:
        raise ValueError(f"posterior path sampling supports at most {NARROW_MAX_STATES} states; got {N}")
    if tuple(log_P.shape) != (N, N):
        raise ValueError(f"log_P must be ({N}, {N}); got {tuple(log_P.shape)}")
    if uniforms.dim() != 3 or uniforms.shape[0] != B or uniforms.shape[2] != T or uniforms.shape[1] < 1:
        raise ValueError(f"uniforms must be (B, K, T) = ({B}, K >= 1, {T}); got {tuple(uniforms.shape)}")
    K = uniforms.shape[1]
    host = None if lengths is None else ragged_lengths(lengths, B, T, N)
    nat.require_gpu(fwd, log_P, uniforms)
    dev = fwd.device
    fwd = fwd.detach()
    if fwd.dtype != torch.float32:
        fwd = fwd.to(torch.float32)
    ld = _row_stride(fwd)
    if ld is None:
        fwd = fwd.contiguous()
        ld = N
    log_P, uniforms = _f32c(log_P.detach()), _f32c(uniforms.detach())
    states = _ffbs_output(_on(dev), B, K, T)
    if B == 0 or T == 0:
        return states
    lens = None if host is None else host.to(torch.int32).to(dev)
    L = nat.lib()
    _call(dev, L.hmm355_ffbs_f32, nat.ptr(fwd), int(ld), nat.ptr(log_P), nat.ptr(lens), nat.ptr(uniforms), B, T, N, K,
          nat.ptr(states), ws=L.hmm355_ffbs_workspace_bytes(N))
    return states


@ffbs.register_fake
def _(fwd, log_P, uniforms, lengths=None):
    return _ffbs_output(fwd.new_empty, fwd.shape[0], uniforms.shape[1], fwd.shape[1])


def posterior_sample(obs: Tensor, log_P: Tensor, log_p0: Tensor, obs_mode: int, num_samples: int, *,
                     uniforms: Optional[Tensor] = None, lengths=None, plan: Optional[Tensor] = None,
                     generator: Optional[torch.Generator] = None) -> Tuple[Tensor, Tensor]:
    """num_samples state paths per sequence drawn from p(z | x): (states (B,K,T) int64, loglik (B)).
    One forward-backward call that keeps its scaled forward rows U (the plan entry point without the
    FB_PAIR / FB_PLAN_BANDED hints, the ragged one when the lengths differ: autograd._run_fb),
    then ffbs on them.  uniforms (B,K,T) in [0, 1), or None to draw torch.rand with `generator`.
    Padded frames (t >= lengths[b]) get state -1.  No gradients: the inputs are detached."""
    from . import autograd
    if obs.dim() != 3:
        raise ValueError(f"obs must be (B, T, N); got {tuple(obs.shape)}")
    B, T, N = obs.shape
    K = int(num_samples)
    if K < 1:
        raise ValueError(f"num_samples must be at least 1; got {num_samples}")
    if N > NARROW_MAX_STATES:
        raise ValueError(f"posterior path sampling supports at most {NARROW_MAX_STATES} states; got {N}")
    if uniforms is not None and tuple(uniforms.shape) != (B, K, T):
        raise ValueError(f"uniforms must be (B, K, T) = ({B}, {K}, {T}); got {tuple(uniforms.shape)}")
    lens = active_lengths(lengths, B, T, N)
    nat.require_gpu(obs, log_P, log_p0, uniforms)
    dev = obs.device
    if uniforms is None:
        uniforms = torch.rand((B, K, T), device=dev, generator=generator)
    obs_c, lP, l0 = (_f32c(t.detach()) for t in (obs, log_P, log_p0))
    if B == 0:
        return torch.empty((0, K, T), dtype=torch.int64, device=dev), torch.empty(0, device=dev)
    _, loglik, _, U, *_ = autograd._run_fb(obs_c, lP, l0, obs_mode, plan=None if lens is not None else plan,
                                           lengths=lens)
    return ffbs(U, lP, uniforms, lens), loglik
