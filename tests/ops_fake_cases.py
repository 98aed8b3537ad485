"""Tiny inputs for every custom op of pytorch_hmm_amd.ops, shared by test_ops_fakes_cpu.py (fake
outputs against a literal table) and test_gpu_ops_fakes.py (fake outputs against the real ones).

A variant is an op, or "op/edge" for an edge form of its inputs.  SWITCHES[variant] names the
optional outputs of that variant; call(variant, fdtype, device, on) returns the (op, args, kwargs) of
one call with the switches in `on` switched on and every floating input of dtype `fdtype`.  Only
shapes, dtypes and lengths matter here: no test that uses these inputs looks at a value.
"""
import itertools

import torch

from pytorch_hmm_amd import ops

B, T, N, D, DMAX = 2, 5, 7, 3, 4
C_MIX = 2        # mixture components per state (gmm_*)
K = 3            # samples per sequence (ffbs)
L = 3            # labels / chain positions per sequence (ctc, forced, durforced)
M = 6            # columns of the DTW distance matrices (B, T, M)

_FB = ("post", "fwd", "bwd")
SWITCHES = {
    "forward_backward": _FB, "forward_backward_ragged": _FB, "tv_forward_backward": _FB,
    "viterbi": (), "viterbi_ragged": (), "tv_viterbi": (), "hsmm_viterbi": (),
    "gmm_diag_logprob": (), "gmm_stats": (), "semimarkov_quad": (), "semimarkov_viterbi": (),
    "stream_greedy": (), "soft_dtw": (), "soft_dtw_grad": (), "ffbs": (),
    "hsmm_forward_backward": ("want_gamma", "want_dur", "want_trans", "want_init"),
    "semimarkov_forward": ("want_alpha",),
    "dtw": ("want_cost", "want_path"),
    "ctc": ("alpha", "beta", "viterbi"), "ctc/Lmax0": ("alpha", "beta", "viterbi"),
    "ctc_grad": ("want_gamma",),
    "forced": ("alpha", "beta", "viterbi"), "forced/identity": ("alpha", "beta", "viterbi"),
    "forced/identity+weight": ("alpha", "beta", "viterbi"),
    "forced_grad": ("want_gamma", "want_grad", "want_stay", "want_next", "want_skip"),
    "durforced": ("tables", "viterbi"),
    "durforced_grad": ("want_gamma", "want_grad", "want_dur"),
    "duration_constrained_viterbi": ("want_trellis",),
}
# the real ops refuse a call that asks for no output at all (the fakes have no such check)
REFUSED = {("forced_grad", frozenset()), ("durforced_grad", frozenset())}
# the ops that take an empty batch
EMPTY_BATCH = ("forward_backward", "viterbi", "forward_backward_ragged", "viterbi_ragged", "hsmm_viterbi",
               "tv_forward_backward", "tv_viterbi", "semimarkov_viterbi", "semimarkov_forward", "dtw")


def combos(variant):
    """Every on/off combination of the variant's switches, as frozensets of the ones that are on."""
    names = SWITCHES[variant]
    return [frozenset(n for n, bit in zip(names, bits) if bit)
            for bits in itertools.product((False, True), repeat=len(names))]


def call(variant, fdtype, device, on=frozenset(), nb=B):
    """(op, args, kwargs) of one call of `variant` on a batch of `nb` sequences."""
    g = torch.Generator().manual_seed(0)
    f = lambda *shape: torch.rand(shape, generator=g).to(device=device, dtype=fdtype)
    logp = lambda *shape: torch.log_softmax(torch.rand(shape, generator=g), -1).to(device=device, dtype=fdtype)
    ints = lambda vals, dtype=torch.int64: torch.tensor(vals, dtype=dtype, device=device)
    full = lambda v, dtype=torch.int64: torch.full((nb,), v, dtype=dtype, device=device)
    sw = {name: name in on for name in SWITCHES[variant]}
    mask = sum(bit for name, bit in zip(_FB, (1, 2, 4)) if name in on)
    ragged = ints([T, T - 2][:nb])
    name = variant.split("/")[0]
    op = getattr(ops, name)

    if name == "forward_backward":
        return op, (f(nb, T, N), logp(N, N), logp(N), ops.OBS_PROB, mask), {}
    if name == "forward_backward_ragged":
        return op, (f(nb, T, N), logp(N, N), logp(N), ops.OBS_PROB, ragged, mask), {}
    if name == "tv_forward_backward":
        return op, (logp(nb, T, N), logp(N, N), logp(N), mask), {}
    if name == "viterbi":
        return op, (logp(nb, T, N), logp(N, N), logp(N), ops.OBS_LOG), {}
    if name == "viterbi_ragged":
        return op, (logp(nb, T, N), logp(N, N), logp(N), ops.OBS_LOG, ragged), {}
    if name == "tv_viterbi":
        return op, (logp(nb, T, N), logp(nb, T, N, N), logp(N)), {}
    if name == "gmm_diag_logprob":
        return op, (f(nb, T, D), f(N, C_MIX, D), f(N, C_MIX, D), logp(N, C_MIX), 1), {}
    if name == "gmm_stats":
        return op, (f(nb, T, D), f(nb, T, N), f(N, C_MIX, D), f(N, C_MIX, D), logp(N, C_MIX), 1, ragged), {}
    if name == "hsmm_viterbi":
        return op, (logp(nb, T, N), logp(N, DMAX), logp(N, N)), {}
    if name == "hsmm_forward_backward":
        return op, (logp(nb, T, N), logp(N, DMAX), logp(N, N), logp(N)), sw
    if name == "semimarkov_quad":
        return op, (f(nb, T, D), f(D, N), f(D, N) + 0.5), {}
    if name == "semimarkov_viterbi":
        return op, (f(nb, T, N), f(N), logp(N), logp(N, N), logp(N, DMAX)), {}
    if name == "semimarkov_forward":
        return op, (f(nb, T, N), None, logp(N), logp(N, N), logp(N, DMAX), sw["want_alpha"]), {}
    if name == "stream_greedy":
        return op, (logp(nb, T, N), logp(N, N), full(-1, torch.int32), 0.0), {}
    if name == "dtw":
        return op, (f(nb, T, M), ops.DTW_SYMMETRIC, None, full(M - 1, torch.int32)), sw
    if name == "soft_dtw":
        return op, (f(nb, T, M), 0.5), {}
    if name == "soft_dtw_grad":
        return op, (f(nb, T, M), f(nb, T + 1, M + 1), 0.5), {}
    if name == "ctc":
        if variant == "ctc/Lmax0":
            return op, (logp(T, nb, N), ints([[]] * nb), full(T), full(0)), sw
        return op, (logp(T, nb, N), ints([[1, 2, 3], [4, 4, 0]][:nb]), ragged, ints([L, L - 1][:nb])), sw
    if name == "ctc_grad":
        S = 2 * L + 1
        return op, (-f(nb, T, S), -f(nb, T, S), -f(nb), ints([[1, 2, 3], [4, 4, 0]][:nb]), ragged,
                    ints([L, L - 1][:nb]), N), sw
    if name == "forced":
        if variant == "forced/identity":
            return op, (logp(nb, T, N), None, ragged, full(T - 2)), sw
        if variant == "forced/identity+weight":
            return op, (logp(nb, T, N), None, ragged, full(DMAX - 1), None, -f(nb, DMAX)), sw
        return op, (logp(nb, T, N), ints([[1, 2, 3], [4, 4, 0]][:nb]), ragged, ints([L, L - 1][:nb]),
                    -f(nb, L), -f(nb, L), -f(nb, L)), sw
    if name == "forced_grad":
        return op, (-f(nb, T, L), -f(nb, T, L), -f(nb), logp(nb, T, N), ints([[1, 2, 3], [4, 4, 0]][:nb]), ragged,
                    ints([L, L - 1][:nb]), -f(nb, L), -f(nb, L), -f(nb, L)), sw
    if name == "durforced":
        return op, (logp(nb, T, N), ints([[1, 2, 3], [4, 4, 0]][:nb]), ragged, ints([L, L - 1][:nb]),
                    logp(nb, L, DMAX)), sw
    if name == "durforced_grad":
        return op, (-f(nb, T, L), -f(nb, T, L), -f(nb, T, L), -f(nb, T, L), f(nb, T), -f(nb), logp(nb, T, N),
                    ints([[1, 2, 3], [4, 4, 0]][:nb]), ragged, ints([L, L - 1][:nb]), logp(nb, L, DMAX)), sw
    if name == "duration_constrained_viterbi":
        return op, (logp(nb, T, N), logp(N, N), 1, DMAX), sw
    if name == "ffbs":
        return op, (f(nb, T, N), logp(N, N), f(nb, K, T), ragged), {}
    raise KeyError(variant)
