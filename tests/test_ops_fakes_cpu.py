"""The fake (shape-only) implementation of every custom op in pytorch_hmm_amd.ops reports the shapes
and dtypes the real op returns -- float32 / int64 / int32 whatever the dtype of the inputs (the real
ops convert fp64 / fp16 inputs and always allocate float32) -- and the ops' schemas are the recorded
ones.  Runs without a GPU; test_gpu_ops_fakes.py holds the fakes against the real outputs."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.utils._pytree import tree_map

from pytorch_hmm_amd import ops

import ops_fake_cases as cases

f32, i64, i32 = torch.float32, torch.int64, torch.int32

# variant -> one (switch, shape, dtype) per output: the output has `shape` when its switch is on (or is
# None), and is the empty (0,) tensor otherwise.  Sizes as in ops_fake_cases: B=2, T=5, N=7, D=3, Dmax=4,
# 2 mixture components, 3 samples, 3 labels / chain positions, DTW matrices (2, 5, 6).
_FB = [("post", (2, 5, 7), f32), ("fwd", (2, 5, 7), f32), ("bwd", (2, 5, 7), f32), (None, (2,), f32),
       (None, (2,), f32)]
_VIT = [(None, (2, 5), i64), (None, (2, 5, 7), f32), (None, (2,), f32)]
EXPECT = {
    "forward_backward": _FB,
    "forward_backward_ragged": _FB,
    "tv_forward_backward": _FB,
    "viterbi": _VIT,
    "viterbi_ragged": _VIT,
    "tv_viterbi": [(None, (2, 5), i64), (None, (2, 5, 7), f32)],
    "gmm_diag_logprob": [(None, (2, 5, 7), f32)],
    "gmm_stats": [(None, (7, 2), f32), (None, (7, 2, 3), f32), (None, (7, 2, 3), f32)],
    "hsmm_viterbi": [(None, (2, 5), i64), (None, (2,), f32)],
    "hsmm_forward_backward": [(None, (2,), f32), ("want_gamma", (2, 5, 7), f32), ("want_dur", (2, 7, 4), f32),
                              ("want_trans", (2, 7, 7), f32), ("want_init", (2, 7), f32)],
    "semimarkov_quad": [(None, (2, 5, 7), f32)],
    "semimarkov_viterbi": [(None, (2, 5), i64), (None, (2, 5), i64), (None, (2,), i32), (None, (2,), f32)],
    "semimarkov_forward": [(None, (2,), f32), ("want_alpha", (2, 5, 7, 4), f32)],
    "stream_greedy": [(None, (2, 5), i64), (None, (2, 5), f32)],
    "dtw": [("want_cost", (2, 5, 6), f32), (None, (2,), f32), ("want_path", (2, 10), i32),
            ("want_path", (2, 10), i32), ("want_path", (2,), i32)],
    "soft_dtw": [(None, (2, 6, 7), f32), (None, (2,), f32)],
    "soft_dtw_grad": [(None, (2, 5, 6), f32)],
    "ctc": [(None, (2,), f32), ("alpha", (2, 5, 7), f32), ("beta", (2, 5, 7), f32), ("viterbi", (2, 5), i32),
            ("viterbi", (2,), f32)],
    "ctc/Lmax0": [(None, (2,), f32), ("alpha", (2, 5, 1), f32), ("beta", (2, 5, 1), f32), ("viterbi", (2, 5), i32),
                  ("viterbi", (2,), f32)],
    "ctc_grad": [(None, (5, 2, 7), f32), ("want_gamma", (2, 5, 7), f32)],
    "forced": [(None, (2,), f32), ("alpha", (2, 5, 3), f32), ("beta", (2, 5, 3), f32), ("viterbi", (2, 5), i32),
               ("viterbi", (2,), f32), ("viterbi", (2, 3), i32)],
    "forced/identity": [(None, (2,), f32), ("alpha", (2, 5, 7), f32), ("beta", (2, 5, 7), f32),
                        ("viterbi", (2, 5), i32), ("viterbi", (2,), f32), ("viterbi", (2, 7), i32)],
    "forced/identity+weight": [(None, (2,), f32), ("alpha", (2, 5, 4), f32), ("beta", (2, 5, 4), f32),
                               ("viterbi", (2, 5), i32), ("viterbi", (2,), f32), ("viterbi", (2, 4), i32)],
    "forced_grad": [("want_gamma", (2, 5, 3), f32), ("want_grad", (2, 5, 7), f32), ("want_stay", (2, 3), f32),
                    ("want_next", (2, 3), f32), ("want_skip", (2, 3), f32)],
    "durforced": [(None, (2,), f32), ("tables", (2, 5, 3), f32), ("tables", (2, 5, 3), f32),
                  ("tables", (2, 5, 3), f32), ("tables", (2, 5, 3), f32), ("tables", (2, 5), f32),
                  ("tables", (2,), f32), ("viterbi", (2, 5), i32), ("viterbi", (2,), f32), ("viterbi", (2, 3), i32)],
    "durforced_grad": [("want_gamma", (2, 5, 3), f32), ("want_grad", (2, 5, 7), f32), ("want_dur", (2, 3, 4), f32)],
    "duration_constrained_viterbi": [(None, (2, 5), i64), (None, (2,), f32), ("want_trellis", (2, 5, 7), f32),
                                     ("want_trellis", (2, 5, 7), i32)],
    "ffbs": [(None, (2, 3, 5), i64)],
}

SCHEMAS = {
    "forward_backward": "hmm355::forward_backward(Tensor obs, Tensor log_P, Tensor log_p0, SymInt obs_mode, SymInt out_mask, Tensor? plan=None, bool? pair=None, bool? follow=None, bool? wide=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "viterbi": "hmm355::viterbi(Tensor obs, Tensor log_P, Tensor init, SymInt obs_mode, Tensor? plan=None, bool? follow=None, bool? wide=None) -> (Tensor, Tensor, Tensor)",
    "forward_backward_ragged": "hmm355::forward_backward_ragged(Tensor obs, Tensor log_P, Tensor log_p0, SymInt obs_mode, Tensor lengths, SymInt out_mask, Tensor? log_beta_T=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "viterbi_ragged": "hmm355::viterbi_ragged(Tensor obs, Tensor log_P, Tensor init, SymInt obs_mode, Tensor lengths) -> (Tensor, Tensor, Tensor)",
    "gmm_diag_logprob": "hmm355::gmm_diag_logprob(Tensor x, Tensor means, Tensor log_vars, Tensor log_w, SymInt mix_lse) -> Tensor",
    "gmm_stats": "hmm355::gmm_stats(Tensor x, Tensor weight, Tensor means, Tensor log_vars, Tensor log_w, SymInt mix_lse, Tensor? lengths=None) -> (Tensor, Tensor, Tensor)",
    "hsmm_viterbi": "hmm355::hsmm_viterbi(Tensor lp, Tensor dur_lp, Tensor log_T, SymInt flags=0) -> (Tensor, Tensor)",
    "hsmm_forward_backward": "hmm355::hsmm_forward_backward(Tensor lp, Tensor dur_lp, Tensor log_T, Tensor? log_init=None, *, bool want_gamma=False, bool want_dur=False, bool want_trans=False, bool want_init=False, SymInt flags=0) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "tv_forward_backward": "hmm355::tv_forward_backward(Tensor log_obs, Tensor log_A, Tensor log_p0, SymInt out_mask) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "tv_viterbi": "hmm355::tv_viterbi(Tensor log_obs, Tensor log_A, Tensor init) -> (Tensor, Tensor)",
    "semimarkov_quad": "hmm355::semimarkov_quad(Tensor x, Tensor means_t, Tensor vars_t) -> Tensor",
    "semimarkov_viterbi": "hmm355::semimarkov_viterbi(Tensor quad, Tensor? seg_const, Tensor log_init, Tensor log_T, Tensor dur_lp, SymInt flags=0) -> (Tensor, Tensor, Tensor, Tensor)",
    "semimarkov_forward": "hmm355::semimarkov_forward(Tensor quad, Tensor? seg_const, Tensor log_init, Tensor log_T, Tensor dur_lp, bool want_alpha, SymInt flags=0) -> (Tensor, Tensor)",
    "stream_greedy": "hmm355::stream_greedy(Tensor emis, Tensor log_T, Tensor prev_state, float log_n) -> (Tensor, Tensor)",
    "dtw": "hmm355::dtw(Tensor dist, SymInt pattern, Tensor? n_len=None, Tensor? m_len=None, bool want_cost=True, bool want_path=True) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "soft_dtw": "hmm355::soft_dtw(Tensor dist, float gamma, Tensor? n_len=None, Tensor? m_len=None) -> (Tensor, Tensor)",
    "soft_dtw_grad": "hmm355::soft_dtw_grad(Tensor dist, Tensor R, float gamma, Tensor? n_len=None, Tensor? m_len=None) -> Tensor",
    "ctc": "hmm355::ctc(Tensor log_probs, Tensor targets, Tensor input_lengths, Tensor target_lengths, SymInt blank=0, bool alpha=False, bool beta=False, bool viterbi=False) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "ctc_grad": "hmm355::ctc_grad(Tensor alpha, Tensor beta, Tensor loglik, Tensor targets, Tensor input_lengths, Tensor target_lengths, SymInt num_classes, SymInt blank=0, bool want_gamma=False) -> (Tensor, Tensor)",
    "forced": "hmm355::forced(Tensor log_probs, Tensor? state_ids, Tensor input_lengths, Tensor state_lengths, Tensor? log_stay=None, Tensor? log_next=None, Tensor? log_skip=None, bool alpha=False, bool beta=False, bool viterbi=False) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "forced_grad": "hmm355::forced_grad(Tensor alpha, Tensor beta, Tensor loglik, Tensor log_probs, Tensor? state_ids, Tensor input_lengths, Tensor state_lengths, Tensor? log_stay=None, Tensor? log_next=None, Tensor? log_skip=None, bool want_gamma=False, bool want_grad=True, bool want_stay=False, bool want_next=False, bool want_skip=False) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "durforced": "hmm355::durforced(Tensor log_probs, Tensor? state_ids, Tensor input_lengths, Tensor state_lengths, Tensor dur_lp, *, bool tables=False, bool viterbi=False) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "durforced_grad": "hmm355::durforced_grad(Tensor begin, Tensor F, Tensor Bend, Tensor Bbeg, Tensor frame_shift, Tensor loglik_shifted, Tensor log_probs, Tensor? state_ids, Tensor input_lengths, Tensor state_lengths, Tensor dur_lp, *, bool want_gamma=False, bool want_grad=True, bool want_dur=False) -> (Tensor, Tensor, Tensor)",
    "duration_constrained_viterbi": "hmm355::duration_constrained_viterbi(Tensor emission_log_probs, Tensor log_transitions, SymInt min_duration, SymInt max_duration, float penalty_weight=0.10000000000000001, bool per_sequence=False, bool want_trellis=False) -> (Tensor, Tensor, Tensor, Tensor)",
    "ffbs": "hmm355::ffbs(Tensor fwd, Tensor log_P, Tensor uniforms, Tensor? lengths=None) -> Tensor",
}


def custom_ops():
    """Every CustomOpDef the module defines, by its attribute name."""
    return {k: v for k, v in vars(ops).items() if isinstance(v, torch.library.CustomOpDef)}


def test_every_op_is_covered():
    names = set(custom_ops())
    assert names == set(SCHEMAS), "an op without a recorded schema (or a schema without an op)"
    assert names == {v.split("/")[0] for v in EXPECT}, "an op without an expectation row"
    assert set(EXPECT) == set(cases.SWITCHES)


@pytest.mark.parametrize("fdtype", [torch.float32, torch.float64, torch.float16], ids=["f32", "f64", "f16"])
@pytest.mark.parametrize("variant", sorted(EXPECT))
def test_fake_outputs(variant, fdtype):
    for on in cases.combos(variant):
        op, args, kwargs = cases.call(variant, fdtype, "cpu", on)
        with FakeTensorMode() as mode:
            fake = lambda a: mode.from_tensor(a) if isinstance(a, torch.Tensor) else a
            out = op(*tree_map(fake, args), **tree_map(fake, kwargs))
        out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
        got = [(tuple(o.shape), o.dtype) for o in out]
        want = [(shape if switch is None or switch in on else (0,), dtype) for switch, shape, dtype in EXPECT[variant]]
        assert got == want, f"{variant} with {sorted(on)} on"


@pytest.mark.parametrize("name", sorted(SCHEMAS))
def test_schema_is_the_recorded_one(name):
    assert str(custom_ops()[name]._opoverload._schema) == SCHEMAS[name]
