"""CPU: the CTC alignment feature without a device.

  * The numpy restatements in tests/ctc_numpy.py (the GPU tests' oracle on shapes without a
    fixture) reproduce every fixture the reference wrote (tests/golden/ctc_*.npz,
    make_golden_ctc.py): the -inf pattern of beta exactly, its finite entries and loglik within the
    fp32 step bound of the reference's own run, the fp64 tables to 1e-12; the occupancies sum to
    one per frame; the Viterbi path is a valid path whose score is its own sum.
  * The C ABI (include/hmm355.h, csrc/ctc.hip) declares and exports the CTC entry points, reports
    version >= 4 and rejects bad arguments with the documented codes before any launch.
  * pytorch_hmm_amd.alignment exports the reference's CTC names, imports without a GPU, refuses
    CPU tensors by name where a kernel would run, and its host-only functions reproduce the
    reference's outputs on CPU tensors.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_numpy as cn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")
EPS24 = 2.0 ** -24


def inputs(g):
    return g["lp"], g["targets"], g["input_lengths"], g["target_lengths"], int(g["blank"])


def steps_alpha(g):
    """(B,T,1): the recursion steps behind alpha[b,t,:]: t + 1"""
    B, T = g["alpha64"].shape[:2]
    return np.broadcast_to(np.arange(1, T + 1)[None, :, None], (B, T, 1))


def steps_beta(g):
    """(B,T,1): the recursion steps behind beta[b,t,:]: T_b - t (beta runs from T_b - 1 down)"""
    B, T = g["beta64"].shape[:2]
    return np.maximum(g["input_lengths"][:, None, None] - np.arange(T)[None, :, None], 1)


def within_step_bound(x, x64, steps):
    """|x - x64| <= 4 steps 2^-24 max(1, |x64|) on the finite entries; identical -inf pattern"""
    if not np.array_equal(np.isneginf(x), np.isneginf(x64)):
        return False
    fin = np.isfinite(x64)
    err = np.abs(np.where(fin, x.astype(np.float64) - np.where(fin, x64, 0), 0))
    return bool((err <= 4 * steps * EPS24 * np.maximum(1.0, np.abs(np.where(fin, x64, 0)))).all())


# ------------------------------------------------------------------------- restatements
@pytest.mark.parametrize("name", cn.FIXTURES)
def test_restatement_reproduces_fixture(gold, name):
    g = gold("ctc_" + name)
    args = inputs(g)
    A64, ll64 = cn.alpha(*args, dtype=np.float64)
    B64 = cn.beta(*args, dtype=np.float64)
    assert np.array_equal(np.isneginf(A64), np.isneginf(g["alpha64"]))
    assert np.array_equal(np.isneginf(B64), np.isneginf(g["beta64"]))
    for got, want in ((A64, g["alpha64"]), (B64, g["beta64"]), (ll64, g["loglik64"])):
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got))
        assert np.abs(got[fin] - want[fin]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want[fin]).max(initial=0.0))
    # the reference's own fp32 tables and the fp32 restatement against fp64: the step bound
    assert within_step_bound(g["ref_beta"], g["beta64"], steps_beta(g))
    assert within_step_bound(g["ref_loglik"], g["loglik64"], g["input_lengths"])
    A32, ll32 = cn.alpha(*args, dtype=np.float32)
    assert A32.dtype == np.float32
    assert within_step_bound(A32, g["alpha64"], steps_alpha(g))
    assert within_step_bound(cn.beta(*args, dtype=np.float32), g["beta64"], steps_beta(g))
    assert within_step_bound(ll32, g["loglik64"], g["input_lengths"])
    assert np.array_equal(cn.expand(g["targets"], args[4]), g["ref_expand"])


@pytest.mark.parametrize("name", cn.FIXTURES)
def test_occupancy_restatement(gold, name):
    g = gold("ctc_" + name)
    gamma, grad = cn.occupancy(*inputs(g))
    assert np.abs(gamma - g["gamma64"]).max() <= 1e-12 and np.abs(grad - g["grad64"]).max() <= 1e-12
    T = gamma.shape[1]
    for b in range(gamma.shape[0]):
        live = np.arange(T) < g["input_lengths"][b] if np.isfinite(g["loglik64"][b]) else np.zeros(T, bool)
        # every frame of a feasible pair is in exactly one position; nothing elsewhere
        assert np.abs(gamma[b].sum(1) - live).max() <= 1e-9
        assert np.abs(grad[:, b].sum(1) - live).max() <= 1e-9
        assert (grad[~live, b] == 0).all()


@pytest.mark.parametrize("name", cn.FIXTURES)
def test_viterbi_restatement_is_a_best_path(gold, name):
    g = gold("ctc_" + name)
    lp, targets, il, tl, blank = inputs(g)
    pos, score = cn.viterbi(lp, targets, il, tl, blank)
    ext = cn.expand(targets, blank)
    for b in range(len(il)):
        Tb, Sb = int(il[b]), 2 * int(tl[b]) + 1
        assert (pos[b, Tb:] == -1).all()
        if not np.isfinite(g["loglik64"][b]):
            assert np.isneginf(score[b]) and (pos[b] == -1).all()
            continue
        p = pos[b, :Tb]
        assert p[0] in (0, 1) and p[-1] in (Sb - 1, Sb - 2) and (np.diff(p) >= 0).all() and (np.diff(p) <= 2).all()
        for t in np.nonzero(np.diff(p) == 2)[0]:
            assert ext[b, p[t + 1]] != ext[b, p[t]]
        path_sum = lp[np.arange(Tb), b, ext[b, p]].astype(np.float64).sum()
        assert abs(path_sum - float(score[b])) <= Tb * EPS24 * max(1.0, abs(path_sum))
        # one path's probability is at most the sum over all of them, and for these small
        # lattices not far below it
        assert float(score[b]) <= g["loglik64"][b] + 1e-5 * abs(g["loglik64"][b])


def test_fixtures_hold_what_they_are_for(gold):
    assert np.isneginf(gold("ctc_infeasible")["ref_loglik"][0]) and np.isfinite(gold("ctc_infeasible")["ref_loglik"][1])
    assert (gold("ctc_empty")["target_lengths"] == 0).any()
    assert (gold("ctc_one_frame")["input_lengths"] == 1).sum() >= 2
    n = gold("ctc_neginf")
    assert np.isneginf(n["lp"][:, :, 2]).all() and np.isneginf(n["ref_loglik"][0]) and np.isfinite(n["ref_loglik"][1:]).all()
    assert int(gold("ctc_blank3")["blank"]) == 3
    bl = gold("ctc_blank_label")
    assert (bl["targets"] == int(bl["blank"])).any()
    b = gold("ctc_basic")
    assert b["lp"].shape == (12, 3, 5) and (b["targets"][:, 1:] == b["targets"][:, :-1]).any()
    assert len(set(b["input_lengths"])) == 3 and len(set(b["target_lengths"])) == 3
    lg = gold("ctc_long")
    assert lg["lp"].shape[0] == 200 and lg["targets"].shape[1] == 30
    for name in cn.FIXTURES:
        g = gold("ctc_" + name)
        # the reference's alignment: its alpha is never filled, so every frame is the blank
        for row, n in zip(g["ref_align"], g["input_lengths"]):
            assert (row[:n] == int(g["blank"])).all() and (row[n:] == -1).all()
        assert bool(g["ref_beam_equal"])


# ---------------------------------------------------------------------------------- ABI
@pytest.fixture(scope="module")
def L():
    from pytorch_hmm_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from pytorch_hmm_amd import build_native
        build_native.build()
    return nat.lib()


@pytest.fixture(scope="module")
def d():
    return dict((m.group(1), int(m.group(2).rstrip("u"), 0))
                for m in re.finditer(r"#define\s+(HMM355_[A-Z0-9_]+)\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+)u?)\)?",
                                     open(HEADER).read()))


FAKE = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
BIG = 1 << 40
CTC_SYMBOLS = ("hmm355_ctc_workspace_bytes", "hmm355_ctc_f32", "hmm355_ctc_grad_f32")


def fwd(L, lp=FAKE, targets=FAKE, il=FAKE, tl=FAKE, T=20, B=2, C=5, Lmax=4, blank=0, flags=7, alpha=FAKE, beta=FAKE,
        loglik=FAKE, path=FAKE, score=FAKE, wsp=FAKE, ws=BIG):
    return L.hmm355_ctc_f32(lp, targets, il, tl, T, B, C, Lmax, blank, flags, alpha, beta, loglik, path, score, wsp, ws,
                            None)


def grd(L, alpha=FAKE, beta=FAKE, loglik=FAKE, targets=FAKE, il=FAKE, tl=FAKE, T=20, B=2, C=5, Lmax=4, blank=0,
        gamma=None, grad=FAKE):
    return L.hmm355_ctc_grad_f32(alpha, beta, loglik, targets, il, tl, T, B, C, Lmax, blank, gamma, grad, None)


def test_header_exports_and_version(L, d):
    from pytorch_hmm_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hmm355_[a-z0-9_]+)\s*\(", src))
    for name in CTC_SYMBOLS:
        assert name in declared and name in nat.EXPORTS and hasattr(L, name)
    assert declared == set(nat.EXPORTS)
    assert L.hmm355_version() >= 4
    assert (d["HMM355_CTC_ALPHA"], d["HMM355_CTC_BETA"], d["HMM355_CTC_VITERBI"]) == \
        (nat.CTC_ALPHA, nat.CTC_BETA, nat.CTC_VITERBI) == (1, 2, 4)
    assert d["HMM355_CTC_MAX_TARGET"] == nat.CTC_MAX_TARGET == 2048
    src = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "ctc.hip")).read()
    threads = int(re.search(r"constexpr int kCtcThreads = (\d+);", src).group(1))
    wide = int(re.search(r"constexpr int kCtcPosWide = (\d+);", src).group(1))
    assert threads * wide >= 2 * nat.CTC_MAX_TARGET + 1     # the widest form covers the ABI's limit


@pytest.mark.parametrize("call", [fwd, grd])
def test_ctc_argument_checks(L, d, call):
    ARG, STATES, SHAPE = d["HMM355_E_ARG"], d["HMM355_E_STATES"], d["HMM355_E_SHAPE"]
    for dim in ("T", "B", "C"):
        assert call(L, **{dim: 0}) == ARG and call(L, **{dim: -3}) == ARG
    assert call(L, blank=-1) == ARG and call(L, blank=5) == ARG
    assert call(L, Lmax=0) == STATES and call(L, Lmax=2049) == STATES and call(L, Lmax=-1) == STATES
    for ptr in ("targets", "il", "tl", "loglik"):
        assert call(L, **{ptr: None}) == ARG
    assert call(L, T=1 << 30, B=1 << 30) == SHAPE


def test_forward_argument_checks(L, d):
    ARG = d["HMM355_E_ARG"]
    assert fwd(L, lp=None) == ARG
    assert fwd(L, flags=8) == ARG
    assert fwd(L, alpha=None) == ARG                       # each flag needs its output
    assert fwd(L, beta=None) == ARG and fwd(L, path=None) == ARG and fwd(L, score=None) == ARG
    assert fwd(L, wsp=None) == ARG and fwd(L, wsp=ctypes.c_void_p(0x1004)) == ARG
    need = L.hmm355_ctc_workspace_bytes(2, 20, 4, 7)
    assert fwd(L, ws=need - 1) == d["HMM355_E_WORKSPACE"]
    assert fwd(L, ws=16, flags=0) == d["HMM355_E_WORKSPACE"]


def test_gradient_argument_checks(L, d):
    for ptr in ("alpha", "beta", "grad"):
        assert grd(L, **{ptr: None}) == d["HMM355_E_ARG"]


def test_workspace_sizes(L):
    B, T, Lmax = 3, 100, 40
    value_only = L.hmm355_ctc_workspace_bytes(B, T, Lmax, 0)
    tables = L.hmm355_ctc_workspace_bytes(B, T, Lmax, 3)
    with_path = L.hmm355_ctc_workspace_bytes(B, T, Lmax, 7)
    assert 0 < value_only == tables < B * T           # alpha / beta are outputs; no table in the workspace
    assert with_path >= value_only + B * T * (2 * Lmax + 1) // 4    # 2 bits per cell
    assert value_only < with_path
    assert L.hmm355_ctc_workspace_bytes(B, T, 2048, 4) > 0
    for bad in ((0, T, Lmax, 0), (B, 0, Lmax, 0), (B, T, 0, 0), (B, T, 2049, 0), (-1, T, Lmax, 0), (B, T, Lmax, 8),
                (1 << 30, 1 << 30, Lmax, 4)):
        assert L.hmm355_ctc_workspace_bytes(*bad) == 0


# ------------------------------------------------------------------------------- Python
REFERENCE_NAMES = ("CTCAligner", "CTCSegmentationAligner", "ctc_alignment_path", "expand_targets_with_blank",
                   "ctc_forward_algorithm", "ctc_backward_algorithm", "remove_ctc_blanks", "collapse_repeated_tokens",
                   "ctc_decode_sequence")


def test_import_surface():
    import pytorch_hmm_amd
    from pytorch_hmm_amd.alignment import CTCAligner, ctc_forward_algorithm  # noqa: F401
    import pytorch_hmm_amd.alignment as al
    for name in REFERENCE_NAMES + ("ctc_forced_align",):
        assert hasattr(al, name) and name in al.__all__
    assert pytorch_hmm_amd.CTCAligner is al.CTCAligner
    assert pytorch_hmm_amd.CTCSegmentationAligner is al.CTCSegmentationAligner
    assert "CTC" in al.__doc__ and "out of scope" not in al.__doc__
    for op in ("ctc", "ctc_grad"):
        assert hasattr(torch.ops.hmm355, op)
    from pytorch_hmm_amd.autograd import CTCLogLik
    assert "log_softmax" in CTCLogLik.__doc__


def test_cpu_tensors_are_refused_by_name(gold):
    import pytorch_hmm_amd.alignment as al
    from pytorch_hmm_amd import ops
    from pytorch_hmm_amd.autograd import CTCLogLik
    g = gold("ctc_basic")
    lp, tg, il, tl = (torch.from_numpy(g[k]) for k in ("lp", "targets", "input_lengths", "target_lengths"))
    tab = torch.zeros(3, 12, 9)
    aligner = al.CTCAligner(5)
    for call in (lambda: al.ctc_forward_algorithm(lp, tg, il, tl), lambda: al.ctc_backward_algorithm(lp, tg, il, tl),
                 lambda: al.ctc_forward_algorithm(lp.clone().requires_grad_(), tg, il, tl),
                 lambda: al.ctc_alignment_path(lp, tg, il, tl, method="viterbi"),
                 lambda: al.ctc_alignment_path(lp, tg, il, tl, method="posterior"),
                 lambda: al.ctc_forced_align(lp, tg, il, tl), lambda: aligner.align(lp, tg, il, tl, method="viterbi"),
                 lambda: ops.ctc(lp, tg, il, tl), lambda: ops.ctc_grad(tab, tab, torch.zeros(3), tg, il, tl, 5),
                 lambda: CTCLogLik.apply(lp, tg, il, tl, 0)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()
    with pytest.raises(ValueError):
        al.ctc_alignment_path(lp, tg, il, tl, method="best")


def test_host_side_checks_raise_value_error():
    """_ctc_args runs before any launch; exercised directly, as a device is not needed for it."""
    from pytorch_hmm_amd import ops
    tg = torch.tensor([[1, 2, 1], [3, 0, 0]])
    ok = ((12, 2, 5), "cpu", tg, torch.tensor([12, 7]), torch.tensor([3, 1]), 0)
    t32, il, tl, blank, Lmax = ops._ctc_args(*ok)
    assert t32.dtype == il.dtype == tl.dtype == torch.int32 and (blank, Lmax) == (0, 3)

    def bad(**kw):
        a = dict(zip(("shape", "dev", "targets", "il", "tl", "blank"), ok))
        a.update(kw)
        with pytest.raises(ValueError):
            ops._ctc_args(a["shape"], a["dev"], a["targets"], a["il"], a["tl"], a["blank"])
    bad(il=torch.tensor([13, 7]))
    bad(il=torch.tensor([12, 0]))
    bad(tl=torch.tensor([4, 1]))
    bad(tl=torch.tensor([3, -1]))
    bad(il=torch.tensor([12]))
    bad(blank=5)
    bad(blank=-1)
    bad(targets=torch.tensor([[1, 2, 5], [3, 0, 0]]))       # a label outside [0, C) that is used
    bad(targets=torch.tensor([[1, 2, 1], [-1, 0, 0]]))
    bad(targets=tg.float())
    bad(targets=tg[:1])
    bad(targets=torch.zeros(2, 2049, dtype=torch.long))
    # an unused label past target_lengths[b] is never read and is not checked
    ops._ctc_args((12, 2, 5), "cpu", torch.tensor([[1, 2, 1], [3, 99, -7]]), torch.tensor([12, 7]), torch.tensor([3, 1]), 0)


# --------------------------------------------------------- host-only functions vs the reference
@pytest.mark.parametrize("name", cn.FIXTURES)
def test_host_functions_reproduce_the_reference(gold, name):
    import pytorch_hmm_amd.alignment as al
    g = gold("ctc_" + name)
    lp, tg, il, tl = (torch.from_numpy(g[k]) for k in ("lp", "targets", "input_lengths", "target_lengths"))
    blank = int(g["blank"])
    T, B, C = lp.shape
    ext = al.expand_targets_with_blank(tg, blank)
    assert ext.dtype == torch.int64 and np.array_equal(ext.numpy(), g["ref_expand"])
    # the reference's alignment (no kernel, so CPU tensors pass)
    aligner = al.CTCAligner(C, blank_id=blank)
    for paths in (al.ctc_alignment_path(lp, tg, il, tl, blank), aligner.align(lp, tg, il, tl)):
        assert len(paths) == B
        for b, p in enumerate(paths):
            assert p.dtype == torch.int64 and np.array_equal(p.numpy(), g["ref_align"][b, :il[b]])
    for decoded in (aligner.decode(lp, il), aligner.decode(lp, il, beam_width=4)):
        assert isinstance(decoded, list) and len(decoded) == B
        for b, seq in enumerate(decoded):
            n = int(g["ref_greedy_len"][b])
            assert seq.dim() == 1 and seq.numel() == n
            assert seq.dtype == (torch.int64 if n else torch.float32)
            assert np.array_equal(seq.numpy(), g["ref_greedy"][b, :n])
    seq = torch.from_numpy(g["seq"])
    for fn, key in ((al.collapse_repeated_tokens, "ref_collapse"), (lambda s: al.remove_ctc_blanks(s, blank), "ref_remove"),
                    (lambda s: al.ctc_decode_sequence(s, blank), "ref_decode")):
        out = fn(seq)
        assert out.dtype == torch.int64 and np.array_equal(out.numpy(), g[key])
    # nn.CTCLoss on the concatenated targets, as the reference's forward builds them
    for reduction in ("mean", "sum", "none"):
        want = torch.nn.CTCLoss(blank=blank, reduction=reduction, zero_infinity=True)(
            lp, torch.cat([tg[b, :tl[b]] for b in range(B)]), il, tl)
        assert torch.equal(al.CTCAligner(C, blank_id=blank, reduction=reduction)(lp, tg, il, tl), want)


def test_decode_utilities_edge_cases():
    import pytorch_hmm_amd.alignment as al
    empty = torch.tensor([], dtype=torch.int64)
    assert al.collapse_repeated_tokens(empty) is empty
    assert al.collapse_repeated_tokens(torch.tensor([2, 2, 2])).tolist() == [2]
    assert al.collapse_repeated_tokens(torch.tensor([1, 1, 0, 1, 3, 3], dtype=torch.int32)).dtype == torch.int64
    assert al.collapse_repeated_tokens(torch.tensor([1.0, 1.0, 2.0], dtype=torch.float64)).dtype == torch.float32
    assert al.ctc_decode_sequence(torch.tensor([0, 1, 1, 0, 1, 2, 2, 0])).tolist() == [1, 1, 2]
    # every frame blank: the reference's torch.tensor([]) -- float32, empty
    lp = torch.log_softmax(torch.tensor([[[5.0, 0.0, 0.0]], [[5.0, 0.0, 0.0]]]), dim=2)
    out = al.CTCAligner(3).decode(lp, torch.tensor([2]))
    assert out[0].dtype == torch.float32 and out[0].numel() == 0


def test_segmentation_reproduces_the_reference(gold):
    import pytorch_hmm_amd.alignment as al
    g = gold("ctc_segment")
    lp, transcript = torch.from_numpy(g["lp"]), torch.from_numpy(g["transcript"])
    seg = al.CTCSegmentationAligner(3, min_segment_length=50, max_segment_length=700)
    assert seg.blank_id == 0 and seg.num_classes == 3
    for tag, cuts in (("auto", None), ("given", torch.tensor([30, 90, 100, 2000]))):
        segs = seg.segment_and_align(lp, transcript, cuts)
        assert [s[2] for s in segs] == g[tag + "_start"].tolist() and [s[3] for s in segs] == g[tag + "_end"].tolist()
        assert [len(s[1]) for s in segs] == g[tag + "_text_len"].tolist()
        assert np.array_equal(torch.cat([s[1] for s in segs]).numpy(), g[tag + "_text"])
        for audio, _, s, e in segs:
            assert torch.equal(audio, lp[s:e])
