"""CPU: explicit-duration forced alignment without a GPU -- the numpy model
(tests/durforced_numpy.py) against enumeration of every segmentation, the C ABI's argument checks
(nothing is launched) and the host-side validation of ops.durforced and the alignment functions."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import durforced_numpy as M  # noqa: E402

HEADER = os.path.join(ROOT, "include", "hmm355.h")


# ------------------------------------------------------------------------------- the model
def tiny(seed, B=4, T=9, L=4, D=4, C=3, integer=False):
    """A ragged batch with repeated classes (C < L); the last pair has more positions than frames"""
    rng = np.random.default_rng(seed)
    if integer:
        lp = rng.integers(-2, 1, (B, T, C)).astype(np.float32)
        du = rng.integers(-1, 1, (B, L, D)).astype(np.float32)
    else:
        lp = rng.normal(-3, 2, (B, T, C)).astype(np.float32)
        du = np.log(rng.random((B, L, D)) + 1e-2).astype(np.float32)
    ids = rng.integers(0, C, (B, L)).astype(np.int32)
    il = np.array([9, 7, 5, 2][:B], np.int32)
    sl = np.array([4, 3, 2, 3][:B], np.int32)
    return lp, ids, il, sl, du


def against_brute_force(case, exact=False):
    lp, ids, il, sl, du = case
    ref = M.model(*case)
    for b in range(len(il)):
        Tb, Lb = int(il[b]), int(sl[b])
        bf = M.brute_force(lp[b], None if ids is None else ids[b], Tb, Lb, du[b])
        if bf["durations"] is None:
            assert ref["loglik"][b] == -np.inf and ref["score"][b] == -np.inf
            assert not ref["gamma"][b].any() and not ref["dur_post"][b].any() and not ref["grad_lp"][b].any()
            assert np.all(ref["path"][b] == -1) and not ref["durations"][b].any()
            continue
        assert abs(ref["loglik"][b] - bf["loglik"]) < 1e-10
        assert np.abs(ref["gamma"][b, :Tb, :Lb] - bf["gamma"]).max() < 1e-10
        assert np.abs(ref["dur_post"][b, :Lb] - bf["dur_post"]).max() < 1e-10
        assert not ref["gamma"][b, Tb:].any() and not ref["gamma"][b, :, Lb:].any() and not ref["dur_post"][b, Lb:].any()
        assert np.abs(ref["gamma"][b, :Tb, :Lb].sum(1) - 1).max() < 1e-10
        assert np.abs(ref["dur_post"][b, :Lb].sum(1) - 1).max() < 1e-10
        assert abs(ref["score"][b] - bf["score"]) < 1e-10
        d = ref["durations"][b]
        assert d[:Lb].sum() == Tb and not d[Lb:].any()
        assert np.array_equal(ref["path"][b, :Tb], np.repeat(np.arange(Lb), d[:Lb])) and np.all(ref["path"][b, Tb:] == -1)
        assert abs(M.rescore(lp[b], None if ids is None else ids[b], du[b], d, Tb, Lb) - bf["score"]) < 1e-10
        if exact:
            assert ref["score"][b] == bf["score"] and np.array_equal(d[:Lb], bf["durations"])
        # the emission gradient: gamma summed over the positions of each class
        want = np.zeros_like(ref["grad_lp"][b])
        for q in range(Lb):
            c = q if ids is None else int(ids[b, q])
            if 0 <= c < lp.shape[2]:
                want[:Tb, c] += bf["gamma"][:, q]
        assert np.abs(ref["grad_lp"][b] - want).max() < 1e-10
    return ref


@pytest.mark.parametrize("seed", range(4))
def test_model_matches_enumeration(seed):
    ref = against_brute_force(tiny(seed))
    assert np.isfinite(ref["loglik"][:3]).all() and ref["loglik"][3] == -np.inf   # T_b < L_b


def test_model_with_forbidden_durations_and_emissions():
    lp, ids, il, sl, du = tiny(7)
    du[:, :, 0] = -np.inf                      # a minimum duration of two frames
    du[1, 1, :] = -np.inf                      # a position with no duration at all
    lp[0, 3, :2] = -np.inf
    lp[2, 0, :] = -np.inf                      # no position can take frame 0
    ids[0, 2] = 17                             # a class outside [0, C)
    il[3], sl[3] = 9, 2                        # T_b > L_b Dmax
    ref = against_brute_force((lp, ids, il, sl, du))
    assert (ref["loglik"] == -np.inf).all()
    lp, ids, il, sl, du = tiny(10)             # feasible pairs with both kinds of -inf
    du[:, :, 0] = -np.inf
    lp[0, 3, 0] = lp[1, 2, 1] = -np.inf
    ref = against_brute_force((lp, ids, il, sl, du))
    assert np.isfinite(ref["loglik"][:3]).all()


def test_model_identity_chain_and_single_cells():
    lp, _, il, sl, du = tiny(9, C=4)
    against_brute_force((lp, None, il, sl, du))
    one = (lp[:1, :1], np.zeros((1, 1), np.int32), np.array([1], np.int32), np.array([1], np.int32), du[:1, :1, :1])
    ref = against_brute_force(one)
    assert ref["durations"][0, 0] == 1 and ref["gamma"][0, 0, 0] == 1.0


@pytest.mark.parametrize("seed", range(6))
def test_model_tie_rule_on_integer_scores(seed):
    """Integer scores tie often; of equal segmentations the smallest d_{L-1} wins, then d_{L-2}, ..."""
    against_brute_force(tiny(20 + seed, integer=True), exact=True)


def test_model_tie_rule_flat():
    lp = np.zeros((1, 7, 1), np.float32)
    du = np.zeros((1, 3, 4), np.float32)
    ref = M.model(lp, np.zeros((1, 3), np.int32), [7], [3], du)
    assert ref["durations"][0].tolist() == [4, 2, 1] and ref["path"][0].tolist() == [0, 0, 0, 0, 1, 1, 2]


def test_float32_model_is_close():
    case = tiny(3)
    a, b = M.model(*case), M.model(*case, dtype=np.float32)
    for k in ("loglik", "gamma", "dur_post", "grad_lp"):
        fin = np.isfinite(a[k])
        assert np.array_equal(fin, np.isfinite(b[k])) and np.abs(a[k][fin] - b[k][fin]).max() < 1e-4, k


# ------------------------------------------------------------------------------- C ABI
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
SYMBOLS = ("hmm355_durforced_workspace_bytes", "hmm355_durforced_f32", "hmm355_durforced_grad_f32")


def fwd(L, lp=FAKE, ids=FAKE, il=FAKE, sl=FAKE, du=FAKE, B=2, T=20, C=5, Lmax=4, Dmax=6, flags=3, begin=FAKE, F=FAKE,
        Bend=FAKE, Bbeg=FAKE, shift=FAKE, lls=FAKE, loglik=FAKE, path=FAKE, score=FAKE, dur=FAKE, wsp=FAKE,
        nbytes=BIG):
    return L.hmm355_durforced_f32(lp, ids, il, sl, du, B, T, C, Lmax, Dmax, flags, begin, F, Bend, Bbeg, shift, lls,
                                  loglik, path, score, dur, wsp, nbytes, None)


def grd(L, begin=FAKE, F=FAKE, Bend=FAKE, Bbeg=FAKE, shift=FAKE, lls=FAKE, lp=FAKE, ids=FAKE, il=FAKE, sl=FAKE,
        du=FAKE, B=2, T=20, C=5, Lmax=4, Dmax=6, gamma=None, grad=FAKE, gdur=FAKE, wsp=FAKE, nbytes=BIG):
    return L.hmm355_durforced_grad_f32(begin, F, Bend, Bbeg, shift, lls, lp, ids, il, sl, du, B, T, C, Lmax, Dmax,
                                       gamma, grad, gdur, wsp, nbytes, None)


def test_header_exports_and_version(L, d):
    from pytorch_hmm_amd import _native as nat
    from pytorch_hmm_amd import build_native, ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hmm355_[a-z0-9_]+)\s*\(", src))
    for name in SYMBOLS:
        assert name in declared and name in nat.EXPORTS and hasattr(L, name)
    assert declared == set(nat.EXPORTS)
    assert L.hmm355_version() >= 9
    assert (d["HMM355_DURFORCED_TABLES"], d["HMM355_DURFORCED_VITERBI"], d["HMM355_DURFORCED_GRAD"]) == \
        (nat.DURFORCED_TABLES, nat.DURFORCED_VITERBI, nat.DURFORCED_GRAD) == (1, 2, 4)
    assert d["HMM355_DURFORCED_MAX_POSITIONS"] == nat.DURFORCED_MAX_POSITIONS == ops.DURFORCED_MAX_POSITIONS >= 1024
    assert d["HMM355_DURFORCED_MAX_DURATION"] == nat.DURFORCED_MAX_DURATION == ops.DURFORCED_MAX_DURATION >= 128
    assert d["HMM355_DURFORCED_MAX_CELLS"] == nat.DURFORCED_MAX_CELLS == ops.DURFORCED_MAX_CELLS >= 16384
    assert "durforced.hip" in build_native.SOURCES
    assert "explicit-duration" in L.hmm355_strerror(d["HMM355_E_STATES"]).decode()


@pytest.mark.parametrize("call", [fwd, grd])
def test_argument_checks(L, d, call):
    ARG, STATES, SHAPE = d["HMM355_E_ARG"], d["HMM355_E_STATES"], d["HMM355_E_SHAPE"]
    for dim in ("T", "B", "C"):
        assert call(L, **{dim: 0}) == ARG and call(L, **{dim: -3}) == ARG
    pmax, dmax, cells = (d["HMM355_DURFORCED_MAX_" + k] for k in ("POSITIONS", "DURATION", "CELLS"))
    for bad in (dict(Lmax=0), dict(Lmax=-1), dict(Lmax=pmax + 1, Dmax=1), dict(Dmax=0), dict(Dmax=dmax + 1),
                dict(Lmax=cells // dmax + 1, Dmax=dmax), dict(Lmax=pmax, Dmax=cells // pmax + 1)):
        assert call(L, **bad) == STATES, bad
    for ptr in ("lp", "il", "sl", "du"):
        assert call(L, **{ptr: None}) == ARG
    assert call(L, ids=None, C=3, Lmax=4) == ARG           # the identity chain needs C >= Lmax
    assert call(L, T=1 << 30, B=1 << 30) == SHAPE


def test_forward_argument_checks(L, d):
    ARG = d["HMM355_E_ARG"]
    assert fwd(L, loglik=None) == ARG
    assert fwd(L, flags=4) == ARG                          # HMM355_DURFORCED_GRAD belongs to the size query
    assert fwd(L, flags=8) == ARG
    for out in ("begin", "F", "Bend", "Bbeg", "shift", "lls", "path", "score", "dur"):
        assert fwd(L, **{out: None}) == ARG                # each flag needs its outputs
    assert fwd(L, wsp=None) == ARG and fwd(L, wsp=ctypes.c_void_p(0x1004)) == ARG
    need = L.hmm355_durforced_workspace_bytes(2, 20, 4, 6, 3)
    assert fwd(L, nbytes=need - 1) == d["HMM355_E_WORKSPACE"]
    assert fwd(L, nbytes=16, flags=0) == d["HMM355_E_WORKSPACE"]


def test_gradient_argument_checks(L, d):
    ARG = d["HMM355_E_ARG"]
    for ptr in ("begin", "F", "Bend", "Bbeg", "shift", "lls"):
        assert grd(L, **{ptr: None}) == ARG
    assert grd(L, grad=None, gdur=None) == ARG             # no output at all
    need = L.hmm355_durforced_workspace_bytes(2, 20, 4, 6, d["HMM355_DURFORCED_GRAD"])
    assert grd(L, wsp=None) == ARG and grd(L, wsp=ctypes.c_void_p(0x1004)) == ARG
    assert grd(L, nbytes=need - 1) == d["HMM355_E_WORKSPACE"]
    assert grd(L, gdur=None, nbytes=need - 1) == d["HMM355_E_WORKSPACE"]   # class sums without gamma: a copy of it


def test_workspace_sizes(L, d):
    B, T, Lm, Dm = 3, 100, 81, 20
    value_only = L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, 0)
    tables = L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, 1)
    with_path = L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, 3)
    assert 0 < value_only == tables < B * T * Lm           # the tables are outputs, not workspace
    assert with_path >= value_only + B * T * Lm            # one byte per cell
    grad = L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, 4)
    assert grad >= B * T * Lm * 16 + B * Lm * Dm * 8
    assert L.hmm355_durforced_workspace_bytes(B, T, Lm, Dm, 4 | 2) == max(grad, with_path)
    assert L.hmm355_durforced_workspace_bytes(B, T, 1024, 16, 3) > 0 and L.hmm355_durforced_workspace_bytes(B, T, 128, 128, 3) > 0
    for bad in ((0, T, Lm, Dm, 0), (B, 0, Lm, Dm, 0), (B, T, 0, Dm, 0), (B, T, Lm, 0, 0), (B, T, 1025, 1, 0),
                (B, T, 4, 129, 0), (B, T, 1024, 17, 0), (B, T, 129, 128, 0), (-1, T, Lm, Dm, 0), (B, T, Lm, Dm, 8),
                (1 << 30, 1 << 30, Lm, Dm, 2)):
        assert L.hmm355_durforced_workspace_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------- Python
NAMES = ("DurationForcedAligner", "duration_forced_align", "duration_forced_loglik", "duration_forced_posteriors")


def test_import_surface():
    import pytorch_hmm_amd
    import pytorch_hmm_amd.alignment as al
    from pytorch_hmm_amd import ops
    for name in NAMES:
        assert hasattr(al, name) and name in al.__all__
        assert getattr(pytorch_hmm_amd, name) is getattr(al, name) and name in pytorch_hmm_amd.__all__
    for op in ("durforced", "durforced_grad"):
        assert hasattr(torch.ops.hmm355, op)
    from pytorch_hmm_amd.autograd import DurForcedLogLik
    assert "dur_lp" in DurForcedLogLik.__doc__
    assert ops.durforced_supported(1024, 16) and ops.durforced_supported(128, 128) and ops.durforced_supported(1, 1)
    for bad in ((1025, 1), (1, 129), (1024, 17), (0, 4), (4, 0)):
        assert not ops.durforced_supported(*bad)


def test_fake_registrations_give_shapes():
    lp, ids, du = (torch.empty(s, device="meta", dtype=t) for s, t in
                   (((2, 12, 5), torch.float32), ((2, 3), torch.int32), ((2, 3, 4), torch.float32)))
    il = sl = torch.empty(2, device="meta", dtype=torch.int32)
    out = torch.ops.hmm355.durforced(lp, ids, il, sl, du, tables=True, viterbi=True)
    assert [tuple(t.shape) for t in out] == [(2,)] + [(2, 12, 3)] * 4 + [(2, 12), (2,), (2, 12), (2,), (2, 3)]
    assert out[7].dtype == out[9].dtype == torch.int32
    out = torch.ops.hmm355.durforced(lp, ids, il, sl, du)
    assert tuple(out[0].shape) == (2,) and all(t.numel() == 0 for t in out[1:])
    g = torch.ops.hmm355.durforced_grad(*[torch.empty((2, 12, 3), device="meta")] * 4, torch.empty((2, 12), device="meta"),
                                        torch.empty(2, device="meta"), lp, ids, il, sl, du, want_gamma=True,
                                        want_grad=True, want_dur=True)
    assert [tuple(t.shape) for t in g] == [(2, 12, 3), (2, 12, 5), (2, 3, 4)]


def test_cpu_tensors_are_refused_by_name():
    import pytorch_hmm_amd.alignment as al
    from pytorch_hmm_amd import ops
    from pytorch_hmm_amd.autograd import DurForcedLogLik
    lp = torch.zeros(2, 6, 4)
    ids = torch.tensor([[0, 1, 2], [3, 3, 0]])
    il, sl = torch.tensor([6, 4]), torch.tensor([3, 2])
    du = torch.zeros(2, 3, 4)
    tab = torch.zeros(2, 6, 3)
    aligner = al.DurationForcedAligner(4, 4)
    for call in (lambda: al.duration_forced_align(lp, ids, il, sl, du),
                 lambda: al.duration_forced_loglik(lp, ids, il, sl, du),
                 lambda: al.duration_forced_loglik(lp.clone().requires_grad_(), ids, il, sl, du),
                 lambda: al.duration_forced_posteriors(lp, ids, il, sl, du),
                 lambda: aligner(lp, ids, il, sl), lambda: aligner.align(lp, ids, il, sl),
                 lambda: aligner.posteriors(lp, ids, il, sl, dur_lp=du), lambda: ops.durforced(lp, ids, il, sl, du),
                 lambda: ops.durforced_grad(tab, tab, tab, tab, torch.zeros(2, 6), torch.zeros(2), lp, ids, il, sl, du),
                 lambda: DurForcedLogLik.apply(lp, ids, il, sl, du)):
        with pytest.raises(RuntimeError, match="ROCm"):
            call()


def test_host_side_checks_raise_before_any_device_call():
    """_durforced_args runs before any launch; exercised directly, as a device is not needed for it."""
    from pytorch_hmm_amd import _native as nat
    from pytorch_hmm_amd import ops
    ids = torch.tensor([[1, 2, 1], [3, 0, 0]])
    ok = dict(lp=torch.zeros(2, 12, 5), ids=ids, il=torch.tensor([12, 7]), sl=torch.tensor([3, 1]),
              du=torch.zeros(2, 3, 4, dtype=torch.float64))

    def run(**kw):
        a = dict(ok)
        a.update(kw)
        return ops._durforced_args(a["lp"], "cpu", a["ids"], a["il"], a["sl"], a["du"])
    i32, il, sl, du, Lm, Dm = run()
    assert i32.dtype == il.dtype == sl.dtype == torch.int32 and du.dtype == torch.float32 and (Lm, Dm) == (3, 4)
    assert run(ids=None)[0] is None
    run(ids=torch.tensor([[1, 99, 1], [-3, 0, 0]]))        # ids are not checked: -inf emissions
    for bad in (dict(lp=torch.zeros(12, 5)), dict(lp=torch.zeros(2, 12, 5, 1)), dict(lp=torch.zeros(2, 0, 5)),
                dict(lp=torch.zeros(2, 12, 5, dtype=torch.int32)),                          # rank, size, dtype
                dict(du=torch.zeros(3, 4)), dict(du=torch.zeros(3, 3, 4)), dict(du=torch.zeros(2, 3, 4, dtype=torch.int64)),
                dict(ids=ids.float()), dict(ids=ids[:1]), dict(ids=ids[0]), dict(ids=torch.zeros(2, 4, dtype=torch.long)),
                dict(ids=None, du=torch.zeros(2, 6, 4)),                                     # identity chain: C < Lmax
                dict(il=torch.tensor([13, 7])), dict(il=torch.tensor([12, 0])), dict(il=torch.tensor([12])),
                dict(il=torch.tensor([12.0, 7.0])), dict(sl=torch.tensor([4, 1])), dict(sl=torch.tensor([3, 0]))):
        with pytest.raises(ValueError):
            run(**bad)
    # beyond the kernel's limits: the native library's error, naming them
    for Lm, Dm in ((1025, 1), (2, 129), (1024, 17), (129, 128)):
        with pytest.raises(nat.NativeError, match="positions \\* durations <= 16384"):
            run(ids=None, lp=torch.zeros(2, 12, 1025), du=torch.zeros(2, Lm, Dm))


def test_aligner_module_host_side():
    import pytorch_hmm_amd.alignment as al
    m = al.DurationForcedAligner(6, 5)
    assert isinstance(m.duration_logits, torch.nn.Parameter) and tuple(m.duration_logits.shape) == (6, 5)
    tokens = torch.tensor([[4, 0, 5], [2, 2, 77]])
    ids, sl = m.chain(tokens, torch.tensor([3, 2]))
    assert ids.dtype == sl.dtype == torch.int32 and sl.tolist() == [3, 2] and ids[0].tolist() == [4, 0, 5]
    du = m.duration_log_probs(ids)
    assert tuple(du.shape) == (2, 3, 5) and du.requires_grad
    assert torch.allclose(du.exp(), torch.full((2, 3, 5), 0.2))                # uniform over the durations
    for bad_tokens, bad_len in ((tokens, [3, 3]), (tokens, [0, 2]), (tokens, [4, 2]), (tokens.float(), [3, 2]),
                                (torch.tensor([[1, -1, 0], [0, 0, 0]]), [3, 2]), (tokens[0], [3])):
        with pytest.raises(ValueError):
            m.chain(bad_tokens, torch.tensor(bad_len))
    fixed = al.DurationForcedAligner(4, 3, learnable_durations=False)
    assert not list(fixed.parameters()) and tuple(fixed.duration_logits.shape) == (4, 3)
    for bad in ((0, 3), (3, 0), (3, 129)):
        with pytest.raises(ValueError):
            al.DurationForcedAligner(*bad)
    lp = torch.zeros(2, 9, 6)
    with pytest.raises(ValueError):
        m._args(torch.zeros(2, 9, 5), tokens, torch.tensor([3, 2]), None)     # C != num_tokens
    with pytest.raises(ValueError):
        m._args(lp, tokens, torch.tensor([3, 2]), torch.zeros(2, 3, 6))       # longer than max_duration
    with pytest.raises(ValueError):
        m._args(lp, tokens, torch.tensor([3, 2]), torch.zeros(2, 4, 5))       # not over the tokens
