"""GPU parity of the diagonal-GMM emission scorer (csrc/gmm.hip; ops.gmm_diag_logprob;
autograd.GmmLogProb): every launch form at its edges, and the analytic gradient on features that are
not centred.

Contracts:
  * Forward value, against the fp64 oracle of the direct (x - mu)^2 / exp(lv) form (O.c_gmm64, the
    reference's clamp and isinf rule).  The kernel accumulates the quadratic form in fp64 and
    rounds once, so with mix_lse = 0
        |lp - lp64| <= 2^-23 |lp64|                        (one fp32 ulp),
    and with mix_lse = 1 the fp32 LSE over terms <= 1 (expf, a C-term sum in [1, C], logf) adds
        |lp - lp64| <= 2^-23 |lp64| + (C + 4) 2^-23.
    Both are derived, not tuned.  Measured on MI355X, the largest fraction of the bound used
    (printed per test as "gmm bound use") is 0.498 over every forward case here -- the one rounding
    to fp32, as derived; per group of tests: BOUND_USE below.
  * A state whose components all have log_w = -inf gives the reference's clamp, log(1e-8) + 0:
    bit-equal to the oracle's value rounded to fp32.
  * Bitwise: C = 1 with log_w = 0 scores the same with and without the LSE; permuting the states
    permutes the output columns; a frame scores the same alone, in (1, F, D) and in (B, T, D); two
    calls are torch.equal.
  * Gradient (the contract of test_gpu_ctc.py / test_gpu_dtw.py): with g_64 / g_32 the fp64 / fp32
    autograd gradients of the reference expression (O.mixture_log_probs / O.hsmm_log_probs) on the
    CPU, for each of x, means, log_vars and the mixture logits
        max |g_gpu - g_64| <= 8 x max |g_32 - g_64|.
    Measured ratios on MI355X: at most 0.69 (GRADIENT_RATIOS below).  The fp32 expanded-form
    backward that the float64 one replaced scored up to 4490 and failed every case with off != 0
    (GRADIENT_RATIOS_FP32_EXPANDED).

The shapes sit on the kernels' own boundaries, read from gmm.hip: the v2 scorer's three workgroup
shapes (64 / 128 / 256 components, FT frames each) at a single group, group limit +- 1, a second and
third y-block with a few components, frame counts FT - 1 / FT / FT + 1 and D through both parities
of the chunk double buffer; the v1 scorer (C not in {1, 2, 4}) at each of its four thread counts,
with idle tail lanes, spb = 1 and 2, two y-blocks, C up to 256 and frame counts around its 16-frame
LSE tile and its 64-frame workgroup.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import hmm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "pytorch_hmm_amd", "csrc", "gmm.hip")).read()
EPS23 = 2.0 ** -23


def _const(name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, _SRC).group(1))


THREADS, FRAMES, DC, SUB, DMAX = (_const(n) for n in ("kGmmThreads", "kGmmFrames", "kGmmDc", "kGmmSub", "kGmmDMax"))
# the default v2 launches G4R(FG, NW, NF) of the 256 / 128 / 64 component groups, in source order
_G4 = [tuple(int(v) for v in m) for m in re.findall(r": G4R\((\d+), (\d+), (\d+)\);", _SRC)]
V2_FT = {4 * (64 // fg): nw * fg * nf for fg, nw, nf in _G4}     # components per group -> frames per group

# measured on MI355X: the largest |lp - lp64| / bound per group of forward tests (bound: 1)
BOUND_USE = {"v2-sc": 0.498, "v2-fd": 0.478, "v1-sc": 0.406, "v1-fd": 0.478, "val-o1": 0.409, "val-offset": 0.482,
             "val-smallvar": 0.496, "val-far": 0.416, "val-winf_one": 0.416, "val-winf_all": 0.409,
             "gradient cases": 0.488}
# measured on MI355X: max |g_gpu - g_64| / max |g_32 - g_64| as (x, means, log_vars, logits) for the
# mixture shape (S, C, D = 6, 3, 40) and (x, means, log_vars) for the single-Gaussian one (5, 1, 7)
GRADIENT_RATIOS = {
    "mix/centred": (0.0995, 0.114, 0.0422, 0.192), "single/centred": (0.392, 0.693, 0.0489),
    "mix/off10": (0.0639, 0.0421, 0.0335, 0.0997), "single/off10": (0.345, 0.226, 0.153),
    "mix/off30_xs3": (0.0271, 0.021, 0.0122, 0.075), "single/off30_xs3": (0.281, 0.521, 0.181),
    "mix/off30_lvm-3": (0.0226, 0.0233, 0.0233, 0.108), "single/off30_lvm-3": (0.573, 0.249, 0.193),
    "mix/off100_xs5": (0.0626, 0.0471, 0.0622, 0.0863), "single/off100_xs5": (0.619, 0.215, 0.281),
    "mix/tight_off0": (0.000505, 0.00057, 0.000288, 0.000988), "single/tight_off0": (0.41, 0.178, 0.241),
    "mix/tight_off50": (0.312, 0.401, 0.291, 0.251), "single/tight_off50": (0.459, 0.25, 0.435),
    "masked (x, means, log_vars, log_w)": (0.0992, 0.0421, 0.0258, 0.0435), "layer (means, log_vars)": (0.337, 0.546),
    "layer fitted (means, log_vars)": (0.0375, 0.0207)}
# the same ratios, on MI355X, of the fp32 expanded-form backward that the float64 one replaced: every case
# with off != 0 is over the bound of 8
GRADIENT_RATIOS_FP32_EXPANDED = {
    "mix/centred": (2.42, 1.5, 1.36, 2.21), "single/centred": (1.58, 2.52, 0.349),
    "mix/off10": (136, 244, 248, 319), "single/off10": (7.13, 7.08, 68.8),
    "mix/off30_xs3": (396, 321, 372, 394), "single/off30_xs3": (5.98, 18.3, 166),
    "mix/off30_lvm-3": (2720, 3230, 3490, 3260), "single/off30_lvm-3": (27.8, 22.6, 333),
    "mix/off100_xs5": (4490, 4460, 3800, 1910), "single/off100_xs5": (20.9, 16.2, 225),
    "mix/tight_off0": (0.15, 0.15, 0.15, 0.151), "single/tight_off0": (1.14, 1.88, 0.544),
    "mix/tight_off50": (6.11, 9.42, 85, 1), "single/tight_off50": (8.85, 7.71, 40.6)}


@pytest.fixture(scope="module", autouse=True)
def _native():
    import pytorch_hmm_amd._native as nat
    nat.lib()  # fail loudly if the HIP library is missing
    assert torch.cuda.is_available()


def ops():
    from pytorch_hmm_amd import ops as o
    return o


def dev(a):
    return torch.as_tensor(np.asarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---------------------------------------------------------------------------- launch forms
def is_v2(C):
    return C in (1, 2, 4)


def v2_group(P):
    return 256 if P > 128 else (128 if P > 64 else 64)


def form(S, C):
    """The launch gmm_run picks for (S, C), restated (test_launch_constants pins it to the source)."""
    P = S * C
    if is_v2(C):
        g = v2_group(P)
        return dict(kind="v2", group=g, ft=V2_FT[g], yblocks=-(-P // g), partial=P % g != 0)
    nt = 64 if P <= 64 else (128 if P <= 128 else (192 if P <= 192 else THREADS))
    spb = nt // C
    return dict(kind="v1", nt=nt, spb=spb, ft=FRAMES, yblocks=-(-S // spb), idle=nt - spb * C)


V2_SC = [(1, 1), (5, 1), (63, 1), (64, 1), (65, 1), (128, 1), (129, 1), (257, 1), (65, 2), (16, 4), (17, 4), (32, 4),
         (33, 4), (65, 4), (129, 4)]
V2_D = [1, 7, 8, 9, 16, 17, 80]          # 1 / 1 / 1 / 2 / 2 / 3 / 10 chunks
V1_SC = [(21, 3), (22, 3), (9, 7), (38, 5), (39, 5), (120, 3), (3, 100), (1, 65), (2, 256), (1, 3)]
V1_D = [1, 8, 9, 17, 80]
# one (S, C) per v2 group and per v1 thread count
VALUE_SC = [(16, 4), (32, 4), (65, 4), (21, 3), (22, 3), (38, 5), (120, 3)]


def v2_frames(S, C):
    ft = form(S, C)["ft"]
    return [(1, 1), (1, ft - 1), (1, ft), (1, ft + 1), (3, 43)]


V1_FRAMES = [(1, 1), (1, SUB - 1), (1, SUB), (1, SUB + 1), (1, FRAMES - 1), (1, FRAMES), (1, FRAMES + 1), (3, 43)]


def test_launch_constants():
    """The launch forms the cases below are built on are still the source's."""
    assert (THREADS, FRAMES, DC, SUB) == (256, 64, 8, 16)
    assert "return C == 1 || C == 2 || C == 4;" in _SRC
    assert "return P > 128 ? 256 : (P > 64 ? 128 : 64);" in _SRC
    assert "P <= 64 ? 64 : (P <= 128 ? 128 : (P <= 192 ? 192 : kGmmThreads))" in _SRC
    assert "constexpr int kG4Dc = 8;" in _SRC
    assert "static constexpr int FT = NW * FW;" in _SRC and "static constexpr int FW = FG * kG4Nf;" in _SRC
    assert "static constexpr int CG = 4 * CL;" in _SRC and "static constexpr int CL = 64 / FG;" in _SRC
    assert len(_G4) == 3 and [4 * (64 // fg) for fg, _, _ in _G4] == [256, 128, 64]
    assert V2_FT == {64: 32, 128: 32, 256: 64}


def test_cases_cover_every_launch_form():
    v2 = [form(S, C) for S, C in V2_SC]
    assert all(f["kind"] == "v2" for f in v2)
    assert {f["group"] for f in v2} == {64, 128, 256}
    assert any(64 < S * C <= 128 for S, C in V2_SC)
    assert any(f["partial"] and f["yblocks"] == 2 for f in v2) and any(f["partial"] and f["yblocks"] == 3 for f in v2)
    assert any(C == 1 and S % 4 and S > 256 for S, C in V2_SC)      # a lane whose later states fall past P
    v1 = [form(S, C) for S, C in V1_SC]
    assert all(f["kind"] == "v1" for f in v1)
    assert {f["nt"] for f in v1} == {64, 128, 192, 256}
    assert any(f["yblocks"] == 2 and f["spb"] > 2 for f in v1)
    assert {1, 2} <= {f["spb"] for f in v1} and any(f["idle"] > 0 for f in v1)
    assert any(C == 256 for _, C in V1_SC) and any(64 < C < 256 for _, C in V1_SC)
    # the value and bitwise cases reach every group size of both scorers
    vf = [form(S, C) for S, C in VALUE_SC]
    assert {f["group"] for f in vf if f["kind"] == "v2"} == {64, 128, 256}
    assert {f["nt"] for f in vf if f["kind"] == "v1"} == {64, 128, 192, 256}
    # D: one chunk, an odd and an even chunk count, last chunks of 1 and of 8 dims
    for dims in (V2_D, V1_D):
        chunks = [-(-d // DC) for d in dims]
        assert 1 in chunks and any(c > 1 and c % 2 for c in chunks) and any(c % 2 == 0 for c in chunks)
        assert any(d % DC == 1 for d in dims) and any(d % DC == 0 for d in dims) and min(dims) < DC


# ---------------------------------------------------------------------------- data, bound
def draw(S, C, D, B, T, off=0.0, xs=1.0, lvm=0.0, kind="o1"):
    """x ~ N(off, xs^2), mu ~ N(off, (xs / 2)^2), log_vars ~ N(lvm, 0.2^2), log_w a log-softmax."""
    rng = np.random.default_rng([S, C, D, B, T])
    x = (off + xs * rng.standard_normal((B, T, D))).astype(np.float32)
    mu = (off + 0.5 * xs * rng.standard_normal((S, C, D))).astype(np.float32)
    lv = (lvm + 0.2 * rng.standard_normal((S, C, D))).astype(np.float32)
    z = rng.standard_normal((S, C))
    lw = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    if kind == "far":                     # component 0 of every state far from every frame: expf -> 0
        mu[:, 0] += 1000.0
    elif kind == "winf_one":
        lw[:, 0] = -np.inf
    elif kind == "winf_all":              # every component of two states (the last one included)
        lw[[S // 2, S - 1]] = -np.inf
    return x, mu, lv, lw


def score(x, mu, lv, lw, mix):
    lp = ops().gmm_diag_logprob(dev(x), dev(mu), dev(lv), dev(lw), mix)
    assert lp.dtype == torch.float32 and tuple(lp.shape) == (x.shape[0], x.shape[1], mu.shape[0])
    return lp.cpu().numpy()


def bound_use(lp, lp64, C, mix):
    """max |lp - lp64| / bound (the module docstring's), over finite lp64."""
    assert lp.shape == lp64.shape and np.isfinite(lp64).all() and np.isfinite(lp).all()
    tol = EPS23 * np.abs(lp64) + ((C + 4) * EPS23 if mix else 0.0)
    err = np.abs(lp.astype(np.float64) - lp64)
    use = np.where(tol > 0, err / np.maximum(tol, 1e-300), np.where(err == 0, 0.0, np.inf))
    return float(use.max())


def check(tag, x, mu, lv, lw, mix):
    lp = score(x, mu, lv, lw, mix)
    use = bound_use(lp, O.c_gmm64(x, mu, lv, lw), mu.shape[1], mix)
    print("gmm bound use [%s] S=%d C=%d D=%d frames=%dx%d mix=%d: %.3f"
          % (tag, mu.shape[0], mu.shape[1], x.shape[2], x.shape[0], x.shape[1], mix, use))
    assert use <= 1.0, use
    return lp


# ---------------------------------------------------------------------------- 1.2 v2 shapes
@pytest.mark.parametrize("S,C", V2_SC)
def test_v2_state_counts(S, C):
    x, mu, lv, lw = draw(S, C, 17, 3, 43)
    check("v2-sc", x, mu, lv, lw, 1)
    if C == 1:
        check("v2-sc", x, mu, lv, np.zeros_like(lw), 0)


@pytest.mark.parametrize("S,C,dims", [(65, 2, V2_D), (33, 4, V2_D), (17, 4, V2_D), (63, 1, V2_D), (129, 4, [17, 80])])
def test_v2_frame_counts_and_dims(S, C, dims):
    for B, T in v2_frames(S, C):
        for D in dims:
            check("v2-fd", *draw(S, C, D, B, T), 1)


# ---------------------------------------------------------------------------- 1.3 v1 shapes
@pytest.mark.parametrize("S,C", V1_SC)
def test_v1_shapes(S, C):
    check("v1-sc", *draw(S, C, 17, 3, 43), 1)


@pytest.mark.parametrize("S,C,dims", [(120, 3, V1_D), (9, 7, V1_D), (2, 256, [17, 80])])
def test_v1_frame_counts_and_dims(S, C, dims):
    for B, T in V1_FRAMES:
        for D in dims:
            check("v1-fd", *draw(S, C, D, B, T), 1)


# ---------------------------------------------------------------------------- 1.4 values
@pytest.mark.parametrize("S,C", VALUE_SC)
@pytest.mark.parametrize("name,kw", [("o1", {}), ("offset", dict(off=100.0, xs=5.0)), ("smallvar", dict(lvm=-8.0)),
                                     ("far", dict(kind="far")), ("winf_one", dict(kind="winf_one"))])
def test_values(name, kw, S, C):
    check("val-" + name, *draw(S, C, 17, 3, 43, **kw), 1)


@pytest.mark.parametrize("S,C", VALUE_SC)
def test_all_components_masked_gives_the_clamp(S, C):
    x, mu, lv, lw = draw(S, C, 17, 3, 43, kind="winf_all")
    lp = score(x, mu, lv, lw, 1)
    lp64 = O.c_gmm64(x, mu, lv, lw)
    off = [S // 2, S - 1]
    on = [s for s in range(S) if s not in off]
    assert (lp64[..., off] == math.log(1e-8)).all()
    assert np.array_equal(bits(lp[..., off]), bits(lp64[..., off].astype(np.float32)))
    if on:
        use = bound_use(lp[..., on], lp64[..., on], C, 1)
        print("gmm bound use [val-winf_all] S=%d C=%d: %.3f" % (S, C, use))
        assert use <= 1.0, use


# ---------------------------------------------------------------------------- 1.5 bitwise
@pytest.mark.parametrize("S", [5, 65, 257])
def test_single_component_lse_is_the_identity(S):
    x, mu, lv, lw = draw(S, 1, 17, 3, 43)
    zero = np.zeros_like(lw)
    assert np.array_equal(bits(score(x, mu, lv, zero, 1)), bits(score(x, mu, lv, zero, 0)))


@pytest.mark.parametrize("S,C", [(257, 1), (65, 2), (129, 4), (120, 3), (3, 100), (39, 5)])
def test_state_permutation_permutes_columns(S, C):
    x, mu, lv, lw = draw(S, C, 17, 3, 43)
    perm = np.random.default_rng(S * C).permutation(S)
    lp = score(x, mu, lv, lw, 1)
    lpp = score(x, mu[perm], lv[perm], lw[perm], 1)
    assert np.array_equal(bits(lpp), bits(lp[..., perm]))


@pytest.mark.parametrize("S,C", [(16, 4), (32, 4), (65, 4), (120, 3), (9, 7)])
def test_frame_rows_do_not_depend_on_the_batch(S, C):
    ft = form(S, C)["ft"]
    F = ft + 1
    b = next(k for k in range(2, F) if F % k == 0)
    x, mu, lv, lw = draw(S, C, 17, 1, F)
    flat = score(x, mu, lv, lw, 1)
    batched = score(x.reshape(b, F // b, 17), mu, lv, lw, 1)
    assert np.array_equal(bits(batched.reshape(1, F, S)), bits(flat))
    for f in sorted({0, 1, SUB - 1, SUB, ft - 1, ft}):
        alone = score(x[:, f:f + 1], mu, lv, lw, 1)
        assert np.array_equal(bits(alone[0, 0]), bits(flat[0, f])), f


@pytest.mark.parametrize("S,C", [(129, 4), (120, 3)])
def test_two_calls_are_equal(S, C):
    t = [dev(a) for a in draw(S, C, 17, 3, 43)]
    assert torch.equal(ops().gmm_diag_logprob(*t, 1), ops().gmm_diag_logprob(*t, 1))


# ---------------------------------------------------------------------------- 1.6 arguments
def test_argument_errors():
    import pytorch_hmm_amd._native as nat
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    g = ops().gmm_diag_logprob
    with pytest.raises(nat.NativeError):
        g(z(1, 2, 3), z(2, 2, 3), z(2, 2, 3), z(2, 2), 0)                   # mix_lse == 0 needs C == 1
    with pytest.raises(nat.NativeError):
        g(z(1, 1, DMAX + 1), z(1, 1, DMAX + 1), z(1, 1, DMAX + 1), z(1, 1), 1)
    with pytest.raises(nat.NativeError):
        g(z(1, 1, 1), z(65537, 1, 1), z(65537, 1, 1), z(65537, 1), 1)       # S * C > 65536
    with pytest.raises(nat.NativeError):
        g(z(1, 1, 1), z(1, 257, 1), z(1, 257, 1), z(1, 257), 1)             # C > 256
    with pytest.raises(ValueError):
        g(z(1, 2, 3), z(2, 2, 4), z(2, 2, 4), z(2, 2), 1)
    for B, T in ((0, 5), (2, 0)):
        out = g(z(B, T, 3), z(2, 2, 3), z(2, 2, 3), z(2, 2), 1)
        assert tuple(out.shape) == (B, T, 2) and out.numel() == 0 and out.dtype == torch.float32
    # the limits themselves are accepted
    assert tuple(g(z(1, 1, 1), z(1, 256, 1), z(1, 256, 1), z(1, 256), 1).shape) == (1, 1, 1)


# ---------------------------------------------------------------------------- 2. gradients
# name -> (off, xs, lvm, tight)
GRAD_CASES = {"centred": (0.0, 1.0, 0.0, False), "off10": (10.0, 1.0, 0.0, False), "off30_xs3": (30.0, 3.0, 0.0, False),
              "off30_lvm-3": (30.0, 1.0, -3.0, False), "off100_xs5": (100.0, 5.0, 0.0, False),
              "tight_off0": (0.0, 10.0, -4.0, True), "tight_off50": (50.0, 10.0, -4.0, True)}
GRAD_SHAPES = {"mix": (6, 3, 40, 2, 20), "single": (5, 1, 7, 2, 20)}      # S, C, D, B, T


def grad_inputs(name, shape):
    off, xs, lvm, tight = GRAD_CASES[name]
    S, C, D, B, T = GRAD_SHAPES[shape]
    gen = torch.Generator().manual_seed(1000 * sorted(GRAD_CASES).index(name) + S)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    mu = off + 0.5 * xs * rn(S, C, D)
    lv = lvm + 0.2 * rn(S, C, D)
    if tight:   # each frame from one component: its mean plus noise of its own variance
        p = torch.randint(S * C, (B, T), generator=gen)
        x = mu.view(-1, D)[p] + torch.exp(0.5 * lv.view(-1, D)[p]) * rn(B, T, D)
    else:
        x = off + xs * rn(B, T, D)
    return x, mu, lv, 0.5 * rn(S, C), rn(B, T, S)


def reference_grads(x, mu, lv, logits, W, mix, dtype):
    leaves = (x, mu, lv, logits) if mix else (x, mu[:, 0], lv[:, 0])
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in leaves]
    lp = O.mixture_log_probs(*[leaves[i] for i in (0, 3, 1, 2)]) if mix else O.hsmm_log_probs(*leaves)
    (lp * W.to(dtype)).sum().backward()
    return [t.grad.double() for t in leaves]


def ratios(got, g64, g32):
    out = []
    for a, r64, r32 in zip(got, g64, g32):
        assert a.shape == r64.shape and torch.isfinite(a).all()
        yard = (r32 - r64).abs().max().item()
        # the yardstick is itself an accurate gradient (4e-8 .. 8e-5 of the largest entry over the cases)
        assert 0 < yard <= 1e-3 * r64.abs().max().item()
        out.append((a.double().cpu() - r64).abs().max().item() / yard)
    return out


@pytest.mark.parametrize("shape", sorted(GRAD_SHAPES))
@pytest.mark.parametrize("name", sorted(GRAD_CASES))
def test_gradients_on_offset_features(name, shape):
    from pytorch_hmm_amd.autograd import GmmLogProb
    mix = int(shape == "mix")
    x, mu, lv, logits, W = grad_inputs(name, shape)
    g64 = reference_grads(x, mu, lv, logits, W, mix, torch.float64)
    g32 = reference_grads(x, mu, lv, logits, W, mix, torch.float32)
    ours = [t.clone().to(DEV).requires_grad_(True) for t in (x, mu, lv, logits)]
    if mix:
        log_w = torch.log(torch.clamp(torch.softmax(ours[3], -1), min=1e-8))
    else:
        log_w = torch.zeros(mu.shape[0], 1, device=DEV)
    lp = GmmLogProb.apply(ours[0], ours[1], ours[2], log_w, mix)
    lp64 = O.c_gmm64(x.numpy(), mu.numpy(), lv.numpy(), log_w.detach().cpu().numpy())
    use = bound_use(lp.detach().cpu().numpy(), lp64, mu.shape[1], mix)
    (lp * W.to(DEV)).sum().backward()
    got = [t.grad for t in ours[:4 if mix else 3]]
    assert [t.dtype for t in got] == [torch.float32] * len(got)
    if not mix:
        got[1], got[2] = got[1][:, 0], got[2][:, 0]
    r = ratios(got, g64, g32)
    print("gmm gradient ratios [%s/%s] value bound use %.3f, x means log_vars logits: %s"
          % (shape, name, use, " ".join("%.3g" % v for v in r)))
    assert use <= 1.0, use
    assert max(r) <= 8.0, r


def masked_case():
    """The off10 mixture case with log_w a leaf: every component of state 2 and one of state 4 at -inf."""
    x, mu, lv, logits, W = grad_inputs("off10", "mix")
    lw = torch.log_softmax(logits, -1)
    lw[2] = -math.inf
    lw[4, 1] = -math.inf
    return x, mu, lv, lw, W


def masked_reference_grads(x, mu, lv, lw, W, dtype):
    leaves = [t.clone().to(dtype).requires_grad_(True) for t in (x, mu, lv, lw)]
    xr, m, v, w = leaves
    diff = xr.unsqueeze(2).unsqueeze(3) - m
    comp = -0.5 * (torch.sum(diff ** 2 / torch.exp(v), -1) + v.sum(-1) + x.shape[-1] * math.log(2 * math.pi)) + w
    (O._mix_lse(comp, -1) * W.to(dtype)).sum().backward()
    return [t.grad.double() for t in leaves]


def test_gradients_with_masked_components():
    """log_w = -inf: a masked component gets no gradient, and a state with every component masked
    (the reference's m = -inf -> 0 and clamp: a constant) passes none to x, its means or variances."""
    from pytorch_hmm_amd.autograd import GmmLogProb
    x, mu, lv, lw, W = masked_case()
    g64 = masked_reference_grads(x, mu, lv, lw, W, torch.float64)
    g32 = masked_reference_grads(x, mu, lv, lw, W, torch.float32)
    ours = [t.clone().to(DEV).requires_grad_(True) for t in (x, mu, lv, lw)]
    lp = GmmLogProb.apply(*ours, 1)
    assert np.array_equal(bits(lp[..., 2].detach().cpu().numpy()), bits(np.full((2, 20), math.log(1e-8))))
    (lp * W.to(DEV)).sum().backward()
    got = [t.grad for t in ours]
    for t in got[1:]:
        assert (t[2] == 0).all() and (t[4, 1] == 0).all() and (g64[3][2] == 0).all()
    r = ratios(got, g64, g32)
    print("gmm gradient ratios [masked] x means log_vars log_w: %s" % " ".join("%.3g" % v for v in r))
    assert max(r) <= 8.0, r


@pytest.mark.parametrize("fitted", [False, True])
def test_layer_gradients_on_offset_features(fitted):
    """MixtureGaussianHMMLayer in train mode on x ~ N(30, 9): the gradients of -mean(score) into the
    means and log-variances against autograd of the reference expression along the same Viterbi
    path (the path's transition and start terms do not depend on them).  fitted: the means moved
    onto the features, as training leaves them (x - mu small against x: the expansion cancels)."""
    import pytorch_hmm_amd as ph
    torch.manual_seed(5)
    layer = ph.MixtureGaussianHMMLayer(6, 40, num_components=3).to(DEV)
    if fitted:
        with torch.no_grad():
            layer.means.copy_(30.0 + 1.5 * torch.randn_like(layer.means))
    layer.train()
    x = 30.0 + 3.0 * torch.randn(2, 20, 40)
    states, log_probs = layer(x.to(DEV), return_log_probs=True)
    (-log_probs.mean()).backward()
    path = states.cpu().unsqueeze(-1)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        mu, lv, logits = (p.detach().cpu().to(dtype).requires_grad_(True)
                          for p in (layer.means, layer.log_vars, layer.mixture_weights_logits))
        lp = O.mixture_log_probs(x.to(dtype), logits, mu, lv)
        (-lp.gather(2, path).squeeze(-1).sum(1).mean()).backward()
        ref[dtype] = [mu.grad.double(), lv.grad.double()]
    r = ratios([layer.means.grad, layer.log_vars.grad], ref[torch.float64], ref[torch.float32])
    print("gmm gradient ratios [layer%s] means log_vars: %s" % (" fitted" * fitted, " ".join("%.3g" % v for v in r)))
    assert max(r) <= 8.0, r
