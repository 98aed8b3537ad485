"""CPU: DurationConstrainedHMM without a device.

  * The numpy restatement in tests/dchmm_numpy.py (the GPU tests' oracle on shapes without a
    fixture) decodes the reference's states in every fixture (tests/golden/dchmm_*.npz,
    make_golden_dchmm.py) exactly, its group-of-one form decodes b3's single-sequence results, and
    the vectorised form agrees with the plain three-loop form bit for bit.
  * The C ABI (include/hmm355.h, csrc/dchmm.hip) declares and exports the two entry points,
    reports version >= 6 and rejects bad arguments with the documented codes before any launch.
  * The package exports DurationConstrainedHMM and the two duration utilities, imports without a
    GPU and refuses CPU tensors by name where the kernel would run.
  * The module's seeded parameters are the reference's; the utilities reproduce their fixture.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dchmm_numpy as dn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hmm355.h")


def settings(g):
    return g["e"], g["lT"], int(g["min_duration"]), int(g["max_duration"])


# ------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("name", dn.FIXTURES)
def test_restatement_decodes_the_reference_states(gold, name):
    g = gold("dchmm_" + name)
    states, delta, dur = dn.viterbi(*settings(g))
    assert states.dtype == np.int64 and np.array_equal(states, g["states"])
    assert delta.dtype == np.float32 and delta.shape == g["e"].shape == dur.shape
    assert not np.isnan(delta).any()


def test_restatement_group_of_one_decodes_sequences_alone(gold):
    g = gold("dchmm_b3")
    alone, _, _ = dn.viterbi(*settings(g), group=1)
    assert np.array_equal(alone, g["states_alone"])
    assert not np.array_equal(g["states_alone"], g["states"])      # the batch couples its sequences
    for b in range(3):
        one, _, _ = dn.viterbi(g["e"][b:b + 1], g["lT"], 3, 4)
        assert np.array_equal(one[0], g["states_alone"][b])


@pytest.mark.parametrize("name", dn.FIXTURES)
@pytest.mark.parametrize("group", [None, 1, 2])
def test_vectorised_restatement_equals_the_loops(gold, name, group):
    g = gold("dchmm_" + name)
    e, lT, mn, mx = settings(g)
    if name == "long":
        e = e[:, :60]       # the loops are slow; the first 60 frames pass max_duration = 30
    if group is not None and group > e.shape[0]:
        group = e.shape[0]
    fast, slow = dn.viterbi(e, lT, mn, mx, group=group), dn.viterbi_loops(e, lT, mn, mx, group=group)
    for x, y in zip(fast, slow):
        assert np.array_equal(x, y)


def test_fixtures_are_what_they_claim(gold):
    shapes = {"b1": (1, 12, 3), "b3": (3, 20, 5), "ties": (3, 25, 6), "neginf": (4, 12, 5), "long": (2, 200, 16)}
    for name, shape in shapes.items():
        assert gold("dchmm_" + name)["e"].shape == shape
    assert gold("dchmm_t1")["e"].shape[1] == 1
    assert settings(gold("dchmm_long"))[2:] == (3, 30)
    for name in ("b3", "ties"):     # both kinds of penalty are applied
        g = gold("dchmm_" + name)
        _, _, dur = dn.viterbi(*settings(g))
        prev = dur[:, :-1]
        assert (prev.max(axis=0) + 1 > int(g["max_duration"])).any() and (prev.min(axis=0) < int(g["min_duration"])).any()
    t = gold("dchmm_ties")
    assert np.array_equal(t["e"] * 2, np.round(t["e"] * 2)) and np.array_equal(t["lT"] * 2, np.round(t["lT"] * 2))
    n = gold("dchmm_neginf")
    assert 0.15 < np.isneginf(n["e"]).mean() < 0.35 and (n["e"][:, 0, 0] == 0).all()
    _, delta, dur = dn.viterbi(*settings(n))
    assert (dur[:, 0] == 1).all()                       # the first row counts 1 whatever its score
    dead = np.isneginf(delta[:, 1:])
    assert dead.any() and ((dur[:, 1:] == 0) == dead).all()     # later, a dead cell has run length 0


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
SYMBOLS = ("hmm355_dchmm_workspace_bytes", "hmm355_dchmm_viterbi_f32")


def call(L, e=FAKE, lT=FAKE, B=4, T=20, S=8, group=4, mn=3, mx=30, w=0.1, states=FAKE, score=FAKE, delta=None,
         dur=None, wsp=FAKE, ws=BIG):
    return L.hmm355_dchmm_viterbi_f32(e, lT, B, T, S, group, mn, mx, w, states, score, delta, dur, wsp, ws, None)


def test_header_exports_and_version(L, d):
    from pytorch_hmm_amd import _native as nat
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(hmm355_[a-z0-9_]+)\s*\(", src))
    for name in SYMBOLS:
        assert name in declared and name in nat.EXPORTS and hasattr(L, name)
    assert declared == set(nat.EXPORTS)
    assert L.hmm355_version() >= 6
    assert d["HMM355_DCHMM_MAX_STATES"] == nat.DCHMM_MAX_STATES == 256
    assert d["HMM355_DCHMM_MAX_CELLS"] == nat.DCHMM_MAX_CELLS == 4096


def test_argument_checks_return_the_documented_codes(L, d):
    ARG, STATES, SHAPE, WS = (d["HMM355_E_" + k] for k in ("ARG", "STATES", "SHAPE", "WORKSPACE"))
    assert call(L, S=0) == STATES and call(L, S=257) == STATES and call(L, S=-1) == STATES
    assert call(L, B=16, group=16, S=256, ws=0) == WS          # exactly the limit passes the size checks ...
    assert call(L, B=17, group=17, S=241) == STATES            # ... 17 * 241 = 4097 does not
    assert call(L, B=4097, group=4097, S=1) == STATES
    assert call(L, B=17, group=1, S=256, ws=0) == WS           # a group of one: no limit on B
    assert call(L, T=0) == SHAPE and call(L, T=-2) == SHAPE
    assert call(L, group=0) == ARG and call(L, group=5) == ARG and call(L, group=-1) == ARG
    assert call(L, B=0, group=0) == ARG
    for ptr in ("e", "lT", "states", "score", "wsp"):
        assert call(L, **{ptr: None}) == ARG
    assert call(L, wsp=ctypes.c_void_p(0x1004)) == ARG
    need = L.hmm355_dchmm_workspace_bytes(4, 20, 8)
    assert call(L, ws=need - 1) == WS
    assert call(L, T=1 << 30, B=1 << 30, group=1) == SHAPE


def test_workspace_sizes(L):
    assert L.hmm355_dchmm_workspace_bytes(4, 20, 8) >= 4 * 20 * 8      # one byte per cell
    assert L.hmm355_dchmm_workspace_bytes(4, 20, 8) < 4 * 20 * 8 + 1024
    assert L.hmm355_dchmm_workspace_bytes(100, 50, 256) >= 100 * 50 * 256
    for bad in ((0, 20, 8), (4, 0, 8), (4, 20, 0), (4, 20, 257), (-1, 20, 8), (1 << 30, 1 << 30, 8)):
        assert L.hmm355_dchmm_workspace_bytes(*bad) == 0


# ------------------------------------------------------------------------------- Python
def test_import_surface():
    import pytorch_hmm_amd as ph
    from pytorch_hmm_amd import DurationConstrainedHMM, compute_state_durations, create_duration_constrained_matrix
    for name in ("DurationConstrainedHMM", "compute_state_durations", "create_duration_constrained_matrix"):
        assert name in ph.__all__
    assert DurationConstrainedHMM is ph.hsmm.DurationConstrainedHMM
    assert compute_state_durations is ph.utils.compute_state_durations
    assert create_duration_constrained_matrix is ph.utils.create_duration_constrained_matrix
    assert hasattr(torch.ops.hmm355, "duration_constrained_viterbi")
    assert "duration_constrained_viterbi" in ph.ops.__doc__


def test_module_interface():
    from pytorch_hmm_amd import DurationConstrainedHMM
    m = DurationConstrainedHMM(5, 7)
    assert (m.num_states, m.feature_dim, m.min_duration, m.max_duration) == (5, 7, 3, 30)
    assert m.duration_penalty_weight == 0.1 and m.per_sequence is False
    assert DurationConstrainedHMM(5, 7, 2, 9, per_sequence=True).per_sequence is True
    with pytest.raises(TypeError):
        DurationConstrainedHMM(5, 7, 2, 9, True)       # the extension is keyword-only
    assert isinstance(m.transition_logits, torch.nn.Parameter) and m.transition_logits.shape == (5, 5)
    kinds = [type(x) for x in m.emission_net]
    assert kinds == [torch.nn.Linear, torch.nn.ReLU, torch.nn.Linear, torch.nn.LogSoftmax]
    assert (m.emission_net[0].in_features, m.emission_net[0].out_features) == (7, 128)
    assert (m.emission_net[2].in_features, m.emission_net[2].out_features) == (128, 5)
    with pytest.raises(ValueError, match="256"):
        DurationConstrainedHMM(257, 7)


def test_cpu_tensors_are_refused_by_name(gold):
    from pytorch_hmm_amd import DurationConstrainedHMM, ops
    g = gold("dchmm_b1")
    e, lT = torch.from_numpy(g["e"]), torch.from_numpy(g["lT"])
    m = DurationConstrainedHMM(3, 4, 3, 4)
    for run in (lambda: ops.duration_constrained_viterbi(e, lT, 3, 4), lambda: m._constrained_viterbi(e, lT),
                lambda: m(torch.zeros(1, 12, 4))):
        with pytest.raises(RuntimeError, match="ROCm"):
            run()


def test_module_parameters_from_a_seed(gold):
    from pytorch_hmm_amd import DurationConstrainedHMM
    g = gold("dchmm_module")
    S, D = g["log_transitions"].shape[0], int(g["feature_dim"])
    torch.manual_seed(int(g["seed"]))
    m = DurationConstrainedHMM(S, D, int(g["min_duration"]), int(g["max_duration"]))
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    for k, v in sd.items():
        want = g["sd." + k]
        assert tuple(v.shape) == want.shape and v.numpy().dtype == want.dtype
        # the initialisers (randn, kaiming uniform) are host arithmetic: equal up to its last bits
        np.testing.assert_allclose(v.numpy(), want, rtol=1e-6, atol=1e-7)
    # and the reference's state_dict loads
    m.load_state_dict({k: torch.from_numpy(g["sd." + k]) for k in sd})


def test_utilities_equal_the_fixture(gold):
    from pytorch_hmm_amd import compute_state_durations, create_duration_constrained_matrix
    g = gold("dchmm_utils")
    assert (g["matrix_args"][:, 2] < 0).any()       # max_duration=None is among the cases
    for i, (K, mn, mx) in enumerate(g["matrix_args"].tolist()):
        P = create_duration_constrained_matrix(K, mn, None if mx < 0 else mx)
        want = g[f"matrix_{i}"]
        assert P.dtype == torch.float32 and tuple(P.shape) == want.shape
        assert np.array_equal(P.numpy(), want)
    empties = 0
    for i in range(int(g["num_sequences"])):
        seq, want = g[f"sequence_{i}"], g[f"durations_{i}"]
        got = compute_state_durations(torch.from_numpy(seq))
        assert tuple(got.shape) == want.shape and got.numpy().dtype == want.dtype
        assert np.array_equal(got.numpy(), want)
        empties += seq.size == 0
    assert empties == 1 and compute_state_durations(torch.zeros(0, dtype=torch.long)).numel() == 0
    assert create_duration_constrained_matrix(2, 1).shape == (6, 6)
