"""Writes tests/golden/dchmm_*.npz from the reference's DurationConstrainedHMM (torch-CPU).

    python tests/golden/make_golden_dchmm.py /path/to/reference

The fixtures hold data only.  dchmm_<case>.npz: e (B,T,S) fp32 emission log-probs, lT (S,S) fp32
log-transitions, min_duration, max_duration, and states (B,T): what the reference's
DurationConstrainedHMM._constrained_viterbi returns for them (the whole batch in one call, so
the sequences share their penalties).  dchmm_b3.npz also has states_alone: the three sequences
decoded one at a time.  dchmm_module.npz: a seeded module's parameters (sd_keys in state_dict
order, sd.<key>), observations, the emission_log_probs / log_transitions its forward formed and
the states it returned.  dchmm_utils.npz: create_duration_constrained_matrix and
compute_state_durations on a few inputs.

The cases are checked here before they are written: tests/dchmm_numpy.py reproduces the
reference's states; in b3 and ties both kinds of penalty are applied; in b3 the batch decode
differs from the three single-sequence decodes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dchmm_numpy as dn  # noqa: E402


def emissions(rng, B, T, S, boost=2.5, seg=(4, 9)):
    """log-softmax rows that favour a piecewise-constant state sequence, so that paths stay"""
    x = rng.standard_normal((B, T, S)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(seg[0], seg[1] + 1))
            x[b, t:t + n, int(rng.integers(0, S))] += boost
            t += n
    return torch.log_softmax(torch.from_numpy(x), dim=2).numpy()


def transitions(rng, S):
    return torch.log(torch.softmax(torch.from_numpy(rng.standard_normal((S, S)).astype(np.float32)), dim=1) + 1e-8).numpy()


def both_penalties_fire(dur, min_duration, max_duration):
    prev = dur[:, :-1]
    return bool((prev.max(axis=0) + 1 > max_duration).any()) and bool((prev.min(axis=0) < min_duration).any())


def main():
    sys.path.insert(0, sys.argv[1])
    import pytorch_hmm.hsmm as ref_hsmm
    import pytorch_hmm.utils as ref_utils

    def decode(e, lT, mn, mx):
        m = ref_hsmm.DurationConstrainedHMM(e.shape[2], 4, mn, mx)
        with torch.no_grad():
            return m._constrained_viterbi(torch.from_numpy(e), torch.from_numpy(lT)).numpy()

    def write(name, e, lT, mn, mx, **extra):
        states = decode(e, lT, mn, mx)
        mine, _, dur = dn.viterbi(e, lT, mn, mx)
        assert np.array_equal(mine, states), name
        np.savez_compressed(os.path.join(HERE, f"dchmm_{name}.npz"), e=e, lT=lT, min_duration=np.array(mn),
                            max_duration=np.array(mx), states=states, **extra)
        return states, dur

    rng = np.random.default_rng(41)
    write("b1", emissions(rng, 1, 12, 3), transitions(rng, 3), 3, 4)

    for seed in range(100):  # b3: the batch decode must differ from the sequences decoded alone
        r = np.random.default_rng(1000 + seed)
        e, lT = emissions(r, 3, 20, 5), transitions(r, 5)
        together, _, dur = dn.viterbi(e, lT, 3, 4)
        alone, _, _ = dn.viterbi(e, lT, 3, 4, group=1)
        if not np.array_equal(together, alone) and both_penalties_fire(dur, 3, 4):
            break
    else:
        raise SystemExit("no seed gives a b3 case whose batch decode differs")
    states_alone = np.concatenate([decode(e[b:b + 1], lT, 3, 4) for b in range(3)])
    assert np.array_equal(states_alone, alone)
    states, dur = write("b3", e, lT, 3, 4, states_alone=states_alone, seed=np.array(1000 + seed))
    assert not np.array_equal(states, states_alone) and both_penalties_fire(dur, 3, 4)

    e, lT = emissions(rng, 3, 25, 6), transitions(rng, 6)
    e, lT = (np.round(2 * e) / 2).astype(np.float32), (np.round(2 * lT) / 2).astype(np.float32)
    _, dur = write("ties", e, lT, 3, 4)
    assert both_penalties_fire(dur, 3, 4)

    e, lT = emissions(rng, 4, 12, 5), transitions(rng, 5)
    e[rng.random(e.shape) < 0.25] = -np.inf
    e[:, 0, 0] = 0.0
    write("neginf", e, lT, 3, 4)

    write("t1", emissions(rng, 2, 1, 4), transitions(rng, 4), 3, 4)
    write("long", emissions(rng, 2, 200, 16, seg=(2, 45)), transitions(rng, 16), 3, 30)

    # the module: parameters from a seed, forward on CPU
    seed, B, T, S, D = 7, 2, 16, 4, 6
    torch.manual_seed(seed)
    m = ref_hsmm.DurationConstrainedHMM(S, D, 3, 4)
    obs = torch.from_numpy(rng.standard_normal((B, T, D)).astype(np.float32))
    with torch.no_grad():
        elp = m.emission_net(obs)
        lT = torch.log(torch.softmax(m.transition_logits, dim=-1) + 1e-8)
        states = m(obs)
        assert torch.equal(states, m._constrained_viterbi(elp, lT))
    sd = m.state_dict()
    out = {"sd." + k: v.numpy() for k, v in sd.items()}
    np.savez_compressed(os.path.join(HERE, "dchmm_module.npz"), seed=np.array(seed), obs=obs.numpy(),
                        emission_log_probs=elp.numpy(), log_transitions=lT.numpy(), states=states.numpy(),
                        min_duration=np.array(3), max_duration=np.array(4), feature_dim=np.array(D),
                        sd_keys=np.array(list(sd.keys())), **out)

    # the two utility functions; max_duration -1 stands for None
    out = {}
    matrix_args = [(3, 1, -1), (2, 2, 4), (3, 2, -1), (1, 1, 3), (4, 3, 3), (2, 1, 1), (3, 4, 2)]
    out["matrix_args"] = np.array(matrix_args)
    for i, (K, mn, mx) in enumerate(matrix_args):
        out[f"matrix_{i}"] = ref_utils.create_duration_constrained_matrix(K, mn, None if mx < 0 else mx).numpy()
    seqs = [[0, 0, 1, 1, 1, 2], [5], [], [1, 2, 3], [2, 2, 2, 2], [0, 1, 1, 0, 0, 0, 3, 3, 1]]
    out["num_sequences"] = np.array(len(seqs))
    for i, s in enumerate(seqs):
        out[f"sequence_{i}"] = np.array(s, dtype=np.int64)
        out[f"durations_{i}"] = ref_utils.compute_state_durations(torch.tensor(s, dtype=torch.long)).numpy()
    np.savez_compressed(os.path.join(HERE, "dchmm_utils.npz"), **out)


if __name__ == "__main__":
    main()
