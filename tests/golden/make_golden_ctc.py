"""Writes tests/golden/ctc_*.npz from the reference's pytorch_hmm.alignment.ctc (torch-CPU).

    python tests/golden/make_golden_ctc.py /path/to/reference

The fixtures hold data only.  Each ctc_<case>.npz has the inputs (lp (T,B,C) fp32 log-softmax
rows, targets (B,Lmax), input_lengths, target_lengths, blank); what the reference computes from
them: ref_loglik (ctc_forward_algorithm; its alpha table is not returned), ref_beta
(ctc_backward_algorithm), ref_expand (expand_targets_with_blank), ref_align (ctc_alignment_path,
padded with -1: all blank, its alpha is never filled), ref_greedy / ref_greedy_len
(CTCAligner.decode, padded with -1) and ref_beam_equal (decode(beam_width=4) gave the same),
seq / ref_collapse / ref_remove / ref_decode (the utilities on sequence 0's best path); and alpha64,
beta64, loglik64, gamma64, grad64 from the fp64 restatement in tests/ctc_numpy.py.
ctc_segment.npz holds CTCSegmentationAligner.segment_and_align's cuts of a 2300-frame recording.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ctc_numpy as cn  # noqa: E402


def log_softmax_rows(rng, T, B, C):
    return torch.log_softmax(torch.from_numpy(rng.standard_normal((T, B, C)).astype(np.float32)), dim=2).numpy()


def pad_list(seqs, width):
    out = np.full((len(seqs), width), -1, dtype=np.int64)
    for b, s in enumerate(seqs):
        out[b, :len(s)] = s.numpy().astype(np.int64)
    return out, np.array([len(s) for s in seqs], dtype=np.int64)


def cases(rng):
    c = {}
    c["basic"] = (log_softmax_rows(rng, 12, 3, 5), [[1, 1, 2, 3], [2, 3, 3, 0], [4, 1, 0, 0]], [12, 9, 7], [4, 3, 2], 0)
    c["empty"] = (log_softmax_rows(rng, 6, 2, 4), [[0, 0], [3, 1]], [6, 5], [0, 2], 0)
    c["one_frame"] = (log_softmax_rows(rng, 5, 4, 4), [[2, 0], [0, 0], [1, 3], [3, 3]], [1, 1, 1, 5], [1, 0, 2, 2], 0)
    # sequence 0 needs L + repeats = 4 frames and has 3; sequence 1 has exactly the 4 it needs
    c["infeasible"] = (log_softmax_rows(rng, 8, 2, 4), [[1, 1, 2], [1, 1, 2]], [3, 4], [3, 3], 0)
    lp = log_softmax_rows(rng, 10, 3, 5)
    lp[:, :, 2] = -np.inf       # a class that never occurs: sequence 0 asks for it
    lp[3:5, 1, 1] = -np.inf     # and one that is impossible in two frames of sequence 1
    c["neginf"] = (lp, [[1, 2, 3], [1, 4, 1], [3, 4, 4]], [10, 10, 8], [3, 3, 3], 0)
    c["blank3"] = (log_softmax_rows(rng, 11, 2, 5), [[0, 4, 4, 1], [2, 0, 1, 1]], [11, 9], [4, 3], 3)
    c["blank_label"] = (log_softmax_rows(rng, 10, 2, 4), [[1, 0, 2], [0, 0, 3]], [10, 9], [3, 3], 0)
    tg = rng.integers(1, 8, (2, 30))
    tg[0, 5] = tg[0, 4]
    tg[1, 11] = tg[1, 10]
    c["long"] = (log_softmax_rows(rng, 200, 2, 8), tg.tolist(), [200, 173], [30, 26], 0)
    return c


def main():
    sys.path.insert(0, sys.argv[1])
    import pytorch_hmm.alignment.ctc as ref
    rng = np.random.default_rng(23)
    for name, (lp, targets, il, tl, blank) in cases(rng).items():
        lp = np.asarray(lp, dtype=np.float32)
        targets, il, tl = (np.asarray(a, dtype=np.int64) for a in (targets, il, tl))
        T, B, C = lp.shape
        tlp, ttg, til, ttl = (torch.from_numpy(a) for a in (lp, targets, il, tl))
        out = {"lp": lp, "targets": targets, "input_lengths": il, "target_lengths": tl, "blank": np.array(blank)}
        out["ref_loglik"] = ref.ctc_forward_algorithm(tlp, ttg, til, ttl, blank).numpy()
        out["ref_beta"] = ref.ctc_backward_algorithm(tlp, ttg, til, ttl, blank).numpy()
        out["ref_expand"] = ref.expand_targets_with_blank(ttg, blank).numpy()
        out["ref_align"], _ = pad_list(ref.ctc_alignment_path(tlp, ttg, til, ttl, blank), T)
        aligner = ref.CTCAligner(C, blank_id=blank)
        greedy = aligner.decode(tlp, til)
        out["ref_greedy"], out["ref_greedy_len"] = pad_list(greedy, T)
        beam = aligner.decode(tlp, til, beam_width=4)
        out["ref_beam_equal"] = np.array(all(torch.equal(g, h) for g, h in zip(greedy, beam)))
        seq = torch.argmax(tlp[:il[0], 0], dim=1)
        out["seq"] = seq.numpy()
        out["ref_collapse"] = ref.collapse_repeated_tokens(seq).numpy()
        out["ref_remove"] = ref.remove_ctc_blanks(seq, blank).numpy()
        out["ref_decode"] = ref.ctc_decode_sequence(seq, blank).numpy()
        A, ll = cn.alpha(lp, targets, il, tl, blank, np.float64)
        out["alpha64"], out["loglik64"] = A, ll
        out["beta64"] = cn.beta(lp, targets, il, tl, blank, np.float64)
        out["gamma64"], out["grad64"] = cn.occupancy(lp, targets, il, tl, blank, np.float64)
        np.savez_compressed(os.path.join(HERE, f"ctc_{name}.npz"), **out)

    # segmentation: fixed cuts and a proportional share of the transcript
    lp = log_softmax_rows(rng, 2300, 1, 3)[:, 0]
    transcript = rng.integers(1, 3, 60)
    seg = ref.CTCSegmentationAligner(3, min_segment_length=50, max_segment_length=700)
    auto = seg.segment_and_align(torch.from_numpy(lp), torch.from_numpy(transcript))
    given = seg.segment_and_align(torch.from_numpy(lp), torch.from_numpy(transcript), torch.tensor([30, 90, 100, 2000]))
    out = {"lp": lp, "transcript": transcript}
    for tag, segs in (("auto", auto), ("given", given)):
        out[tag + "_start"] = np.array([int(s[2]) for s in segs], dtype=np.int64)
        out[tag + "_end"] = np.array([int(s[3]) for s in segs], dtype=np.int64)
        out[tag + "_text_len"] = np.array([len(s[1]) for s in segs], dtype=np.int64)
        out[tag + "_text"] = np.concatenate([s[1].numpy() for s in segs] + [np.zeros(0, dtype=np.int64)])
        assert all(torch.equal(s[0], torch.from_numpy(lp)[int(s[2]):int(s[3])]) for s in segs)
    np.savez_compressed(os.path.join(HERE, "ctc_segment.npz"), **out)


if __name__ == "__main__":
    main()
