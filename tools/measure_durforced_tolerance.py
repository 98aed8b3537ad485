"""The allowances of tests/test_gpu_durforced.py, measured: the numpy model of explicit-duration
forced alignment in float32 (tables kept the way the kernels keep them) against the same model in
float64, over exactly the cases of that file.  CPU only.

    python tools/measure_durforced_tolerance.py [--quick]

Prints the largest error per quantity with the case it came from, once over the calls of at most
T_CAP frames and once over the longer ones (chains longer than T_CAP need that many frames, and an
fp32 table's rounding grows with its values): the tables for the test file's docstring and its
MEASURED / MEASURED_LONG lines.  --quick takes every fourth case (a smoke run of the tool).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import durforced_numpy as M  # noqa: E402
import test_gpu_durforced as G  # noqa: E402

ROWS = (("loglik_abs", "loglik       absolute"), ("loglik_rel", "loglik       relative to max(|.|, 1)"),
        ("gamma_abs", "gamma        absolute"), ("gamma_row", "gamma        |row sum - 1|"),
        ("grad_lp_abs", "grad_lp      absolute"), ("dur_abs", "dur_post     absolute"),
        ("dur_rel", "dur_post     relative (>= floor)"), ("dur_row", "dur_post     |row sum - 1|"),
        ("layer_grad_rel", "aligner logit gradient, relative to its max-norm"))


def main():
    quick = "--quick" in sys.argv
    worst = {k: (0.0, "-") for k, _ in ROWS}   # calls of at most T_CAP frames
    worst_long = {k: v for k, v in worst.items() if k != "layer_grad_rel"}   # the longer ones (Lmax above T_CAP)
    n = [0, 0]
    for i, (name, *case) in enumerate(G.all_cases()):
        if quick and i % 4:
            continue
        ref = M.model(*case, viterbi=False)
        low = M.model(*case, dtype=np.float32, viterbi=False)
        assert np.array_equal(np.isfinite(ref["loglik"]), np.isfinite(low["loglik"])), name
        long = case[0].shape[1] > G.T_CAP
        w = worst_long if long else worst
        for k, v in G.errors(low, ref, case[2], case[3]).items():
            if v > w[k][0]:
                w[k] = (v, name)
        n[long] += 1
    lp, tokens, il, tl, logits = G.aligner_case()
    case = (lp, tokens.astype(np.int32), il, tl, G.aligner_dur_lp(tokens, logits))
    g64 = G.aligner_logit_grad(M.model(*case, viterbi=False)["dur_post"], tokens, tl, logits)
    g32 = G.aligner_logit_grad(M.model(*case, dtype=np.float32, viterbi=False)["dur_post"], tokens, tl, logits)
    worst["layer_grad_rel"] = (float(np.abs(g32 - g64).max() / np.abs(g64).max()), "aligner")
    for title, w, var in ((f"T <= {G.T_CAP}: {n[0]} calls", worst, "MEASURED"),
                          (f"T > {G.T_CAP}: {n[1]} calls", worst_long, "MEASURED_LONG")):
        print(f"    quantity, {title:<38s} fp32 model, largest                    allowance (8x)")
        for k, label in ROWS:
            if k in w:
                v, name = w[k]
                print(f"    {label:<48s} {v:.3e}  ({name})".ljust(92) + f"{G.FACTOR * v:.2e}")
        print(var + " = dict(" + ", ".join(f"{k}={w[k][0]:.3e}" for k, _ in ROWS if k in w) + ")")


if __name__ == "__main__":
    main()
