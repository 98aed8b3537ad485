"""The allowances of tests/test_gpu_sparse.py, measured: the numpy model of the HMM over an arc
list in float32 (tables kept the way the kernels keep them) against the same model in float64,
over exactly the cases of that file (tests/sparse_numpy.py sum_cases).  CPU only.

    python tools/measure_sparse_tolerance.py [--quick]

Prints the largest error per quantity with the case it came from: the table for the test file's
docstring and its MEASURED line.  --quick takes every fourth case (a smoke run of the tool).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sparse_numpy as M  # noqa: E402

FACTOR = 8.0
ROWS = (("loglik_abs", "loglik       absolute"), ("loglik_rel", "loglik       relative to max(|.|, 1)"),
        ("gamma_abs", "gamma        absolute"), ("xi_abs", "xi           absolute"),
        ("xi_rel", f"xi           relative (>= {M.COUNT_FLOOR:g})"),
        ("grad_rel", "gradient, relative to its max-norm"))


def main():
    quick = "--quick" in sys.argv
    worst = {k: (0.0, "-") for k, _ in ROWS}
    n = 0
    for i, case in enumerate(M.sum_cases()):
        if quick and i % 4:
            continue
        ref = M.sums(*M.model_args(case), weight=case["weight"])
        low = M.sums(*M.model_args(case), weight=case["weight"], dtype=np.float32)
        assert np.array_equal(np.isfinite(ref["loglik"]), np.isfinite(low["loglik"])), case["name"]
        for k, v in M.errors(low, ref, case).items():
            if v > worst[k][0]:
                worst[k] = (v, case["name"])
        n += 1
    print(f"    quantity, {n} cases".ljust(53) + "fp32 model, largest                    allowance (8x)")
    for k, label in ROWS:
        v, name = worst[k]
        print(f"    {label:<48s} {v:.3e}  ({name})".ljust(92) + f"{FACTOR * v:.2e}")
    print("MEASURED = dict(" + ", ".join(f"{k}={worst[k][0]:.3e}" for k, _ in ROWS) + ")")


if __name__ == "__main__":
    main()
