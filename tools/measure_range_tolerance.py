"""The sparse allowances of tests/test_gpu_range.py, measured: the numpy model of the HMM over an
arc list in float32 (tests/sparse_numpy.py sums, the tables kept the way the kernels keep them)
against the float64 log-space reference (tests/logspace_numpy.py), over the in-range (class A)
cases of tests/range_cases.py up to 256 states.  CPU only.

    python tools/measure_range_tolerance.py

The table of tests/test_gpu_sparse.py was measured on log-likelihoods of a few hundred nats; here
they reach -12000, where one fp32 ulp of the stored loglik is already 1e-3, so the absolute loglik
allowance of that table cannot hold.  Prints the largest error per quantity with its case: the
table of the test file's docstring and its SPARSE_MEASURED line.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logspace_numpy as L  # noqa: E402
import range_cases as R  # noqa: E402
import sparse_numpy as M  # noqa: E402
from measure_sparse_tolerance import FACTOR, ROWS  # noqa: E402


def main():
    worst = {k: (0.0, "-") for k, _ in ROWS}
    n = 0
    for c in R.range_cases():
        if c["cls"] != "A" or c["N"] > 256:
            continue
        ref = L.forward_backward_arcs(c["log_obs"], c["src"], c["dst"], c["log_w"], c["log_p0"], c["lengths"])
        low = M.sums(c["log_obs"], c["src"], c["dst"], c["log_w"], c["log_p0"], c["lengths"], dtype=np.float32)
        case = dict(c, weight=np.ones(c["B"], np.float32))
        for k, v in M.errors(low, ref, case).items():
            if v > worst[k][0]:
                worst[k] = (v, c["name"])
        n += 1
    print(f"    quantity, {n} cases".ljust(53) + "fp32 model, largest                    allowance (8x)")
    for k, label in ROWS:
        v, name = worst[k]
        print(f"    {label:<48s} {v:.3e}  ({name})".ljust(100) + f"{FACTOR * v:.2e}")
    print("SPARSE_MEASURED = dict(" + ", ".join(f"{k}={worst[k][0]:.3e}" for k, _ in ROWS) + ")")


if __name__ == "__main__":
    main()
