"""The error of the HSMM forward-backward recursions in float32: the numpy model
(tests/hsmm_fb_numpy.py) in float32 against float64 over exactly the cases of
tests/test_gpu_hsmm_fb.py, the largest figure per quantity.  CPU only.  The GPU tests allow the
kernels 8x these figures; paste the table into the test's docstring and DESIGN.md.

    python tools/measure_hsmm_fb_tolerance.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hsmm_fb_numpy as M  # noqa: E402
import test_gpu_hsmm_fb as C  # noqa: E402


def all_cases():
    for name in C.FIXTURES:
        yield C.fixture_case(name)
    for S, Dm in C.PAIRS:
        yield from C.boundary_cases(S, Dm)
    for make in C.SPECIAL:
        yield make()


def layer_gradient_error():
    """The layer's parameter gradients when the counts come from the float32 model on the float32
    tables, against float64 autograd through the whole layer; relative to each gradient's max-norm."""
    z = np.load(os.path.join(C.GOLDEN, "hsmm_s5.npz"), allow_pickle=True)
    p = C.layer_params64(z)
    x = torch.tensor(np.asarray(z["x"], np.float64), requires_grad=True)
    leaves = list(p.values()) + [x]
    tabs = C.layer_tables64(p, x, 20)
    want = torch.autograd.grad(C.layer_loss64(*tabs), leaves, retain_graph=True)
    m = M.hsmm_fb(*(a.detach().numpy().astype(np.float32) for a in tabs), None, dtype=np.float32)
    B = x.shape[0]
    up = (-torch.tensor(m["gamma"], dtype=torch.float64) / B,
          -torch.tensor(m["dur_counts"].sum(0), dtype=torch.float64) / B,
          -torch.tensor(m["trans_counts"].sum(0), dtype=torch.float64) / B)
    got = torch.autograd.grad(tabs, leaves, grad_outputs=up)
    return max(float((g - w).abs().max() / w.abs().max()) for g, w in zip(got, want))


def main():
    worst = {}
    where = {}
    n = 0
    for case in all_cases():
        name, lp, du, lt, li = case
        ref = C.reference(case)
        got = M.hsmm_fb(lp, du, lt, li, dtype=np.float32)
        e = C.errors(got, ref)
        assert e.pop("ll_inf_ok"), name
        for k, v in e.items():
            if v > worst.get(k, -1.0):
                worst[k], where[k] = v, name
        n += 1
    worst["layer_grad_rel"] = layer_gradient_error()
    where["layer_grad_rel"] = "hsmm_s5 layer"
    for k in worst:
        print(f"{k:16s} {worst[k]:.3e}   x8 = {8 * worst[k]:.2e}   ({where[k]})")
    print(json.dumps({"cases": n, "fp32_model_max_error": worst}))


if __name__ == "__main__":
    main()
