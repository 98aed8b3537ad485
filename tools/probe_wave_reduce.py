"""Diagnostic: every form of the banded chains' wave reduction (recur.h wave_red_level,
HMM355_RED_FORM 0 .. 3) on caller-given 64-lane vectors, through the kernel a HMM355_RED_PROBE=1
build exports.  The forms with row_shr triples issue their second and third shift unpadded behind
the first, on the premise that only the register read THROUGH DPP needs the two wait states; this
is the test of that premise on the device.
Build here:           [PROBE_LIB=path] python tools/probe_wave_reduce.py build
Run on the GPU box:   [PROBE_LIB=path] python tools/probe_wave_reduce.py
Vectors: 4096 random ones (all negative, mixed signs, positive over 30 binades) and the extreme
value at each of the 64 lanes (max: 0 among values near -50, and the reverse; sum: 1 among values
near e^-50, and e^-50 among ones).  Max of forms 1 .. 3 must be the bits of form 0 (and of numpy);
every sum must be within 64 * 2^-24 of sum|x| of the fp64 sum.  Exit status 1 on any miss."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.environ.get("PROBE_LIB", os.path.join(HERE, "ablate_libs", "libhmm355_probe.so"))
if sys.argv[1:2] == ["build"]:
    sys.path.insert(0, os.path.dirname(HERE))
    from pytorch_hmm_amd import build_native as bn
    print(bn.build(force=True, defines=["HMM355_RED_PROBE=1"], out=LIB, sources=bn.RECURSION_SOURCES))
    sys.exit(0)
import numpy as np


def vectors():
    rng = np.random.default_rng(11)
    sets = {}
    sets["random negative"] = -60.0 * rng.random((1024, 64))
    sets["random mixed signs"] = rng.standard_normal((1024, 64)) * 10.0
    sets["random positive, 30 binades"] = np.exp2(-30.0 * rng.random((1024, 64)))
    sets["random probabilities"] = rng.random((1024, 64))
    lanes = np.arange(64)
    noise = 1.0 + 1e-3 * rng.random((64, 64))
    hi = np.full((64, 64), -50.0) * noise
    hi[lanes, lanes] = 0.0
    sets["max: 0 at lane k, about -50 elsewhere"] = hi
    lo = -1.0 * noise
    lo[lanes, lanes] = -50.0
    sets["max: -50 at lane k, about -1 elsewhere"] = lo
    one = np.exp(-50.0) * noise
    one[lanes, lanes] = 1.0
    sets["sum: 1 at lane k, about e^-50 elsewhere"] = one
    tiny = noise.copy()
    tiny[lanes, lanes] = np.exp(-50.0)
    sets["sum: e^-50 at lane k, about 1 elsewhere"] = tiny
    return {k: v.astype(np.float32) for k, v in sets.items()}


def main():
    L = ctypes.CDLL(LIB)
    L.hmm355_debug_red_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    bad = 0
    for name, x in vectors().items():
        x = np.ascontiguousarray(x)
        out = np.full((x.shape[0], 8), np.nan, np.float32)
        rc = L.hmm355_debug_red_probe(x.ctypes.data, out.ctypes.data, x.shape[0])
        assert rc == 0, f"hip error {rc}"
        ref_max = x.max(axis=1)
        ref_sum = x.astype(np.float64).sum(axis=1)
        bound = 64 * 2.0 ** -24 * np.abs(x.astype(np.float64)).sum(axis=1)
        line = f"{name:42s} n {x.shape[0]:5d}"
        for f in range(4):
            mdiff = int((out[:, f].view(np.uint32) != out[:, 0].view(np.uint32)).sum())
            ndiff = int((out[:, f].view(np.uint32) != ref_max.view(np.uint32)).sum())
            err = np.abs(out[:, 4 + f].astype(np.float64) - ref_sum) / bound
            sdiff = int((out[:, 4 + f].view(np.uint32) != out[:, 4].view(np.uint32)).sum())
            miss = int((err > 1.0).sum())
            bad += mdiff + ndiff + miss
            line += (f" | form {f}: max != form 0 {mdiff}, != numpy {ndiff}; sum err/bound max {err.max():.3f},"
                     f" misses {miss}, bits != form 0 {sdiff}")
        print(line, flush=True)
    print("PASS" if bad == 0 else f"FAIL: {bad} misses", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
