"""Writes tests/golden/workspace_bytes.json: what every exported `size_t hmm355_*_bytes*` function
and hmm355_fb_workspace_layout return over a grid of shapes, with the commit they were recorded at.

    python tests/golden/make_golden_workspace.py        (on a built tree, no GPU)

Run once, at the commit whose layouts are to be pinned; tests/test_workspace_abi_cpu.py then holds
every later commit to the file.  The grid: state counts on both sides of 64, 128 and 256 (the wide
entry points 257 and 4096 too), B in {0, 1, 3}, T in {1, 63, 64, 65, 1025}, every flag or mode that
changes a layout, and for each function shapes it rejects (0 bytes)."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_bytes.json")
PER_FUNCTION = 36

B = [0, 1, 3]
T = [1, 63, 64, 65, 1025]
N = [1, 63, 64, 65, 127, 128, 129, 255, 256]
NW = [1, 64, 256, 257, 4096]           # the wide entry points
OBS = [0, 1]
DUR = [1, 8, 40, 128]
# name -> (the values of each argument, shapes the function rejects)
SPECS = {
    "hmm355_fb_workspace_bytes": ([B, T, N], [(1, 64, 257), (1, 0, 64), (-1, 64, 64)]),
    "hmm355_plan_bytes": ([[1, 2, 3, 17, 32, 63, 64, 65, 100, 127, 128, 129, 192, 200, 250, 255, 256]], [(0,), (257,), (-1,)]),
    "hmm355_viterbi_workspace_bytes": ([B, T, N], [(1, 64, 257), (1, 0, 64)]),
    "hmm355_viterbi_workspace_bytes_ex": ([B, T, N, OBS], [(1, 64, 64, 2), (1, 64, 0, 0)]),
    "hmm355_viterbi_ragged_workspace_bytes": ([B, T, N, OBS], [(1, 64, 257, 0), (-1, 64, 64, 1)]),
    "hmm355_viterbi_nbest_workspace_bytes": ([B, T, N, [1, 2, 4, 5, 8, 16], OBS], [(1, 64, 64, 0, 0), (1, 64, 257, 4, 1)]),
    "hmm355_tv_fb_workspace_bytes": ([B, T, N], [(1, 64, 257), (1, 0, 64)]),
    "hmm355_tv_viterbi_workspace_bytes": ([B, T, N], [(1, 64, 257), (-1, 64, 64)]),
    "hmm355_viterbi_wide_workspace_bytes": ([B, T, NW, OBS], [(1, 64, 4097, 0), (1, 64, 64, 2)]),
    "hmm355_fb_wide_workspace_bytes": ([B, T, NW + [65, 1000]], [(1, 64, 4097), (1, 0, 64)]),
    "hmm355_ffbs_workspace_bytes": ([[1, 2, 3, 17, 32, 63, 64, 65, 100, 127, 128, 129, 192, 200, 250, 255, 256]], [(0,), (257,), (-1,)]),
    "hmm355_gmm_workspace_bytes": ([B, T, [1, 8, 39, 80], [1, 3, 64, 65], [1, 2, 3, 4, 8]], [(1, 64, 0, 3, 1), (1, 64, 8, 3, 257)]),
    "hmm355_gmm_stats_workspace_bytes": ([B, T, [1, 8, 39, 80], [1, 3, 64, 65], [1, 2, 3, 4, 8]], [(1, 64, 0, 3, 1), (1, 64, 8, 3, 257)]),
    "hmm355_hsmm_workspace_bytes": ([B, T, [1, 2, 63, 64, 65, 128, 129, 256], DUR], [(1, 64, 0, 8), (1, 64, 64, 0)]),
    "hmm355_hsmm_workspace_bytes_ex": ([B, T, [1, 2, 63, 64, 65, 128, 129, 256], DUR, [0, 1, 2, 3]], [(1, 64, 0, 8, 0), (1, 64, 64, 8, 4)]),
    "hmm355_semimarkov_workspace_bytes": ([B, T, [1, 2, 63, 64, 65, 128, 129, 256], DUR], [(1, 64, 0, 8), (1, 64, 64, 0)]),
    "hmm355_semimarkov_workspace_bytes_ex": ([B, T, [1, 2, 63, 64, 65, 128, 129, 256], DUR, [0, 1]], [(1, 64, 0, 8, 0), (1, 64, 64, 8, 2)]),
    "hmm355_hsmm_fb_workspace_bytes": ([B, T, [1, 2, 63, 64, 65, 128], DUR, [f | g for f in range(0, 0x100, 0x10) for g in (0, 1)]],
                                       [(1, 64, 64, 129, 0x10), (1, 64, 256, 128, 0x10), (1, 64, 64, 8, 0x2)]),
    "hmm355_durforced_workspace_bytes": ([B, T, [1, 3, 64, 65, 128], DUR, list(range(8))], [(1, 64, 1024, 128, 1), (1, 64, 64, 8, 8)]),
    "hmm355_ctc_workspace_bytes": ([B, T, [1, 31, 32, 127, 128, 2048], list(range(8))], [(1, 64, 2049, 1), (1, 64, 32, 8)]),
    "hmm355_forced_workspace_bytes": ([B, T, [1, 64, 65, 256, 1024, 4096], list(range(8))], [(1, 64, 4097, 1), (1, 64, 64, 16)]),
    "hmm355_dtw_workspace_bytes": ([B, [1, 3, 64, 65, 1025], [1, 3, 64, 65, 1025], [0, 1]], [(1, 0, 64, 0), (1, 64, 64, 2)]),
    "hmm355_sparse_viterbi_workspace_bytes": ([B, T, [1, 64, 65, 256, 257, 4096], [1, 64, 1000, 12288]], [(1, 64, 0, 64), (1, 64, 64, 0)]),
    "hmm355_sparse_forward_backward_workspace_bytes": ([B, T, [1, 64, 65, 256, 257, 4096], [1, 64, 1000, 12288]], [(1, 64, 0, 64), (1, 64, 64, 0)]),
    "hmm355_sparse_arc_counts_workspace_bytes": ([B, T, [1, 64, 65, 256, 257, 4096], [1, 64, 1000, 12288]], [(1, 64, 0, 64), (1, 64, 64, 0)]),
    "hmm355_dchmm_workspace_bytes": ([B, T, [1, 2, 3, 4, 5, 63, 64, 65, 128, 256]], [(1, 0, 64), (1, 64, 0)]),
}


def cases(domains, rejects):
    """PER_FUNCTION tuples spread over the product of the domains (a stride coprime to its size), one
    more for each value the stride missed, then the rejected shapes"""
    total = 1
    for d in domains:
        total *= len(d)
    step = max(1, total // PER_FUNCTION) | 1
    while any(step % p == 0 and total % p == 0 for p in (3, 5, 7, 11, 13)):
        step += 2

    def decode(i):
        out = []
        for d in domains:
            out.append(d[i % len(d)])
            i //= len(d)
        return tuple(out)

    picked = list(dict.fromkeys(decode((i * step) % total) for i in range(min(PER_FUNCTION, total))))
    for j, d in enumerate(domains):
        for v in d:
            if not any(c[j] == v for c in picked):
                picked.append(tuple(v if k == j else dk[len(dk) // 2] for k, dk in enumerate(domains)))
    return picked + [tuple(r) for r in rejects]


def main():
    sys.path.insert(0, ROOT)
    from pytorch_hmm_amd import _native as nat
    lib = ctypes.CDLL(nat.LIB_PATH)
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    functions = {}
    for name, (domains, rejects) in SPECS.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * len(domains)
        rows = [[*c, f(*c)] for c in cases(domains, rejects)]
        assert len(rows) >= 20 and any(r[-1] == 0 for r in rows) and any(r[-1] > 0 for r in rows), name
        functions[name] = rows
    lay = lib.hmm355_fb_workspace_layout
    lay.restype, lay.argtypes = ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p]
    layout = []
    for b, t, n, _ in functions["hmm355_fb_workspace_bytes"]:
        off = (ctypes.c_size_t * 10)(*([0] * 10))
        layout.append([b, t, n, lay(b, t, n, off), *off])
    with open(OUT, "w") as fh:
        fh.write("{\n \"commit\": \"%s\",\n \"functions\": {\n" % commit)
        fh.write(",\n".join("  \"%s\": %s" % (k, json.dumps(v, separators=(",", ":"))) for k, v in functions.items()))
        fh.write("\n },\n \"fb_workspace_layout\": %s\n}\n" % json.dumps(layout, separators=(",", ":")))
    print(OUT, sum(len(v) for v in functions.values()), "tuples,", len(layout), "layouts")


if __name__ == "__main__":
    main()
