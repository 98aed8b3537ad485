"""bench.py --dump-outputs: the writer (bench.dump_outputs) and the options, on the CPU.

Small arrays are written whole; when a dump would exceed its size limit the large arrays are
cut to the same seeded sample of rows in every run, so two builds can be compared file by file.
"""
import os
import sys

import numpy as np
import torch

import bench


def test_full_and_dump_options_default_off():
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]
        a = bench.parse()
        assert not a.full and a.dump_outputs is None and a.steps == 3
        sys.argv = ["bench.py", "--full", "--dump-outputs", "some/dir"]
        a = bench.parse()
        assert a.full and a.dump_outputs == "some/dir"
    finally:
        sys.argv = argv


def test_dump_small_outputs_whole(tmp_path):
    g = torch.Generator().manual_seed(0)
    post = torch.rand(2, 7, 5, generator=g)
    states = torch.randint(0, 5, (2, 7), generator=g)
    d64 = torch.rand(3, generator=g, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), [("posterior", post), ("states", states), ("lik", d64)])
    assert sorted(os.listdir(tmp_path / "d")) == ["lik.npy", "posterior.npy", "states.npy"]
    p = np.load(tmp_path / "d" / "posterior.npy")
    s = np.load(tmp_path / "d" / "states.npy")
    assert p.dtype == np.float32 and np.array_equal(p, post.numpy())
    assert s.dtype == np.float64 and np.array_equal(s, states.numpy())
    assert np.load(tmp_path / "d" / "lik.npy").dtype == np.float64


def test_dump_large_outputs_sampled_the_same_way(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4096)
    g = torch.Generator().manual_seed(1)
    a = torch.rand(4, 50, 8, generator=g)          # 6400 bytes: above its share
    b = torch.rand(4, 50, 8, generator=g)
    small = torch.arange(100).reshape(4, 25)        # 800 bytes as float64, below its share: whole
    for run in ("r1", "r2"):
        bench.dump_outputs(str(tmp_path / run), [("a", a), ("b", b), ("small", small)])
    out = {n: np.load(tmp_path / "r1" / f"{n}.npy") for n in ("a", "b", "small")}
    assert sum(v.nbytes for v in out.values()) <= 4096
    assert np.array_equal(out["small"], small.numpy())
    assert out["a"].shape == out["b"].shape and out["a"].shape[1] == 8 and 1 <= out["a"].shape[0] < 200
    # the kept rows are rows of the input, in order, and the same rows for both arrays
    rows_a, rows_b = a.reshape(-1, 8).numpy(), b.reshape(-1, 8).numpy()
    idx = [int(np.flatnonzero((rows_a == r).all(axis=1))[0]) for r in out["a"]]
    assert idx == sorted(set(idx))
    assert np.array_equal(out["b"], rows_b[idx])
    for n, v in out.items():
        assert np.array_equal(v, np.load(tmp_path / "r2" / f"{n}.npy"))


def test_flat_tensors_names_by_position():
    t = [torch.zeros(1), torch.ones(2), torch.full((3,), 2.0)]
    named = bench.flat_tensors((t[0], None, (t[1], [t[2]])))
    assert [n for n, _ in named] == ["out0", "out2", "out3"]
    assert all(x is y for (_, x), y in zip(named, t))
