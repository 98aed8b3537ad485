"""The poison harness (tests/poison.py) on toy CPU custom ops: it catches an unwritten output
element and a workspace byte folded into a result, passes a correct op, undoes its patch after an
exception, handles every dtype the ops allocate, and its vacuity guard refuses an op that
allocates elsewhere."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import poison  # noqa: E402
from poison import PATTERNS, check_four, covers, poisoned, same_bytes  # noqa: E402


def _mk():
    # as ops._on: a partial over torch.empty made at call time
    return functools.partial(torch.empty, device="cpu")


@torch.library.custom_op("poisontoy::correct", mutates_args=())
def toy_correct(x: torch.Tensor) -> torch.Tensor:
    out = _mk()(x.shape, dtype=torch.float32)
    ws = torch.empty(64, dtype=torch.uint8)
    ws[:] = 3                       # written before it is read
    out.copy_(x * 2 + ws[0].float())
    return out


@torch.library.custom_op("poisontoy::leaves_one", mutates_args=())
def toy_leaves_one(x: torch.Tensor) -> torch.Tensor:
    out = _mk()(x.shape, dtype=torch.float32)
    out[:-1] = x[:-1] * 2           # the last element is never written
    return out


@torch.library.custom_op("poisontoy::reads_workspace", mutates_args=())
def toy_reads_workspace(x: torch.Tensor) -> torch.Tensor:
    out = _mk()(x.shape, dtype=torch.float32)
    ws = torch.empty(64, dtype=torch.uint8)
    out.copy_(x * 2 + ws[5].float())   # a workspace byte nobody wrote
    return out


@torch.library.custom_op("poisontoy::zeros_alloc", mutates_args=())
def toy_zeros_alloc(x: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(x.shape, dtype=torch.float32)
    out[:-1] = x[:-1] * 2
    return out


X = torch.arange(1.0, 8.0)


def test_correct_op_passes():
    clean = check_four(lambda: toy_correct(X), min_workspace_bytes=64, device="cpu")
    assert torch.equal(clean[0], X * 2 + 3)


def test_unwritten_output_element_is_caught():
    with pytest.raises(AssertionError, match="output 0 under poison"):
        check_four(lambda: toy_leaves_one(X), device="cpu")
    # and it is the last element, under each pattern, that shows the poison
    seen = []
    for p in PATTERNS:
        with poisoned(p, "cpu"):
            out = toy_leaves_one(X)
        assert torch.equal(out[:-1], X[:-1] * 2)
        seen.append(out[-1:].clone())
    assert seen[0].item() == 0.0 and torch.isnan(seen[1]).all() and seen[2].item() == 1.0


def test_workspace_byte_in_result_is_caught():
    with pytest.raises(AssertionError, match="output 0 under poison"):
        check_four(lambda: toy_reads_workspace(X), device="cpu")
    outs = []
    for p in PATTERNS:
        with poisoned(p, "cpu"):
            outs.append(toy_reads_workspace(X))
    assert not same_bytes(outs[0], outs[1]) and not same_bytes(outs[1], outs[2])
    assert torch.equal(outs[0], X * 2) and torch.equal(outs[1], X * 2 + 255)


def test_patch_is_undone_after_an_exception():
    real_empty, real_empty_like = torch.empty, torch.empty_like
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned("ff", "cpu"):
            assert torch.empty is not real_empty and torch.empty_like is not real_empty_like
            raise RuntimeError("boom")
    assert torch.empty is real_empty and torch.empty_like is real_empty_like
    with poisoned("zero", "cpu"):
        pass
    assert torch.empty is real_empty and torch.empty_like is real_empty_like
    with pytest.raises(ValueError):
        with poisoned("random", "cpu"):
            pass
    assert torch.empty is real_empty


EXPECT = {  # the value of an element under (zero, ff, one), per dtype
    torch.float32: (0.0, None, 1.0),
    torch.float64: (0.0, None, None),   # (one: 0x3F8000003F800000, checked through its bytes)
    torch.int16: (0, -1, None),
    torch.int32: (0, -1, 0x3F800000),
    torch.int64: (0, -1, 0x3F8000003F800000),
    torch.uint8: (0, 255, None),
}


@pytest.mark.parametrize("dtype", list(EXPECT), ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("shape", [(5,), (3, 7), (0,), (2, 0, 3)], ids=str)
def test_every_dtype_and_zero_size(dtype, shape):
    numel = 1
    for s in shape:
        numel *= s
    for p, want in zip(PATTERNS, EXPECT[dtype]):
        with poisoned(p, "cpu") as record:
            t = torch.empty(shape, dtype=dtype)
            u = torch.empty_like(t)
        assert t.shape == torch.Size(shape) and t.dtype == dtype and u.shape == t.shape and u.dtype == dtype
        assert len(record) == 2
        for r, x in zip(record, (t, u)):
            assert r.data_ptr == x.data_ptr() and r.nbytes == numel * x.element_size() and r.dtype == dtype
        if numel == 0:
            continue
        raw = t.reshape(-1).view(torch.uint8)
        if p == "zero":
            assert bool((raw == 0).all())
        elif p == "ff":
            assert bool((raw == 255).all())
        else:
            word = torch.tensor([0x00, 0x00, 0x80, 0x3F], dtype=torch.uint8)
            assert torch.equal(raw, word.repeat(raw.numel() // 4 + 1)[: raw.numel()])
        assert same_bytes(t, u)
        if want is None and p == "ff":
            assert bool(torch.isnan(t).all())
        elif want is not None and dtype != torch.float64:
            assert bool((t == want).all())


def test_odd_byte_counts_under_one():
    with poisoned("one", "cpu"):
        a = torch.empty(7, dtype=torch.uint8)
        b = torch.empty(3, dtype=torch.int16)
    assert a.tolist() == [0, 0, 0x80, 0x3F, 0, 0, 0x80]
    assert b.tolist() == [0, 0x3F80, 0]


def test_other_devices_and_factories_are_left_alone():
    with poisoned("ff", "cpu") as record:
        m = torch.empty(4, device="meta")
        z = torch.zeros(4)
        n = z.new_empty(4)
    assert m.device.type == "meta" and record == [] and n.shape == (4,)


def test_same_bytes():
    nan = torch.tensor([float("nan"), 1.0])
    assert same_bytes(nan, nan.clone())
    assert not same_bytes(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not same_bytes(torch.zeros(2), torch.zeros(3))
    assert not same_bytes(torch.zeros(2), torch.zeros(2, dtype=torch.float64))
    assert same_bytes(torch.zeros(0), torch.zeros(0))
    assert same_bytes(torch.arange(6).reshape(2, 3).t(), torch.arange(6).reshape(2, 3).t().contiguous())
    assert "first at (1,)" in poison.first_difference(torch.tensor([1, 2]), torch.tensor([1, 3]))


def test_guard_fails_for_torch_zeros():
    with poisoned("zero", "cpu") as record:
        out = toy_zeros_alloc(X)
    assert not covers(record, [out])
    with pytest.raises(AssertionError, match="no allocation went through|not allocated through"):
        check_four(lambda: toy_zeros_alloc(X), device="cpu")


def test_guard_wants_the_workspace():
    with poisoned("zero", "cpu") as record:
        out = toy_correct(X)
    assert covers(record, [out]) and covers(record, [out], 64) and not covers(record, [out], 65)
    assert covers(record, [out[2:5], torch.empty(0)])          # a view of an allocation; an empty tensor
    assert not covers(record, [out, torch.zeros(3)])
