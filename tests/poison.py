"""Poisoned allocations: a harness for the two promises every launcher makes about the memory
ops.py hands it.

ops.py allocates every output and every workspace with torch.empty, so a launcher runs on memory
whose earlier contents are unknown.  It must (1) never read a byte of its workspace or outputs
before writing it and (2) write every element of every output it was asked for.  `poisoned(pattern)`
makes the unknown contents known: for its duration torch.empty and torch.empty_like fill what they
return, byte-wise, with one of three patterns.  An op that keeps both promises returns the same
bytes under every pattern; an element that changes with the pattern was never written, an output
that changes everywhere was computed from a read before a write.

    with poisoned("ff") as record:
        outs = op(*inputs)
    assert all(same_bytes(a, b) for a, b in zip(outs, clean_outs))
    assert covers(record, outs, workspace_bytes)

Importable without a GPU (test_poison_cpu.py runs it on toy CPU ops).
"""
import contextlib
from collections import namedtuple

import torch

PATTERNS = ("zero", "ff", "one")   # the order the tests run them in
_ONE = 0x3F800000                  # fp32 1.0; a large positive int32
_ONE_BYTES = (0x00, 0x00, 0x80, 0x3F)
_REAL_EMPTY = torch.empty          # (_fill runs while the module's torch.empty is the patched one)

Allocation = namedtuple("Allocation", "data_ptr nbytes dtype")


def default_device() -> str:
    return "cuda" if torch.cuda.is_available() else "cpu"


def _fill(t: torch.Tensor, pattern: str) -> None:
    """Fills the whole (freshly made, so exclusively owned) storage of t, on the current stream."""
    raw = _REAL_EMPTY(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    n = raw.numel()
    if n == 0:
        return
    if pattern == "zero":
        raw.fill_(0x00)
    elif pattern == "ff":
        raw.fill_(0xFF)
    elif pattern == "one":
        n4 = n // 4 * 4
        if n4:
            raw[:n4].view(torch.int32).fill_(_ONE)
        for i in range(n4, n):
            raw[i] = _ONE_BYTES[i - n4]
    else:
        raise ValueError(f"unknown poison pattern {pattern!r}; expected one of {PATTERNS}")


@contextlib.contextmanager
def poisoned(pattern: str, device=None):
    """Replaces torch.empty and torch.empty_like on the torch module; restores them in a finally.
    Every tensor they return on `device` (a device type; default: cuda where there is one) is filled
    with `pattern` before it is handed out and recorded as an Allocation(data_ptr, nbytes, dtype) in
    the list this yields.  The patch reaches functools.partial(torch.empty, ...) objects made while
    it holds and the bodies of torch.library.custom_op functions, which look torch.empty up per call."""
    if pattern not in PATTERNS:
        raise ValueError(f"unknown poison pattern {pattern!r}; expected one of {PATTERNS}")
    kind = torch.device(default_device() if device is None else device).type
    real_empty, real_empty_like = torch.empty, torch.empty_like
    record = []

    def hand_out(t):
        if isinstance(t, torch.Tensor) and t.device.type == kind and not t.is_meta:
            with torch.no_grad():
                _fill(t, pattern)
            record.append(Allocation(t.data_ptr(), t.untyped_storage().nbytes(), t.dtype))
        return t

    def empty(*args, **kwargs):
        return hand_out(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return hand_out(real_empty_like(*args, **kwargs))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield record
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


def _bytes_of(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bytes(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal shape, dtype and bytes (a uint8 view: NaN equals the same NaN, -0.0 differs from 0.0)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return bool(torch.equal(_bytes_of(a), _bytes_of(b)))


def first_difference(a: torch.Tensor, b: torch.Tensor) -> str:
    """Where two tensors of one shape differ, for an assertion's message."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"{tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    width = a.element_size()
    diff = (_bytes_of(a) != _bytes_of(b)).reshape(-1, width).any(1).nonzero().reshape(-1)
    if diff.numel() == 0:
        return "no difference"
    i = int(diff[0])
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), a.shape)) if a.dim() else ()
    fa, fb = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return (f"{diff.numel()} of {a.numel()} elements differ, first at {idx}: "
            f"{fa[i].item()!r} vs {fb[i].item()!r}")


def covers(record, outputs, min_workspace_bytes: int = 0) -> bool:
    """The vacuity guard: True when every non-empty tensor of `outputs` lies inside an allocation of
    `record`, and (with a size query's answer in min_workspace_bytes) the record holds an allocation
    of at least that many bytes.  An op that allocates elsewhere -- torch.zeros, new_empty, the native
    library -- fails it, instead of passing the poison test emptily."""
    for t in outputs:
        if not isinstance(t, torch.Tensor) or t.numel() == 0:
            continue
        lo = t.data_ptr()
        hi = lo + t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()
        if not any(a.data_ptr <= lo and hi <= a.data_ptr + a.nbytes for a in record):
            return False
    if min_workspace_bytes > 0 and not any(a.nbytes >= min_workspace_bytes for a in record):
        return False
    return True


def check_four(call, min_workspace_bytes: int = 0, compare=None, device=None, guard=True):
    """The poison test of one launch form.  call() runs the op on fresh copies of one set of inputs
    and returns the tuple of tensors to compare (outputs, then arguments it updated in place).  It is
    run unpatched, then under zero, ff and one; every tensor must have the same bytes in all four,
    and every poisoned run must pass covers().  compare: the indices to compare and guard (default
    all) -- for an output that is a workspace handed to another library call, leave it out and put
    what its consumer produces into the tuple instead.  guard: the indices covers() is asked about
    (True: the compared ones; False: none, only the workspace size) -- out of it stay the caller's own
    tensors that an op updates in place and autograd's copies, which are not the op's allocations."""
    def run():
        outs = call()
        outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
        if outs and outs[0].is_cuda:
            torch.cuda.synchronize()
        return outs

    clean = run()
    pick = range(len(clean)) if compare is None else compare
    guarded = pick if guard is True else (() if guard is False else guard)
    for pattern in PATTERNS:
        with poisoned(pattern, device) as record:
            outs = run()
        assert len(outs) == len(clean)
        assert record, f"{pattern}: no allocation went through torch.empty"
        for i in pick:
            assert same_bytes(outs[i], clean[i]), (
                f"output {i} under poison '{pattern}' differs from the unpatched call: "
                f"{first_difference(outs[i], clean[i])}")
        assert covers(record, [outs[i] for i in guarded], min_workspace_bytes), (
            f"{pattern}: an output or the workspace ({min_workspace_bytes} bytes) was not allocated "
            f"through torch.empty: {[(tuple(outs[i].shape), outs[i].dtype) for i in guarded]} vs {record}")
    return clean
