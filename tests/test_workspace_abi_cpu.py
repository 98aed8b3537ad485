"""CPU: every exported workspace-size function, and the ten offsets of hmm355_fb_workspace_layout,
return what tests/golden/workspace_bytes.json recorded (tests/golden/make_golden_workspace.py, at
the commit named in the file): callers size and carve their buffers by these numbers, so a change
of a layout is a change of the ABI.  No GPU and no compute calls."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")))


@pytest.fixture(scope="module")
def L():
    from pytorch_hmm_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from pytorch_hmm_amd import build_native
        build_native.build()
    return ctypes.CDLL(nat.LIB_PATH)


def test_golden_covers_every_size_function():
    csrc = os.path.join(ROOT, "pytorch_hmm_amd", "csrc")
    exported = set()
    for f in os.listdir(csrc):
        exported.update(re.findall(r"^HMM355_API size_t (hmm355_\w+)\(", open(os.path.join(csrc, f)).read(), flags=re.M))
    assert len(exported) == 26 and exported == set(GOLDEN["functions"])
    assert re.fullmatch(r"[0-9a-f]{40}", GOLDEN["commit"])
    for name, rows in GOLDEN["functions"].items():
        assert len(rows) >= 20 and any(r[-1] == 0 for r in rows), name


@pytest.mark.parametrize("name", sorted(GOLDEN["functions"]))
def test_workspace_bytes(L, name):
    rows = GOLDEN["functions"][name]
    f = getattr(L, name)
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * (len(rows[0]) - 1)
    got = [[*r[:-1], f(*r[:-1])] for r in rows]
    assert got == rows


def test_fb_workspace_layout_offsets(L):
    f = L.hmm355_fb_workspace_layout
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert len(GOLDEN["fb_workspace_layout"]) == len(GOLDEN["functions"]["hmm355_fb_workspace_bytes"])
    for b, t, n, rc, *want in GOLDEN["fb_workspace_layout"]:
        off = (ctypes.c_size_t * 10)(*([0] * 10))
        assert (f(b, t, n, off), list(off)) == (rc, want), (b, t, n)
