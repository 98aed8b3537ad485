"""Every custom op of pytorch_hmm_amd.ops against its own fake implementation on the GPU: the real
outputs and the fake ones agree in shape, dtype and device, for every on/off combination of the
optional outputs, for float64 inputs (which the real op converts) and for an empty batch.  Nothing
here looks at a value; the ops' own suites do.  Inputs: ops_fake_cases.py."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode
from torch.utils._pytree import tree_map

import ops_fake_cases as cases

pytestmark = pytest.mark.gpu


def _meta(out):
    out = (out,) if isinstance(out, torch.Tensor) else tuple(out)
    return [(tuple(o.shape), o.dtype, o.device) for o in out]


def _real_and_fake(variant, fdtype, on, nb=cases.B):
    op, args, kwargs = cases.call(variant, fdtype, torch.device("cuda", 0), on, nb)
    real = _meta(op(*args, **kwargs))
    with FakeTensorMode() as mode:
        fake = lambda a: mode.from_tensor(a) if isinstance(a, torch.Tensor) else a
        faked = _meta(op(*tree_map(fake, args), **tree_map(fake, kwargs)))
    return real, faked


@pytest.mark.parametrize("variant", sorted(cases.SWITCHES))
def test_fake_matches_real(variant):
    for on in cases.combos(variant):
        if (variant, on) in cases.REFUSED:
            continue
        real, faked = _real_and_fake(variant, torch.float32, on)
        assert real == faked, f"{variant} with {sorted(on)} on"
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", sorted(cases.SWITCHES))
def test_fake_matches_real_float64_inputs(variant):
    real, faked = _real_and_fake(variant, torch.float64, frozenset(cases.SWITCHES[variant]))
    assert real == faked
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", cases.EMPTY_BATCH)
def test_fake_matches_real_empty_batch(variant):
    for on in cases.combos(variant):
        real, faked = _real_and_fake(variant, torch.float32, on, nb=0)
        assert real == faked, f"{variant} with {sorted(on)} on"
        assert all(shape[0] == 0 for shape, _, _ in real)
