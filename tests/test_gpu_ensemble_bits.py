"""Every output bit of csrc/ensemble.hip's selection kernels on a real MI355X against tests/golden/ensemble_bits.json (tests/
ensemble_bits.py: the cases, the inputs and how the fixture is written).

The bound is equality of SHA-256 digests over the raw bytes of the map, the uncertainty and the min / max table: the fixture was
taken from the kernels as they stood before their shared functions were factored out (docs/history/ensemble_one_reduction.md names
the commit), and nothing since is meant to move a bit - not the fp32 mean / std, which the other tests hold to a tolerance, and not
a NaN's payload.  A few hundred launches on maps of 1023 and 1280 elements."""
import json

import pytest

from tests import ensemble_bits as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got():
    import torch
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return B.digests(L.init(0))


@pytest.fixture(scope="module")
def want():
    with open(B.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(want):
    assert list(want) == [c[0] for c in B.cases()]
    for label, op, E, n, red, st, outs, nonfinite, misalign in B.cases():
        names = (["map", "unc"] if outs else []) + ["minmax"] if op == "depth" else ["map"] + (["unc"] if outs else [])
        assert list(want[label]) == names, label


@pytest.mark.parametrize("op", ["depth", "iid"])
def test_every_output_bit(got, want, op):
    moved = [f"{label}:{name}" for label in want if label.startswith(op + "/") for name in want[label] if got[label].get(name) != want[label][name]]
    assert not moved, f"{len(moved)} buffers differ from the fixture: {moved[:20]}"


def test_the_inputs_do_what_they_are_built_for():
    """Ties and copies among the members, and the two planted non-finite values at interior elements of different members."""
    import numpy as np
    x, st = B.inputs(10, 1280, False)
    assert x.min() >= 0.5 and x.max() < 1.5 and np.array_equal(x * 64, np.round(x * 64))
    assert any(np.array_equal(x[i], x[j]) for i in range(10) for j in range(i)) and len({x[e].tobytes() for e in range(10)}) > 3
    assert (0.5 <= st[:10]).all() and (st[:10] < 2).all() and (-0.5 <= st[10:]).all() and (st[10:] < 0.5).all()
    for E in B.NONFINITE_SIZES:
        for n in B.LENGTHS:
            x, _ = B.inputs(E, n, True)
            assert np.isnan(x).sum() == 1 and np.isnan(x[E // 2, n // 3]) and np.isposinf(x).sum() == 1 and np.isposinf(x[E - 1, 2 * n // 3])
