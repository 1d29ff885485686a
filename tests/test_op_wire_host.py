"""Every builder of marigold_amd/ops.py, byte for byte, against tests/golden/op_wire.json (tests/op_wire.py; no GPU, no library).
A change to the wire format on purpose regenerates the fixture (``python -m tests.op_wire --write``) and its review sees which ops moved."""
import ctypes
import json

from marigold_amd import _lib as L
from tests import op_wire as OW


def test_builders_give_the_fixtures_bytes():
    with open(OW.FIXTURE) as f:
        want = json.load(f)
    got = OW.built()
    assert ctypes.sizeof(L.MgOp) == 360 and all(len(h) == 720 for h in got.values())
    assert {op.kind for _, op in OW.calls()} == set(L.OP_NAMES), "a kind no call of op_wire.calls() builds"
    assert list(got) == list(want), "the fixture and op_wire.calls() name different calls"
    moved = [label for label in got if got[label] != want[label]]
    assert not moved, f"ops whose bytes differ from the fixture: {moved}"
