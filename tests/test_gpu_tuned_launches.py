"""Every (launch form, tile, split-K count) that marigold_amd/tuning/gfx950.json puts into the production programs, run once on
a real MI355X at the table's own N and K and a reduced M (tests/tuned_forms.py: one whole and one ragged row tile), against
float64 from the operands as stored.  The parameter list is ``tuned_forms.classes()`` itself: an entry added to the table is
tested without anyone remembering to.

Per class: outputs pre-filled with NaN (the V^T section with zeros: its padding must stay zero); max|err| <= 1.5e-2 * max|ref|
(2e-2 with the folded LayerNorm, 2e-3 for the fp32 epilogue - the bounds of tests/test_gpu_kernels.py); rmse / rms at most
max(op_reference.RMS_BOUND["igemm"], 1.25 x that of torch's own bf16 chain on the same operands against the same reference);
row statistics within 2e-4 of their scale on three launches in a row (the tickets reset themselves); an explicit split taken as
given and bit-identical on a second launch.  ``MARIGOLD_TUNED_TABLE=<path>`` also writes the table of
docs/history/tuned_launch_parity.md."""
import os

import pytest
import torch

from marigold_amd import ops as O
from tests import op_reference as R
from tests import tuned_forms as TF

pytestmark = pytest.mark.gpu

CLASSES = TF.classes()
YARDSTICK_MARGIN = 1.25    # "fused may lose this much against unfused": tests/test_gpu_fullsize.py, tests/test_gpu_fp16.py
STATS_BOUND = 2e-4         # tests/test_gpu_kernels.py::test_igemm_layernorm_fold


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from marigold_amd import _lib
    _lib.init(0, False)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def table():
    rows = []
    yield rows
    path = os.environ.get("MARIGOLD_TUNED_TABLE")
    if path:
        with open(path, "w") as fh:
            fh.write("| class | output | max err / max ref | rmse / rms | yardstick | ratio |\n|---|---|---|---|---|---|\n" + "\n".join(rows) + "\n")


def _launch(bt):
    from marigold_amd import ops
    ops.launch(bt.op)
    torch.cuda.synchronize()


def _max_bound(cls):
    from marigold_amd import _lib as L
    return 2e-3 if cls.epi == L.EPI_F32 else (2e-2 if cls.ln else R.MAX_REL_BOUND)


@pytest.mark.parametrize("cls", CLASSES, ids=[c.id for c in CLASSES])
def test_tuned_launch(dev, table, cls):
    bt = TF.build(cls, None, dev)
    assert (O.Raw(bt.op).variant, O.Raw(bt.op).splits) == (cls.tile, cls.splits)
    _launch(bt)
    got = {k: v.clone() for k, v in TF.outputs(bt).items()}
    ref, yard = TF.reference(bt), TF.yardstick(bt)
    if "out2_tail" in got:
        assert (got["out2_tail"] == 0).all(), f"{cls.id}: the V^T padding was written"
    failures = []
    for name in ("out", "out2"):
        if name not in ref:
            continue
        assert got[name].shape == ref[name].shape, (name, got[name].shape, ref[name].shape)
        assert torch.isfinite(got[name]).all(), f"{cls.id}: non-finite {name} (NaN pre-fill left, or written)"
        mx, rm = R.metrics(got[name], ref[name])
        _, yr = R.metrics(yard[name], ref[name])
        bound = max(R.RMS_BOUND["igemm"], YARDSTICK_MARGIN * yr)
        print(f"[parity] {cls.id} {name}: max|err|/max|ref|={mx:.3e} rmse/rms={rm:.3e} yardstick={yr:.3e} ratio={rm / max(yr, 1e-30):.3f}")
        table.append(f"| `{cls.id}` | {name} | {mx:.3e} | {rm:.3e} | {yr:.3e} | {rm / max(yr, 1e-30):.3f} |")
        if mx > _max_bound(cls):
            failures.append(f"{name}: max|err|/max|ref| {mx:.3e} > {_max_bound(cls)}")
        if rm > bound:
            failures.append(f"{name}: rmse/rms {rm:.3e} > {bound:.3e} (yardstick {yr:.3e})")
    if cls.stats:
        M = ref["mean"].shape[0]
        for rep in range(3):   # the tickets reset themselves: every launch finalizes again
            if rep:
                bt.t["ln_out"][M * (cls.N // 32):] = float("nan")
                _launch(bt)
            now = TF.outputs(bt)
            for name in ("slots", "mean", "rstd"):
                assert torch.isfinite(now[name]).all(), f"{cls.id}: launch {rep}: non-finite {name}"
                mx, _ = R.metrics(now[name], ref[name])
                print(f"[parity] {cls.id} {name} (launch {rep}): max|err|/max|ref|={mx:.3e}")
                if mx > STATS_BOUND:
                    failures.append(f"{name} (launch {rep}): {mx:.3e} > {STATS_BOUND}")
        assert int(bt.t["ctr"].abs().sum()) == 0, f"{cls.id}: row-block tickets not back at zero"
    if cls.splits > 1:         # the reduce launch has a fixed order
        bt.t["out"].fill_(float("nan"))
        _launch(bt)
        assert torch.equal(TF.outputs(bt)["out"].view(torch.int16), got["out"].view(torch.int16)), f"{cls.id}: split-K result differs between two launches"
    assert not failures, f"{cls.id} ({', '.join(sorted(set(cls.labels)))}): " + "; ".join(failures)
