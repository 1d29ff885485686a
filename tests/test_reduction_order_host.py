"""The emulation of the device's summation order (tests/reduction_order.py), no GPU: on every case the GPU test holds the kernels to,
it agrees with the order-free fp64 restatements - tests/align_reference.py, the tile reference of tests/test_gpu_tiles.py, the host's
least-squares sums (marigold_amd/evaluation/alignment.py) - within their self-difference bound of 1e-11: it differs from them in the
order of the sums and in nothing else.  And the rule csrc/reduce.h states for itself: whoever includes it is built with contraction off."""
import os
import re

import numpy as np

from tests import reduction_order as R
from tests.align_reference import align_fit_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELF = 1e-11


def _rel(got, want):
    return abs(got - want) / max(1.0, abs(want))


def test_the_butterfly_and_the_combines_on_exact_integers():
    v = np.arange(64, dtype=np.float64)[:, None] * np.array([1.0, 3.0])
    assert np.array_equal(R.butterfly(v), np.broadcast_to([2016.0, 6048.0], (64, 2)))
    acc = np.arange(256 * 2, dtype=np.float64).reshape(1, 256, 2)
    assert np.array_equal(R.block_sum(acc), acc.sum(axis=1))
    table = np.arange(131 * 3, dtype=np.float64).reshape(131, 3)
    assert np.array_equal(R.rows_sum(table), table.sum(axis=0)) and np.array_equal(R.lane_rows_sum(table), table.sum(axis=0))


def test_the_order_is_not_numpys():
    """what the bit test is for: on the largest case the device's order and numpy's pairwise order give different bits"""
    d, ref, mask, _ = next(c for c in R.align_cases() if len(c[0]) == R.ALIGN_SIZES[-1])
    emu, want = R.align_fit(d, ref, mask, 1), align_fit_reference(d, ref, mask, fit_shift=1, iters=0)
    assert emu[:2] != want[:2] and _rel(emu[0], want[0]) <= SELF


def test_align_emulation_agrees_with_the_restatement():
    cases = R.align_cases()
    assert sorted({len(c[0]) for c in cases}) == list(R.ALIGN_SIZES) and len(cases) == 36
    worst = 0.0
    for d, ref, mask, fit_shift in cases:
        s, t, flag = R.align_fit(d, ref, mask, fit_shift)
        for start in ((1.0, 0.0), "ls"):   # with no weighted solve the start plays no part
            want = align_fit_reference(d, ref, mask, fit_shift=fit_shift, iters=0, start=start)
            what = (len(d), mask is not None, fit_shift, start)
            assert flag == want[2], what
            worst = max(worst, _rel(s, want[0]), _rel(t, want[1]))
            assert _rel(s, want[0]) <= SELF and _rel(t, want[1]) <= SELF, (what, (s, t), want)
    assert sum(1 for c in cases if R.align_fit(*c)[2] == 0) >= 32   # (n = 1 is the degenerate one)
    print(f"[order] align: largest difference to the restatement {worst:.2e}")


def test_tile_emulation_agrees_with_the_restatement():
    import torch
    import torch.nn.functional as F
    from tests.test_gpu_tiles import _fit_restated
    assert [c[0].shape for c in R.tile_cases()] == [(2,) + s for s in R.TILE_SHAPES]
    for tiles, ys, xs, canvas, guide in R.tile_cases():
        assert guide.shape[0] < canvas[0] and guide.shape[1] < canvas[1]
        full = R.guide_on_canvas(guide, canvas)
        # the reference's sampling, as tests/test_gpu_tiles.py takes it: the same samples up to their last bits (values in [0, 1))
        ref_full = F.interpolate(torch.from_numpy(guide).double()[None, None], canvas, mode="bilinear", align_corners=False)[0, 0]
        assert np.abs(full - ref_full.numpy()).max() <= 1e-13
        coef, flags = R.tile_fit(tiles, ys, xs, full)
        want_c, want_f = _fit_restated(torch.from_numpy(tiles), ys, xs, ref_full)
        assert flags.tolist() == want_f.tolist() == [0, 0], tiles.shape
        err = np.abs(coef - want_c) / np.maximum(1.0, np.abs(want_c))
        print(f"[order] tile fit {tiles.shape}: largest difference to the restatement {err.max():.2e}")
        assert err.max() <= SELF, (tiles.shape, coef, want_c)


def test_eval_emulation_agrees_with_the_host_sums():
    from marigold_amd.evaluation.alignment import _nearest_downscale
    seen = set()
    for pred, gt, mask, max_res, disparity in R.eval_cases():
        got = R.eval_depth_ls(pred, gt, mask, max_res, disparity)
        p, g, m = pred, gt, mask != 0
        if max_res is not None:
            factor = float(np.min(max_res / np.array(pred.shape)))
            assert factor < 1
            p, g, m = (_nearest_downscale(a, factor) for a in (p, g, m))
        if disparity:
            m = m & (g > 0) & (p > 0)
            with np.errstate(all="ignore"):
                g = np.float32(1.0) / g
        x, y = p[m].astype(np.float64), g[m].astype(np.float64)
        want = np.array([x.size, x.sum(), y.sum(), x @ x, x @ y])
        assert got[0] == want[0] and x.size > 0
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        assert err.max() <= SELF, (pred.shape, max_res, disparity, got, want)
        seen.add((pred.shape, max_res, disparity))
    assert len(seen) == 6 and {(256, 512), (384, 384), (3, 5), (37, 53)} == {s[0] for s in seen}


def test_every_file_that_includes_reduce_h_is_built_without_contraction():
    csrc = os.path.join(ROOT, "marigold_amd", "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    users = sorted(f[:-4] for f in os.listdir(csrc) if f.endswith((".hip", ".h")) and '#include "reduce.h"' in open(os.path.join(csrc, f)).read())
    assert users == ["align", "evalscore", "lpips", "tiles"]
    for name in users:
        assert re.search(rf"^FLAGS_{name}\s*:=\s*-ffp-contract=off\s*$", makefile, re.M), name
        assert re.search(rf"^\$\(BUILD\)/.*\b{name}\.o\b.*:.*\breduce\.h\b", makefile, re.M), name
        assert "__shfl_xor" not in open(os.path.join(csrc, name + ".hip")).read(), name   # the butterfly is reduce.h's alone
