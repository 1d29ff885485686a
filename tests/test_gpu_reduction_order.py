"""The order of the fp64 sums of the fit and score kernels, pinned on a real MI355X: the outputs of ``mg_depth_align_fit`` (no weighted
solve), ``mg_tile_fit`` and ``MG_OP_EVAL_DEPTH_LS`` are, BIT FOR BIT, those of the numpy emulation of csrc/reduce.h's order
(tests/reduction_order.py), on both operand libraries.  The other GPU tests of these kernels hold them to order-free restatements
within 1e-9, which a changed summation order passes; this file is what a changed order fails.  The cases - built once, in
tests/reduction_order.py, and checked against the restatements by tests/test_reduction_order_host.py - reach past 64 rows of each
fit's partial table, where the solve's lanes take a second row, and past 512 blocks' worth of pixels in the score."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests import reduction_order as R

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _align_emulated():
    return [R.align_fit(*case) for case in R.align_cases()]


@LIBS
def test_align_fit_without_weights_gives_the_emulations_bits(f16):
    lib, cases, want = _lib(f16), R.align_cases(), _align_emulated()
    modes = ((L.ALIGN_START_GIVEN, "given"), (L.ALIGN_START_LS, "ls"))   # iters = 0: one unweighted solve either way
    coef = torch.full((len(cases), 2, 2), float("nan"), dtype=torch.float64, device="cuda")
    flag = torch.full((len(cases), 2), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mg_depth_align_workspace_bytes(max(R.ALIGN_SIZES)), dtype=torch.uint8, device="cuda")
    uploaded = {}
    for i, (d, ref, mask, fit_shift) in enumerate(cases):
        if id(d) not in uploaded:
            uploaded[id(d)] = (_dev(d), _dev(ref), _dev(mask))
        dd, rr, mm = uploaded[id(d)]
        for j, (mode, _) in enumerate(modes):
            rc = lib.mg_depth_align_fit(dd.data_ptr(), rr.data_ptr(), None if mm is None else mm.data_ptr(), dd.numel(), fit_shift, 0, mode, 1.0, 0.0,
                                        0.05, coef[i, j].data_ptr(), flag[i, j:j + 1].data_ptr(), ws.data_ptr(), ws.numel(), None)
            assert rc == 0, lib.mg_last_error().decode()
    torch.cuda.synchronize()
    coef, flag = coef.cpu().numpy(), flag.cpu().numpy()
    fits = 0
    for i, (d, ref, mask, fit_shift) in enumerate(cases):
        s, t, bad = want[i]
        for j, (_, name) in enumerate(modes):
            what = (len(d), mask is not None, fit_shift, name)
            assert flag[i, j] == bad, (what, flag[i, j], want[i])
            assert np.array_equal(_bits(coef[i, j]), _bits([s, t])), (what, coef[i, j].tolist(), want[i])
            fits += not bad
    assert fits >= 64   # (every size but n = 1 fits)


@LIBS
def test_tile_fit_gives_the_emulations_bits(f16):
    lib = _lib(f16)
    for tiles, ys, xs, canvas, guide in R.tile_cases():
        n, th, tw = tiles.shape
        want_c, want_f = R.tile_fit(tiles, ys, xs, R.guide_on_canvas(guide, canvas))
        need = lib.mg_tiles_workspace_bytes(n, th, tw)
        assert need == n * -(-th * tw // R.CHUNK) * 40
        d_tiles, d_guide = _dev(tiles), _dev(guide)
        coef = torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
        flags = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        rc = lib.mg_tile_fit(d_tiles.data_ptr(), th, tw, (ctypes.c_int * len(ys))(*ys), len(ys), (ctypes.c_int * len(xs))(*xs), len(xs), canvas[0],
                             canvas[1], d_guide.data_ptr(), guide.shape[0], guide.shape[1], coef.data_ptr(), flags.data_ptr(), ws.data_ptr(), need,
                             None)
        assert rc == 0, lib.mg_last_error().decode()
        torch.cuda.synchronize()
        got_c, got_f = coef.cpu().numpy(), flags.cpu().numpy()
        assert got_f.tolist() == want_f.tolist() == [0] * n, (tiles.shape, got_f)
        assert np.array_equal(_bits(got_c), _bits(want_c)), (tiles.shape, got_c.tolist(), want_c.tolist())


@LIBS
def test_eval_depth_ls_gives_the_emulations_bits(f16):
    from marigold_amd import ops
    lib = _lib(f16)
    for pred, gt, mask, max_res, disparity in R.eval_cases():
        h, w = pred.shape
        want = R.eval_depth_ls(pred, gt, mask, max_res, disparity)
        sums = torch.full((5,), float("nan"), dtype=torch.float64, device="cuda")
        scratch = torch.full((R.EV_BLOCKS * 5,), float("nan"), dtype=torch.float64, device="cuda")
        d_pred, d_gt, d_mask = _dev(pred), _dev(gt), _dev(mask)
        ops.launch(ops.eval_depth_ls(d_pred, d_gt, d_mask, sums, scratch, H=h, W=w, disparity=disparity, max_res=max_res), lib=lib)
        torch.cuda.synchronize()
        got = sums.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), ((h, w), max_res, disparity, got.tolist(), want.tolist())
