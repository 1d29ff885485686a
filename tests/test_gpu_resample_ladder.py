"""MG_OP_RESIZE (csrc/resize.hip) against torch on the CPU where a separable resampler goes wrong: at a few lengths out of many, and
at the ends of the scale range.  The reference is the host branch of ``marigold_amd.util.image_util.resize`` - what
``test_resize_vs_torch_cpu`` (tests/test_gpu_kernels.py) uses at its six shapes - and the rule is ``tests/resample_accept.py``:
fp32 within 2e-5 on data in [-1, 1], nearest-exact equal, uint8 within one byte and only next to a tie, under 2e-3 of the outputs
of a test.  Every launch writes into a buffer pre-filled so that an element left unwritten fails (NaN; the reference byte +- 128),
and the fp32 temporary between the two passes starts as NaN.

1. ``test_ladder``: every length pair a -> b, a != b, a, b in 1..40, each pass on its own with three rows / columns beside it
   (horizontal [1,1,3,a] -> (3,b), vertical [1,1,a,3] -> (b,3)): window starts and lengths are roundings of
   ``scale * (i + 0.5) +- support + 0.5``, and this is where one of them would be off by one.  1 560 launches per case; the
   results of one ``b`` stay on the device and come back in one copy.
2. ``test_edges_and_extremes``: one axis shrinking while the other grows (six planes: the plane stride of the temporary), lengths
   1 and 2, a 4032 x 3024 photo to 768 (5.25 x, 11 - 22 taps) and a prediction back up (0.19), strips (2 x 6000 -> 2 x 768,
   768 <-> 5 rows), and the ensemble's nearest-exact down-size of three members above ``max_res`` = 1024.

Measured values and run times: docs/history/resample_ladder.md.
"""
import functools

import pytest
import torch

from tests import resample_accept as A

pytestmark = pytest.mark.gpu

MODES = ("bilinear", "bicubic", "nearest-exact")
DTYPES = {"fp32": torch.float32, "uint8": torch.uint8}
LADDER = range(1, 41)
LADDER_SEED = 20


def _random(shape, dtype, g):
    """fp32 in [-1, 1) or every byte value."""
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.rand(shape, generator=g) * 2 - 1


def ladder_inputs(axis, dtype):
    """length a -> the host tensor [1,1,3,a] (axis 'w') or [1,1,a,3] (axis 'h'); one seed per (axis, dtype), the same for every mode."""
    g = torch.Generator().manual_seed(LADDER_SEED + 2 * (axis == "h") + (dtype == torch.uint8))
    return {a: _random((1, 1, 3, a) if axis == "w" else (1, 1, a, 3), dtype, g) for a in LADDER}


def _launch(x, out, mode):
    """One MG_OP_RESIZE from the CUDA tensor ``x`` [..., H, W] into the pre-filled ``out`` [..., h, w]; returns the temporary (kept
    alive by the caller until the stream has run)."""
    from marigold_amd import ops as O
    assert x.is_cuda and out.is_cuda and x.is_contiguous() and out.is_contiguous() and x.dtype == out.dtype
    (Hin, Win), (h, w) = x.shape[-2:], out.shape[-2:]
    planes = x.numel() // (Hin * Win)
    assert out.numel() == planes * h * w and (Hin, Win) != (h, w)
    tmp = None
    if mode != "nearest-exact" and Hin != h and Win != w:
        tmp = torch.full((planes * Hin * w,), float("nan"), dtype=torch.float32, device=x.device)
    O.launch(O.resize(x, out, tmp, planes=planes, Hin=Hin, Win=Win, Hout=h, Wout=w, mode=O.RESIZE_MODES[mode], u8=x.dtype == torch.uint8))
    return tmp


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("axis", ["w", "h"])
@pytest.mark.parametrize("mode", MODES)
def test_ladder(mode, axis, dtype):
    assert torch.cuda.is_available()
    xs = ladder_inputs(axis, DTYPES[dtype])
    dev = {a: x.cuda() for a, x in xs.items()}
    tally = A.Tally(f"ladder {mode} {axis} {dtype}")
    launches = 0
    for b in LADDER:
        size = (3, b) if axis == "w" else (b, 3)
        src = [a for a in LADDER if a != b]
        refs = torch.stack([A.host_resize(xs[a], size, mode) for a in src])   # [39, 1, 1, h, w]
        out = A.prefill(refs).cuda()
        for k, a in enumerate(src):
            _launch(dev[a], out[k], mode)
            launches += 1
        got = out.cpu()
        for k, a in enumerate(src):
            A.accept(got[k], refs[k], xs[a], size, mode, tally, f"{a} -> {b}")
    assert launches == 1560
    tally.close()


@functools.lru_cache(maxsize=None)
def _edge_input(shape, dtype):
    """One input per (shape, type), shared by the three modes."""
    g = torch.Generator().manual_seed(sum(shape) + (dtype == torch.uint8))
    return _random(shape, dtype, g)


BOTH = (torch.float32, torch.uint8)
EDGES = [
    # one axis shrinks, the other grows; six planes with both axes changing
    ((2, 3, 13, 17), (29, 11), BOTH), ((2, 3, 29, 11), (13, 17), BOTH),
    # lengths 1 and 2
    ((1, 1, 1, 1), (7, 9), BOTH), ((1, 2, 7, 9), (1, 1), BOTH), ((1, 1, 2, 2), (1, 3), BOTH), ((1, 1, 1, 64), (5, 64), BOTH),
    # the photo to the processing size, and a prediction back to the photo's
    ((1, 3, 3024, 4032), (576, 768), BOTH), ((1, 1, 576, 768), (3024, 4032), (torch.float32,)),
    # strips: extreme shrink and growth
    ((1, 1, 2, 6000), (2, 768), BOTH), ((1, 1, 768, 2), (5, 2), BOTH), ((1, 1, 5, 2), (768, 2), BOTH),
]
ENSEMBLE_DOWNSIZE = ((3, 1, 1100, 1400), (804, 1024), (torch.float32,))   # nearest-exact only: ensemble members above max_res


@pytest.mark.parametrize("mode", MODES)
def test_edges_and_extremes(mode):
    assert torch.cuda.is_available()
    from marigold_amd.util.image_util import max_res_size
    assert max_res_size(ENSEMBLE_DOWNSIZE[0][-2:], 1024) == ENSEMBLE_DOWNSIZE[1]
    tally = A.Tally(f"edges {mode}")
    for shape, size, dtypes in EDGES + ([ENSEMBLE_DOWNSIZE] if mode == "nearest-exact" else []):
        for dtype in dtypes:
            x = _edge_input(shape, dtype)
            ref = A.host_resize(x, size, mode)
            assert tuple(ref.shape) == shape[:2] + size
            out = A.prefill(ref).cuda()
            tmp = _launch(x.cuda(), out, mode)
            got = out.cpu()
            del tmp
            A.accept(got, ref, x, size, mode, tally, f"{shape} -> {size} {dtype}")
    tally.close()
