"""GPU checks of ``mg_guided_upsample`` (csrc/guided.hip) through ``marigold_amd.guided``'s entry point, on both operand libraries:
against the float64 restatement of tests/guided_reference.py over a ladder of sizes, channel counts, radii, sigmas, guide layouts and
guides; the two exact properties (equal sizes and R = 1: the prediction itself; a flat guide and R = 1: bilinear enlargement); the edge
property the feature exists for; and the integrity of the output (canaries, unaligned buffers, repeatability, both libraries).

The TOLERANCE is computed, not chosen: FACTOR x the largest deviation of a float32 CPU evaluation of the restatement from the float64
one over the ladder's cases (values in [0, 1]; ``_tolerance``).  The factor covers the summation order and the device's expf."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd.util.image_util import InterpolationMode, resize

from tests.guided_reference import guided_reference

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
FACTOR = 8
# (h, w) -> (H, W): the issue's ladder, then two of this file's own - a tile grid of several workgroups with ragged edges at a ratio
# above 4, and a reduction whose footprint exceeds what a launch stages in LDS (the kernel then reads its taps from global memory)
LADDER = [((5, 7), (16, 24)), ((8, 8), (64, 64)), ((12, 20), (37, 61)), ((1, 1), (4, 4)), ((3, 40), (24, 320)), ((9, 9), (9, 9)),
          ((16, 16), (8, 12)), ((7, 9), (33, 70)), ((64, 96), (5, 9))]
CHANNELS, RADII, SIGMAS = (1, 3, 6, 16), (1, 2, 3, 4), (0.05, 0.1, 1000.0)
GUIDES = ("random", "step")


def _ids(case):
    (h, w), (H, W) = case
    return f"{h}x{w}-{H}x{W}"


def _guides(kind, hw, HW, seed):
    """-> (guide_lo uint8 [3, h, w], guide_hi uint8 [H, W, 3]): a picture and its antialiased reduction (torch on the CPU), so that some
    taps resemble the pixel and some do not.  "random": smooth blobs plus noise; "step": dark left of the middle column, bright from it."""
    (h, w), (H, W) = hw, HW
    g = torch.Generator().manual_seed(seed)
    if kind == "step":
        hi = torch.zeros(3, H, W)
        hi[:, :, W // 2:] = 255.0
        hi = hi + torch.randint(0, 3, (3, H, W), generator=g) * torch.where(hi > 0, -1.0, 1.0)
    else:
        coarse = torch.rand(1, 3, 3, 4, generator=g) * 255.0
        hi = torch.nn.functional.interpolate(coarse, size=(H, W), mode="nearest")[0] + torch.randn(3, H, W, generator=g) * 6.0
    hi = hi.clamp(0, 255).round()
    lo = hi if (h, w) == (H, W) else torch.nn.functional.interpolate(hi[None], size=(h, w), mode="bilinear", antialias=True)[0].round().clamp(0, 255)
    return lo.to(torch.uint8).numpy(), hi.to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def _case(case_index, guide, radius, sigma):
    """One case of the ladder at 16 channels (fewer channels are its first ones) -> (pred, guide_lo, guide_hi HWC, float64 reference,
    the float32 evaluation's largest deviation from it).  Computed once and shared; nothing changes it."""
    hw, HW = LADDER[case_index]
    seed = 1000 * case_index + 10 * GUIDES.index(guide) + radius
    pred = torch.rand(16, *hw, generator=torch.Generator().manual_seed(seed)).numpy()
    lo, hi = _guides(guide, hw, HW, seed + 1)
    ref = guided_reference(pred, lo, hi, True, radius, sigma, np.float64)
    dev = float(np.abs(guided_reference(pred, lo, hi, True, radius, sigma, np.float32).astype(np.float64) - ref).max())
    for a in (pred, lo, hi, ref):
        a.setflags(write=False)
    return pred, lo, hi, ref, dev


ISSUE_CASES = 7   # the first entries of LADDER


@functools.lru_cache(maxsize=None)
def _tolerance(case_index=0):
    """FACTOR x the largest float32-against-float64 deviation of the restatement: over every case of the issue's ladder for one of its
    sizes (one number for all of them), over the size's own cases for the two sizes this file adds - they are worse conditioned (a
    pixel whose only similar tap has almost no spatial weight: 5e-6 to 9e-6 on the CPU) and must not widen the bound of the others."""
    sizes = range(ISSUE_CASES) if case_index < ISSUE_CASES else (case_index,)
    worst = max(_case(k, guide, R, s)[4] for k in sizes for guide in GUIDES for R in RADII for s in SIGMAS)
    assert 0.0 < worst < 1e-4, worst   # (values in [0, 1] at fp32: 2e-6 on the issue's ladder)
    return FACTOR * worst


def _run(lib, pred, lo, hi, hwc, radius, sigma, out=None):
    """``mg_guided_upsample`` on CUDA tensors -> out [C, H, W]"""
    C, h, w = pred.shape
    H, W = (hi.shape[0], hi.shape[1]) if hwc else (hi.shape[1], hi.shape[2])
    if out is None:
        out = torch.empty((C, H, W), dtype=torch.float32, device=pred.device)
    assert pred.is_contiguous() and lo.is_contiguous() and hi.is_contiguous() and out.is_contiguous()
    L.check(lib.mg_guided_upsample(pred.data_ptr(), C, h, w, lo.data_ptr(), hi.data_ptr(), int(hwc), H, W, radius, sigma, out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "mg_guided_upsample", lib)
    return out


def _cuda(*arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]   # (a copy: the shared cases are read-only)


@LIBS
@pytest.mark.parametrize("case_index", range(len(LADDER)), ids=[_ids(c) for c in LADDER])
def test_against_the_float64_restatement(case_index, f16):
    lib = L.init(0, f16)
    tol = _tolerance(case_index)
    worst = 0.0
    for guide in GUIDES:
        for R in RADII:
            for sigma in SIGMAS:
                pred, lo, hi, ref, _ = _case(case_index, guide, R, sigma)
                pred_d, lo_d, hwc_d = _cuda(pred, lo, hi)
                chw_d = hwc_d.permute(2, 0, 1).contiguous()
                for C in CHANNELS:
                    for hwc in (True, False):
                        out = _run(lib, pred_d[:C].contiguous(), lo_d, hwc_d if hwc else chw_d, hwc, R, sigma).cpu().numpy()
                        err = float(np.abs(out.astype(np.float64) - ref[:C]).max())
                        worst = max(worst, err)
                        assert err <= tol, (LADDER[case_index], guide, R, sigma, C, hwc, err, tol)
    print(f"guided {_ids(LADDER[case_index])}: worst error {worst:.3e}, tolerance {tol:.3e} ({worst / (tol / FACTOR):.2f} x the float32 evaluation's deviation)")


@LIBS
def test_equal_sizes_and_radius_one_return_the_prediction_bit_for_bit(f16):
    lib = L.init(0, f16)
    for (h, w) in ((9, 9), (40, 70)):
        for guide in GUIDES:
            g = torch.Generator().manual_seed(h)
            pred = (torch.rand(6, h, w, generator=g) * 3.0 - 1.0).cuda()
            lo, hi = _guides(guide, (h, w), (h, w), 5)
            # the guides need not agree: the only tap of non-zero spatial weight is the pixel itself, whatever its range weight
            lo2 = np.ascontiguousarray(lo[:, ::-1, :])
            for lo_used in (lo, lo2):
                lo_d, hi_d = _cuda(lo_used, hi)
                for sigma in SIGMAS:
                    out = _run(lib, pred, lo_d, hi_d, True, 1, sigma)
                    assert torch.equal(out, pred), (h, w, guide, sigma)


@LIBS
def test_a_flat_guide_and_radius_one_give_the_bilinear_enlargement(f16):
    lib = L.init(0, f16)
    tol = _tolerance()
    for (hw, HW) in LADDER[:5] + LADDER[7:8]:
        pred = torch.rand(3, *hw, generator=torch.Generator().manual_seed(hw[0])).cuda()
        lo = torch.full((3,) + hw, 77, dtype=torch.uint8).cuda()
        hi = torch.full(HW + (3,), 77, dtype=torch.uint8).cuda()
        out = _run(lib, pred, lo, hi, True, 1, 0.1)
        want = resize(pred, HW, InterpolationMode.BILINEAR, antialias=True)
        err = float((out - want).abs().max())
        print(f"flat guide {hw} -> {HW}: {err:.3e} from resize, tolerance {tol:.3e}")
        assert err <= tol, (hw, HW, err, tol)


@LIBS
def test_the_enlargement_keeps_a_step_of_the_picture_sharp(f16):
    """guide_lo 8 x 8: 0 left of column 4, 255 from it; guide_hi 64 x 64 steps at column 32; pred 0.2 | 0.9; sigma 0.05.  A cross-edge tap
    carries at most the floor 1e-4 relative to a same-side tap of at least equal spatial weight, so every output pixel stays within
    1e-3 x 0.7 of its side's value (the CPU restatement gives 8e-5 to 9e-5 of the step); bilinear puts 0.44 of the step there."""
    lib = L.init(0, f16)
    lo = torch.zeros(3, 8, 8, dtype=torch.uint8)
    lo[:, :, 4:] = 255
    hi = torch.zeros(64, 64, 3, dtype=torch.uint8)
    hi[:, 32:] = 255
    pred = torch.full((1, 8, 8), 0.2)
    pred[:, :, 4:] = 0.9
    for R in (1, 2):
        out = _run(lib, pred.cuda(), lo.cuda(), hi.cuda(), True, R, 0.05)[0].cpu()
        left, right = float((out[:, :32] - 0.2).abs().max()), float((out[:, 32:] - 0.9).abs().max())
        print(f"edge R = {R}: {left / 0.7:.3e} and {right / 0.7:.3e} of the step")
        assert left <= 1e-3 * 0.7 and right <= 1e-3 * 0.7, (R, left, right)
    blurred = resize(pred.cuda(), (64, 64), InterpolationMode.BILINEAR, antialias=True)[0].cpu()
    assert float((blurred[:, :32] - 0.2).abs().max()) > 0.4 * 0.7   # what the feature is for


def test_output_integrity():
    """Canaries either side of ``out`` survive; ``out`` and ``pred`` one float off a 16-byte boundary give the same values; two runs and
    the two libraries agree bit for bit."""
    libs = [L.init(0, False), L.init(0, True)]
    for case_index, C, R in ((2, 3, 2), (7, 16, 4), (4, 1, 3), (8, 6, 2)):
        pred, lo, hi, _, _ = _case(case_index, "random", R, 0.1)
        (H, W) = LADDER[case_index][1]
        pred_d, lo_d, hi_d = _cuda(pred[:C], lo, hi)
        first = _run(libs[0], pred_d, lo_d, hi_d, True, R, 0.1)
        for lib in libs:
            assert torch.equal(_run(lib, pred_d, lo_d, hi_d, True, R, 0.1), first), (case_index, "runs / libraries differ")
        n = C * H * W
        for shift in (4, 5):   # floats in front of out: 16 bytes on, then one float off
            buf = torch.full((n + 16,), -7.25, dtype=torch.float32, device="cuda")
            src = torch.zeros(pred_d.numel() + 8, dtype=torch.float32, device="cuda")
            src_view = src[shift:shift + pred_d.numel()].view(pred_d.shape)
            src_view.copy_(pred_d)
            assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0   # shift 4: on a 16-byte boundary, 5: one float off
            out = _run(libs[0], src_view, lo_d, hi_d, True, R, 0.1, out=buf[shift:shift + n].view(C, H, W))
            assert torch.equal(out, first), (case_index, shift)
            assert bool((buf[:shift] == -7.25).all()) and bool((buf[shift + n:] == -7.25).all()), (case_index, shift, "a canary changed")


def test_refusals_leave_the_output_alone():
    lib = L.init(0)
    pred, lo, hi, _, _ = _case(0, "random", 2, 0.1)
    pred_d, lo_d, hi_d = _cuda(pred[:1], lo, hi)
    out = torch.full((1, 16, 24), -7.25, device="cuda")
    for radius, sigma in ((0, 0.1), (5, 0.1), (2, 0.0), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(L.MarigoldHipError, match="mg_guided_upsample:"):
            _run(lib, pred_d, lo_d, hi_d, True, radius, sigma, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
    assert ctypes.sizeof(L.MgOp) == 360
