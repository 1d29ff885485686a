"""The device I/O stages (MG_OP_RGB_PREP, MG_OP_NORMALS_VIS), the parts that need no GPU: the slots the builders fill (the names against
the header: tests/test_host.py); their contracts through both libraries' dry run; the C entry points; and the host branch of
``_preprocess``, which every input other than a PIL image or a uint8 tensor on a CUDA pipeline still takes."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from marigold_amd import _lib as L, ops, opstats
from marigold_amd.pipeline import MarigoldNormalsPipeline, _MarigoldPipelineBase
from marigold_amd.util.image_util import InterpolationMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "marigold_hip.h")).read()


# ---- the ops -----------------------------------------------------------------------------------------------------------------


def _slots(op):
    return list(op.i), list(op.f), [x or 0 for x in op.p], list(op.l)


def test_builders_fill_the_documented_slots():
    op = ops.rgb_prep(101, 102, 103, Hin=375, Win=1242, Hout=231, Wout=768, mode="bicubic", hwc=True, out16=True, reciprocal=True)
    assert op.kind == L.OP_RGB_PREP
    assert _slots(op) == ([375, 1242, 231, 768, 1, 1, 1, 1] + [0] * 32, [0.0] * 8, [101, 102, 103] + [0] * 13, [0] * 4)
    raw = ops.Raw(op)
    assert (raw.hin, raw.win, raw.hout, raw.wout, raw.mode, raw.hwc, raw.out16, raw.reciprocal, raw.src, raw.dst, raw.tmp) == \
        (375, 1242, 231, 768, 1, 1, 1, 1, 101, 102, 103)
    op = ops.rgb_prep(201, 202, Hin=16, Win=20, hwc=False)   # the CHW layout, the same size, fp32, IEEE division, no temporary
    assert _slots(op) == ([16, 20, 16, 20, 0, 0, 0, 0] + [0] * 32, [0.0] * 8, [201, 202] + [0] * 14, [0] * 4)
    assert [ops.Raw(ops.rgb_prep(1, 2, Hin=4, Win=4, Hout=2, Wout=2, mode=m)).mode for m in ("bilinear", "bicubic", "nearest-exact", 2)] == [0, 1, 2, 2]
    op = ops.normals_vis(301, 302, H=33, W=64)
    assert op.kind == L.OP_NORMALS_VIS
    assert _slots(op) == ([33, 64] + [0] * 38, [0.0] * 8, [301, 302] + [0] * 14, [0] * 4)
    assert (ops.Raw(op).h, ops.Raw(op).w, ops.Raw(op).pred, ops.Raw(op).out) == (33, 64, 301, 302)
    with pytest.raises(AttributeError, match="no field"):
        ops.Raw(op).hwc
    # cost model: one byte per source element, the temporary once each way, the output in its type; 3 x 4 bytes in, 3 bytes out
    assert opstats.op_cost(ops.rgb_prep(1, 2, 3, Hin=375, Win=1242, Hout=231, Wout=768, mode=0)) == \
        ("resize", 0, 3 * (375 * 1242 + 231 * 768 * 4) + 2 * 3 * 375 * 768 * 4)
    assert opstats.op_cost(ops.rgb_prep(1, 2, Hin=768, Win=768, out16=True)) == ("resize", 0, 3 * 768 * 768 * 3)
    assert opstats.op_cost(ops.normals_vis(1, 2, H=768, W=768)) == ("resize", 0, 3 * 768 * 768 * 5)


def test_op_contracts_dry_run_in_both_libraries():
    a = 0x10000   # a fake, aligned device address
    for f16 in (False, True):
        seq = ops.OpSeq("io", f16=f16)
        for hwc in (True, False):
            for out16 in (False, True):
                seq.add(ops.rgb_prep(a, a, Hin=768, Win=768, hwc=hwc, out16=out16))
                seq.add(ops.rgb_prep(a + 1, a + (2 if out16 else 4), Hin=5, Win=7, hwc=hwc, out16=out16))       # unaligned: one pixel per lane
                seq.add(ops.rgb_prep(a, a, a, Hin=375, Win=1242, Hout=231, Wout=768, mode="bicubic", hwc=hwc, out16=out16, reciprocal=True))
                seq.add(ops.rgb_prep(a, a, None, Hin=37, Win=64, Hout=37, Wout=32, mode="bilinear", hwc=hwc, out16=out16))   # one axis: no temporary
                seq.add(ops.rgb_prep(a, a, None, Hin=33, Win=47, Hout=24, Wout=34, mode="nearest-exact", hwc=hwc, out16=out16))
        seq.add(ops.normals_vis(a, a, H=768, W=768))
        seq.add(ops.normals_vis(a + 4, a + 1, H=5, W=7))
        seq.validate()
        for op, msg in ((ops.rgb_prep(a, a, None, Hin=33, Win=47, Hout=24, Wout=34, mode="bilinear"), "temporary"),
                        (ops.rgb_prep(a, a, a + 2, Hin=33, Win=47, Hout=24, Wout=34, mode="bicubic"), "temporary"),
                        (ops.rgb_prep(None, a, Hin=8, Win=8), "null"),
                        (ops.rgb_prep(a, None, Hin=8, Win=8), "null"),
                        (ops.rgb_prep(a, a + 2, Hin=8, Win=8), "aligned"),
                        (ops.rgb_prep(a, a + 1, Hin=8, Win=8, out16=True), "aligned"),
                        (ops.rgb_prep(a, a, Hin=0, Win=8), "bad size"),
                        (ops.rgb_prep(a, a, a, Hin=8, Win=8, Hout=4, Wout=0), "bad size"),
                        (ops.rgb_prep(a, a, a, Hin=8, Win=8, Hout=4, Wout=4, mode=3), "mode"),
                        (ops.normals_vis(None, a, H=8, W=8), "null"),
                        (ops.normals_vis(a, None, H=8, W=8), "null"),
                        (ops.normals_vis(a + 2, a, H=8, W=8), "4-byte aligned"),
                        (ops.normals_vis(a, a, H=8, W=0), "bad size")):
            s = ops.OpSeq("bad", f16=f16)
            s.add(op)
            with pytest.raises(L.MarigoldHipError, match=msg):
                s.validate()


def test_c_entry_points_in_header_binding_and_libraries():
    header = _header()
    assert re.search(r"\bint mg_rgb_prepare\(const uint8_t\* src, int hwc, int Hin, int Win, void\* dst, int out16, int Hout, int Wout, int mode, "
                     r"int reciprocal,\s+float\* tmp_or_null, void\* stream\);", header)
    assert re.search(r"\bint mg_normals_visualize\(const float\* pred, int H, int W, uint8_t\* out_hwc, void\* stream\);", header)
    for name, nargs in (("mg_rgb_prepare", 12), ("mg_normals_visualize", 5)):
        assert name in L.EXPORTS
        for f16 in (False, True):
            assert len(getattr(L.load(f16), name).argtypes) == nargs


def test_device_wrappers_refuse_what_they_cannot_take():
    from marigold_amd.util.image_util import normals_visualization_device, prepare_rgb_device
    with pytest.raises(AssertionError, match="fp32 CUDA"):
        normals_visualization_device(torch.zeros(3, 4, 4))
    with pytest.raises(AssertionError, match="uint8 expected"):
        prepare_rgb_device(torch.zeros(4, 4, 3), None)
    with pytest.raises(ValueError, match="io_dtype"):
        prepare_rgb_device(torch.zeros(4, 4, 3, dtype=torch.uint8), None, io_dtype=torch.float64)
    with pytest.raises(AssertionError, match=r"\[H, W, 3\]"):
        prepare_rgb_device(torch.zeros(3, 4, 4, dtype=torch.uint8), None, hwc=True)


# ---- the host branch stays ---------------------------------------------------------------------------------------------------


def _picture(h, w, seed):
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_host_preprocess_returns_what_it_returned(device):
    """A host pipeline takes the host code for every input; a CUDA pipeline (a stand-in: nothing here touches a GPU) takes it for
    float tensors.  The result is the formula written out."""
    stand_in = SimpleNamespace(device=torch.device(device), io_dtype=torch.float32, device_io_stages=True)
    stand_in._preprocess_device = lambda *a: _MarigoldPipelineBase._preprocess_device(stand_in, *a)
    hwc = _picture(12, 20, 1)
    chw = hwc.permute(2, 0, 1)[None].contiguous()
    want = chw / 255.0 * 2.0 - 1.0
    assert want.dtype == torch.float32 and want.min() == -1.0 and want.max() <= 1.0
    inputs = [chw.float()] + ([Image.fromarray(hwc.numpy()), chw] if device == "cpu" else [])
    for image in inputs:
        rgb_norm, input_size = _MarigoldPipelineBase._preprocess(stand_in, image, 0, InterpolationMode.BILINEAR)
        assert not rgb_norm.is_cuda and rgb_norm.dtype == torch.float32 and torch.equal(rgb_norm, want)
        assert tuple(input_size) == (1, 3, 12, 20)
    # the longer edge already has the processing resolution: no resampling, the host formula
    rgb_norm, input_size = _MarigoldPipelineBase._preprocess(stand_in, chw.float(), 20, InterpolationMode.BICUBIC)
    assert torch.equal(rgb_norm, want) and tuple(input_size) == (1, 3, 12, 20)
    # only PIL images and uint8 [1,3,H,W] tensors are the device stage's
    for image in (chw.float(), chw.to(torch.int16), chw[0], torch.cat([chw, chw])):
        assert _MarigoldPipelineBase._preprocess_device(stand_in, image, 0, InterpolationMode.BILINEAR) is None
    if device == "cpu":   # a host pipeline resamples with torch: uint8 in, rounded uint8 out, then the formula
        rgb_norm, _ = _MarigoldPipelineBase._preprocess(stand_in, chw, 10, InterpolationMode.BILINEAR)
        res = torch.nn.functional.interpolate(chw.float(), size=(6, 10), mode="bilinear", align_corners=False, antialias=True).round().to(torch.uint8)
        assert torch.equal(rgb_norm, res / 255.0 * 2.0 - 1.0)


@pytest.mark.parametrize("device", ["cpu", "cuda"])
def test_float_tensor_out_of_range_still_trips_the_assert(device):
    stand_in = SimpleNamespace(device=torch.device(device), io_dtype=torch.float32, device_io_stages=True)
    stand_in._preprocess_device = lambda *a: _MarigoldPipelineBase._preprocess_device(stand_in, *a)
    ok = _picture(8, 8, 2).permute(2, 0, 1)[None].float()
    for bad in (256.0, -1.0):
        x = ok.clone()
        x[0, 1, 3, 4] = bad
        with pytest.raises(AssertionError):
            _MarigoldPipelineBase._preprocess(stand_in, x, 0, InterpolationMode.BILINEAR)
    _MarigoldPipelineBase._preprocess(stand_in, ok, 0, InterpolationMode.BILINEAR)
    with pytest.raises(TypeError, match="Unknown input type"):
        _MarigoldPipelineBase._preprocess(stand_in, ok.numpy(), 0, InterpolationMode.BILINEAR)
    with pytest.raises(AssertionError, match="Wrong input shape"):
        _MarigoldPipelineBase._preprocess(stand_in, ok[0], 0, InterpolationMode.BILINEAR)


def test_host_normals_prediction_keeps_the_numpy_picture():
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(1, 3, 9, 14, generator=g)
    pred[0, :, 2, 3] = torch.tensor([-1.5, 1.5, 1.0])
    out = MarigoldNormalsPipeline._tail(SimpleNamespace(), pred, None)
    clipped = pred[0].numpy().clip(-1, 1)
    assert np.array_equal(out.normals_np, clipped) and out.uncertainty is None
    assert np.array_equal(np.asarray(out.normals_img), np.moveaxis(((clipped + 1) * 127.5).astype(np.uint8), 0, -1))
    assert tuple(np.asarray(out.normals_img)[2, 3]) == (0, 255, 255)
