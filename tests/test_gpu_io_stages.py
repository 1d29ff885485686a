"""The device I/O stages on a real MI355X: MG_OP_RGB_PREP (``prepare_rgb_device``) and MG_OP_NORMALS_VIS
(``normals_visualization_device``), csrc/resize.hip, against the code they replace on a CUDA pipeline, bit for bit, in both library
builds (bf16 and fp16 operands) and for both destination types of each (fp32 and the build's 16-bit type).

Why bit equality is the bound, and against what.
* The normalisation ``x / 255.0 * 2.0 - 1.0`` is three fp32 roundings of a byte value.  torch's HOST kernel divides (IEEE); torch's
  DEVICE kernel for a tensor divided by a scalar multiplies by fp32(1 / 255) instead, and 111 of the 256 byte values end up one ulp
  apart between the two (``test_the_two_torch_chains_differ``).  The op restates either (``reciprocal``), and ``_preprocess`` asks
  for the one the pipeline ran before the stage existed: the host chain for a picture that is not resampled (it never left the
  host), the device chain after a device resample.  So the same-size cases compare with the torch chain on the CPU and the resampled
  cases with the device chain - ``_resize_hip`` on the uint8 CHW tensor, then the torch ops on the device.
* Resampling: the passes are MG_OP_RESIZE's own kernel template, reading the same bytes (from HWC or CHW) and producing the same
  fp32 sums in the same order; the last pass applies the same rounding (and bicubic's clamp) and normalises the byte it would have
  stored.  The same operations in the same order: equality is derived, not measured.
  That equality alone would be the template against itself, so the ``_resize_hip`` bytes of every case are in turn held against
  torch on the CPU (``_resampled_reference``, by the rule of tests/resample_accept.py; docs/history/resample_ladder.md).
* The normals picture: a clip that keeps NaN, two fp32 roundings, a truncation - numpy's element operations restated.  NaN has no
  defined uint8 value; the stage gives 0 (what x86-64 numpy leaves, MG_OP_IID_VIS's convention) and the test asserts that 0 by name.
* Pipelines: the stage changes where the bits are computed, not the bits, so every array and picture of ``pipe(pil_image)`` equals
  that of the host branch.  At ``processing_res=0`` the host branch is reached with the float tensor of the same image.  With a resize a
  float tensor is a different input - it is resampled in fp32, with no rounding to bytes - so there the host branch is the same
  pipeline with ``device_io_stages = False``: the code of the commit before, on the same PIL image.
"""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch
from PIL import Image

from tests import resample_accept as RA

pytestmark = pytest.mark.gpu

MODES = ("bilinear", "bicubic", "nearest-exact")
BUILDS = [(False, torch.float32), (False, torch.bfloat16), (True, torch.float32), (True, torch.float16)]   # (fp16-operand library, dst type)
BUILD_IDS = ["bf16lib-f32", "bf16lib-bf16", "fp16lib-f32", "fp16lib-fp16"]


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {False: L.init(0), True: L.init(0, True)}


def _picture(h, w, seed, kind="random", coarse=1):
    """uint8 [h, w, 3] on the host; ``coarse`` multiplies the checker's block size."""
    if kind == "ramp":      # every byte value, three times over at 16 x 16
        return (torch.arange(h * w * 3) % 256).to(torch.uint8).reshape(h, w, 3)
    if kind == "checker":   # saturated black / white blocks of 5 x 7 pixels: bicubic overshoots on both sides of every edge
        yy, xx = torch.meshgrid(torch.arange(h) // (5 * coarse), torch.arange(w) // (7 * coarse), indexing="ij")
        return (((yy + xx) % 2) * 255).to(torch.uint8)[:, :, None].expand(h, w, 3).contiguous()
    return torch.randint(0, 256, (h, w, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _off_by(t, nbytes):
    """A contiguous copy of the CUDA tensor ``t`` that starts ``nbytes`` bytes past an allocation boundary."""
    n = nbytes // t.element_size()
    flat = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
    flat[n:] = t.flatten()
    v = flat[n:].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == nbytes % 16
    return v


def _prep(libs, f16, dtype, src, hwc, size=None, mode="bilinear", reciprocal=False):
    """One MG_OP_RGB_PREP through the chosen library build: ``src`` uint8 CUDA ([H,W,3] | [3,H,W]) -> [3,h,w] of ``dtype``."""
    from marigold_amd import ops as O
    Hin, Win = src.shape[:2] if hwc else src.shape[-2:]
    h, w = size or (Hin, Win)
    dst = torch.full((3, h, w), float("nan"), dtype=dtype, device="cuda")
    tmp = torch.empty(3 * Hin * w, dtype=torch.float32, device="cuda") if (mode != "nearest-exact" and Hin != h and Win != w) else None
    O.launch(O.rgb_prep(src, dst, tmp, Hin=Hin, Win=Win, Hout=h, Wout=w, mode=mode, hwc=hwc, out16=dtype != torch.float32,
                        reciprocal=reciprocal), lib=libs[f16])
    torch.cuda.synchronize()
    return dst


def test_the_two_torch_chains_differ():
    """What makes ``reciprocal`` necessary (module docstring): torch's device kernel does not divide."""
    x = torch.arange(256, dtype=torch.uint8)
    host, dev = x / 255.0 * 2.0 - 1.0, (x.cuda() / 255.0 * 2.0 - 1.0).cpu()
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(host.numpy(), k / np.float32(255) * np.float32(2) - np.float32(1))
    assert np.array_equal(dev.numpy(), k * (np.float32(1) / np.float32(255)) * np.float32(2) - np.float32(1))
    print(f"[parity] host and device normalisation differ at {int((host != dev).sum())} of 256 byte values")
    assert (host != dev).any() and host.min() == dev.min() == -1.0 and host.max() == dev.max() == 1.0


# ---- 1. MG_OP_RGB_PREP, the same size ----------------------------------------------------------------------------------------

SAME = [(1, 1, "random"), (5, 7, "random"), (16, 20, "random"), (31, 64, "random"), (16, 16, "ramp")]


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("case", SAME, ids=lambda c: f"{c[0]}x{c[1]}{'' if c[2] == 'random' else c[2]}")
def test_rgb_prep_same_size(libs, build, case):
    f16, dtype = build
    h, w, kind = case
    hwc = _picture(h, w, 10 * h + w, kind)
    chw = hwc.permute(2, 0, 1).contiguous()
    if kind == "ramp":
        assert len(torch.unique(hwc)) == 256
    want = (chw / 255.0 * 2.0 - 1.0).to(dtype)                     # the host chain
    want_dev = (chw.cuda() / 255.0 * 2.0 - 1.0).to(dtype).cpu()    # the device chain
    for layout, src in (("hwc", hwc.cuda()), ("chw", chw.cuda())):
        views = [("aligned", src)] + ([("off by one byte", _off_by(src, 1))] if h * w > 1 else [])   # the vector path must refuse the second
        for tag, s in views:
            got = _prep(libs, f16, dtype, s, layout == "hwc").cpu()
            assert torch.equal(got, want), (layout, tag)
            got = _prep(libs, f16, dtype, s, layout == "hwc", reciprocal=True).cpu()
            assert torch.equal(got, want_dev), (layout, tag, "reciprocal")


def test_rgb_prep_wrapper_same_size(libs):
    from marigold_amd.util.image_util import InterpolationMode, prepare_rgb_device
    hwc = _picture(31, 64, 5)
    chw = hwc.permute(2, 0, 1)[None].contiguous()
    want = chw / 255.0 * 2.0 - 1.0
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for image, is_hwc in ((hwc, True), (chw, False), (chw[0].cuda(), False), (hwc.cuda(), True)):
            for size in (None, (31, 64)):
                got = prepare_rgb_device(image, size, InterpolationMode.BICUBIC, dtype, is_hwc, device="cuda:0")
                assert got.is_cuda and got.dtype == dtype and tuple(got.shape) == (1, 3, 31, 64) and got.is_contiguous()
                assert torch.equal(got.cpu(), want.to(dtype))


# ---- 2. MG_OP_RGB_PREP, resampling --------------------------------------------------------------------------------------------

# ((13, 17), (29, 11)): one axis shrinks and the other grows; ((756, 1008), (144, 192)): a 4032 x 3024 photo's 5.25 x down-size to 768,
# a quarter of the size - 11 to 22 taps per output, read from 3-byte pixels in the hwc layout
RESAMPLE = [((33, 47), (24, 34)), ((20, 31), (40, 62)), ((37, 64), (37, 32)), ((375, 1242), (231, 768)), ((13, 17), (29, 11)),
            ((756, 1008), (144, 192))]
ANCHOR = {mode: RA.Tally(f"rgb_prep anchor {mode}") for mode in MODES}   # `_resize_hip`'s bytes against torch on the CPU, per mode


@functools.lru_cache(maxsize=None)
def _resampled_reference(src_hw, dst_hw, mode, kind):
    """(the picture [H,W,3] on the host, today's device chain up to fp32 on the device): computed once per case.  The bytes of the
    chain are themselves held against the host branch of ``resize`` (torch on the CPU) by the rule of tests/resample_accept.py, so
    that equality with them is equality with torch's resampler and not only with the same kernel template; the share of differing
    bytes is counted per mode in ``ANCHOR`` and asserted by ``test_resampled_reference_is_torchs``."""
    from marigold_amd.util.image_util import _resize_hip
    # (a strong down-size averages 5 x 7 blocks to grey: the blocks grow with it, so that edges stay edges and still saturate)
    coarse = max(1, min(src_hw[0] // dst_hw[0], src_hw[1] // dst_hw[1]))
    hwc = _picture(src_hw[0], src_hw[1], src_hw[0] + src_hw[1], kind, coarse)
    chw = hwc.permute(2, 0, 1).contiguous().cuda()
    res = _resize_hip(chw, dst_hw[0], dst_hw[1], mode)
    assert res.dtype == torch.uint8 and tuple(res.shape) == (3,) + dst_hw
    x = chw.cpu()[None]
    RA.accept(res.cpu()[None], RA.host_resize(x, dst_hw, mode), x, dst_hw, mode, ANCHOR[mode], (src_hw, dst_hw, mode, kind))
    return hwc, res, res / 255.0 * 2.0 - 1.0


@pytest.mark.parametrize("build", BUILDS, ids=BUILD_IDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", RESAMPLE, ids=lambda c: f"{c[0][0]}x{c[0][1]}to{c[1][0]}x{c[1][1]}")
def test_rgb_prep_resampled(libs, build, mode, case):
    f16, dtype = build
    src_hw, dst_hw = case
    for kind in ("random", "checker") if mode == "bicubic" else ("random",):
        hwc, res_u8, chain = _resampled_reference(src_hw, dst_hw, mode, kind)
        if kind == "checker" and dst_hw != src_hw:
            assert (res_u8 == 0).any() and (res_u8 == 255).any()   # saturated on both sides: the clamp has work to do
        want = chain.to(dtype)
        want_host = (res_u8.cpu() / 255.0 * 2.0 - 1.0).to(dtype)
        for layout, src in (("hwc", hwc.cuda()), ("chw", hwc.permute(2, 0, 1).contiguous().cuda())):
            got = _prep(libs, f16, dtype, src, layout == "hwc", dst_hw, mode, reciprocal=True)
            assert torch.equal(got, want), (layout, kind)
            got = _prep(libs, f16, dtype, src, layout == "hwc", dst_hw, mode, reciprocal=False)   # the same bytes, the host's rounding
            assert torch.equal(got.cpu(), want_host), (layout, kind, "division")


@pytest.mark.parametrize("mode", MODES)
def test_resampled_reference_is_torchs(mode):
    """Every reference of ``test_rgb_prep_resampled`` is, byte for byte up to ties, what torch computes on the CPU (checked where each
    is made); here: over all of a mode's cases fewer than 2e-3 of the bytes differ."""
    for src_hw, dst_hw in RESAMPLE:
        for kind in ("random", "checker") if mode == "bicubic" else ("random",):
            _resampled_reference(src_hw, dst_hw, mode, kind)
    assert mode == "nearest-exact" or ANCHOR[mode].outputs >= 3 * sum(h * w for _, (h, w) in RESAMPLE)
    ANCHOR[mode].close()


def test_rgb_prep_wrapper_resampled(libs):
    """``prepare_rgb_device`` picks the device chain's rounding by itself when it resamples, for a host picture in either layout."""
    from marigold_amd.util.image_util import InterpolationMode, prepare_rgb_device
    for mode in MODES:
        hwc, _, chain = _resampled_reference((33, 47), (24, 34), mode, "random")
        for image, is_hwc in ((hwc, True), (hwc.permute(2, 0, 1)[None].contiguous(), False)):
            got = prepare_rgb_device(image, (24, 34), InterpolationMode(mode), torch.float32, is_hwc, device="cuda:0")
            assert tuple(got.shape) == (1, 3, 24, 34) and torch.equal(got[0], chain)


# ---- 3. MG_OP_NORMALS_VIS -----------------------------------------------------------------------------------------------------


def _normals_input(h, w, seed):
    x = torch.randn(3, h, w, generator=torch.Generator().manual_seed(seed)) * 0.8   # a good share beyond +-1
    special = [-1.0, 1.0, -1.5, 1.5, 0.0, -0.0, float("nan"), float("inf"), float("-inf")]
    for k in (1, 2, 64, 127, 128, 200, 254, 255):   # (x + 1) * 127.5 within an ulp or three of the integer k
        v = np.float32(k / 127.5 - 1.0)
        lo = hi = v
        special.append(float(v))
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2))
            special += [float(lo), float(hi)]
    assert len(special) <= x.numel()
    x.flatten()[:len(special)] = torch.tensor(special, dtype=torch.float32)
    return x


def _numpy_picture(pred):
    """The three numpy lines of ``MarigoldNormalsPipeline._finish`` on fp32 [3,H,W]; a NaN is replaced by -1 first, i.e. byte 0: the
    convention, stated here and not taken from this machine's numpy."""
    final_pred = np.where(np.isnan(pred), np.float32(-1), pred)
    final_pred = final_pred.clip(-1, 1)
    normals_img = ((final_pred + 1) * 127.5).astype(np.uint8)
    return np.moveaxis(normals_img, 0, -1)


@pytest.mark.parametrize("f16", [False, True], ids=["bf16lib", "fp16lib"])
@pytest.mark.parametrize("shape", [(5, 7), (16, 20), (33, 64)], ids=lambda s: f"3x{s[0]}x{s[1]}")
def test_normals_vis(libs, f16, shape):
    from marigold_amd import ops as O
    h, w = shape
    x = _normals_input(h, w, h)
    want = _numpy_picture(x.numpy())
    dev = x.cuda()
    for tag, src in (("aligned", dev), ("off by four bytes", _off_by(dev, 4))):
        out = torch.full((h, w, 3), 7, dtype=torch.uint8, device="cuda")
        O.launch(O.normals_vis(src, out, H=h, W=w), lib=libs[f16])
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:5])
        nan = np.moveaxis(np.isnan(x.numpy()), 0, -1)
        assert nan.sum() == 1 and (got[nan] == 0).all()                       # NaN -> 0
        flat = np.moveaxis(got, -1, 0).flatten()
        assert list(flat[:6]) == [0, 255, 0, 255, 127, 127] and list(flat[7:9]) == [255, 0]   # -1, 1, -1.5, 1.5, 0, -0; +inf, -inf


def test_normals_vis_wrapper(libs):
    from marigold_amd.util.image_util import normals_visualization_device
    x = _normals_input(33, 64, 9)
    got = normals_visualization_device(x.cuda())
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (33, 64, 3) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), _numpy_picture(x.numpy()))
    planes = torch.zeros(3, 33, 80).cuda()
    planes[:, :, :64] = x.cuda()
    assert torch.equal(normals_visualization_device(planes[:, :, :64]), got)   # a strided view is made contiguous first


# ---- 4. the C entry points ----------------------------------------------------------------------------------------------------


def test_c_entry_points(libs):
    from marigold_amd import _lib as L
    lib = libs[False]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hwc, _, chain = _resampled_reference((33, 47), (24, 34), "bicubic", "checker")
    src = hwc.cuda()
    dst = torch.full((3, 24, 34), float("nan"), device="cuda")
    tmp = torch.empty(3 * 33 * 34, device="cuda")
    L.check(lib.mg_rgb_prepare(src.data_ptr(), 1, 33, 47, dst.data_ptr(), 0, 24, 34, 1, 1, tmp.data_ptr(), stream), "mg_rgb_prepare", lib)
    torch.cuda.synchronize()
    assert torch.equal(dst, chain)
    assert lib.mg_rgb_prepare(src.data_ptr(), 1, 33, 47, dst.data_ptr(), 0, 24, 34, 1, 1, None, stream) != 0   # no temporary: refused
    assert b"temporary" in lib.mg_last_error()
    x = _normals_input(16, 20, 4)
    out = torch.full((16, 20, 3), 7, dtype=torch.uint8, device="cuda")
    xd = x.cuda()
    L.check(lib.mg_normals_visualize(xd.data_ptr(), 16, 20, out.data_ptr(), stream), "mg_normals_visualize", lib)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _numpy_picture(x.numpy()))


# ---- 5. the pipelines ---------------------------------------------------------------------------------------------------------

IID_PROPS = {"target_names": ["albedo", "shading"], "albedo": {"prediction_space": "srgb"},
             "shading": {"prediction_space": "linear", "up_to_scale": True}}


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind):
    """The tiny synthetic model of tests/test_gpu_pipeline.py behind each of the three pipelines."""
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    assert torch.cuda.is_available()
    kw = dict(default_denoising_steps=2, default_processing_resolution=0)
    ucfg = TINY_UNET
    if kind == "iid":
        ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8)
        kw["target_properties"] = IID_PROPS
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, **kw).to("cuda:0")


def _fields(out):
    """name -> array | PIL image | None of a pipeline output, whichever pipeline made it."""
    if hasattr(out, "entries"):
        return {f"{e.name}.{a}": getattr(e, a) for e in out.entries for a in ("array", "image", "uncertainty")}
    return dict(vars(out))


def _assert_same_outputs(a, b, tag):
    fa, fb = _fields(a), _fields(b)
    assert fa.keys() == fb.keys() and len(fa) >= 3
    for k in fa:
        x, y = fa[k], fb[k]
        assert (x is None) == (y is None), (tag, k)
        if x is None:
            continue
        if isinstance(x, Image.Image):
            assert x.mode == y.mode and x.size == y.size
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=True), (tag, k)


def _latent_channels(kind):
    return 8 if kind == "iid" else 4


@pytest.mark.parametrize("kind", ["depth", "normals", "iid"])
def test_pipeline_outputs_are_those_of_the_host_branch(kind):
    from marigold_amd import synthetic as syn
    pipe = _tiny_pipe(kind)
    E = 2
    kw = dict(ensemble_size=E, show_progress_bar=False, ensemble_kwargs=dict(output_uncertainty=True))
    seen = []
    prep = pipe._preprocess_device
    pipe._preprocess_device = lambda *a: (seen.append(r := prep(*a)), r)[1]
    try:
        # processing_res = 0: the float tensor of the same image takes the host branch
        u8 = syn.synthetic_image(64, 128, seed=3)                          # uint8 [1,3,64,128]
        pil = Image.fromarray(u8[0].permute(1, 2, 0).numpy())
        lat = torch.randn(E, _latent_channels(kind), 8, 16, generator=torch.Generator().manual_seed(11))
        outs = {}
        for tag, image in (("pil", pil), ("uint8 tensor", u8), ("uint8 cuda tensor", u8.cuda()), ("float tensor", u8.float())):
            seen.clear()
            outs[tag] = pipe(image, processing_res=0, init_latents=lat, **kw)
            staged, = seen
            assert (staged is None) == (tag == "float tensor"), tag       # the stage ran exactly where it should
            if staged is not None:
                assert staged[0].is_cuda and staged[0].dtype == torch.float32 and tuple(staged[0].shape) == (1, 3, 64, 128)
                assert tuple(staged[1]) == (1, 3, 64, 128)
        _assert_same_outputs(outs["pil"], outs["float tensor"], f"{kind} res 0 pil")
        _assert_same_outputs(outs["uint8 tensor"], outs["float tensor"], f"{kind} res 0 uint8")
        # (a CUDA uint8 tensor was normalised by torch's device kernel before: the other rounding, so its reference is the host branch)
        pipe.device_io_stages = False
        try:
            _assert_same_outputs(outs["uint8 cuda tensor"], pipe(u8.cuda(), processing_res=0, init_latents=lat, **kw), f"{kind} res 0 cuda")
        finally:
            del pipe.device_io_stages
        # with a resize: 128 x 256 -> 64 x 128 and back, against the host branch of the same pipeline on the same PIL image
        u8 = syn.synthetic_image(128, 256, seed=4)
        pil = Image.fromarray(u8[0].permute(1, 2, 0).numpy())
        for resample in ("bilinear", "bicubic"):
            seen.clear()
            got = pipe(pil, processing_res=128, resample_method=resample, init_latents=lat, **kw)
            assert seen[0] is not None and tuple(seen[0][0].shape) == (1, 3, 64, 128) and tuple(seen[0][1]) == (1, 3, 128, 256)
            pipe.device_io_stages = False
            try:
                seen.clear()
                want = pipe(pil, processing_res=128, resample_method=resample, init_latents=lat, **kw)
                assert seen == []
            finally:
                del pipe.device_io_stages
            _assert_same_outputs(got, want, f"{kind} res 128 {resample}")
            size = next(v for v in _fields(got).values() if isinstance(v, Image.Image)).size
            assert size == (256, 128)
    finally:
        del pipe._preprocess_device
    assert pipe.device_io_stages is True


@pytest.mark.parametrize("kind", ["depth", "normals", "iid"])
def test_map_images_two_images_per_program(kind):
    from marigold_amd import synthetic as syn
    pipe = _tiny_pipe(kind)
    u8s = [syn.synthetic_image(64, 128, seed=s) for s in (5, 6, 7)]
    pils = [Image.fromarray(u[0].permute(1, 2, 0).numpy()) for u in u8s]
    kw = dict(denoising_steps=2, ensemble_size=2, processing_res=0, show_progress_bar=False, images_per_program=2)
    gens = lambda: [torch.Generator(device="cuda:0").manual_seed(60 + k) for k in range(3)]   # noqa: E731
    got = list(pipe.map_images(pils, generators=gens(), **kw))
    want = list(pipe.map_images([u.float() for u in u8s], generators=gens(), **kw))
    assert len(got) == len(want) == 3
    for k, (a, b) in enumerate(zip(got, want)):
        _assert_same_outputs(a, b, f"{kind} image {k}")
