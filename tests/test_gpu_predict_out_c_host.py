"""``mg_model_predict_out`` on a real MI355X: the depth and normals pipelines' whole output - the map at the input picture's size,
clipped, the 16-bit depth, the picture, the uncertainty - from a C host (examples/host_picture.cpp, a fresh process) and through ctypes
(``ModelImage.predict_out``), every result against the existing Python pipeline called with ``match_input_res=True`` and
``generator=NativeNoise(seed)``.

The bound is equality (``np.array_equal``): both sides run the same kernels on the same inputs in the same order.  The models are the
tiny synthetic ones of tests/test_gpu_native_noise.py, two steps, 64 x 128.

The reference and the picture sizes.  ``pipe(pil, ...)`` brings a picture to its processing size keeping the aspect ratio, so no
picture of 96 x 160 or 64 x 160 reaches a 64 x 128 model through it, while the C entry resamples any picture to the model's size.
For those sizes the reference is still the one ``pipe(pil, match_input_res=True, ...)`` call, with ``pipe._preprocess`` swapped for
the same device input stage (``prepare_rgb_device``) aimed at 64 x 128; everything after it - members, ensemble, resize, clip, picture -
is the pipeline's own code, unchanged.  A 96 x 192 picture with ``processing_res=128`` (which the pipeline maps to 64 x 128 by itself)
is compared too, through the untouched call."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests import c_hosts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_HW = (64, 128)
# (name, picture size, resample method, processing_res of the untouched pipeline call | None = the swapped input stage)
CASES = [("same", (64, 128), "bilinear", 0), ("both-bilinear", (96, 160), "bilinear", None), ("both-bicubic", (96, 160), "bicubic", None),
         ("one-axis", (64, 160), "bilinear", None), ("nearest-exact", (96, 160), "nearest-exact", None), ("pipeline-sized", (96, 192), "bilinear", 128)]
MODELS = [("depth", 1), ("depth", 3), ("normals", 1), ("normals", 3)]
HOST_CASE = {("depth", 1): "both-bicubic", ("depth", 3): "same", ("normals", 1): "one-axis", ("normals", 3): "nearest-exact"}
SEED = (1 << 63) + 11


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind):
    """``_tiny_pipe`` of tests/test_gpu_native_noise.py."""
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _pil(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


@functools.lru_cache(maxsize=None)
def _reference(kind, E, size, method, res, seed=SEED, match=True):
    """The pipeline's output for the picture of ``size`` (computed once per case, shared, never modified)."""
    import marigold_amd as M
    from marigold_amd.util.image_util import prepare_rgb_device
    pipe = _tiny_pipe(kind)
    pil = _pil(*size)
    if res is None:
        def to_model_size(image, processing_res, resample):
            u8 = torch.from_numpy(np.array(image.convert("RGB")))
            return prepare_rgb_device(u8, MODEL_HW, resample, pipe.io_dtype, True, device=pipe.device, reciprocal=True), torch.Size((1, 3) + size)
        pipe._preprocess = to_model_size
    try:
        return pipe(pil, denoising_steps=2, ensemble_size=E, processing_res=res or 0, match_input_res=match, resample_method=method,
                    generator=M.NativeNoise(seed), ensemble_kwargs=dict(output_uncertainty=True), show_progress_bar=False)
    finally:
        pipe.__dict__.pop("_preprocess", None)


def _ref_arrays(kind, ref):
    """(map [C, h, w], picture [h, w, 3], uncertainty | None)"""
    if kind == "depth":
        return ref.depth_np[None], np.asarray(ref.depth_colored), ref.uncertainty
    return ref.normals_np, np.asarray(ref.normals_img), ref.uncertainty


@pytest.fixture(scope="module")
def table():
    from marigold_amd.util.image_util import colormap_lut_u8
    return colormap_lut_u8("Spectral")


@pytest.fixture(scope="module")
def models(lib, tmp_path_factory):
    """One model image per (kind, E), exported once; -> {(kind, E): path}."""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("predict_out")
    paths = {}
    for kind, E in MODELS:
        paths[kind, E] = str(d / f"{kind}{E}.mgimg")
        image.export_model_image(_tiny_pipe(kind), paths[kind, E], ensemble_size=E, height=MODEL_HW[0], width=MODEL_HW[1])
    return paths


@pytest.fixture(scope="module")
def host_picture(tmp_path_factory):
    """examples/host_picture.cpp, built as the ``host_map`` fixture of tests/test_gpu_native_noise.py builds its example."""
    return c_hosts.build_example("host_picture", tmp_path_factory.mktemp("host_picture"))


def _check(kind, E, got, ref, size):
    """(pred, unc, u16, picture) as numpy against the pipeline's output."""
    pred, unc, u16, pic = got
    want, want_pic, want_unc = _ref_arrays(kind, ref)
    assert want.shape == (1 if kind == "depth" else 3,) + size and np.isfinite(want).all()
    assert np.array_equal(pred, want)
    assert pic.shape == size + (3,) and np.array_equal(pic, want_pic)
    if E > 1:
        assert want_unc.shape == MODEL_HW and np.array_equal(unc, want_unc)   # at the decoded size
    else:
        assert unc is None and want_unc is None
    if kind == "depth":
        assert np.array_equal(u16, (ref.depth_np * 65535.0).astype(np.uint16))   # the line the command line runs
        assert u16.max() > u16.min()
    else:
        assert u16 is None


# ---- through ctypes ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind,E", MODELS, ids=[f"{k}-E{e}" for k, e in MODELS])
def test_predict_out_matches_the_pipeline(lib, models, table, kind, E):
    from marigold_amd import _lib as L, image, ops as O
    mi = image.ModelImage(models[kind, E])
    lut = torch.from_numpy(table).cuda() if kind == "depth" else None
    try:
        infos = {}
        for name, size, method, res in CASES:
            u8 = torch.from_numpy(np.array(_pil(*size))).cuda()
            pred, unc, u16, pic, info = mi.predict_out(u8, SEED, out_size=size, out_mode=method, mode=method, lut=lut, u16=kind == "depth", picture=True)
            torch.cuda.synchronize()
            got = tuple(None if t is None else t.cpu().numpy() for t in (pred, unc, u16, pic))
            _check(kind, E, got, _reference(kind, E, size, method, res), size)
            infos[name] = info
        # mg_model_predict on the same bytes and seed: the same alignment report, and its own map - unclipped, at the decoded size -
        # with the bits it had before (the pipeline's with match_input_res=False)
        for name, size, method, res in (CASES[0], CASES[1]):
            u8 = torch.from_numpy(np.array(_pil(*size))).cuda()
            C = mi.pred_channels
            plain = torch.full((C,) + MODEL_HW, float("nan"), device="cuda")
            info = (ctypes.c_double * 4)(9, 9, 9, 9)
            L.check(lib.mg_model_predict(mi.handle, u8.data_ptr(), 1, size[0], size[1], O.RESIZE_MODES[method], int(size != MODEL_HW), SEED, None,
                                         plain.data_ptr(), None, info, O.current_stream_handle()), "mg_model_predict", lib)
            torch.cuda.synchronize()
            assert list(info) == infos[name] and (info[1] >= 1) == (kind == "depth" and E > 1)
            want = _ref_arrays(kind, _reference(kind, E, size, method, res, match=False))[0]
            assert want.shape == (C,) + MODEL_HW and np.array_equal(plain.cpu().numpy(), want)
        # the defaults: no out_opts = the decoded size, nothing but the clipped map
        u8 = torch.from_numpy(np.array(_pil(*MODEL_HW))).cuda()
        pred = torch.full((mi.pred_channels,) + MODEL_HW, float("nan"), device="cuda")
        L.check(lib.mg_model_predict_out(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, SEED, None, None, pred.data_ptr(), None, None, None, None,
                                         O.current_stream_handle()), "mg_model_predict_out", lib)
        torch.cuda.synchronize()
        assert np.array_equal(pred.cpu().numpy(), _ref_arrays(kind, _reference(kind, E, MODEL_HW, "bilinear", 0))[0])
    finally:
        mi.close()


def test_temporaries_grow_with_the_output_size(lib, models, table):
    """``mg_model_device_bytes`` counts the ensembled map ahead of a resize and the resize's intermediate, each rounded up to 256 bytes;
    a second call with a larger output grows them and still matches the pipeline; an identical or smaller call does not."""
    from marigold_amd import image
    mi = image.ModelImage(models["depth", 3])
    lut = torch.from_numpy(table).cuda()
    r256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    try:
        base = lib.mg_model_device_bytes(mi.handle)
        size = (96, 160)
        u8 = torch.from_numpy(np.array(_pil(*size))).cuda()
        got = mi.predict_out(u8, SEED, out_size=size, out_mode="bilinear", lut=lut, u16=True, picture=True)
        torch.cuda.synchronize()
        step1 = lib.mg_model_device_bytes(mi.handle)
        # the input resampling temporary [3][96][128], the ensembled map [64][128], the intermediate [64][160], all fp32
        assert step1 - base == 3 * 96 * 128 * 4 + r256(64 * 128 * 4) + r256(64 * 160 * 4)
        _check("depth", 3, tuple(None if t is None else t.cpu().numpy() for t in got[:4]), _reference("depth", 3, size, "bilinear", None), size)
        big = (128, 200)
        u8b = torch.from_numpy(np.array(_pil(*big))).cuda()
        got = mi.predict_out(u8b, SEED, out_size=big, out_mode="bilinear", lut=lut, u16=True, picture=True)
        torch.cuda.synchronize()
        step2 = lib.mg_model_device_bytes(mi.handle)
        assert step2 - step1 == (3 * 128 * 128 * 4 - 3 * 96 * 128 * 4) + (r256(64 * 200 * 4) - r256(64 * 160 * 4))
        _check("depth", 3, tuple(None if t is None else t.cpu().numpy() for t in got[:4]), _reference("depth", 3, big, "bilinear", None), big)
        again = mi.predict_out(u8, SEED, out_size=size, out_mode="bilinear", lut=lut, u16=True, picture=True)   # needs less
        torch.cuda.synchronize()
        assert lib.mg_model_device_bytes(mi.handle) == step2
        _check("depth", 3, tuple(None if t is None else t.cpu().numpy() for t in again[:4]), _reference("depth", 3, size, "bilinear", None), size)
    finally:
        mi.close()


# ---- the C host ----------------------------------------------------------------------------------------------------------------


def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


@pytest.mark.parametrize("kind,E", MODELS, ids=[f"{k}-E{e}" for k, e in MODELS])
def test_c_host_picture(lib, models, host_picture, tmp_path, kind, E):
    """examples/host_picture.cpp in a fresh process: the files it writes - .f32, .unc.f32, the 16-bit .pgm, the .ppm - read back."""
    from marigold_amd import image, ops as O
    name, size, method, res = next(c for c in CASES if c[0] == HOST_CASE[kind, E])
    raw, prefix, lut_path = str(tmp_path / "image.u8"), str(tmp_path / "out"), str(tmp_path / "spectral.lut")
    np.asarray(_pil(*size)).tofile(raw)
    image.export_color_table("Spectral", lut_path)
    args = [host_picture, models[kind, E], raw, str(size[0]), str(size[1]), str(SEED), prefix, str(size[0]), str(size[1]), str(O.RESIZE_MODES[method])]
    r = subprocess.run(args + ([lut_path] if kind == "depth" else []), capture_output=True, text=True, timeout=120)
    print("[predict_out C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    C = 1 if kind == "depth" else 3
    pred = np.fromfile(prefix + ".f32", dtype=np.float32).reshape((C,) + size)
    unc = np.fromfile(prefix + ".unc.f32", dtype=np.float32).reshape(MODEL_HW) if E > 1 else None
    assert os.path.exists(prefix + ".unc.f32") == (E > 1) and os.path.exists(prefix + ".pgm") == (kind == "depth")
    u16 = _pnm(prefix + ".pgm", b"P5", size[0], size[1], 65535, ">u2", 1).astype(np.uint16) if kind == "depth" else None
    pic = _pnm(prefix + ".ppm", b"P6", size[0], size[1], 255, np.uint8, 3)
    _check(kind, E, (pred, unc, u16, pic), _reference(kind, E, size, method, res), size)
    if kind == "depth" and E == 1:   # a depth model without a table: no picture, everything else as before
        r = subprocess.run([a if a != prefix else prefix + "2" for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        assert not os.path.exists(prefix + "2.ppm") and open(prefix + "2.f32", "rb").read() == open(prefix + ".f32", "rb").read()
        assert open(prefix + "2.pgm", "rb").read() == open(prefix + ".pgm", "rb").read()


# ---- refusals ------------------------------------------------------------------------------------------------------------------


def test_refusals(lib, models, table, tmp_path):
    """Every refusal comes before anything is launched: the outputs keep their sentinel fill."""
    from marigold_amd import _lib as L, image
    u8 = torch.from_numpy(np.array(_pil(*MODEL_HW))).cuda()
    out = torch.full((3, 64, 128), -3.0, device="cuda")
    u16 = torch.full((64, 128), 77, dtype=torch.int16, device="cuda").view(torch.uint16)
    pic = torch.full((64, 128, 3), 77, dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(table).cuda()

    def refused(mi, opts, u16_ptr, pic_ptr, *words):
        rc = lib.mg_model_predict_out(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, None if opts is None else ctypes.byref(opts), out.data_ptr(),
                                      None, u16_ptr, pic_ptr, None, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_out:") and all(w in msg for w in words), msg

    path = str(tmp_path / "iid.mgimg")
    image.export_model_image(_tiny_pipe("iid"), path, ensemble_size=1, height=64, width=128)
    mi = image.ModelImage(path)
    try:
        refused(mi, None, None, None, "intrinsic-image", "mg_model_predict_iid")
    finally:
        mi.close()
    mi = image.ModelImage(models["depth", 1])
    try:
        refused(mi, L.MgOutputOpts(out_mode=3), None, None, "out_mode")
        refused(mi, L.MgOutputOpts(out_h=8), None, None, "bad output size")
        refused(mi, L.MgOutputOpts(out_h=-8, out_w=8), None, None, "bad output size")
        refused(mi, None, None, pic.data_ptr(), "lut256x3")                       # a depth picture without a table
        refused(mi, L.MgOutputOpts(), u16.data_ptr(), pic.data_ptr(), "lut256x3")
    finally:
        mi.close()
    mi = image.ModelImage(models["normals", 1])
    try:
        refused(mi, None, u16.data_ptr(), None, "depth model")
        refused(mi, L.MgOutputOpts(lut256x3=lut.data_ptr()), None, pic.data_ptr(), "depth model")
    finally:
        mi.close()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((u16.cpu().numpy() == 77).all()) and bool((pic == 77).all())
