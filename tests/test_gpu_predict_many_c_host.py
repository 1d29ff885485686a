"""``mg_model_predict_many`` on a real MI355X: several pictures per call from a C host (examples/host_many.cpp, a fresh process) and
through ctypes (``ModelImage.predict_many``), every picture against what the Python pipeline returns for it inside
``map_images(images_per_program=K, in_flight=1, generators=[NativeNoise(seed_i)], match_input_res=True)``.

The bound is equality (``np.array_equal``): both sides run the same three programs on the same rows in the same order, and every
stage around them is the code of ``mg_model_predict_out``.  The models are the tiny synthetic ones of
tests/test_gpu_predict_out_c_host.py - 64 x 128, two DDIM steps, four LCM steps for the step-noise case - and both picture sizes are
ones the untouched pipeline maps to 64 x 128 by itself: 64 x 128 at ``processing_res=0`` and 96 x 192 at ``processing_res=128``."""
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
# (kind, members per picture E, pictures per call K, LCM with 4 steps)
GROUPS = [("depth", 1, 3, False), ("depth", 2, 2, False), ("normals", 1, 2, False), ("normals", 3, 2, False), ("depth", 1, 2, True)]
IDS = [f"{k}-E{e}-K{n}" + ("-lcm" if lcm else "") for k, e, n, lcm in GROUPS]
SIZES = [((64, 128), 0), ((96, 192), 128)]   # (picture size, processing_res)
SEEDS = [(1 << 63) + 11, 7, 123456789]       # one per picture; the first needs all 64 bits
PICTURE_SEEDS = [5, 6, 7]                    # of synthetic_image: three different pictures


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind, lcm=False):
    """``_tiny_pipe`` of tests/test_gpu_predict_out_c_host.py; ``lcm``: with the LCM scheduler."""
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.schedulers import LCMScheduler
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=LCMScheduler() if lcm else None,
                                      default_denoising_steps=4 if lcm else 2, default_processing_resolution=0).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _pil(h, w, seed):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _u8s(size, n):
    return [torch.from_numpy(np.array(_pil(*size, PICTURE_SEEDS[i]))).cuda() for i in range(n)]


@functools.lru_cache(maxsize=None)
def _reference(kind, E, K, lcm, size, res):
    """The pipeline's outputs for the K pictures of ``size`` in one group (computed once per case, shared, never modified)."""
    import marigold_amd as M
    pipe = _tiny_pipe(kind, lcm)
    pils = [_pil(*size, PICTURE_SEEDS[i]) for i in range(K)]
    outs = list(pipe.map_images(pils, generators=[M.NativeNoise(s) for s in SEEDS[:K]], images_per_program=K, in_flight=1,
                                denoising_steps=4 if lcm else 2, ensemble_size=E, processing_res=res, match_input_res=True,
                                resample_method="bilinear", ensemble_kwargs=dict(output_uncertainty=True), show_progress_bar=False))
    assert len(outs) == K
    return outs


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
    """One model image per group, exported once, plus the K = 2 DDIM depth image of the module-level test and an image of one picture
    per call; -> {(kind, E, K, lcm): path}."""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("predict_many")
    paths = {}
    for kind, E, K, lcm in GROUPS + [("depth", 1, 2, False), ("depth", 2, 1, False)]:
        paths[kind, E, K, lcm] = str(d / f"{kind}{E}x{K}{'lcm' if lcm else ''}.mgimg")
        got = image.export_model_image(_tiny_pipe(kind, lcm), paths[kind, E, K, lcm], ensemble_size=E, height=MODEL_HW[0], width=MODEL_HW[1],
                                       images_per_program=K)
        assert got["images_per_program"] == K and got["step_noises"] == (3 if lcm else 0)
    return paths


@pytest.fixture(scope="module")
def host_many(tmp_path_factory):
    """examples/host_many.cpp, built as the ``host_picture`` fixture of tests/test_gpu_predict_out_c_host.py builds its example."""
    return c_hosts.build_example("host_many", tmp_path_factory.mktemp("host_many"))


def _check(kind, E, got, ref, size):
    """(pred, unc, u16, picture) of one picture as numpy against the pipeline's output for it."""
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


def _numpy(ts):
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _row(arrays, i):
    return tuple(None if a is None else a[i] for a in arrays)


# ---- through ctypes ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind,E,K,lcm", GROUPS, ids=IDS)
def test_full_groups_match_the_pipeline(lib, models, table, kind, E, K, lcm):
    from marigold_amd import image
    mi = image.ModelImage(models[kind, E, K, lcm])
    lut = torch.from_numpy(table).cuda() if kind == "depth" else None
    try:
        assert (mi.K, mi.B, mi.n_noise) == (K, E, 3 if lcm else 0)
        for size, res in SIZES:
            got = mi.predict_many(_u8s(size, K), SEEDS[:K], out_size=size, out_mode="bilinear", mode="bilinear", lut=lut, u16=kind == "depth",
                                  picture=True)
            torch.cuda.synchronize()
            arrays, infos = _numpy(got[:4]), got[4]
            refs = _reference(kind, E, K, lcm, size, res)
            for i in range(K):
                _check(kind, E, _row(arrays, i), refs[i], size)
                assert (infos[i][1] >= 1) == (kind == "depth" and E > 1)   # the alignment ran per picture
            assert not np.array_equal(arrays[0][0], arrays[0][1])        # different pictures, different seeds
    finally:
        mi.close()


def test_partial_calls(lib, models, table):
    """n < K on the K = 3 depth image: the pictures given are those of the full call, bit for bit; nothing is written from row n on;
    a full call afterwards is the first one again."""
    from marigold_amd import _lib as L, image
    size = (96, 192)
    mi = image.ModelImage(models["depth", 1, 3, False])
    lut = torch.from_numpy(table).cuda()
    try:
        u8s = _u8s(size, 3)
        full = _numpy(mi.predict_many(u8s, SEEDS, out_size=size, lut=lut, u16=True, picture=True)[:4])
        for n in (1, 2):
            pred = torch.full((3, 1) + size, -3.0, device="cuda")
            u16 = torch.full((3,) + size, 77, dtype=torch.int16, device="cuda").view(torch.uint16)
            pic = torch.full((3,) + size + (3,), 77, dtype=torch.uint8, device="cuda")
            info = (ctypes.c_double * 12)(*([9.0] * 12))
            out_opts = L.MgOutputOpts(size[0], size[1], 0, lut.data_ptr())
            rgb = (ctypes.c_void_p * n)(*[u.data_ptr() for u in u8s[:n]])
            seeds = (ctypes.c_uint64 * n)(*SEEDS[:n])
            L.check(lib.mg_model_predict_many(mi.handle, n, rgb, 1, size[0], size[1], 0, 1, seeds, None, ctypes.byref(out_opts), pred.data_ptr(),
                                                    None, u16.data_ptr(), pic.data_ptr(), info, None), "mg_model_predict_many", lib)
            torch.cuda.synchronize()
            got = _numpy((pred, u16, pic))
            for i in range(n):
                assert np.array_equal(got[0][i], full[0][i]) and np.array_equal(got[1][i], full[2][i]) and np.array_equal(got[2][i], full[3][i])
            assert (got[0][n:] == -3.0).all() and (got[1][n:] == 77).all() and (got[2][n:] == 77).all()
            assert list(info)[:4 * n] == [0.0] * (4 * n) and list(info)[4 * n:] == [9.0] * (12 - 4 * n)
        again = _numpy(mi.predict_many(u8s, SEEDS, out_size=size, lut=lut, u16=True, picture=True)[:4])
        for a, b in zip(again, full):
            assert (a is None and b is None) or np.array_equal(a, b)
    finally:
        mi.close()


def test_one_picture_image_is_predict_out(lib, models, table):
    """K = 1 continuity: on an image of one picture per call, n = 1 gives what ``mg_model_predict_out`` gives."""
    from marigold_amd import image
    size = (96, 192)
    mi = image.ModelImage(models["depth", 2, 1, False])
    lut = torch.from_numpy(table).cuda()
    try:
        assert mi.K == 1
        u8 = _u8s(size, 1)[0]
        one = mi.predict_out(u8, SEEDS[0], out_size=size, lut=lut, u16=True, picture=True)
        many = mi.predict_many([u8], SEEDS[:1], out_size=size, lut=lut, u16=True, picture=True)
        torch.cuda.synchronize()
        for a, b in zip(_numpy(one[:4]), _numpy(many[:4])):
            assert b.shape == (1,) + a.shape and np.array_equal(a, b[0])
        assert many[4] == [one[4]] and one[4][1] >= 1
        rgb = (ctypes.c_void_p * 2)(u8.data_ptr(), u8.data_ptr())
        seeds = (ctypes.c_uint64 * 2)(1, 2)
        rc = lib.mg_model_predict_many(mi.handle, 2, rgb, 1, size[0], size[1], 0, 1, seeds, None, None, many[0].data_ptr(), None, None, None, None, None)
        assert rc != 0 and lib.mg_last_error().decode().startswith("mg_model_predict_many: 2 pictures")
    finally:
        mi.close()


def test_module_level_calls_carry_the_batch(lib, models):
    """``encode`` / ``denoise`` / ``decode`` on a K = 2, E = 1 depth image with [2, ...] tensors: the decoded maps, clipped, are the
    ``pred_out`` of ``predict_many`` for the same pictures and seeds."""
    from marigold_amd import image, native_randn
    from marigold_amd.util.image_util import prepare_rgb_device
    mi = image.ModelImage(models["depth", 1, 2, False])
    try:
        u8s = _u8s(MODEL_HW, 2)
        rgb = torch.cat([prepare_rgb_device(u, None, reciprocal=False) for u in u8s])
        x = torch.cat([native_randn((1, 4, mi.h, mi.w), s, stream=0) for s in SEEDS[:2]])
        rgb_latent = mi.encode(rgb)
        assert rgb_latent.shape == (2, 4, mi.h, mi.w)
        pred = mi.decode(mi.denoise(rgb_latent, x))
        assert pred.shape == (2, 1) + MODEL_HW
        many = mi.predict_many(u8s, SEEDS[:2])[0]
        torch.cuda.synchronize()
        assert np.array_equal(pred.clamp(0, 1).cpu().numpy(), many.cpu().numpy())
        assert not torch.equal(many[0], many[1])
    finally:
        mi.close()


def test_refusals(lib, models, table):
    """Every refusal comes before anything is launched: the outputs keep their sentinel fill."""
    from marigold_amd import _lib as L, image
    u8s = _u8s(MODEL_HW, 3)
    out = torch.full((3, 3, 64, 128), -3.0, device="cuda")
    u16 = torch.full((3, 64, 128), 77, dtype=torch.int16, device="cuda").view(torch.uint16)
    pic = torch.full((3, 64, 128, 3), 77, dtype=torch.uint8, device="cuda")
    lut = torch.from_numpy(table).cuda()
    ptrs = [u.data_ptr() for u in u8s]

    def refused(mi, n, rgb, seeds, opts, u16_ptr, pic_ptr, *words):
        rgb_arr = None if rgb is None else (ctypes.c_void_p * len(rgb))(*rgb)
        seed_arr = None if seeds is None else (ctypes.c_uint64 * len(seeds))(*seeds)
        rc = lib.mg_model_predict_many(mi.handle, n, rgb_arr, 1, 64, 128, 0, 0, seed_arr, None, None if opts is None else ctypes.byref(opts),
                                       out.data_ptr(), None, u16_ptr, pic_ptr, None, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_many:") and all(w in msg for w in words), msg

    mi = image.ModelImage(models["depth", 1, 3, False])
    try:
        refused(mi, 0, ptrs, SEEDS, None, None, None, "0 pictures", "1 <= n <= 3")
        refused(mi, 4, ptrs + ptrs[:1], SEEDS + [1], None, None, None, "4 pictures", "1 <= n <= 3")
        refused(mi, 3, None, SEEDS, None, None, None, "null", "rgb")
        refused(mi, 3, ptrs, None, None, None, None, "null", "seeds")
        refused(mi, 3, [ptrs[0], None, ptrs[2]], SEEDS, None, None, None, "null picture 1")
        # the output options, in the words of mg_model_predict_out
        refused(mi, 3, ptrs, SEEDS, L.MgOutputOpts(out_mode=3), None, None, "out_mode must be 0 (bilinear), 1 (bicubic) or 2 (nearest-exact)")
        refused(mi, 3, ptrs, SEEDS, L.MgOutputOpts(out_h=8), None, None, "bad output size 8 x 0")
        refused(mi, 3, ptrs, SEEDS, L.MgOutputOpts(out_h=-8, out_w=8), None, None, "bad output size -8 x 8")
        refused(mi, 3, ptrs, SEEDS, None, None, pic.data_ptr(), "the picture of a depth model needs out_opts.lut256x3 (the colour table)")
        refused(mi, 3, ptrs, SEEDS, L.MgOutputOpts(), u16.data_ptr(), pic.data_ptr(), "lut256x3")
        # the one-picture entry points on this image
        u8 = u8s[0]
        for name, call in (("mg_model_predict", lambda: lib.mg_model_predict(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, out.data_ptr(), None,
                                                                            None, None)),
                           ("mg_model_predict_out", lambda: lib.mg_model_predict_out(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, None,
                                                                                    out.data_ptr(), None, None, None, None, None)),
                           ("mg_model_predict_iid", lambda: lib.mg_model_predict_iid(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, out.data_ptr(),
                                                                                    None, None, None))):
            rc = call()
            msg = lib.mg_last_error().decode()
            assert rc != 0 and msg.startswith(name + ":") and "mg_model_predict_many" in msg and "3 pictures per call" in msg, msg
    finally:
        mi.close()
    mi = image.ModelImage(models["normals", 1, 2, False])
    try:
        refused(mi, 2, ptrs[:2], SEEDS[:2], None, u16.data_ptr(), None, "u16_out and lut256x3 belong to a depth model")
        refused(mi, 2, ptrs[:2], SEEDS[:2], L.MgOutputOpts(lut256x3=lut.data_ptr()), None, pic.data_ptr(), "depth model")
        refused(mi, 3, ptrs, SEEDS, None, None, None, "3 pictures", "1 <= n <= 2")
    finally:
        mi.close()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((u16.cpu().numpy() == 77).all()) and bool((pic == 77).all())


def test_intrinsic_image_model_is_refused(lib, tmp_path):
    """An intrinsic-image model (always one picture per call) does not go through ``mg_model_predict_many``."""
    from marigold_amd import image
    path = str(tmp_path / "iid.mgimg")
    image.export_model_image(_tiny_pipe("iid"), path, ensemble_size=1, height=64, width=128)
    mi = image.ModelImage(path)
    try:
        u8 = _u8s(MODEL_HW, 1)[0]
        out = torch.full((6, 64, 128), -3.0, device="cuda")
        rc = lib.mg_model_predict_many(mi.handle, 1, (ctypes.c_void_p * 1)(u8.data_ptr()), 1, 64, 128, 0, 0, (ctypes.c_uint64 * 1)(1), None, None,
                                       out.data_ptr(), None, None, None, None, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_many:") and "intrinsic-image" in msg, msg
        torch.cuda.synchronize()
        assert bool((out == -3.0).all())
    finally:
        mi.close()


def test_temporaries_are_one_pictures(lib, models, table):
    """``mg_model_device_bytes``: the temporaries serve the pictures of a call one after the other, so a call of K = 2 pictures of 96 x
    192 with E = 2 members each grows the model by ONE picture's input resampling temporary [3][96][128], ONE ensembled map [64][128]
    and ONE resize intermediate [64][192] (fp32; the last two rounded up to 256 bytes each) - what ``mg_model_predict_out`` needs
    for one such picture - and an identical second call by nothing."""
    from marigold_amd import image
    mi = image.ModelImage(models["depth", 2, 2, False])
    lut = torch.from_numpy(table).cuda()
    r256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    try:
        size, res = SIZES[1]
        base = lib.mg_model_device_bytes(mi.handle)
        got = mi.predict_many(_u8s(size, 2), SEEDS[:2], out_size=size, lut=lut, u16=True, picture=True)
        torch.cuda.synchronize()
        step1 = lib.mg_model_device_bytes(mi.handle)
        assert step1 - base == 3 * 96 * 128 * 4 + r256(64 * 128 * 4) + r256(64 * 192 * 4)
        again = mi.predict_many(_u8s(size, 2), SEEDS[:2], out_size=size, lut=lut, u16=True, picture=True)
        torch.cuda.synchronize()
        assert lib.mg_model_device_bytes(mi.handle) == step1
        refs = _reference("depth", 2, 2, False, size, res)
        for arrays in (_numpy(got[:4]), _numpy(again[:4])):
            for i in range(2):
                _check("depth", 2, _row(arrays, i), refs[i], size)
    finally:
        mi.close()


# ---- the C host ----------------------------------------------------------------------------------------------------------------


def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


@pytest.mark.parametrize("kind,E,K,lcm", GROUPS, ids=IDS)
def test_c_host_many(lib, models, host_many, tmp_path, kind, E, K, lcm):
    """examples/host_many.cpp in a fresh process, one call of K pictures: the files it writes per picture read back."""
    from marigold_amd import image
    size, res = SIZES[1]
    prefix, lut_path = str(tmp_path / "out"), str(tmp_path / "spectral.lut")
    image.export_color_table("Spectral", lut_path)
    pictures = []
    for i in range(K):
        raw = str(tmp_path / f"image{i}.u8")
        np.asarray(_pil(*size, PICTURE_SEEDS[i])).tofile(raw)
        pictures += [raw, str(SEEDS[i])]
    args = [host_many, models[kind, E, K, lcm], str(size[0]), str(size[1]), prefix, str(size[0]), str(size[1]), "0"]
    r = subprocess.run(args + ([lut_path] if kind == "depth" else []) + ["--"] + pictures, capture_output=True, text=True, timeout=120)
    print("[predict_many C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    C = 1 if kind == "depth" else 3
    refs = _reference(kind, E, K, lcm, size, res)
    for i in range(K):
        pre = f"{prefix}.{i}"
        pred = np.fromfile(pre + ".f32", dtype=np.float32).reshape((C,) + size)
        unc = np.fromfile(pre + ".unc.f32", dtype=np.float32).reshape(MODEL_HW) if E > 1 else None
        assert os.path.exists(pre + ".unc.f32") == (E > 1) and os.path.exists(pre + ".pgm") == (kind == "depth")
        u16 = _pnm(pre + ".pgm", b"P5", size[0], size[1], 65535, ">u2", 1).astype(np.uint16) if kind == "depth" else None
        pic = _pnm(pre + ".ppm", b"P6", size[0], size[1], 255, np.uint8, 3)
        _check(kind, E, (pred, unc, u16, pic), refs[i], size)
    assert not os.path.exists(f"{prefix}.{K}.f32")
