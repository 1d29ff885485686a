"""``mg_model_predict_tiled`` on a real MI355X: the tiled prediction of a large picture as one C call, through ctypes
(``ModelImage.predict_tiled``) and from a C host (examples/host_tiled.cpp, a fresh process), against what the Python pipeline returns:

    pipe.predict_tiled(pil, tile_size=(64, 128), tile_overlap=(16, 32), guide_res=..., tiles_per_program=K, in_flight=1,
                       generator=NativeNoise(seed), match_input_res=True, ensemble_kwargs=dict(output_uncertainty=True))

Every bound is an equality (``np.array_equal``) on the map, the uncertainty, the 16-bit depth, the picture and ``degenerate_tiles``:
both sides run the same programs and kernels on the same bytes, so any tolerance would hide a defect.  The models are the tiny
synthetic ones of tests/test_gpu_predict_out_c_host.py with two DDIM steps; the picture is 128 x 256 and its 9 tiles of 64 x 128 form
groups of 4, 4, 1 with K = 4 (the short last group) and 2, 2, 2, 2, 1 with K = 2.

The SHORT LAST GROUP.  ``map_images`` runs a group of r < K tiles as a program of r pictures; the C call either does the same, on
``tail_config``, or pads the group to K on the tile configuration (``mg_model_predict_many``'s rule for n < K).  Padding changes the
batch, and with it - for the three members of a tile of the E = 3 cases, batch 3 against 6 - the bits of the tile (first run of this
file: the last tile of depth-E3-K2 differed by up to 3e-6 where the rest was equal).  So the E = 3 cases pass the image's E = 3, K = 1
configuration as the tail, and the E = 1 cases pad: one member's bits did not depend on the batch it ran in.

The RESIZE case.  The C call works at the size of the picture it is given, so the output is resampled only when the host asks for
another size than that.  Python gets there with ``tiled_res``: a 96 x 192 picture and ``tiled_res=256`` are worked at 128 x 256 and
the map goes back to 96 x 192.  The test resamples the picture the way ``predict_tiled`` does, with the same call, hands that to C and
asks for 96 x 192.  That case is the normals model's: the depth guide of Python reads the picture before that resampling."""
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
PICTURE_HW, TILE, OVERLAP = (128, 256), (64, 128), (16, 32)
SEED = (1 << 63) + 31            # needs all 64 bits
SEED_WRAP = (1 << 64) - 3        # seed + 1 + i passes 2^64 at tile 2
# the configurations of the images, (E, H, W, K): depth 0 guide E1 (guide_res 128), 1 tiles E1 K4, 2 guide E3, 3 tiles E3 K2, 4 guide E1 at
# guide_res 256, 5 tiles E1 K2; normals 0 tiles E1 K2, 1 tiles E3 K2, 2 and 3 one picture per call, E1 and E3
DEPTH_CONFIGS = [(1, 64, 128, 1), (1, 64, 128, 4), (3, 64, 128, 1), (3, 64, 128, 2), (1, 128, 256, 1), (1, 64, 128, 2)]
NORMALS_CONFIGS = [(1, 64, 128, 2), (3, 64, 128, 2), (1, 64, 128, 1), (3, 64, 128, 1)]
# (id, kind, E, K, guide_res, seed, tiny)
CASES = [("depth-E1-K4", "depth", 1, 4, 128, SEED, False), ("depth-E3-K2", "depth", 3, 2, 128, SEED, False),
         ("normals-E1-K2", "normals", 1, 2, None, SEED_WRAP, False), ("normals-E3-K2", "normals", 3, 2, None, SEED, False),
         ("depth-E1-K2-guide256", "depth", 1, 2, 256, SEED, False), ("depth-E1-K2-tiny-vae", "depth", 1, 2, 128, SEED, True)]
CASE_IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind, tiny=False):
    """``_tiny_pipe`` of tests/test_gpu_predict_out_c_host.py; ``tiny``: with the tiny autoencoder set into it (tests/test_gpu_tiny_image.py)."""
    import marigold_amd as M
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    pipe = M.build_synthetic_pipeline(kind, TINY_UNET, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0).to("cuda:0")
    if tiny:
        from marigold_amd.modules import AutoencoderTinyHIP
        pipe.set_vae(AutoencoderTinyHIP(syn.synthetic_tiny_vae_state_dict()))
    return pipe


@functools.lru_cache(maxsize=None)
def _pil(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _u8(h, w):
    return torch.from_numpy(np.array(_pil(h, w))).cuda()


def _configs(rows):
    return [dict(ensemble_size=e, height=h, width=w, denoising_steps=2, images_per_program=k) for e, h, w, k in rows]


@pytest.fixture(scope="module")
def models(lib, tmp_path_factory):
    """One image of several configurations per kind, and the tiny-VAE depth image -> {(kind, tiny): path}"""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("predict_tiled")
    paths = {("depth", False): str(d / "depth.mgimg"), ("normals", False): str(d / "normals.mgimg"), ("depth", True): str(d / "depth_tiny.mgimg")}
    image.export_model_image(_tiny_pipe("depth"), paths["depth", False], configs=_configs(DEPTH_CONFIGS))
    image.export_model_image(_tiny_pipe("normals"), paths["normals", False], configs=_configs(NORMALS_CONFIGS))
    info = image.export_model_image(_tiny_pipe("depth", True), paths["depth", True], tiny_vae=True, configs=_configs(DEPTH_CONFIGS[:1] + DEPTH_CONFIGS[5:]))
    assert info["configs"][0]["cfg16"][14] == 1
    return paths


@pytest.fixture(scope="module")
def table():
    from marigold_amd.util.image_util import colormap_lut_u8
    return colormap_lut_u8("Spectral")


@functools.lru_cache(maxsize=None)
def _reference(kind, E, K, guide_res, seed, tiny, size=PICTURE_HW, tiled_res=0):
    """The pipeline's tiled output (computed once per case, shared, never modified)."""
    from marigold_amd import NativeNoise
    return _tiny_pipe(kind, tiny).predict_tiled(_pil(*size), tile_size=TILE, tile_overlap=OVERLAP, guide_res=guide_res, tiled_res=tiled_res,
                                                tiles_per_program=K, in_flight=1, generator=NativeNoise(seed), match_input_res=True,
                                                denoising_steps=2, ensemble_size=E, ensemble_kwargs=dict(output_uncertainty=True))


def _find(mi, kind, E, K, guide_res):
    """The host's part: the configurations through ``mg_model_find_config`` -> (guide, tile, tail | None); the 9 tiles leave a last group
    of one for K = 2 and K = 4, which the E = 3 cases run on the one-picture configuration (see the module docstring)"""
    tile = mi.find(TILE[0], TILE[1], E, 2, K)
    tail = mi.find(TILE[0], TILE[1], E, 2, 1) if E > 1 else None
    if kind != "depth":
        return 0, tile, tail
    H, W = ctypes.c_int(), ctypes.c_int()
    assert mi._lib.mg_processed_size(PICTURE_HW[0], PICTURE_HW[1], guide_res, ctypes.byref(H), ctypes.byref(W)) == 0
    return mi.find(H.value, W.value, E, 2, 1), tile, tail


def _numpy(ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _check(kind, E, got, ref, size=PICTURE_HW):
    """(pred, unc, u16, picture, flagged tiles | None) as numpy against the pipeline's output."""
    pred, unc, u16, pic, flagged = got
    want = ref.depth_np[None] if kind == "depth" else ref.normals_np
    want_pic = np.asarray(ref.depth_colored if kind == "depth" else ref.normals_img)
    assert want.shape == (1 if kind == "depth" else 3,) + size and np.isfinite(want).all() and want.max() > want.min()
    assert np.array_equal(pred, want)
    assert pic.shape == size + (3,) and np.array_equal(pic, want_pic)
    if E > 1:
        assert ref.uncertainty.shape == PICTURE_HW and np.array_equal(unc, ref.uncertainty)   # at the working size
        assert float(unc.max()) > 0.0
    else:
        assert unc is None and ref.uncertainty is None
    if kind == "depth":
        assert np.array_equal(u16, (ref.depth_np * 65535.0).astype(np.uint16)) and u16.max() > u16.min()
        assert flagged == ref.degenerate_tiles and flagged is not None
    else:
        assert u16 is None and flagged is None


def _call(mi, kind, E, K, guide_res, seed, lut, u8=None, **kw):
    guide, tile, tail = _find(mi, kind, E, K, guide_res)
    got = mi.predict_tiled(_u8(*PICTURE_HW) if u8 is None else u8, seed, guide, tile, OVERLAP, tail_config=tail, lut=lut if kind == "depth" else None,
                           u16=kind == "depth", picture=True, **kw)
    arrays = _numpy(got[:4])
    flags = got[5]
    if flags is not None:
        assert flags.shape == (9,) and set(flags.cpu().tolist()) <= {0, 1}
    return arrays + (None if flags is None else int(flags.sum().item()),), got[4]


# ---- through ctypes ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind,E,K,guide_res,seed,tiny", CASES, ids=CASE_IDS)
def test_the_call_is_predict_tiled_bit_for_bit(lib, models, table, name, kind, E, K, guide_res, seed, tiny):
    from marigold_amd import image
    mi = image.ModelImage(models[kind, tiny])
    lut = torch.from_numpy(table).cuda()
    try:
        selected = mi.configs[0]
        got, info = _call(mi, kind, E, K, guide_res, seed, lut)
        _check(kind, E, got, _reference(kind, E, K, guide_res, seed, tiny))
        assert (info[1] >= 1) == (kind == "depth" and E > 1)   # the guide's alignment ran
        cfg = (ctypes.c_int * 16)()
        assert lib.mg_model_info(mi.handle, cfg) == 0 and list(cfg) == selected   # the handle is where it was
        if tiny:
            assert cfg[14] == 1
    finally:
        mi.close()


def test_the_resize_to_another_output_size(lib, models):
    """Normals, E = 3: a 96 x 192 picture worked at 128 x 256 (``tiled_res=256``) and handed back at 96 x 192."""
    from marigold_amd import image
    from marigold_amd.util.image_util import get_tv_resample_method, pil_to_tensor, resize
    ref = _reference("normals", 3, 2, None, SEED, False, size=(96, 192), tiled_res=256)
    rgb = pil_to_tensor(_pil(96, 192)).unsqueeze(0).cuda()
    work = resize(rgb, PICTURE_HW, interpolation=get_tv_resample_method("bilinear"), antialias=True)   # predict_tiled's own line
    assert work.dtype == torch.uint8 and tuple(work.shape) == (1, 3) + PICTURE_HW
    u8 = work[0].permute(1, 2, 0).contiguous()
    mi = image.ModelImage(models["normals", False])
    try:
        got, _ = _call(mi, "normals", 3, 2, None, SEED, None, u8=u8, out_size=(96, 192), out_mode="bilinear")
        _check("normals", 3, got, ref, size=(96, 192))
    finally:
        mi.close()


def test_the_handle_keeps_its_configuration_and_its_results(lib, models, table):
    """``mg_model_predict_out`` on the selected configuration gives the same bits before and after a tiled call on two others; the
    temporaries are counted and a second identical call grows nothing."""
    from marigold_amd import image
    mi = image.ModelImage(models["depth", False])
    lut = torch.from_numpy(table).cuda()
    try:
        mi.select(2)   # E = 3, 64 x 128, one picture per call
        small = _u8(64, 128)
        before = _numpy(mi.predict_out(small, 77, lut=lut, u16=True, picture=True)[:4])
        base = lib.mg_model_device_bytes(mi.handle)
        got, _ = _call(mi, "depth", 1, 4, 128, SEED, lut)
        grown = lib.mg_model_device_bytes(mi.handle)
        # the tiled call's own: crops [4][3][64][128] uint8, maps [9][64][128] fp32, the fit's workspace, coefficients [9][2] fp64, guide
        # [64][128] fp32, each rounded up to 256 bytes (the flags are the caller's); and what mg_model_predict needs to resample the
        # guide's input from 128 x 256 to 64 x 128, fp32 [3][128][128]
        r256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
        own = 4 * 3 * 64 * 128 + 9 * 64 * 128 * 4 + r256(lib.mg_tiles_workspace_bytes(9, 64, 128)) + r256(9 * 16) + 64 * 128 * 4
        assert grown - base == own + 3 * 128 * 128 * 4
        _check("depth", 1, got, _reference("depth", 1, 4, 128, SEED, False))
        cfg = (ctypes.c_int * 16)()
        assert lib.mg_model_info(mi.handle, cfg) == 0 and list(cfg) == mi.configs[2] and mi.selected == 2
        after = _numpy(mi.predict_out(small, 77, lut=lut, u16=True, picture=True)[:4])
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
        again, _ = _call(mi, "depth", 1, 4, 128, SEED, lut)
        assert lib.mg_model_device_bytes(mi.handle) == grown
        _check("depth", 1, again, _reference("depth", 1, 4, 128, SEED, False))
    finally:
        mi.close()


@pytest.mark.parametrize("kind", ["depth", "normals"])
def test_results_do_not_depend_on_what_scratch_held(lib, models, table, kind):
    """``mg_model_scratch_fill(m, 0xff)`` - NaN in every float format, over the programs' scratch and the tiled call's temporaries -
    ahead of the call: the same bits, so the call never reads a temporary it has not written."""
    from marigold_amd import _lib as L, image, ops as O
    mi = image.ModelImage(models[kind, False])
    lut = torch.from_numpy(table).cuda()
    try:
        ref = _reference(kind, 3, 2, 128 if kind == "depth" else None, SEED, False)
        first, _ = _call(mi, kind, 3, 2, 128, SEED, lut)     # (allocates the temporaries the fill then covers)
        _check(kind, 3, first, ref)
        L.check(lib.mg_model_scratch_fill(mi.handle, 0xff, O.current_stream_handle()), "mg_model_scratch_fill", lib)
        filled, _ = _call(mi, kind, 3, 2, 128, SEED, lut)
        _check(kind, 3, filled, ref)
    finally:
        mi.close()


def test_refusals_leave_the_outputs_untouched(lib, models):
    """On the device as on the host (tests/test_tiled_c_host_host.py): a refused call launches nothing."""
    from marigold_amd import _lib as L, image
    mi = image.ModelImage(models["depth", False])
    try:
        u8 = _u8(*PICTURE_HW)
        out = torch.full((1,) + PICTURE_HW, -3.0, device="cuda")
        for tiled, size, words in ((L.MgTiledOpts(1, 1, 16, 32), PICTURE_HW, "the guide configuration runs 4 pictures per call"),
                                   (L.MgTiledOpts(0, 1, 16, 72), PICTURE_HW, "mg_tile_plan: the overlap 72 exceeds half the tile length 128"),
                                   (L.MgTiledOpts(0, 1, 16, 32), (64, 128), "mg_model_predict_out")):
            rc = lib.mg_model_predict_tiled(mi.handle, u8.data_ptr(), 1, size[0], size[1], 0, 1, 1, ctypes.byref(tiled), None, None, out.data_ptr(),
                                            None, None, None, None, None, None)
            msg = lib.mg_last_error().decode()
            assert rc != 0 and msg.startswith("mg_model_predict_tiled:") and words in msg, msg
        torch.cuda.synchronize()
        assert bool((out == -3.0).all())
    finally:
        mi.close()


# ---- the C host ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_tiled(tmp_path_factory):
    """examples/host_tiled.cpp, built as the ``host_picture`` fixture of tests/test_gpu_predict_out_c_host.py builds its example."""
    return c_hosts.build_example("host_tiled", tmp_path_factory.mktemp("host_tiled"))


def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


@pytest.mark.parametrize("kind,E,guide_res", [("depth", 3, 128), ("normals", 1, 0)], ids=["depth-E3", "normals-E1"])
def test_c_host_tiled(lib, models, host_tiled, tmp_path, kind, E, guide_res):
    """examples/host_tiled.cpp in a fresh process: the files it writes, read back.  The program takes the first configuration of the
    tile size with the most tiles per call - normals: E = 1, K = 2 - and for depth the guide configuration with that one's members;
    the depth image of this case holds the two E = 3 configurations only (guide, and tiles with K = 2).  The last tile runs on the
    one-picture configuration of the same members, which both images hold."""
    from marigold_amd import image
    H, W = PICTURE_HW
    path = models[kind, False]
    K = 2
    if kind == "depth":
        path = str(tmp_path / "depth3.mgimg")
        image.export_model_image(_tiny_pipe("depth"), path, configs=_configs(DEPTH_CONFIGS[2:4]))
    prefix, lut_path, raw = str(tmp_path / "out"), str(tmp_path / "spectral.lut"), str(tmp_path / "image.u8")
    image.export_color_table("Spectral", lut_path)
    np.asarray(_pil(H, W)).tofile(raw)
    args = [host_tiled, path, raw, str(H), str(W), str(SEED), str(TILE[0]), str(TILE[1]), str(OVERLAP[0]), str(OVERLAP[1]), str(guide_res), prefix,
            str(H), str(W), "0"] + ([lut_path] if kind == "depth" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[predict_tiled C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ref = _reference(kind, E, K, guide_res or None, SEED, False)
    C = 1 if kind == "depth" else 3
    pred = np.fromfile(prefix + ".f32", dtype=np.float32).reshape((C, H, W))
    unc = np.fromfile(prefix + ".unc.f32", dtype=np.float32).reshape(H, W) if E > 1 else None
    assert os.path.exists(prefix + ".unc.f32") == (E > 1) and os.path.exists(prefix + ".pgm") == (kind == "depth")
    u16 = _pnm(prefix + ".pgm", b"P5", H, W, 65535, ">u2", 1).astype(np.uint16) if kind == "depth" else None
    pic = _pnm(prefix + ".ppm", b"P6", H, W, 255, np.uint8, 3)
    flagged = int(r.stdout.split("degenerate tiles: ")[1].split(";")[0]) if kind == "depth" else None
    _check(kind, E, (pred, unc, u16, pic, flagged), ref)
