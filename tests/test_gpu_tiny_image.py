"""Model images with the tiny autoencoder (``export_model_image(tiny_vae=True)``) on a real MI355X: every C entry point on a tiny
image against what the Python pipeline returns with the same VAE - ``AutoencoderTinyHIP`` set into the tiny synthetic pipelines of
tests/test_gpu_predict_out_c_host.py - under ``generator=NativeNoise(seed)``.

Every bound is equality (``np.array_equal``): both routes run ``mg_rgb_prepare`` on the same bytes, ``mg_tiny_vae_encode`` on its fp32
output, the same denoising program on the same noise, ``mg_tiny_vae_decode`` (bit-reproducible, a member's result independent of the
batch) and the same output stages.  That is the contract of the AutoencoderKL tests in test_gpu_predict_out_c_host.py,
test_gpu_predict_many_c_host.py, test_gpu_sequence.py, test_gpu_iid_c_host.py and test_gpu_model_configs.py.

Sizes: 64 x 128 (latent 8 x 16) and 30 x 44, where the tiny encoder's ceiling rule (latent 4 x 6, decoded 32 x 48) and the
AutoencoderKL's floor (3 x 5) differ - a loader that floors, or a ``cfg`` that assumes H / 8, fails there; its outputs are taken at
the picture's size (a resize from 32 x 48) and, unclipped, at the decoded size."""
import ctypes
import dataclasses
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
WIDE, ODD = (64, 128), (30, 44)
SEED = (1 << 63) + 31
STRENGTH = 0.25


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind, lcm=False):
    """The tiny synthetic pipeline of the AutoencoderKL tests with the tiny autoencoder set into it."""
    import marigold_amd as M
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.modules import AutoencoderTinyHIP
    from marigold_amd.schedulers import LCMScheduler
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    pipe = M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=LCMScheduler() if lcm else None, default_denoising_steps=4 if lcm else 2,
                                      default_processing_resolution=0).to("cuda:0")
    pipe.set_vae(AutoencoderTinyHIP(syn.synthetic_tiny_vae_state_dict()))
    assert type(pipe.vae) is AutoencoderTinyHIP and pipe.vae.device.type == "cuda"
    return pipe


@functools.lru_cache(maxsize=None)
def _pil(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _u8(h, w, seed=5):
    return torch.from_numpy(np.array(_pil(h, w, seed))).cuda()


@pytest.fixture(scope="module")
def table():
    from marigold_amd.util.image_util import colormap_lut_u8
    return colormap_lut_u8("Spectral")


@pytest.fixture(scope="module")
def models(lib, tmp_path_factory):
    """Tiny model images, exported on first use: ``models(kind, E, size, K=1, lcm=False)`` -> path."""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("tiny_image")
    made = {}

    def get(kind, E, size, K=1, lcm=False):
        key = (kind, E, size, K, lcm)
        if key not in made:
            made[key] = str(d / f"{kind}{E}_{size[0]}x{size[1]}_k{K}{'_lcm' if lcm else ''}.mgimg")
            got = image.export_model_image(_tiny_pipe(kind, lcm), made[key], tiny_vae=True, ensemble_size=E, height=size[0], width=size[1],
                                           images_per_program=K)
            assert got["cfg16"][14] == 1 and got["latent_hw"] == tuple(-(-s // 8) for s in size) and got["step_noises"] == (3 if lcm else 0)
        return made[key]
    return get


@functools.lru_cache(maxsize=None)
def _reference(kind, E, size, res=0, seed=SEED, match=True, lcm=False):
    """The pipeline's output for the picture of ``size`` (computed once per case, shared, never modified)."""
    import marigold_amd as M
    return _tiny_pipe(kind, lcm)(_pil(*size), denoising_steps=4 if lcm else 2, ensemble_size=E, processing_res=res, match_input_res=match,
                                 resample_method="bilinear", generator=M.NativeNoise(seed), ensemble_kwargs=dict(output_uncertainty=True),
                                 show_progress_bar=False)


def _ref_arrays(kind, ref):
    """(map [C, h, w], picture [h, w, 3], uncertainty | None)"""
    if kind == "depth":
        return ref.depth_np[None], np.asarray(ref.depth_colored), ref.uncertainty
    return ref.normals_np, np.asarray(ref.normals_img), ref.uncertainty


def _numpy(ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _check(kind, E, got, ref, size, decoded):
    """(pred, unc, u16, picture) as numpy against the pipeline's output."""
    pred, unc, u16, pic = got
    want, want_pic, want_unc = _ref_arrays(kind, ref)
    assert want.shape == (1 if kind == "depth" else 3,) + size and np.isfinite(want).all() and want.max() > want.min()
    assert np.array_equal(pred, want)
    assert pic.shape == size + (3,) and np.array_equal(pic, want_pic)
    if E > 1:
        assert want_unc.shape == decoded and np.array_equal(unc, want_unc)   # at the decoded size
    else:
        assert unc is None and want_unc is None
    if kind == "depth":
        assert np.array_equal(u16, (ref.depth_np * 65535.0).astype(np.uint16)) and u16.max() > u16.min()
    else:
        assert u16 is None


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w)


def _out(mi, kind, u8, seed, size, lut, **kw):
    lut = lut if kind == "depth" else None
    return _numpy(mi.predict_out(u8, seed, out_size=size, out_mode="bilinear", mode="bilinear", lut=lut, u16=kind == "depth", picture=True, **kw)[:4])


# ---- mg_model_predict_out, mg_model_predict, mg_model_predict_iid ------------------------------------------------------------------

# (kind, E, the model's size, LCM, [(picture size, processing_res)])
CASES = [("depth", 1, WIDE, False, [(WIDE, 0), ((96, 192), 128)]), ("depth", 3, ODD, False, [(ODD, 0)]), ("normals", 2, ODD, False, [(ODD, 0)]),
         ("depth", 1, ODD, True, [(ODD, 0)])]


@pytest.mark.parametrize("kind,E,hw,lcm,pictures", CASES, ids=[f"{k}-E{e}-{s[0]}x{s[1]}" + ("-lcm" if l else "") for k, e, s, l, _ in CASES])
def test_predict_out_matches_the_pipeline(lib, models, table, kind, E, hw, lcm, pictures):
    from marigold_amd import _lib as L, image, ops as O
    mi = image.ModelImage(models(kind, E, hw, lcm=lcm))
    lut = torch.from_numpy(table).cuda()
    decoded = tuple(8 * -(-s // 8) for s in hw)
    try:
        assert (mi.B, mi.H, mi.W, mi.h, mi.w, mi.Hout, mi.Wout) == (E,) + hw + tuple(d // 8 for d in decoded) + decoded
        assert mi.configs[0][14] == 1 and mi.n_noise == (3 if lcm else 0) and mi.shared_bytes > 0
        for size, res in pictures:
            got = _out(mi, kind, _u8(*size), SEED, size, lut)
            _check(kind, E, got, _reference(kind, E, size, res, lcm=lcm), size, decoded)
        # mg_model_predict: the map at the DECODED size, unclipped - the pipeline's with match_input_res=False
        size, res = pictures[-1]
        C = mi.pred_channels
        plain = torch.full((C,) + decoded, float("nan"), device="cuda")
        L.check(lib.mg_model_predict(mi.handle, _u8(*size).data_ptr(), 1, size[0], size[1], 0, int(size != hw), SEED, None, plain.data_ptr(), None, None,
                                     O.current_stream_handle()), "mg_model_predict", lib)
        want = _ref_arrays(kind, _reference(kind, E, size, res, match=False, lcm=lcm))[0]
        assert want.shape == (C,) + decoded and np.array_equal(_numpy([plain])[0], want)
    finally:
        mi.close()


@pytest.mark.parametrize("hw", [WIDE, ODD], ids=["64x128", "30x44"])
def test_predict_iid_matches_the_pipeline(lib, models, hw):
    """An intrinsic-image model, one member: both targets of the decoder's batch [2, 4, h, w] in one tiny decode call."""
    from marigold_amd import _lib as L, image
    pipe = _tiny_pipe("iid")
    mi = image.ModelImage(models("iid", 1, hw))
    decoded = tuple(8 * -(-s // 8) for s in hw)
    try:
        assert mi.pred_channels == 6 and (mi.Hout, mi.Wout) == decoded
        arrays = lambda out, field="array": np.concatenate([getattr(out[name], field) for name in out.target_names])   # noqa: E731
        # at the decoded size, and resized to the picture's
        ref = _reference("iid", 1, hw, match=False)
        pred, unc, pics = mi.predict_iid(_u8(*hw), SEED, pictures=True)
        got = _numpy([pred, pics])
        assert unc is None and got[0].shape == (6,) + decoded and np.isfinite(got[0]).all() and np.array_equal(got[0], arrays(ref))
        assert np.array_equal(got[1], np.stack([np.asarray(ref[name].image) for name in ref.target_names]))
        ref = _reference("iid", 1, hw, match=True)
        pred, _unc, pics = mi.predict_iid(_u8(*hw), SEED, opts=L.MgIidOpts(out_h=hw[0], out_w=hw[1], out_mode=0), pictures=True)
        got = _numpy([pred, pics])
        assert got[0].shape == (6,) + hw and np.array_equal(got[0], arrays(ref))
        assert np.array_equal(got[1], np.stack([np.asarray(ref[name].image) for name in ref.target_names]))
    finally:
        mi.close()
    assert pipe.vae.latent_hw(hw) == tuple(d // 8 for d in decoded)


# ---- mg_model_vae_encode / mg_model_vae_decode -------------------------------------------------------------------------------------


@pytest.mark.parametrize("hw", [WIDE, ODD], ids=["64x128", "30x44"])
def test_staged_entry_points_match_the_module(lib, models, hw):
    from marigold_amd import _lib as L, image
    from marigold_amd.util.image_util import prepare_rgb_device
    vae = _tiny_pipe("depth").vae
    mi = image.ModelImage(models("depth", 3, hw))
    try:
        rgb = prepare_rgb_device(_u8(*hw), None, reciprocal=False)   # what _preprocess hands the VAE: fp32 [1, 3, H, W] in [-1, 1]
        assert rgb.dtype == torch.float32 and tuple(rgb.shape) == (1, 3) + hw
        lat = mi.encode(rgb)
        want = vae.encode_rgb_latent(rgb)
        assert lat.shape == want.shape == (1, 4, mi.h, mi.w) and torch.equal(lat, want) and bool(torch.isfinite(lat).all())
        z = torch.randn(3, 4, mi.h, mi.w, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        dec = mi.decode(z)
        want = vae.decode(z, post=L.POST_DEPTH)
        assert dec.shape == want.shape == (3, 1, mi.Hout, mi.Wout) and torch.equal(dec, want) and float(dec.max()) > float(dec.min())
        # a member's result does not depend on the batch it was decoded in
        assert torch.equal(vae.decode(z[1:2], post=L.POST_DEPTH), dec[1:2])
    finally:
        mi.close()


# ---- mg_model_predict_many ---------------------------------------------------------------------------------------------------------

SEEDS = [(1 << 63) + 11, 7, 123456789]
PICTURE_SEEDS = [5, 6, 7]


def test_predict_many_matches_map_images(lib, models, table):
    """K = 3 at 30 x 44: a full call, and n = 2 - whose pictures are those of the full group, bit for bit, and nothing beyond row 1 is written."""
    import marigold_amd as M
    from marigold_amd import image
    pipe = _tiny_pipe("depth")
    lut = torch.from_numpy(table).cuda()
    refs = list(pipe.map_images([_pil(*ODD, s) for s in PICTURE_SEEDS], generators=[M.NativeNoise(s) for s in SEEDS], images_per_program=3, in_flight=1,
                                denoising_steps=2, ensemble_size=1, processing_res=0, match_input_res=True, resample_method="bilinear",
                                show_progress_bar=False))
    mi = image.ModelImage(models("depth", 1, ODD, K=3))
    try:
        assert (mi.K, mi.B, mi.h, mi.w) == (3, 1, 4, 6)
        u8s = [_u8(*ODD, s) for s in PICTURE_SEEDS]
        for n in (3, 2, 3):
            got = mi.predict_many(u8s[:n], SEEDS[:n], out_size=ODD, out_mode="bilinear", lut=lut, u16=True, picture=True)
            arrays = _numpy(got[:4])
            assert arrays[0].shape == (n, 1) + ODD
            for i in range(n):
                _check("depth", 1, tuple(None if a is None else a[i] for a in arrays), refs[i], ODD, (32, 48))
        assert not np.array_equal(arrays[0][0], arrays[0][1])
        # an image of K pictures per call refuses the one-picture entry points by name
        rc = lib.mg_model_predict_out(mi.handle, u8s[0].data_ptr(), 1, 30, 44, 0, 0, 1, None, None, lut.data_ptr(), None, None, None, None, None)
        assert rc != 0 and "use mg_model_predict_many" in lib.mg_last_error().decode()
    finally:
        mi.close()


# ---- mg_model_predict_next ---------------------------------------------------------------------------------------------------------

VIDEO = (5, 6, 6)


def test_predict_next_matches_map_video_and_resets(lib, models, table):
    import marigold_amd as M
    from marigold_amd import image
    pipe = _tiny_pipe("depth")
    lut = torch.from_numpy(table).cuda()
    seeds = [SEED + 100 + k for k in range(3)]
    refs = list(pipe.map_video([_pil(*ODD, p) for p in VIDEO], strength=STRENGTH, generators=[M.NativeNoise(s) for s in seeds], in_flight=1,
                               match_input_res=True, denoising_steps=2, ensemble_size=1, processing_res=0, show_progress_bar=False))
    assert not np.array_equal(refs[1].depth_np, refs[2].depth_np)   # the same picture twice: the carry and the seed make another map
    path = models("depth", 1, ODD)
    mi, fresh = image.ModelImage(path), None
    try:
        base = mi.device_bytes
        frames = [_out(mi, "depth", _u8(*ODD, p), s, ODD, lut, _next=STRENGTH) for p, s in zip(VIDEO, seeds)]
        for got, ref in zip(frames, refs):
            _check("depth", 1, got, ref, ODD, (32, 48))
        assert mi.device_bytes - base >= 4 * 4 * 6 * 4   # the carried latent: the x slot [1, 4, 4, 6] fp32 (and the resize's temporaries)
        # seq_reset: the handle is a fresh one again
        mi.seq_reset()
        fresh = image.ModelImage(path)
        for p, s in zip(VIDEO[1:], seeds[1:]):
            _same(_out(mi, "depth", _u8(*ODD, p), s, ODD, lut, _next=STRENGTH), _out(fresh, "depth", _u8(*ODD, p), s, ODD, lut, _next=STRENGTH))
        mi.seq_reset()
        _same(_out(mi, "depth", _u8(*ODD, VIDEO[0]), seeds[0], ODD, lut, _next=STRENGTH), frames[0])
    finally:
        mi.close()
        if fresh is not None:
            fresh.close()


# ---- configurations, replicas, scratch ---------------------------------------------------------------------------------------------


def test_two_sizes_in_one_image_and_on_a_replica(lib, models, table, tmp_path):
    """One image of 64 x 128 (E = 1) and 30 x 44 (E = 3), run A, B, A and then on a replica, against the single-configuration images."""
    from marigold_amd import image
    lut = torch.from_numpy(table).cuda()
    cfgs = [dict(ensemble_size=1, height=WIDE[0], width=WIDE[1], denoising_steps=2), dict(ensemble_size=3, height=ODD[0], width=ODD[1], denoising_steps=2)]
    want = []
    for c in cfgs:
        size = (c["height"], c["width"])
        one = image.ModelImage(models("depth", c["ensemble_size"], size))
        try:
            want.append(_out(one, "depth", _u8(*size), SEED + 7, size, lut))
        finally:
            one.close()
    info = image.export_model_image(_tiny_pipe("depth"), str(tmp_path / "multi.mgimg"), tiny_vae=True, configs=cfgs)
    assert [c["cfg16"][14] for c in info["configs"]] == [1, 1] and [c["latent_hw"] for c in info["configs"]] == [(8, 16), (4, 6)]
    mi = image.ModelImage(info["path"])
    rep = None
    try:
        assert len(mi.configs) == 2 and mi.shared_bytes == info["shared_bytes"] and mi.device_bytes == info["private_bytes"]
        for i in (0, 1, 0):
            size = (cfgs[i]["height"], cfgs[i]["width"])
            assert mi.find(*size) == i
            _same(_out(mi.select(i), "depth", _u8(*size), SEED + 7, size, lut), want[i])
        rep = mi.select(1).replica()
        assert rep.shared_bytes == mi.shared_bytes and rep.selected == 1
        mi.close()   # the parent first: the replica keeps the weights, the tiny network among them
        for i in (1, 0):
            size = (cfgs[i]["height"], cfgs[i]["width"])
            _same(_out(rep.select(i), "depth", _u8(*size), SEED + 7, size, lut), want[i])
        assert want[1][1] is not None and want[0][1] is None   # E = 3 has an uncertainty
    finally:
        mi.close()
        if rep is not None:
            rep.close()
    torch.cuda.synchronize()


def test_results_do_not_depend_on_what_scratch_held(lib, models, table):
    """The slots and workspaces of the tiny calls are scratch: the same call after the handle's scratch was filled with NaN bytes."""
    from marigold_amd import _lib as L, image, ops as O
    lut = torch.from_numpy(table).cuda()
    path = models("depth", 3, ODD)
    fresh = image.ModelImage(path)
    mi = image.ModelImage(path)
    try:
        want = _out(fresh, "depth", _u8(*ODD), SEED, ODD, lut)
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        for _ in range(2):   # a scratch as allocated, then one that a call has used
            L.check(lib.mg_model_scratch_fill(mi.handle, 0xFF, O.current_stream_handle()), "mg_model_scratch_fill", lib)
            _same(_out(mi, "depth", _u8(*ODD), SEED, ODD, lut), want)
        host = image.ModelImage(path, device=-1)
        try:
            assert lib.mg_model_scratch_fill(host.handle, 0xFF, None) != 0 and lib.mg_last_error().decode().startswith("mg_model_scratch_fill:")
        finally:
            host.close()
    finally:
        fresh.close()
        mi.close()


# ---- the C host --------------------------------------------------------------------------------------------------------------------


def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


def test_c_host_picture_runs_a_tiny_image_unchanged(lib, models, tmp_path_factory, tmp_path):
    """examples/host_picture.cpp, built as tests/test_gpu_predict_out_c_host.py builds it, in a fresh process on the 30 x 44 tiny depth image
    with three members: the files it writes against the pipeline's output."""
    from marigold_amd import image
    exe = c_hosts.build_example("host_picture", tmp_path_factory.mktemp("host_picture_tiny"))
    raw, prefix, lut_path = str(tmp_path / "image.u8"), str(tmp_path / "out"), str(tmp_path / "spectral.lut")
    np.asarray(_pil(*ODD)).tofile(raw)
    image.export_color_table("Spectral", lut_path)
    r = subprocess.run([exe, models("depth", 3, ODD), raw, str(ODD[0]), str(ODD[1]), str(SEED), prefix, str(ODD[0]), str(ODD[1]), "0", lut_path],
                       capture_output=True, text=True, timeout=120)
    print("[tiny image C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    pred = np.fromfile(prefix + ".f32", dtype=np.float32).reshape((1,) + ODD)
    unc = np.fromfile(prefix + ".unc.f32", dtype=np.float32).reshape(32, 48)
    u16 = _pnm(prefix + ".pgm", b"P5", ODD[0], ODD[1], 65535, ">u2", 1).astype(np.uint16)
    pic = _pnm(prefix + ".ppm", b"P6", ODD[0], ODD[1], 255, np.uint8, 3)
    _check("depth", 3, (pred, unc, u16, pic), _reference("depth", 3, ODD), ODD, (32, 48))
