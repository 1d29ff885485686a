"""``mg_model_predict_iid`` on a real MI355X: the intrinsic-image models from a C host (examples/host_iid.cpp, a fresh process) and
through ctypes (``ModelImage.predict_iid``), every result against the existing Python pipeline called with
``generator=NativeNoise(seed)``.

The bound is equality (``np.array_equal``): both sides run the same kernels on the same inputs in the same order, except the
ensemble, where the C side runs MG_OP_ENS_IID and the pipeline MG_OP_ENS_DEPTH_MEDIAN without alignment - bit-identical by
construction (tests/test_gpu_ens_iid.py).  The models are the tiny synthetic ones of tests/test_gpu_native_noise.py, two steps."""
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

# the lighting model's targets, as tools/iid_output_bench.py sets them
LIGHTING = {"target_names": ["albedo", "shading", "residual"], "albedo": {"prediction_space": "linear"},
            "shading": {"prediction_space": "linear", "up_to_scale": True},
            "residual": {"prediction_space": "linear", "up_to_scale": True}}
LIGHTING_BITS = (0b111, 0b110)   # linear, up to scale


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind, lcm=False):
    """``_tiny_pipe`` of tests/test_gpu_native_noise.py; "iid": the appearance-style model (two targets in sRGB space), "lighting": three
    targets with the linear / up-to-scale flags above."""
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.schedulers import LCMScheduler
    kw = {}
    ucfg = TINY_UNET
    if kind == "iid":
        ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8)
    elif kind == "lighting":
        ucfg = dataclasses.replace(TINY_UNET, in_channels=16, out_channels=12)
        kw["target_properties"] = LIGHTING
    return M.build_synthetic_pipeline("iid" if kind == "lighting" else kind, ucfg, TINY_VAE, scheduler=LCMScheduler() if lcm else None,
                                      default_denoising_steps=2, default_processing_resolution=0, **kw).to("cuda:0")


def _pil(h, w, seed):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _reference(pipe, pil, E, seed, res=0, match=False):
    import marigold_amd as M
    return pipe(pil, denoising_steps=2, ensemble_size=E, processing_res=res, match_input_res=match, generator=M.NativeNoise(seed),
                ensemble_kwargs=dict(output_uncertainty=True), show_progress_bar=False)


def _arrays(out, field="array"):
    return np.concatenate([getattr(out[name], field) for name in out.target_names])


@pytest.fixture(scope="module")
def host_iid(tmp_path_factory):
    """examples/host_iid.cpp, built as the ``host_map`` fixture of tests/test_gpu_native_noise.py builds its example."""
    return c_hosts.build_example("host_iid", tmp_path_factory.mktemp("host_iid"))


def _export(pipe, path, E, hw):
    from marigold_amd import image
    image.export_model_image(pipe, str(path), ensemble_size=E, height=hw[0], width=hw[1])
    return str(path)


def _run_host(exe, model, tmp_path, pil, seed, tag, *extra):
    raw, prefix = str(tmp_path / "image.u8"), str(tmp_path / tag)
    np.asarray(pil).tofile(raw)
    r = subprocess.run([exe, model, raw, str(pil.height), str(pil.width), str(seed), prefix] + [str(a) for a in extra],
                       capture_output=True, text=True, timeout=120)
    print("[iid C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    return r, prefix


def _ppm(path, h, w):
    raw = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert raw.startswith(head) and len(raw) == len(head) + 3 * h * w
    return np.frombuffer(raw[len(head):], dtype=np.uint8).reshape(h, w, 3)


# ---- the C host --------------------------------------------------------------------------------------------------------------


def test_c_host_appearance(lib, host_iid, tmp_path):
    """Two targets in sRGB space, 64 x 128 at the model's size, E = 3: arrays, uncertainties and pictures."""
    pipe = _tiny_pipe("iid")
    pil = _pil(64, 128, 5)
    model = _export(pipe, tmp_path / "model.mgimg", 3, (64, 128))
    r, prefix = _run_host(host_iid, model, tmp_path, pil, 31, "out")
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ref = _reference(pipe, pil, 3, 31)
    got = np.fromfile(prefix + ".f32", dtype=np.float32).reshape(6, 64, 128)
    assert np.isfinite(got).all() and np.array_equal(got, _arrays(ref))
    unc = np.fromfile(prefix + ".unc.f32", dtype=np.float32).reshape(6, 64, 128)
    assert np.array_equal(unc, _arrays(ref, "uncertainty"))
    for t, name in enumerate(ref.target_names):
        assert np.array_equal(_ppm(f"{prefix}.{t}.ppm", 64, 128), np.asarray(ref[name].image))
    assert not os.path.exists(prefix + ".2.ppm")


def test_c_host_lighting_resampled(lib, host_iid, tmp_path):
    """Three targets (albedo linear; shading, residual linear and up to scale), 96 x 128 bytes into a 48 x 64 model and the prediction
    back at 96 x 128 (match_input_res, bilinear); the uncertainty stays at the model's size; 2 ** 63 + 5 as the seed."""
    pipe = _tiny_pipe("lighting")
    pil = _pil(96, 128, 6)
    seed = (1 << 63) + 5
    model = _export(pipe, tmp_path / "model.mgimg", 2, (48, 64))
    r, prefix = _run_host(host_iid, model, tmp_path, pil, seed, "out", *LIGHTING_BITS, 96, 128)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ref = _reference(pipe, pil, 2, seed, res=64, match=True)
    got = np.fromfile(prefix + ".f32", dtype=np.float32).reshape(9, 96, 128)
    assert _arrays(ref).shape == (9, 96, 128) and np.array_equal(got, _arrays(ref))
    unc = np.fromfile(prefix + ".unc.f32", dtype=np.float32)
    assert unc.size == 9 * 48 * 64 and np.array_equal(unc.reshape(9, 48, 64), _arrays(ref, "uncertainty"))
    for t, name in enumerate(ref.target_names):
        assert np.array_equal(_ppm(f"{prefix}.{t}.ppm", 96, 128), np.asarray(ref[name].image))
    # another seed, another prediction
    r2, prefix2 = _run_host(host_iid, model, tmp_path, pil, 5, "other", *LIGHTING_BITS, 96, 128)
    assert r2.returncode == 0, (r2.stdout + r2.stderr)[-2000:]
    assert not np.array_equal(np.fromfile(prefix2 + ".f32", dtype=np.float32).reshape(9, 96, 128), got)


# ---- through ctypes ------------------------------------------------------------------------------------------------------------


def test_one_member_is_a_copy(lib, tmp_path):
    """E = 1: the decoded member as it is; the uncertainty buffer is not written (a sentinel fill survives); pictures are made."""
    from marigold_amd import _lib as L, image, ops as O
    pipe = _tiny_pipe("iid")
    pil = _pil(64, 128, 9)
    mi = image.ModelImage(_export(pipe, tmp_path / "m1.mgimg", 1, (64, 128)))
    try:
        u8 = torch.from_numpy(np.array(pil)).cuda()
        ref = _reference(pipe, pil, 1, 41)
        pred, unc, pics = mi.predict_iid(u8, 41, pictures=True)
        torch.cuda.synchronize()
        assert unc is None and all(ref[name].uncertainty is None for name in ref.target_names)
        assert np.array_equal(pred.cpu().numpy(), _arrays(ref))
        assert np.array_equal(pics.cpu().numpy(), np.stack([np.asarray(ref[name].image) for name in ref.target_names]))
        pred2 = torch.full((6, 64, 128), float("nan"), device="cuda")
        sentinel = torch.full((6, 64, 128), -3.0, device="cuda")
        L.check(lib.mg_model_predict_iid(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 41, None, pred2.data_ptr(), sentinel.data_ptr(), None,
                                         O.current_stream_handle()), "mg_model_predict_iid", lib)
        torch.cuda.synchronize()
        assert torch.equal(pred2, pred) and bool((sentinel == -3.0).all())
        assert mi.predict_iid(u8, 41)[2] is None
    finally:
        mi.close()


def test_lcm_is_refused_as_the_pipeline_refuses_it(lib, tmp_path):
    """The IID pipeline does not accept the LCM scheduler (``_check_inference_step`` -> ``_lcm_policy`` raises, as the reference's
    marigold_iid_pipeline.py:443-447 does), so there is no pipeline result an LCM image could be compared with.  In place of the
    issue's LCM comparison this tests the refusal's counterpart: the C entry refuses an image that draws step noise, with the
    reference's words, before it launches anything."""
    from marigold_amd import image
    pipe = _tiny_pipe("iid", lcm=True)
    pil = _pil(64, 128, 9)
    with pytest.raises(RuntimeError, match="does not support the LCMScheduler"):
        _reference(pipe, pil, 2, 41)
    mi = image.ModelImage(_export(pipe, tmp_path / "lcm.mgimg", 2, (64, 128)))
    try:
        assert mi.n_noise == 1
        u8 = torch.from_numpy(np.array(pil)).cuda()
        pred = torch.full((6, 64, 128), -3.0, device="cuda")
        rc = lib.mg_model_predict_iid(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 41, None, pred.data_ptr(), None, None, None)
        msg = lib.mg_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and msg.startswith("mg_model_predict_iid:") and "does not support the LCMScheduler" in msg
        assert bool((pred == -3.0).all())
    finally:
        mi.close()


def test_temporaries_belong_to_the_model(lib, tmp_path):
    """``mg_model_device_bytes`` grows by exactly what a call needs - the input resampling temporary, and for the output the ensembled
    prediction at the model's size, the resize's intermediate and the picture stage's workspace, each rounded up to 256 bytes - and not
    again at a second identical call; a call that needs less keeps what is there.  The results equal the pipeline's."""
    from marigold_amd import _lib as L, image
    pipe = _tiny_pipe("lighting")
    pil = _pil(96, 128, 6)
    mi = image.ModelImage(_export(pipe, tmp_path / "m2.mgimg", 2, (48, 64)))
    r256 = lambda b: (b + 255) // 256 * 256   # noqa: E731
    try:
        u8 = torch.from_numpy(np.array(pil)).cuda()
        base = lib.mg_model_device_bytes(mi.handle)
        # mean reduction, no resize, no pictures: only the input resampling temporary [3][96][64] fp32
        opts = L.MgIidOpts(reduction=1)
        pred, unc, pics = mi.predict_iid(u8, 7, opts=opts)
        torch.cuda.synchronize()
        step1 = lib.mg_model_device_bytes(mi.handle)
        assert step1 - base == 3 * 96 * 64 * 4 and pics is None
        import marigold_amd as M
        ref = pipe(pil, denoising_steps=2, ensemble_size=2, processing_res=64, match_input_res=False, generator=M.NativeNoise(7),
                   ensemble_kwargs=dict(output_uncertainty=True, reduction="mean"), show_progress_bar=False)
        assert np.array_equal(pred.cpu().numpy(), _arrays(ref)) and np.array_equal(unc.cpu().numpy(), _arrays(ref, "uncertainty"))
        # the whole output stage: + [9][48][64] (ensembled), [9][48][128] (resize intermediate), [3][128] (picture workspace), all fp32
        opts = L.MgIidOpts(linear_bits=LIGHTING_BITS[0], up_to_scale_bits=LIGHTING_BITS[1], out_h=96, out_w=128)
        pred, unc, pics = mi.predict_iid(u8, 7, opts=opts, pictures=True)
        torch.cuda.synchronize()
        step2 = lib.mg_model_device_bytes(mi.handle)
        assert step2 - step1 == r256(9 * 48 * 64 * 4) + r256(9 * 48 * 128 * 4) + r256(3 * L.IID_VIS_PARTS * 4)
        ref = _reference(pipe, pil, 2, 7, res=64, match=True)
        assert np.array_equal(pred.cpu().numpy(), _arrays(ref)) and np.array_equal(unc.cpu().numpy(), _arrays(ref, "uncertainty"))
        assert np.array_equal(pics.cpu().numpy(), np.stack([np.asarray(ref[name].image) for name in ref.target_names]))
        again = mi.predict_iid(u8, 7, opts=opts, pictures=True)
        torch.cuda.synchronize()
        assert lib.mg_model_device_bytes(mi.handle) == step2 and all(torch.equal(a, b) for a, b in zip(again, (pred, unc, pics)))
        mi.predict_iid(u8, 7)   # needs less
        torch.cuda.synchronize()
        assert lib.mg_model_device_bytes(mi.handle) == step2
    finally:
        mi.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------


def test_each_entry_refuses_the_other_kind_of_model(lib, tmp_path):
    """``mg_model_predict_iid`` on a depth image; ``mg_model_predict`` on an intrinsic-image one still answers with its pinned words
    (asserted again here on purpose: the new entry did not open the old one)."""
    from marigold_amd import image
    u8 = torch.from_numpy(np.array(_pil(64, 128, 8))).cuda()
    out = torch.full((6, 64, 128), -3.0, device="cuda")
    mi = image.ModelImage(_export(_tiny_pipe("depth"), tmp_path / "depth.mgimg", 1, (64, 128)))
    try:
        rc = lib.mg_model_predict_iid(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, out.data_ptr(), None, None, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_iid: an intrinsic-image model is required")
    finally:
        mi.close()
    mi = image.ModelImage(_export(_tiny_pipe("iid"), tmp_path / "iid.mgimg", 1, (64, 128)))
    try:
        rc = lib.mg_model_predict(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, out.data_ptr(), None, None, None)
        assert rc != 0 and lib.mg_last_error().decode() == "mg_model_predict: intrinsic-image models are not supported yet"
        # ... and bad options are refused before anything is launched
        from marigold_amd import _lib as L
        for opts, words in ((L.MgIidOpts(reduction=2), "Unrecognized reduction method: 2."), (L.MgIidOpts(out_h=8), "bad output size"),
                            (L.MgIidOpts(linear_bits=4), "a flag names a target beyond the 2"), (L.MgIidOpts(out_mode=3), "out_mode")):
            rc = lib.mg_model_predict_iid(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, ctypes.byref(opts), out.data_ptr(), None, None, None)
            assert rc != 0 and words in lib.mg_last_error().decode(), words
    finally:
        mi.close()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())
