"""The native noise generator on a real MI355X: MG_OP_RANDN (csrc/randn.hip) in both library builds against the numpy restatement
of tests/philox_reference.py, ``NativeNoise`` behind the pipelines' ``generator=`` argument, and ``mg_model_predict`` from a C host
(examples/host_map.cpp) against the Python pipeline.

Bounds, and where they come from.
* Words (mode 1): integer arithmetic - bit equality with the restatement, which first has to reproduce Random123's known answers.
* Normals against float64 Box-Muller on the same words: 1e-5 absolute.  r = sqrt(-2 ln u) <= 5.65; logf, sqrtf and sincospif are
  within a few ulp of float64, so the error in r is a few ulp of 5.65 (about 2e-6) and the error in the unit factor a few ulp of 1,
  times r (about 2e-6).  The largest deviation seen is printed.
* Slicing and the 16-bit store: the value of an element depends on (seed, stream, index) alone and the 16-bit store rounds the fp32
  value to nearest even like ``tensor.to(dtype)`` - bit equality.
* Moments of 2^20 values of a fixed seed (deterministic): |mean| < 5 / sqrt(n), |var - 1| < 5 sqrt(2 / n) - five standard errors of
  the sample mean and variance of a unit normal -, max |z| <= 5.66 (the largest value u = 2^-23 can give is 5.647).
* Pipelines and the C host: the same kernels on the same inputs in the same order - bit equality.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests import c_hosts
from tests import philox_reference as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUILDS = [False, True]   # the fp16-operand library?
BUILD_IDS = ["bf16lib", "fp16lib"]
SEED_HI = 0xFEDCBA9876543210   # high bits set
GUARD = 8                       # untouched elements either side of every destination


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    P.check_known_answers()   # the restatement judges the kernel only after it reproduces the published vectors
    return {False: L.init(0), True: L.init(0, True)}


def _draw(lib, n, seed, stream=0, offset=0, dtype=torch.float32, words=False, misalign=0):
    """One MG_OP_RANDN into the middle of a guarded buffer whose destination starts ``misalign`` elements past a 16-byte boundary;
    -> the n elements (a copy).  The guards must come back untouched."""
    from marigold_amd import ops as O
    dt = torch.int32 if words else dtype
    per16 = 16 // torch.empty(0, dtype=dt).element_size()
    lead = per16 * -(-GUARD // per16) + misalign
    buf = torch.full((lead + n + GUARD,), 77, dtype=dt, device="cuda")
    dst = buf[lead:lead + n]
    assert buf.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == misalign * dst.element_size() % 16
    O.launch(O.randn(dst, n=n, seed=seed, stream=stream, offset=offset, words=words, out16=(not words) and dtype != torch.float32), lib=lib)
    torch.cuda.synchronize()
    assert bool((buf[:lead] == 77).all()) and bool((buf[lead + n:] == 77).all()), "a store outside [dst, dst + n)"
    return dst.clone()


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy()


# ---- the words ---------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_words_match_the_restatement(libs, f16):
    lib = libs[f16]
    cases = [(n, offset, 0, 7, 0) for n in (1, 3, 4, 5, 1023, 4096) for offset in (0, 1, 2, 3, 7)]
    cases += [(n, offset, 0, 7, mis) for n in (1, 5, 1023) for offset in (0, 3) for mis in (1, 2, 3)]           # an unaligned dst
    cases += [(1023, 2, stream, 7, 0) for stream in (1, (1 << 32) + 5)]
    cases += [(1023, 1, (1 << 32) + 5, SEED_HI, 1), (4096, 0, 0, SEED_HI, 0), (5, 3, 1, (1 << 64) - 1, 0)]      # a seed with high bits set
    cases += [(8, (1 << 34) - 2, 0, 7, 0), (8, (1 << 34) - 2, (1 << 32) + 5, SEED_HI, 0)]                      # the block index crosses 2^32
    for n, offset, stream, seed, mis in cases:
        got = _draw(lib, n, seed, stream, offset, words=True, misalign=mis).cpu().numpy().view(np.uint32)
        want = P.words(seed, stream, offset, n)
        assert np.array_equal(got, want), f"n={n} offset={offset} stream={stream} seed={seed:#x} misalign={mis}"
    # more than one round of the grid-stride loop: 2048 workgroups x 256 lanes x 4 elements, and a tail
    n = 2048 * 256 * 4 + 4 * 300 + 3
    got = _draw(lib, n, 11, 3, 5, words=True).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, P.words(11, 3, 5, n))


# ---- the normals -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_normals_against_float64_box_muller(libs, f16):
    lib = libs[f16]
    worst = 0.0
    for n, offset, stream, seed, mis in ((1 << 20, 0, 0, 2024, 0), (1023, 3, (1 << 32) + 5, SEED_HI, 1), (5, 2, 1, 7, 0), (1, 7, 0, 7, 3),
                                         (8, (1 << 34) - 2, 0, 7, 0)):
        got = _draw(lib, n, seed, stream, offset, misalign=mis).cpu().numpy().astype(np.float64)
        dev = float(np.abs(got - P.normals(seed, stream, offset, n)).max())
        print(f"[native noise] {BUILD_IDS[f16]} n={n} offset={offset}: max |z - float64 Box-Muller| = {dev:.3e}")
        worst = max(worst, dev)
    assert worst <= 1e-5, worst


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_a_slice_is_the_slice_of_a_larger_draw(libs, f16):
    lib = libs[f16]
    op16 = torch.float16 if f16 else torch.bfloat16
    base, total = 5, 4099
    for dtype in (torch.float32, op16):
        whole = _bits(_draw(lib, total, SEED_HI, 2, base, dtype=dtype))
        for a, m, mis in ((0, total, 1), (0, 1, 0), (1, 3, 0), (2, 4, 2), (3, 5, 3), (6, 1023, 0), (1027, 3072, 0), (4095, 4, 1), (4098, 1, 0)):
            part = _bits(_draw(lib, m, SEED_HI, 2, base + a, dtype=dtype, misalign=mis))
            assert np.array_equal(part, whole[a:a + m]), f"{dtype} [{a}, +{m}) misalign {mis}"
        assert not np.array_equal(whole, _bits(_draw(lib, total, SEED_HI, 3, base, dtype=dtype)))   # another stream: other values


@pytest.mark.parametrize("f16", BUILDS, ids=BUILD_IDS)
def test_the_16_bit_store_rounds_like_tensor_to(libs, f16):
    lib = libs[f16]
    op16 = torch.float16 if f16 else torch.bfloat16
    for n, offset, mis in ((1 << 16, 0, 0), (1023, 3, 1), (5, 2, 3)):
        z32 = _draw(lib, n, 99, 1, offset, misalign=mis % 4)
        z16 = _draw(lib, n, 99, 1, offset, dtype=op16, misalign=mis)
        assert z16.dtype == op16 and np.array_equal(_bits(z16), _bits(z32.to(op16)))
        assert np.array_equal(_bits(z16), _bits(z32.cpu().to(op16)))   # ... and like the host's conversion


def test_moments(libs):
    n = 1 << 20
    z = _draw(libs[False], n, 20240229).cpu().numpy().astype(np.float64)
    mean, var, top = z.mean(), z.var(), np.abs(z).max()
    print(f"[native noise] 2^20 values: mean {mean:+.3e} (bound {5 / np.sqrt(n):.3e}), var - 1 {var - 1:+.3e} (bound {5 * np.sqrt(2 / n):.3e}), max |z| {top:.4f}")
    assert np.isfinite(z).all()
    assert abs(mean) < 5 / np.sqrt(n)
    assert abs(var - 1) < 5 * np.sqrt(2 / n)
    assert top <= 5.66


def test_native_randn_and_the_c_call(libs):
    """``native_randn``: the op behind a tensor of any shape, in each dtype through the library of that operand type; ``mg_randn``: the
    op as a C call."""
    from marigold_amd import native_randn
    from marigold_amd import ops as O
    want = P.normals(7, 2, 5, 3 * 4 * 9).reshape(3, 4, 9)
    z = native_randn((3, 4, 9), 7, stream=2, offset=5, device="cuda:0")
    assert z.dtype == torch.float32 and z.is_cuda and tuple(z.shape) == (3, 4, 9) and np.abs(z.cpu().numpy() - want).max() <= 1e-5
    for dtype in (torch.bfloat16, torch.float16):
        assert np.array_equal(_bits(native_randn((3, 4, 9), 7, stream=2, offset=5, dtype=dtype)), _bits(z.to(dtype)))
    assert native_randn((0, 4), 1).numel() == 0
    assert torch.equal(native_randn((8,), -1), native_randn((8,), (1 << 64) - 1))   # seeds are 64 bits
    out = torch.zeros(108, device="cuda")
    rc = libs[False].mg_randn(7, 2, 5, 108, out.data_ptr(), 0, O.current_stream_handle())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, z.flatten())


# ---- the pipelines -----------------------------------------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind, lcm=False):
    """The tiny synthetic model of tests/test_gpu_pipeline.py behind a pipeline (2 denoising steps, no processing resolution)."""
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.schedulers import LCMScheduler
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=LCMScheduler() if lcm else None, default_denoising_steps=2,
                                      default_processing_resolution=0).to("cuda:0")


def _pil(h, w, seed):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _map_of(out):
    return out.depth_np if hasattr(out, "depth_np") else out.normals_np


@pytest.mark.parametrize("kind", ["depth", "normals"])
def test_pipeline_with_native_noise(libs, kind):
    import marigold_amd as M
    pipe = _tiny_pipe(kind)
    img = _pil(64, 128, 3)
    kw = dict(ensemble_size=2, show_progress_bar=False, **({"color_map": None} if kind == "depth" else {}))
    a = _map_of(pipe(img, generator=M.NativeNoise(7), **kw))
    b = _map_of(pipe(img, generator=M.NativeNoise(7), **kw))
    assert np.isfinite(a).all() and np.array_equal(a, b)
    c = _map_of(pipe(img, init_latents=M.native_randn((2, 4, 8, 16), 7, device="cuda:0"), **kw))
    assert np.array_equal(a, c)
    assert not np.array_equal(a, _map_of(pipe(img, generator=M.NativeNoise(8), **kw)))
    g = M.NativeNoise(7)
    pipe(img, generator=g, **kw)
    assert g.next_stream == 1   # DDIM: one draw per call
    assert np.array_equal(_map_of(pipe(img, generator=g.manual_seed(7), **kw)), a)
    # a torch.Generator still draws torch's stream
    t = _map_of(pipe(img, generator=torch.Generator(device="cuda:0").manual_seed(7), **kw))
    lat = torch.randn((2, 4, 8, 16), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(7))
    assert np.array_equal(t, _map_of(pipe(img, init_latents=lat, **kw))) and not np.array_equal(t, a)


def test_map_images_with_native_noise(libs):
    import marigold_amd as M
    pipe = _tiny_pipe("depth")
    imgs = [_pil(64, 128, 10 + k) for k in range(3)]
    gens = lambda: [M.NativeNoise(100 + k) for k in range(3)]   # noqa: E731
    kw = dict(ensemble_size=2, color_map=None, show_progress_bar=False)
    alone = [pipe(im, generator=g, **kw).depth_np for im, g in zip(imgs, gens())]
    got = [o.depth_np for o in pipe.map_images(imgs, generators=gens(), in_flight=2, **kw)]
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(alone, got))
    # images_per_program = 2: every image's draws are those of its lone call, and so is its map
    draws = []
    base = pipe._randn
    pipe._randn = lambda shape, g: draws.append(base(shape, g)) or draws[-1]
    try:
        got = [o.depth_np for o in pipe.map_images(imgs, generators=gens(), images_per_program=2, in_flight=1, **kw)]
    finally:
        del pipe._randn
    assert len(draws) == 3 and all(torch.equal(d, M.native_randn((2, 4, 8, 16), 100 + k, device="cuda:0")) for k, d in enumerate(draws))
    assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(alone, got))


def test_lcm_step_noise_is_the_next_stream(libs):
    """LCM at T = 2: one noised step - its noise is stream 1 of the seed, the initial latents stream 0."""
    import marigold_amd as M
    pipe = _tiny_pipe("depth", lcm=True)
    img = _pil(64, 128, 4)
    draws = []
    base = pipe._randn
    pipe._randn = lambda shape, g: draws.append(base(shape, g)) or draws[-1]
    g = M.NativeNoise(21)
    try:
        a = pipe(img, denoising_steps=2, ensemble_size=2, color_map=None, show_progress_bar=False, generator=g).depth_np
    finally:
        del pipe._randn
    assert len(draws) == 2 and g.next_stream == 2
    lat, nz = (M.native_randn((2, 4, 8, 16), 21, stream=s, device="cuda:0") for s in (0, 1))
    assert torch.equal(draws[0], lat) and torch.equal(draws[1], nz) and not torch.equal(lat, nz)
    prog = pipe.unet.denoise_program(2, 8, 16, pipe.scheduler, 2, rgb_broadcast=True)
    assert len(prog.noises) == 1 and torch.equal(prog.noises[0], nz)   # what the program consumed
    from marigold_amd.util.image_util import InterpolationMode
    rgb, _ = pipe._preprocess(img, 0, InterpolationMode.BILINEAR)
    members = pipe.single_infer(rgb.expand(2, -1, -1, -1), 2, None, False, init_latents=lat, step_noises=[nz])
    from marigold_amd.ensemble import ensemble_depth
    assert np.array_equal(ensemble_depth(members)[0].squeeze().cpu().numpy().clip(0, 1), a)


# ---- the C host --------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def host_map(tmp_path_factory):
    """examples/host_map.cpp, built as tests/test_gpu_pipeline.py::test_model_image_from_a_c_host builds its example."""
    return c_hosts.build_example("host_map", tmp_path_factory.mktemp("host_map"))


def _run_host(exe, tmp_path, pipe, pil, model_hw, E, seed, **export_kw):
    """Export ``pipe`` for ``model_hw`` and E members, run the C host on the bytes of ``pil`` in a fresh process -> (its
    CompletedProcess, the path of its output)."""
    from marigold_amd import image
    path, raw, out = str(tmp_path / "model.mgimg"), str(tmp_path / "image.u8"), str(tmp_path / "pred.f32")
    image.export_model_image(pipe, path, ensemble_size=E, height=model_hw[0], width=model_hw[1], **export_kw)
    np.asarray(pil).tofile(raw)
    r = subprocess.run([exe, path, raw, str(pil.height), str(pil.width), str(seed), out], capture_output=True, text=True, timeout=120)
    print("[native noise] C host: " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    return r, out


def test_c_host_depth(libs, host_map, tmp_path):
    """Depth, E = 3, the picture at the model's size: the bytes go through the IEEE-division normalisation, as in ``_preprocess``."""
    import marigold_amd as M
    pipe = _tiny_pipe("depth")
    pil = _pil(64, 128, 5)
    r, out = _run_host(host_map, tmp_path, pipe, pil, (64, 128), 3, 31)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = np.fromfile(out, dtype=np.float32).reshape(64, 128)
    ref = pipe(pil, denoising_steps=2, ensemble_size=3, processing_res=0, match_input_res=False, color_map=None, show_progress_bar=False,
               generator=M.NativeNoise(31)).depth_np
    assert np.array_equal(got, ref)
    pgm = open(out + ".pgm", "rb").read()
    assert pgm.startswith(b"P5\n128 64\n65535\n") and len(pgm) == 16 + 2 * 64 * 128
    assert np.array_equal(np.frombuffer(pgm[16:], dtype=">u2").reshape(64, 128), (ref * 65535.0).astype(np.uint16))


def test_c_host_depth_resampled(libs, host_map, tmp_path):
    """96 x 128 bytes into a 48 x 64 model: bilinear on the device and the reciprocal normalisation - what ``_preprocess`` chooses for
    ``processing_res=64`` - and 2 ** 63 + 5 as the seed: all 64 bits reach the key."""
    import marigold_amd as M
    pipe = _tiny_pipe("depth")
    pil = _pil(96, 128, 6)
    seed = (1 << 63) + 5
    r, out = _run_host(host_map, tmp_path, pipe, pil, (48, 64), 2, seed)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = np.fromfile(out, dtype=np.float32).reshape(48, 64)
    ref = pipe(pil, denoising_steps=2, ensemble_size=2, processing_res=64, match_input_res=False, color_map=None, show_progress_bar=False,
               generator=M.NativeNoise(seed)).depth_np
    assert ref.shape == (48, 64) and np.array_equal(got, ref)
    assert not np.array_equal(ref, pipe(pil, denoising_steps=2, ensemble_size=2, processing_res=64, match_input_res=False, color_map=None,
                                        show_progress_bar=False, generator=M.NativeNoise(5)).depth_np)


def test_c_host_normals(libs, host_map, tmp_path):
    import marigold_amd as M
    pipe = _tiny_pipe("normals")
    pil = _pil(64, 128, 7)
    r, out = _run_host(host_map, tmp_path, pipe, pil, (64, 128), 2, 77)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    got = np.fromfile(out, dtype=np.float32).reshape(3, 64, 128)
    ref = pipe(pil, denoising_steps=2, ensemble_size=2, processing_res=0, match_input_res=False, show_progress_bar=False,
               generator=M.NativeNoise(77)).normals_np
    assert np.array_equal(got, ref)
    assert not os.path.exists(out + ".pgm")


def test_c_host_refuses_an_intrinsic_image_model(libs, host_map, tmp_path):
    pipe = _tiny_pipe("iid")
    r, out = _run_host(host_map, tmp_path, pipe, _pil(64, 128, 8), (64, 128), 1, 1)
    assert r.returncode != 0 and not os.path.exists(out)
    assert "mg_model_predict: intrinsic-image models are not supported yet" in r.stderr


def test_c_call_from_python_lcm_and_one_member(libs, tmp_path):
    """``mg_model_predict`` through ctypes: an LCM image (step noise k = stream k + 1) and a single member (a copy; no uncertainty
    written), each against the pipeline; the resampling temporary is counted by ``mg_model_device_bytes``."""
    import marigold_amd as M
    from marigold_amd import _lib as L, image, ops as O
    lib = libs[False]
    for lcm, E, size, res in ((True, 2, (64, 128), 0), (False, 1, (96, 128), 64)):
        pipe = _tiny_pipe("depth", lcm=lcm)
        pil = _pil(*size, 9)
        H, W = (64, 128) if res == 0 else (48, 64)
        path = str(tmp_path / f"m{E}.mgimg")
        image.export_model_image(pipe, path, ensemble_size=E, height=H, width=W)
        mi = image.ModelImage(path)
        try:
            assert mi.n_noise == (1 if lcm else 0)
            u8 = torch.from_numpy(np.array(pil)).cuda()
            pred = torch.full((H, W), float("nan"), device="cuda")
            unc = torch.full((H, W), -3.0, device="cuda")
            info = (ctypes.c_double * 4)(9, 9, 9, 9)
            before = lib.mg_model_device_bytes(mi.handle)
            L.check(lib.mg_model_predict(mi.handle, u8.data_ptr(), 1, size[0], size[1], 0, int(res != 0), 41, None, pred.data_ptr(),
                                         unc.data_ptr(), info, O.current_stream_handle()), "mg_model_predict", lib)
            torch.cuda.synchronize()
            assert lib.mg_model_device_bytes(mi.handle) - before == (3 * size[0] * W * 4 if res else 0)
            ref = pipe(pil, denoising_steps=2, ensemble_size=E, processing_res=res, match_input_res=False, color_map=None,
                       show_progress_bar=False, generator=M.NativeNoise(41), ensemble_kwargs=dict(output_uncertainty=True))
            assert np.array_equal(pred.cpu().numpy(), ref.depth_np)
            if E > 1:
                assert np.array_equal(unc.cpu().numpy(), ref.uncertainty) and info[1] >= 1
            else:
                assert ref.uncertainty is None and bool((unc == -3.0).all()) and list(info) == [0.0] * 4
        finally:
            mi.close()
