"""The tiny autoencoder on a real MI355X (csrc/tinyvae.hip, modules.AutoencoderTinyHIP) against tests/tiny_vae_reference.py, the
fp64 restatement on the CPU, in both library builds (bf16 and fp16 operands).

Single layer (mg_tiny_conv3x3) - the bound is derived, not tuned: |got - ref| <= u |ref| + 1.01 e per element, ref = the fp64 layer on
the rounded operands, u = 2^-8 (bf16) / 2^-11 (fp16) for the one rounding of the result, e = 580 * 2^-24 * (conv(|x|, |w|) + |bias|
+ |residual|) for the fp32 accumulation of the 576 products, the bias and the residual in any order (ReLU is 1-Lipschitz).
The kernel's tiles are 8 x 32 output pixels (stride 1, also with the fused nearest x2) and 2 x 32 (stride 2), on a persistent grid
of one workgroup per compute unit with two patch buffers: the shapes go one below, to and one above a tile, two tiles plus one, and
past 512 tiles (thin images, so that a workgroup's loop takes its third tile on the first buffer again).

Whole encoder / decoder - the yardstick is the CPU emulation (the reference with round_to = the operand type: same roundings at
the same places, fp64 sums), never the code under test: the device's rms error against the fp64 network on the rounded weights may
be at most 2x, its largest error at most 3x the emulation's, computed here for the same inputs; both are printed
(docs/history/tiny_vae.md keeps a copy).

Pipelines (tiny UNet + tiny VAE): every bound is equality.
"""
import itertools

import pytest
import torch

from tests import tiny_vae_reference as R

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
GUARD = 4096   # elements in front of and behind the output


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {"bf16": L.init(0, False), "fp16": L.init(0, True)}


def _nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.float32).to(dt).cuda()


def _operands(B, H, W, dt, seed, bias, res, stride, up2):
    """fp64 NCHW operands that are exact in ``dt`` (bias: fp32)."""
    g = torch.Generator("cpu").manual_seed(seed)
    rnd = R.rounder(dt)
    x = rnd(torch.randn(B, 64, H, W, generator=g, dtype=torch.float64))
    w = rnd(torch.randn(64, 64, 3, 3, generator=g, dtype=torch.float64) * (2.0 / 576) ** 0.5)
    b = (0.1 * torch.randn(64, generator=g)).double() if bias else None
    Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if stride == 2 else ((2 * H, 2 * W) if up2 else (H, W))
    r = rnd(torch.randn(B, 64, Ho, Wo, generator=g, dtype=torch.float64)) if res else None
    return x, w, b, r, (Ho, Wo)


def _launch(lib, dt, x, w, b, r, out_hw, stride, up2, relu):
    """-> (output fp64 NCHW, its raw bits as int16 NHWC); checks the guard regions around the output."""
    from marigold_amd import ops as O
    from marigold_amd import _lib as L
    B = x.shape[0]
    xd = _nhwc(x, dt)
    wd = w.permute(2, 3, 0, 1).reshape(9, 64, 64).contiguous().to(torch.float32).to(dt).cuda()
    bd = b.float().cuda() if b is not None else None
    rd = _nhwc(r, dt) if r is not None else None
    n = B * out_hw[0] * out_hw[1] * 64
    buf = torch.full((n + 2 * GUARD,), 0x7b7b, dtype=torch.int16, device="cuda")
    out = buf[GUARD:GUARD + n]
    L.check(lib.mg_tiny_conv3x3(xd.data_ptr(), wd.data_ptr(), bd.data_ptr() if bd is not None else None,
                                rd.data_ptr() if rd is not None else None, out.data_ptr(), B, x.shape[2], x.shape[3], stride, int(up2),
                                int(relu), O.current_stream_handle()), "mg_tiny_conv3x3", lib)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0x7b7b).all()) and bool((buf[GUARD + n:] == 0x7b7b).all()), "guard region written"
    bits = out.clone()
    val = bits.view(dt).view(B, out_hw[0], out_hw[1], 64).permute(0, 3, 1, 2).double().cpu()
    return val, bits


def _check_layer(lib, name, shape, stride, up2, bias, res, relu, seed):
    dt = DTYPES[name]
    x, w, b, r, out_hw = _operands(*shape, dt, seed, bias, res, stride, up2)
    ref, mag = R.conv_layer(x, w, b, r, stride, up2, relu)
    got, _ = _launch(lib, dt, x, w, b, r, out_hw, stride, up2, relu)
    assert got.shape == ref.shape
    bound = U[name] * ref.abs() + 1.01 * 580 * 2.0 ** -24 * mag
    excess = ((got - ref).abs() - bound).max().item()
    assert torch.isfinite(got).all() and excess <= 0, (shape, stride, up2, bias, res, relu, excess)
    return ((got - ref).abs() / bound.clamp(min=1e-300)).max().item()


FLAGS = list(itertools.product((False, True), repeat=3))   # bias, residual, ReLU
# stride 1: the issue's shapes; 7 / 8 / 9 rows and 31 / 32 / 33 columns around the 8 x 32 tile; two tiles plus one
S1 = [(1, 1, 1), (1, 3, 5), (2, 17, 33), (3, 16, 32), (1, 31, 70), (1, 7, 31), (1, 8, 32), (1, 9, 33), (1, 17, 65)]
# stride 2 (input sizes): the issue's; outputs of 1 / 2 / 3 rows and 31 / 32 / 33 columns around the 2 x 32 tile; two tiles plus one
S2 = [(1, 1, 1), (2, 15, 11), (1, 16, 34), (1, 33, 65), (1, 2, 62), (1, 4, 64), (1, 5, 65), (1, 9, 129)]
# nearest x2 (input sizes): the issue's; outputs of 6 / 8 / 10 rows and 30 / 32 / 34 columns; two tiles plus two
UP = [(1, 1, 1), (2, 5, 7), (1, 9, 17), (1, 3, 15), (1, 4, 16), (1, 5, 17), (1, 9, 33)]
# more tiles than twice the compute units (256): 270 and 540 tiles at stride 1, 900 at stride 2, 540 with nearest x2
MANY = [((3, 360, 33), 1, False), ((3, 1440, 1), 1, False), ((3, 1200, 1), 2, False), ((3, 720, 1), 1, True)]


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", ["stride1", "stride2", "up2"])
def test_single_layer_against_fp64(libs, name, mode):
    shapes, stride, up2 = {"stride1": (S1, 1, False), "stride2": (S2, 2, False), "up2": (UP, 1, True)}[mode]
    worst = 0.0
    for k, shape in enumerate(shapes):
        for j, (bias, res, relu) in enumerate(FLAGS):
            worst = max(worst, _check_layer(libs[name], name, shape, stride, up2, bias, res, relu, 1000 + 8 * k + j))
    print(f"\ntiny conv {name} {mode}: largest |got - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_single_layer_many_tiles_per_workgroup(libs, name):
    for k, (shape, stride, up2) in enumerate(MANY):
        _check_layer(libs[name], name, shape, stride, up2, True, True, True, 2000 + k)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("stride,up2", [(1, False), (2, False), (1, True)])
def test_batch_equals_single_launches_and_repeats(libs, name, stride, up2):
    dt, shape = DTYPES[name], (3, 16, 32) if not up2 else (3, 9, 17)
    x, w, b, r, out_hw = _operands(*shape, dt, 3000, True, True, stride, up2)
    _, all3 = _launch(libs[name], dt, x, w, b, r, out_hw, stride, up2, True)
    _, again = _launch(libs[name], dt, x, w, b, r, out_hw, stride, up2, True)
    assert torch.equal(all3, again)
    singles = [_launch(libs[name], dt, x[i:i + 1], w, b, r[i:i + 1], out_hw, stride, up2, True)[1] for i in range(3)]
    assert torch.equal(all3, torch.cat(singles))


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("stride,up2", [(1, False), (2, False), (1, True)])
@pytest.mark.parametrize("relu", [False, True])
def test_non_finite_pixels_keep_their_class(libs, name, stride, up2, relu):
    dt = DTYPES[name]
    x, w, b, r, out_hw = _operands(2, 17, 33, dt, 4000, True, True, stride, up2)
    x[0, :, 4, 6] = float("nan")       # a NaN pixel
    x[0, 5, 12, 20] = float("inf")     # one channel: the sign of each output follows the weight's
    x[1, 9, 8, 31] = float("-inf")
    ref, mag = R.conv_layer(x, w, b, r, stride, up2, relu)
    got, _ = _launch(libs[name], dt, x, w, b, r, out_hw, stride, up2, relu)
    assert ref.isnan().any() and ref.isposinf().any() and (relu or ref.isneginf().any())
    assert torch.equal(got.isnan(), ref.isnan()) and torch.equal(got.isposinf(), ref.isposinf()) and torch.equal(got.isneginf(), ref.isneginf())
    fin = torch.isfinite(ref)
    bound = U[name] * ref.abs() + 1.01 * 580 * 2.0 ** -24 * mag
    assert ((got - ref).abs()[fin] <= bound[fin]).all()


# ---------------------------------------------------------------------------------------------- whole encoder / decoder

@pytest.fixture(scope="module")
def tiny_sd():
    from marigold_amd.synthetic import synthetic_tiny_vae_state_dict
    return synthetic_tiny_vae_state_dict(seed=1234)


@pytest.fixture(scope="module")
def tiny_vaes(libs, tiny_sd):
    from marigold_amd.modules import AutoencoderTinyHIP
    return {n: AutoencoderTinyHIP(tiny_sd, compute_dtype=dt).to("cuda:0") for n, dt in DTYPES.items()}


def _rounded_weights(sd, dt):
    rnd = R.rounder(dt)
    return {k: (rnd(v.double()) if k.endswith(".weight") else v.double()) for k, v in sd.items()}


def _stats(t):
    return t.pow(2).mean().sqrt().item(), t.abs().max().item()


def _held_to_emulation(what, dev, emu, ref):
    (rd, md), (re, me) = _stats(dev - ref), _stats(emu - ref)
    print(f"\n{what}: device rms {rd:.3e} max {md:.3e} | emulation rms {re:.3e} max {me:.3e}")
    assert re > 0 and rd <= 2 * re and md <= 3 * me, (what, rd, re, md, me)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 40, 56), (1, 15, 11)])
def test_encoder_against_the_emulation(tiny_vaes, tiny_sd, name, shape):
    dt = DTYPES[name]
    rgb = torch.rand(shape[0], 3, *shape[1:], generator=torch.Generator("cpu").manual_seed(11), dtype=torch.float64) * 2 - 1
    ref = R.encode(_rounded_weights(tiny_sd, dt), rgb)
    emu = R.encode(tiny_sd, rgb, round_to=dt)
    dev = tiny_vaes[name].encode_rgb_latent(rgb.float().cuda())
    assert dev.dtype == torch.float32 and tuple(dev.shape) == tuple(ref.shape) == (shape[0], 4, *tiny_vaes[name].latent_hw(shape[1:]))
    _held_to_emulation(f"tiny encode {name} {shape}", dev.double().cpu(), emu, ref)


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (3, 4, 3)])
@pytest.mark.parametrize("post", [R.POST_NONE, R.POST_DEPTH, R.POST_NORMALS, R.POST_UNIT])
def test_decoder_against_the_emulation(tiny_vaes, tiny_sd, name, shape, post):
    dt = DTYPES[name]
    z = torch.randn(shape[0], 4, *shape[1:], generator=torch.Generator("cpu").manual_seed(12), dtype=torch.float64)
    pre = R.decode_preclip(_rounded_weights(tiny_sd, dt), z)
    assert (pre.abs() > 1).double().mean().item() <= 0.05, "the clip would hide the decoder"
    ref, emu = R.tail(pre, post), R.decode(tiny_sd, z, post, round_to=dt)
    dev = tiny_vaes[name].decode(z.float().cuda(), post=post).double().cpu()
    assert tuple(dev.shape) == tuple(ref.shape) == (shape[0], 1 if post == R.POST_DEPTH else 3, 8 * shape[1], 8 * shape[2])
    if post == R.POST_NORMALS:   # a direction of (nearly) no length is decided by rounding: left out, and rare
        keep = (torch.linalg.vector_norm(pre.clip(-1, 1), dim=1, keepdim=True) >= 1e-3).expand_as(ref)
        assert (~keep).double().mean().item() <= 0.01
        dev, emu, ref = dev[keep], emu[keep], ref[keep]
    _held_to_emulation(f"tiny decode {name} {shape} post {post}", dev, emu, ref)


# ---------------------------------------------------------------------------------------------- pipelines: tiny UNet + tiny VAE

import dataclasses   # noqa: E402
import functools   # noqa: E402

import numpy as np   # noqa: E402
from PIL import Image   # noqa: E402

POST_OF = {"depth": R.POST_DEPTH, "normals": R.POST_NORMALS, "iid": R.POST_UNIT}
CALL = dict(denoising_steps=2, processing_res=0, match_input_res=False, show_progress_bar=False)


def _make_pipe(kind, f16=False, tiny_vae=True):
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE, TinyVAEConfig
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TinyVAEConfig() if tiny_vae else TINY_VAE, default_denoising_steps=2,
                                      default_processing_resolution=0, compute_dtype=torch.float16 if f16 else None).to("cuda:0")


_pipe = functools.lru_cache(maxsize=None)(_make_pipe)


@functools.lru_cache(maxsize=None)
def _pil(seed, hw=(30, 44)):
    from marigold_amd.synthetic import synthetic_image
    return Image.fromarray(np.ascontiguousarray(synthetic_image(*hw, seed=seed)[0].permute(1, 2, 0).numpy()))


def _arrays(kind, out):
    if kind == "depth":
        return [out.depth_np]
    if kind == "normals":
        return [out.normals_np]
    return [out[t].array for t in out.target_names]


def _same(kind, a, b):
    for x, y in zip(_arrays(kind, a), _arrays(kind, b)):
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("kind,f16", [("depth", False), ("normals", False), ("iid", False), ("depth", True)],
                         ids=["depth", "normals", "iid", "depth-fp16"])
def test_pipeline_equals_the_stages_by_hand(libs, kind, f16):
    """pipe(image) on a 30 x 44 image at processing_res = 0: latent 4 x 6 (the tiny encoder's ceiling; a floor gives 3 x 5), decoded
    32 x 48 - and, bit for bit, encode -> denoise program -> decode called by hand."""
    from marigold_amd.modules import AutoencoderTinyHIP
    pipe = _pipe(kind, f16)
    assert isinstance(pipe.vae, AutoencoderTinyHIP) and pipe.vae.dtype == (torch.float16 if f16 else torch.bfloat16)
    C = pipe._target_latent_channels
    init = torch.randn(1, C, 4, 6, generator=torch.Generator("cpu").manual_seed(5))
    out = pipe(_pil(0), ensemble_size=1, init_latents=init, **CALL)
    rgb_norm, _ = pipe._preprocess(_pil(0), 0, pipe._call_settings(2, 1, 0, "bilinear")[3])
    lat = pipe.vae.encode_rgb_latent(rgb_norm.to("cuda:0"))
    assert tuple(lat.shape) == (1, 4, 4, 6) == (1, 4, *pipe._latent_hw((30, 44)))
    pipe.unet.set_context(pipe.empty_text_embed)
    prog = pipe.unet.denoise_program(1, 4, 6, pipe.scheduler, 2, rgb_broadcast=True)
    prog.rgb_latent.copy_(lat)
    prog.x.copy_(init.cuda())
    prog.run()
    dec = pipe.vae.decode(prog.x.reshape(C // 4, 4, 4, 6), post=POST_OF[kind])
    assert tuple(dec.shape[-2:]) == (32, 48)
    want = dec.reshape(-1, 32, 48).cpu().numpy()
    got = np.concatenate([a.reshape(-1, 32, 48) for a in _arrays(kind, out)])
    assert got.shape == want.shape and np.array_equal(got, want.clip(-1 if kind == "normals" else 0, 1))
    assert np.isfinite(got).all() and got.std() > 0


@pytest.mark.parametrize("in_flight,per_program", [(2, 1), (3, 1), (2, 2)])
def test_map_images_equals_the_serial_calls(libs, in_flight, per_program):
    import marigold_amd as M
    pipe, n = _pipe("depth"), 5
    want = [pipe(_pil(s), ensemble_size=2, generator=M.NativeNoise(100 + s), **CALL) for s in range(n)]
    assert not np.array_equal(want[0].depth_np, want[1].depth_np)
    got = list(pipe.map_images((_pil(s) for s in range(n)), in_flight=in_flight, images_per_program=per_program,
                               generators=[M.NativeNoise(100 + s) for s in range(n)], ensemble_size=2, **CALL))
    assert len(got) == n
    for a, b in zip(got, want):
        _same("depth", a, b)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_map_video_equals_the_serial_loop(libs, in_flight):
    import marigold_amd as M
    pipe, n = _pipe("normals"), 4
    state = M.SequenceState(0.5)
    want = [pipe(_pil(s), sequence=state, ensemble_size=1, generator=M.NativeNoise(200 + s), **CALL) for s in range(n)]
    got = list(pipe.map_video((_pil(s) for s in range(n)), strength=0.5, in_flight=in_flight,
                              generators=(M.NativeNoise(200 + s) for s in range(n)), ensemble_size=1, **CALL))
    assert len(got) == n
    for a, b in zip(got, want):
        _same("normals", a, b)


def test_checkpoint_folder_with_a_tiny_vae_round_trips(libs, tmp_path):
    import marigold_amd as M
    from marigold_amd import checkpoint as ck
    from marigold_amd.arch import TinyVAEConfig
    from marigold_amd.modules import AutoencoderTinyHIP
    from marigold_amd.schedulers import DDIMScheduler
    pipe = _pipe("depth")
    path = str(tmp_path / "ckpt")
    ck.save_synthetic_checkpoint(path, "MarigoldDepthPipeline", pipe.unet.sd, pipe.vae.sd, pipe.unet.config, TinyVAEConfig(), DDIMScheduler(),
                                 pipe.empty_text_embed, scale_invariant=True, shift_invariant=True, default_denoising_steps=2,
                                 default_processing_resolution=0)
    loaded = M.MarigoldDepthPipeline.from_pretrained(path, torch_dtype=torch.bfloat16).to("cuda:0")
    assert isinstance(loaded.vae, AutoencoderTinyHIP)
    a = loaded(_pil(1), ensemble_size=2, generator=M.NativeNoise(7), **CALL)
    b = pipe(_pil(1), ensemble_size=2, generator=M.NativeNoise(7), **CALL)
    _same("depth", a, b)
    # the VAE folder on its own, swapped into a pipeline that was built with the AutoencoderKL
    ck.save_synthetic_tiny_vae(str(tmp_path / "taesd"), pipe.vae.sd)
    kl = _make_pipe("depth", tiny_vae=False)
    kl.set_vae(ck.load_tiny_vae(str(tmp_path / "taesd"), torch_dtype=torch.bfloat16))
    _same("depth", kl(_pil(1), ensemble_size=2, generator=M.NativeNoise(7), **CALL), b)


def test_set_vae_back_to_the_kl_module_reproduces_its_outputs(libs):
    import marigold_amd as M
    from marigold_amd.arch import TinyVAEConfig
    from marigold_amd.modules import AutoencoderTinyHIP
    from marigold_amd.synthetic import synthetic_tiny_vae_state_dict
    pipe = _make_pipe("depth", tiny_vae=False)
    kl = pipe.vae
    images = [_pil(s, (64, 128)) for s in range(3)]

    def run():
        return list(pipe.map_images(images, in_flight=2, generators=[M.NativeNoise(300 + s) for s in range(3)], ensemble_size=1, **CALL))
    before = run()
    assert before[0].depth_np.shape == (64, 128) and len(pipe._lanes) == 2
    pipe.set_vae(AutoencoderTinyHIP(synthetic_tiny_vae_state_dict(TinyVAEConfig(), 1234)))
    assert pipe._lanes == [] and pipe.vae.device == pipe.unet.device
    tiny = run()
    assert tiny[0].depth_np.shape == (64, 128) and not np.array_equal(tiny[0].depth_np, before[0].depth_np)
    pipe.set_vae(kl)
    for a, b in zip(run(), before):
        _same("depth", a, b)
