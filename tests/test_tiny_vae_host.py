"""The tiny autoencoder without a GPU: its shape table and config rules, the latent-size rule of both VAE kinds, the C calls'
declarations, bindings and refusals in both libraries, loading from checkpoint folders, ``set_vae``, the model-image refusal, the
``--tiny_vae`` flag, and the pin against diffusers where one was recorded (tools/pin_tiny_vae_against_diffusers.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import tiny_vae_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_table_is_the_134_tensors():
    from marigold_amd.arch import TinyVAEConfig, tiny_vae_layers, tiny_vae_param_shapes
    shapes = tiny_vae_param_shapes(TinyVAEConfig())
    assert len(shapes) == 134 and {k: tuple(v) for k, v in shapes.items()} == R.param_shapes()
    assert tiny_vae_layers() == (R.ENCODER, R.DECODER)
    assert shapes["encoder.layers.0.weight"] == (64, 3, 3, 3) and shapes["encoder.layers.14.weight"] == (4, 64, 3, 3)
    assert shapes["decoder.layers.0.weight"] == (64, 4, 3, 3) and shapes["decoder.layers.18.bias"] == (3,)
    for n in ("encoder.layers.2", "encoder.layers.6", "encoder.layers.10", "decoder.layers.6", "decoder.layers.11", "decoder.layers.16"):
        assert f"{n}.weight" in shapes and f"{n}.bias" not in shapes          # the stride-2 / post-upsample convolutions carry no bias
    assert sum(k.endswith(".conv.4.bias") for k in shapes) == 20              # ten Blocks per half


def test_config_rules():
    from marigold_amd import config_check as CC
    from marigold_amd.arch import TinyVAEConfig
    good = dict(CC.TAESD_VAE_CONFIG)
    assert CC.tiny_vae_config_from_json(good) == TinyVAEConfig()
    assert CC.tiny_vae_config_from_json({"_class_name": "AutoencoderTiny", "_anything": 1}) == TinyVAEConfig()   # defaults, '_' keys ignored
    assert CC.tiny_vae_config_from_json(dict(good, force_upcast=False, latent_magnitude=3.0, scaling_factor=1)) == TinyVAEConfig()
    bad = dict(in_channels=4, out_channels=1, latent_channels=16, encoder_block_out_channels=[64, 64, 64], decoder_block_out_channels=[64, 128, 64, 64],
               num_encoder_blocks=[1, 3, 3], num_decoder_blocks=[3, 3, 3, 3], act_fn="swish", upsampling_scaling_factor=4, latent_magnitude=2,
               latent_shift=0.0, scaling_factor=0.18215, force_upcast=True, shift_factor=0.1, block_out_channels=[64] * 4)
    for k, v in bad.items():
        with pytest.raises(CC.UnsupportedConfigError, match=k):
            CC.tiny_vae_config_from_json(dict(good, **{k: v}))
    with pytest.raises(CC.UnsupportedConfigError, match="_class_name"):
        CC.tiny_vae_config_from_json(dict(good, _class_name="AutoencoderKL"))


def test_latent_size_of_both_vae_kinds():
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_VAE
    from marigold_amd.modules import AutoencoderKLHIP, AutoencoderTinyHIP
    kl = AutoencoderKLHIP(syn.synthetic_vae_state_dict(TINY_VAE), TINY_VAE)
    tiny = AutoencoderTinyHIP(syn.synthetic_tiny_vae_state_dict())
    assert kl.scale_factor == tiny.scale_factor == 8
    assert kl.latent_hw((231, 768)) == (28, 96) and tiny.latent_hw((231, 768)) == (29, 96)
    for hw in ((768, 768), (64, 128), (8, 8)):
        assert kl.latent_hw(hw) == tiny.latent_hw(hw) == (hw[0] // 8, hw[1] // 8)
    assert kl.latent_hw((30, 44)) == (3, 5) and tiny.latent_hw((30, 44)) == (4, 6) and tiny.latent_hw((1, 1)) == (1, 1)
    with pytest.raises(KeyError, match="tiny VAE"):
        AutoencoderTinyHIP({})
    with pytest.raises(RuntimeError, match="cuda"):
        tiny.decode(torch.zeros(1, 4, 2, 2))


NAMES = ("mg_tiny_vae_workspace_bytes", "mg_tiny_vae_encode", "mg_tiny_vae_decode", "mg_tiny_conv3x3")


@pytest.fixture(scope="module", params=[False, True], ids=["bf16-lib", "f16-lib"])
def lib(request):
    from marigold_amd import _lib as L
    return L.load(request.param)


def test_symbols_declared_bound_and_exported(lib):
    from marigold_amd import _lib as L
    hdr = " ".join(open(os.path.join(ROOT, "include", "marigold_hip.h")).read().split())
    for proto in ("long long mg_tiny_vae_workspace_bytes(int which, int B, int H, int W);",
                  "int mg_tiny_vae_encode(const mg_tiny_vae* net, const float* rgb, float* latent, int B, int H, int W, void* ws, long long ws_bytes, void* stream);",
                  "int mg_tiny_vae_decode(const mg_tiny_vae* net, const float* latent, float* out, int B, int h, int w, int post, void* ws, long long ws_bytes, void* stream);",
                  "int mg_tiny_conv3x3(const void* x, const void* w, const float* bias_or_null, const void* residual_or_null, void* out, int B, int H, int W, "
                  "int stride, int up2, int relu, void* stream);"):
        assert proto in hdr, proto
    for name in NAMES:
        assert name in L.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert "typedef struct mg_tiny_vae {" in hdr and "#define MG_TINY_VAE_LAYERS 33" in hdr and L.TINY_VAE_LAYERS == 33
    assert ctypes.sizeof(L.MgTinyVae) == 8 * (2 * (4 + 2 * 33))
    # the ABI pins: no new op kind, the descriptor as it was
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr) and L.ABI_VERSION == 4 and lib.mg_abi_version() == 4
    assert ctypes.sizeof(L.MgOp) == 360 and "tiny" not in " ".join(L.OP_NAMES.values()) and max(L.OP_NAMES) == max(L.FIELDS)
    assert "tinyvae.hip" in open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()


def _net(half=None, drop=None):
    """A struct of fake (never dereferenced: every refusal comes before the first device call) 16-byte aligned addresses."""
    from marigold_amd import _lib as L
    net, a = L.MgTinyVae(), 0x10000
    for h in ("enc", "dec"):
        if half not in (None, h):
            continue
        for f in ("in_w", "in_b", "out_w", "out_b"):
            setattr(net, f"{h}_{f}", a)
        for l in range(L.TINY_VAE_LAYERS):
            getattr(net, f"{h}_w")[l] = a
            getattr(net, f"{h}_b")[l] = a
        for l in ((3, 13, 23) if h == "enc" else (9, 19, 29)):   # the bias-free layers: NULL is accepted
            getattr(net, f"{h}_b")[l] = None
    if drop:
        h, f, l = drop
        if l is None:
            setattr(net, f"{h}_{f}", None)
        else:
            getattr(net, f"{h}_{f}")[l] = None
    return net


def test_c_calls_refuse_before_any_device_call(lib):
    err = lambda: lib.mg_last_error().decode()   # noqa: E731
    P = 0x20000
    # workspace sizes: three 64-channel operand-typed buffers of the largest level
    assert lib.mg_tiny_vae_workspace_bytes(0, 2, 40, 56) == 3 * 2 * 40 * 56 * 128
    assert lib.mg_tiny_vae_workspace_bytes(1, 2, 5, 7) == 3 * 2 * 40 * 56 * 128
    assert lib.mg_tiny_vae_workspace_bytes(0, 10, 768, 768) == lib.mg_tiny_vae_workspace_bytes(1, 10, 96, 96) == 3 * 10 * 768 * 768 * 128
    for args in ((2, 1, 8, 8), (-1, 1, 8, 8), (0, 0, 8, 8), (0, 1, 0, 8), (1, 1, 8, 0), (0, 1, 1 << 14, 1 << 14), (1, 1, 2048, 1024)):
        assert lib.mg_tiny_vae_workspace_bytes(*args) == -1 and err().startswith("mg_tiny_vae_workspace_bytes:")
    big = 1 << 40
    enc = lambda net=None, rgb=P, lat=P, B=1, H=8, W=8, ws=P, n=big: lib.mg_tiny_vae_encode(   # noqa: E731
        ctypes.byref(net if net is not None else _net("enc")), rgb, lat, B, H, W, ws, n, None)
    dec = lambda net=None, lat=P, out=P, B=1, h=2, w=2, post=0, ws=P, n=big: lib.mg_tiny_vae_decode(   # noqa: E731
        ctypes.byref(net if net is not None else _net("dec")), lat, out, B, h, w, post, ws, n, None)
    for call, name in ((enc, "mg_tiny_vae_encode"), (dec, "mg_tiny_vae_decode")):
        h = name[-6:-3]
        for kw, text in ((dict(B=0), ">= 1"), (dict(ws=None), "null pointer"), (dict(n=1024), "workspace too small"), (dict(ws=P + 8), "aligned"),
                         (dict(net=_net(h, (h, "in_w", None))), "null pointer in the network"),
                         (dict(net=_net(h, (h, "w", 7))), "layer 7"), (dict(net=_net(h, (h, "b", 4))), "layer 4"),
                         (dict(net=_net("dec" if h == "enc" else "enc")), "null pointer in the network")):
            assert call(**kw) != 0 and err().startswith(name + ":") and text in err(), (name, kw, err())
    assert enc(rgb=None) != 0 and "null pointer" in err() and enc(lat=None) != 0 and enc(H=0) != 0 and enc(W=-3) != 0
    assert lib.mg_tiny_vae_encode(None, P, P, 1, 8, 8, P, big, None) != 0 and "null pointer" in err()
    assert dec(out=None) != 0 and dec(h=0) != 0 and dec(w=0) != 0
    for post in (-1, 4, 5):   # MG_POST_SCHED is no tail of a decoder
        assert dec(post=post) != 0 and "unknown post" in err()
    need = lib.mg_tiny_vae_workspace_bytes(1, 3, 4, 3)
    assert dec(B=3, h=4, w=3, n=need - 1) != 0 and str(need) in err()
    conv = lambda x=P, w=P, b=None, r=None, out=2 * P, B=1, H=4, W=4, stride=1, up2=0, relu=1: lib.mg_tiny_conv3x3(   # noqa: E731
        x, w, b, r, out, B, H, W, stride, up2, relu, None)
    for kw, text in ((dict(x=None), "null pointer"), (dict(w=None), "null pointer"), (dict(out=None), "null pointer"), (dict(B=0), ">= 1"),
                     (dict(H=0), ">= 1"), (dict(W=-1), ">= 1"), (dict(stride=0), "stride"), (dict(stride=3), "stride"),
                     (dict(stride=2, up2=1), "stride 2 (up2 0)"), (dict(up2=2), "up2"), (dict(x=P + 2), "alignment"), (dict(b=P + 4), "alignment"),
                     (dict(out=P), "alias"), (dict(r=2 * P), "alias"), (dict(B=1 << 12, H=1 << 8, W=1 << 8), "2^26")):
        assert conv(**kw) != 0 and err().startswith("mg_tiny_conv3x3:") and text in err(), (kw, err())


def _folders(tmp_path):
    from marigold_amd import checkpoint as ck, synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE, TinyVAEConfig
    from marigold_amd.schedulers import DDIMScheduler
    common = dict(scale_invariant=True, shift_invariant=True, default_denoising_steps=2, default_processing_resolution=0)
    usd, emb = syn.synthetic_unet_state_dict(TINY_UNET), syn.synthetic_text_embedding(TINY_UNET.cross_attention_dim)
    ck.save_synthetic_checkpoint(str(tmp_path / "kl"), "MarigoldDepthPipeline", usd, syn.synthetic_vae_state_dict(TINY_VAE), TINY_UNET, TINY_VAE,
                                 DDIMScheduler(), emb, **common)
    ck.save_synthetic_checkpoint(str(tmp_path / "tiny"), "MarigoldDepthPipeline", usd, syn.synthetic_tiny_vae_state_dict(), TINY_UNET,
                                 TinyVAEConfig(), DDIMScheduler(), emb, **common)
    ck.save_synthetic_tiny_vae(str(tmp_path / "taesd"), syn.synthetic_tiny_vae_state_dict(seed=5))
    return tmp_path


def test_load_pipeline_picks_the_vae_class_and_set_vae_drops_the_lanes(tmp_path):
    import json
    import marigold_amd as M
    from marigold_amd import checkpoint as ck, config_check as CC, image, synthetic as syn
    from marigold_amd.modules import AutoencoderKLHIP, AutoencoderTinyHIP
    root = _folders(tmp_path)
    kl = M.MarigoldDepthPipeline.from_pretrained(str(root / "kl"))
    tiny = M.MarigoldDepthPipeline.from_pretrained(str(root / "tiny"), torch_dtype=torch.float16)
    assert type(kl.vae) is AutoencoderKLHIP and type(tiny.vae) is AutoencoderTinyHIP and tiny.vae.dtype == torch.float16 == tiny.unet.dtype
    assert json.load(open(root / "tiny" / "vae" / "config.json")) == CC.TAESD_VAE_CONFIG
    assert kl._latent_hw((30, 44)) == (3, 5) and tiny._latent_hw((30, 44)) == (4, 6)
    want = syn.synthetic_tiny_vae_state_dict()
    assert set(tiny.vae.sd) == set(want) and all(torch.equal(tiny.vae.sd[k], want[k]) for k in want)
    # a folder without _class_name is an AutoencoderKL, as before; an unknown class or field stops the load
    cfg = json.load(open(root / "kl" / "vae" / "config.json"))
    json.dump({k: v for k, v in cfg.items() if k != "_class_name"}, open(root / "kl" / "vae" / "config.json", "w"))
    assert type(M.MarigoldDepthPipeline.from_pretrained(str(root / "kl")).vae) is AutoencoderKLHIP
    json.dump(dict(CC.TAESD_VAE_CONFIG, act_fn="gelu"), open(root / "tiny" / "vae" / "config.json", "w"))
    with pytest.raises(CC.UnsupportedConfigError, match="act_fn"):
        M.MarigoldDepthPipeline.from_pretrained(str(root / "tiny"))
    json.dump(dict(CC.TAESD_VAE_CONFIG, _class_name="VQModel"), open(root / "tiny" / "vae" / "config.json", "w"))
    with pytest.raises(CC.UnsupportedConfigError, match="VQModel"):
        M.MarigoldDepthPipeline.from_pretrained(str(root / "tiny"))
    # load_tiny_vae + set_vae
    vae = ck.load_tiny_vae(str(root / "taesd"))
    assert type(vae) is AutoencoderTinyHIP and vae.dtype == torch.bfloat16
    with pytest.raises(CC.UnsupportedConfigError, match="AutoencoderTiny"):
        ck.load_tiny_vae(str(root / "kl" / "vae"))
    kl._lanes = [object(), object()]
    assert kl.set_vae(vae) is kl and kl.vae is vae and kl._lanes == [] and kl._latent_hw((30, 44)) == (4, 6)
    with pytest.raises(ValueError, match="float16"):
        kl.set_vae(ck.load_tiny_vae(str(root / "taesd"), torch_dtype=torch.float16))
    with pytest.raises(ValueError, match="model images carry an AutoencoderKL"):
        image.export_model_image(kl, str(tmp_path / "m.mgm"), ensemble_size=1, height=64, width=64)


class _CliPipe:
    """What cli.main and the evaluation harness need of a pipeline, recording the VAE it is handed."""
    scale_invariant = shift_invariant = True
    default_denoising_steps, default_processing_resolution = 4, 768

    def __init__(self):
        self.vaes, self.calls = [], 0

    def set_vae(self, vae):
        self.vaes.append(vae)
        return self

    def map_images(self, images, in_flight=None, generators=None, **kw):
        from PIL import Image
        from marigold_amd import MarigoldDepthOutput
        images = list(images)
        self.calls += len(images)
        return [MarigoldDepthOutput(np.linspace(0, 1, 48, dtype=np.float32).reshape(6, 8), Image.fromarray(np.zeros((6, 8, 3), np.uint8)), None)
                for _ in images]


def test_tiny_vae_flag_reaches_the_pipeline(tmp_path):
    from PIL import Image
    from marigold_amd import cli
    from marigold_amd.evaluation import harness
    from marigold_amd.modules import AutoencoderTinyHIP
    root = _folders(tmp_path)
    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / "a.png")
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    for kind in ("depth", "normals", "iid"):
        assert cli.build_parser(kind).parse_args(base).tiny_vae is None
        assert cli.build_parser(kind).parse_args(base + ["--tiny_vae", "x"]).tiny_vae == "x"
        assert harness.infer_parser(kind).get_default("tiny_vae") is None
    assert harness.validate_iid_parser().get_default("tiny_vae") is None
    pipe = _CliPipe()
    assert cli.main("depth", base, pipeline=pipe) == 0 and pipe.vaes == [] and pipe.calls == 1
    assert cli.main("depth", base + ["--tiny_vae", str(root / "taesd")], pipeline=pipe) == 0
    assert len(pipe.vaes) == 1 and type(pipe.vaes[0]) is AutoencoderTinyHIP and pipe.vaes[0].dtype == torch.bfloat16 and pipe.calls == 2
    assert cli.main("depth", base + ["--tiny_vae", str(root / "taesd"), "--fp16"], pipeline=pipe) == 0 and pipe.vaes[1].dtype == torch.float16
    # the evaluation command lines go through one loader
    args = harness.infer_parser("depth").parse_args(["--dataset_config", "c", "--base_data_dir", "d", "--output_dir", "o", "--denoise_steps", "1",
                                                     "--processing_res", "0", "--ensemble_size", "1", "--tiny_vae", str(root / "taesd")])
    pipe = _CliPipe()
    assert harness._load_pipeline("depth", args, pipe) is pipe and type(pipe.vaes[0]) is AutoencoderTinyHIP
    for script in ("script/depth/run.py", "script/normals/run.py", "script/iid/run.py"):
        assert os.path.exists(os.path.join(ROOT, script))


def test_synthetic_weights_keep_the_network_alive():
    """The init the GPU tests rely on: the fp64 decoder's [-1, 1]-space output leaves [-1, 1] on few values, the probe is calibrated."""
    from marigold_amd.synthetic import synthetic_tiny_vae_state_dict
    for seed in (1234, 7):
        sd = synthetic_tiny_vae_state_dict(seed=seed)
        probe = torch.randn(1, 4, 8, 8, generator=torch.Generator("cpu").manual_seed(99))
        y = (R.decode_preclip(sd, probe) + 1) / 2
        assert abs(y.mean().item() - 0.5) < 1e-4 and abs(y.std().item() - 0.2) < 1e-4   # (fp32 storage of the calibrated layer)
        z = torch.randn(2, 4, 5, 7, generator=torch.Generator("cpu").manual_seed(12), dtype=torch.float64)
        pre = R.decode_preclip(sd, z)
        assert (pre.abs() > 1).double().mean().item() < 0.02 and pre.std().item() > 0.1
        lat = R.encode(sd, torch.rand(1, 3, 40, 56, generator=torch.Generator("cpu").manual_seed(11), dtype=torch.float64) * 2 - 1)
        assert tuple(lat.shape) == (1, 4, 5, 7) and 0.1 < lat.pow(2).mean().sqrt().item() < 10
    assert all(torch.equal(a, b) for a, b in zip(synthetic_tiny_vae_state_dict(seed=3).values(), synthetic_tiny_vae_state_dict(seed=3).values()))


PIN = os.path.join(ROOT, "tests", "golden", "tiny_vae_diffusers.npz")


def test_reference_pinned_against_diffusers():
    """tests/golden/tiny_vae_diffusers.npz (tools/pin_tiny_vae_against_diffusers.py, run where diffusers imports): diffusers' own state-dict
    names and shapes, and its encoder / decoder outputs on small inputs with the seeded synthetic weights, against this repository's restatement."""
    if not os.path.exists(PIN):
        pytest.skip("unpinned against diffusers: tests/golden/tiny_vae_diffusers.npz is absent (tools/pin_tiny_vae_against_diffusers.py writes it)")
    pin = np.load(PIN, allow_pickle=False)
    names, shapes = [str(n) for n in pin["names"]], [tuple(int(d) for d in s if d >= 0) for s in pin["shapes"]]
    assert dict(zip(names, shapes)) == R.param_shapes()
    from marigold_amd.synthetic import synthetic_tiny_vae_state_dict
    sd = synthetic_tiny_vae_state_dict(seed=int(pin["seed"]))
    assert np.allclose([float(sd[n].double().sum()) for n in names], pin["sums"], rtol=0, atol=1e-6), "the seeded weights are not the pinned ones"
    lat = R.encode(sd, torch.from_numpy(pin["rgb"]))
    img = R.decode_preclip(sd, torch.from_numpy(pin["latent"]))
    assert float((lat - torch.from_numpy(pin["encoded"]).double()).abs().max()) < 1e-4
    assert float((img - torch.from_numpy(pin["decoded"]).double()).abs().max()) < 1e-4
