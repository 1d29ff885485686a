"""Host checks of edge-guided upsampling, no GPU: ``mg_guided_upsample`` is declared, bound and exported by both operand
libraries without touching the ABI version or the op kinds; it refuses bad arguments before any GPU work (no GPU is here: a call that
got as far as a launch would fail differently, so the message proves where it stopped); ``marigold_amd.guided`` refuses what it must;
the pipelines refuse the keyword where it cannot work, before anything is launched (stand-in pipelines whose engines are namespaces);
the command line hands the flags on as the keyword and passes nothing without them; the C host example compiles; and the numpy
restatement the GPU tests are measured against has the two properties the definition promises."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import guided
from marigold_amd.pipeline import MarigoldDepthOutput, MarigoldDepthPipeline, MarigoldIIDPipeline, MarigoldNormalsPipeline
from marigold_amd.schedulers import DDIMScheduler
from tests import c_hosts
from tests.guided_reference import guided_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototype_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int mg_guided_upsample(const float* pred, int C, int h, int w, const uint8_t* guide_lo, const uint8_t* guide_hi, int hwc, "
            "int H, int W, int radius, float sigma, float* out, void* stream);") in flat
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bguided\.hip\b", makefile, re.M)
    assert re.search(r"^FLAGS_guided\s*:=\s*-ffp-contract=off\s*$", makefile, re.M)
    vp, i = ctypes.c_void_p, ctypes.c_int
    for f16 in (False, True):
        lib = L.load(f16)
        assert "mg_guided_upsample" in L.EXPORTS and hasattr(lib, "mg_guided_upsample")
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_guided_upsample.argtypes == [vp, i, i, i, vp, vp, i, i, i, i, ctypes.c_float, vp, vp]
    assert ctypes.sizeof(L.MgOp) == 360
    assert "guided" not in " ".join(L.OP_NAMES.values())   # a plain C call, no op kind
    import marigold_amd
    assert marigold_amd.guided_upsample is guided.guided_upsample


@LIBS
def test_the_entry_point_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_float * 64)()                      # stands for every device buffer: no call gets as far as reading it
    p = ctypes.addressof(mem)

    def args(**kw):
        a = dict(pred=p, C=3, h=5, w=7, lo=p, hi=p, hwc=1, H=16, W=24, radius=2, sigma=0.1, out=p)
        a.update(kw)
        return tuple(a[k] for k in ("pred", "C", "h", "w", "lo", "hi", "hwc", "H", "W", "radius", "sigma", "out")) + (None,)

    def refused(*words, **kw):
        rc = lib.mg_guided_upsample(*args(**kw))
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_guided_upsample:") and all(w in msg for w in words), (kw, rc, msg)

    for name in ("pred", "lo", "hi", "out"):
        refused("null pointer", **{name: None})
    for C in (0, -1, 17):
        refused("channels", "1 to 16", C=C)
    for name in ("h", "w", "H", "W"):
        for v in (0, -3):
            refused("bad size", **{name: v})
    refused("2^30", H=1 << 16, W=1 << 15)
    refused("2^30", h=1 << 16, w=1 << 15)
    for radius in (0, -1, 5):
        refused("radius", "1 to 4", radius=radius)
    for sigma in (0.0, -0.1, float("nan"), float("inf"), 1e-30, 1e30):
        refused("sigma", sigma=sigma)
    refused("4-byte aligned", pred=p + 2)
    refused("4-byte aligned", out=p + 1)
    assert list(mem) == [0.0] * 64


# ---- marigold_amd.guided -----------------------------------------------------------------------------------------------------------

def test_the_keyword_s_settings():
    assert guided.settings(None) is None and guided.settings(False) is None
    assert guided.settings(True) == (2, 0.1) == (guided.DEFAULT_RADIUS, guided.DEFAULT_SIGMA)
    assert guided.settings({}) == (2, 0.1)
    assert guided.settings(dict(radius=1)) == (1, 0.1) and guided.settings(dict(sigma=0.25)) == (2, 0.25)
    assert guided.settings(dict(radius=4, sigma=1)) == (4, 1.0)
    for bad in (dict(radius=0), dict(radius=5), dict(radius=1.5), dict(radius=True), dict(sigma=0), dict(sigma=-1.0), dict(sigma=float("nan")),
                dict(sigma=float("inf")), dict(reach=2), 2, "yes", (2, 0.1)):
        with pytest.raises(ValueError, match="guided_upsample"):
            guided.settings(bad)


def test_guided_upsample_refuses_what_is_not_a_device_prediction():
    picture = torch.zeros(16, 24, 3, dtype=torch.uint8)
    for pred in (np.zeros((1, 5, 7), np.float32), torch.zeros(1, 5, 7), torch.zeros(5, 7, dtype=torch.float64), torch.zeros(5, 7, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="guided_upsample: the prediction must be an fp32 CUDA tensor"):
            guided.guided_upsample(pred, picture)


# ---- the pipelines' keyword: the refusals ------------------------------------------------------------------------------------------

def _engine(name, device, launched):
    def boom(*a, **k):
        launched.append(name)
        raise AssertionError(f"{name}: reached a launch")
    return SimpleNamespace(name=name, device=device, replica=boom, config=SimpleNamespace(block_out_channels=(1, 1, 1, 1)),
                           encode_rgb_latent=boom, denoise_program=boom, set_context=boom, f16=False, dtype=torch.bfloat16)


def _stand_in(cls, device_type="cuda"):
    launched = []
    device = SimpleNamespace(type=device_type)
    kw = dict(default_denoising_steps=2, default_processing_resolution=0, empty_text_embed=torch.zeros(1, 2, 4))
    if cls is MarigoldIIDPipeline:
        unet = _engine("unet", device, launched)
        unet.config = SimpleNamespace(in_channels=12, out_channels=8)
        pipe = cls(unet, _engine("vae", device, launched), DDIMScheduler(), target_properties={"target_names": ["albedo", "material"]}, **kw)
    else:
        pipe = cls(_engine("unet", device, launched), _engine("vae", device, launched), DDIMScheduler(), **kw)

    def reached(name):
        def stop(*a, **k):
            launched.append(name)
            raise AssertionError(f"reached {name}")
        return stop
    pipe._preprocess, pipe._preprocess_device = reached("preprocessing"), reached("preprocessing")
    pipe.launched = launched
    return pipe


PICTURE = torch.zeros(1, 3, 128, 256, dtype=torch.uint8)
KINDS = pytest.mark.parametrize("cls", [MarigoldDepthPipeline, MarigoldNormalsPipeline, MarigoldIIDPipeline], ids=["depth", "normals", "iid"])


@KINDS
def test_the_pipelines_refuse_the_keyword_before_any_launch(cls):
    pipe = _stand_in(cls)
    with pytest.raises(ValueError, match="cannot be combined with match_input_res=False"):
        pipe(PICTURE, guided_upsample=True, match_input_res=False)
    for image in (torch.zeros(1, 3, 128, 256), torch.zeros(3, 128, 256, dtype=torch.uint8), torch.zeros(2, 3, 8, 8, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="PIL image or a uint8 \\[1, 3, H, W\\] tensor"):
            pipe(image, guided_upsample=True)
    with pytest.raises(ValueError, match="radius must be an integer from 1 to 4"):
        pipe(PICTURE, guided_upsample=dict(radius=9))
    with pytest.raises(ValueError, match="unknown keys"):
        pipe(PICTURE, guided_upsample=dict(sigmas=0.1))
    with pytest.raises(ValueError, match="images_per_program|cannot be combined with match_input_res=False"):
        list(pipe.map_images([PICTURE, PICTURE], images_per_program=2, in_flight=1, guided_upsample=True, match_input_res=False))
    with pytest.raises(ValueError, match="needs a CUDA pipeline"):
        _stand_in(cls, "cpu")(PICTURE, guided_upsample=True)
    pipe._sharded = lambda: True
    with pytest.raises(ValueError, match="guided_upsample is not available on a member-parallel pipeline"):
        pipe(PICTURE, guided_upsample=dict(sigma=0.2))
    assert pipe.launched == []
    # accepted, the call goes on - in the stand-in, to its preprocessing; so does a call without the keyword, or with it off
    pipe._sharded = lambda: False
    for kw in (dict(guided_upsample=True), dict(guided_upsample=None), dict()):
        with pytest.raises(AssertionError, match="reached preprocessing"):
            pipe(PICTURE, **kw)


@pytest.mark.parametrize("cls", [MarigoldDepthPipeline, MarigoldNormalsPipeline], ids=["depth", "normals"])
def test_predict_tiled_refuses_the_keyword(cls):
    pipe = _stand_in(cls)
    with pytest.raises(ValueError, match="predict_tiled: guided_upsample cannot be combined with tiles"):
        pipe.predict_tiled(PICTURE, tile_size=(64, 128), tile_overlap=(16, 32), guided_upsample=True)
    assert pipe.launched == []


# ---- the command line --------------------------------------------------------------------------------------------------------------

class _FakeCliPipe:
    scale_invariant = shift_invariant = True
    default_denoising_steps, default_processing_resolution = 4, 768
    target_names = ["albedo"]

    def __init__(self, kind):
        self.kind, self.calls = kind, []

    def _out(self):
        from PIL import Image
        from marigold_amd.pipeline import MarigoldIIDOutput, MarigoldNormalsOutput
        picture = Image.fromarray(np.zeros((6, 8, 3), np.uint8))
        if self.kind == "depth":
            return MarigoldDepthOutput(np.linspace(0, 1, 48, dtype=np.float32).reshape(6, 8), picture, None)
        if self.kind == "normals":
            return MarigoldNormalsOutput(np.zeros((3, 6, 8), np.float32), picture, None)
        out = MarigoldIIDOutput(self.target_names)
        out._set_entry("albedo", np.zeros((3, 6, 8), np.float32), np.zeros((6, 8, 3), np.uint8))
        return out

    def map_images(self, images, in_flight=None, generators=None, **kw):
        images = list(images)
        self.calls.append(("map_images", len(images), kw))
        return [self._out() for _ in images]

    def map_video(self, frames, strength=0.1, in_flight=None, generators=None, **kw):
        frames = list(frames)
        self.calls.append(("map_video", len(frames), kw))
        return [self._out() for _ in frames]

    def predict_tiled(self, image, **kw):
        raise AssertionError("predict_tiled")


@pytest.mark.parametrize("kind", ["depth", "normals", "iid"])
def test_cli_guided_flags(tmp_path, kind):
    from PIL import Image
    from marigold_amd import cli
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    a = cli.build_parser(kind).parse_args(io)
    assert (a.guided_upsample, a.guided_sigma, a.guided_radius) == (False, 0.1, 2)
    a = cli.build_parser(kind).parse_args(io + ["--guided_upsample", "--guided_sigma", "0.25", "--guided_radius", "3"])
    assert (a.guided_upsample, a.guided_sigma, a.guided_radius) == (True, 0.25, 3)
    inp = tmp_path / "in"
    inp.mkdir()
    for name in ("b.png", "a.png"):
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / name)
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    # without the flag no keyword is passed, whatever the other two say
    for extra in ([], ["--guided_sigma", "0.3", "--guided_radius", "1"]):
        pipe = _FakeCliPipe(kind)
        assert cli.main(kind, base + extra, pipeline=pipe) == 0
        (name, n, kw), = pipe.calls
        assert (name, n) == ("map_images", 2) and "guided_upsample" not in kw
    # with it: the keyword, through map_images (with images per program too) and map_video
    pipe = _FakeCliPipe(kind)
    assert cli.main(kind, base + ["--guided_upsample"], pipeline=pipe) == 0
    assert pipe.calls[0][0] == "map_images" and pipe.calls[0][2]["guided_upsample"] == dict(radius=2, sigma=0.1)
    assert pipe.calls[0][2]["match_input_res"] is True
    pipe = _FakeCliPipe(kind)
    assert cli.main(kind, base + ["--guided_upsample", "--guided_sigma", "0.05", "--guided_radius", "4", "--images_per_program", "2"], pipeline=pipe) == 0
    assert pipe.calls[0][2]["guided_upsample"] == dict(radius=4, sigma=0.05) and pipe.calls[0][2]["images_per_program"] == 2
    pipe = _FakeCliPipe(kind)
    assert cli.main(kind, base + ["--guided_upsample", "--sequence", "--seed", "3"], pipeline=pipe) == 0
    assert pipe.calls[0][0] == "map_video" and pipe.calls[0][2]["guided_upsample"] == dict(radius=2, sigma=0.1)
    # refused before anything is loaded
    with pytest.raises(ValueError, match="--output_processing_res"):
        cli.main(kind, base + ["--guided_upsample", "--output_processing_res"], pipeline=_FakeCliPipe(kind))
    with pytest.raises(ValueError, match="radius"):
        cli.main(kind, base + ["--guided_upsample", "--guided_radius", "7"], pipeline=_FakeCliPipe(kind))
    with pytest.raises(ValueError, match="sigma"):
        cli.main(kind, base + ["--guided_upsample", "--guided_sigma", "0"], pipeline=_FakeCliPipe(kind))
    if kind != "iid":
        with pytest.raises(ValueError, match="--tile_size"):
            cli.main(kind, base + ["--guided_upsample", "--tile_size", "64"], pipeline=_FakeCliPipe(kind))


def test_the_nine_launchers_are_untouched_and_reach_the_flags():
    for kind in ("depth", "normals", "iid"):
        src = open(os.path.join(ROOT, "script", kind, "run.py")).read()
        assert "guided" not in src and "cli" in src


# ---- the C host example ------------------------------------------------------------------------------------------------------------

def test_the_c_host_example_compiles(tmp_path):
    c_hosts.compile_only(os.path.join(ROOT, "examples", "host_guided.cpp"), tmp_path / "host_guided.o")
    assert os.path.getsize(tmp_path / "host_guided.o") > 0
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "host_guided" in readme


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw,HW", [((5, 7), (16, 24)), ((7, 7), (24, 24)), ((8, 8), (64, 64)), ((6, 9), (24, 36)), ((1, 1), (4, 4))],
                         ids=["16/5", "24/7", "8", "4", "1x1"])
def test_reference_flat_guide_and_radius_one_is_bilinear(hw, HW):
    pred = torch.rand(3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(hw[0]))
    lo, hi = np.full((3,) + hw, 130, np.uint8), np.full(HW + (3,), 130, np.uint8)
    want = torch.nn.functional.interpolate(pred[None], size=HW, mode="bilinear", align_corners=False, antialias=True)[0].numpy()
    for sigma in (0.05, 0.1, 1000.0):
        got = guided_reference(pred.numpy(), lo, hi, True, 1, sigma)
        assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-6
    got32 = guided_reference(pred.numpy(), lo, np.ascontiguousarray(hi.transpose(2, 0, 1)), False, 1, 0.1, np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 1e-6


def test_reference_equal_sizes_and_radius_one_is_the_identity():
    g = np.random.default_rng(3)
    for dtype in (np.float64, np.float32):
        pred = (g.random((4, 9, 11)) * 3 - 1).astype(dtype)
        lo = g.integers(0, 256, (3, 9, 11), dtype=np.uint8)
        hi = g.integers(0, 256, (9, 11, 3), dtype=np.uint8)          # the guides need not agree
        for sigma in (0.05, 0.1, 1000.0):
            assert np.array_equal(guided_reference(pred, lo, hi, True, 1, sigma, dtype), pred)


def test_reference_keeps_a_step_sharp():
    lo = np.zeros((3, 8, 8), np.uint8)
    lo[:, :, 4:] = 255
    hi = np.zeros((64, 64, 3), np.uint8)
    hi[:, 32:] = 255
    pred = np.full((1, 8, 8), 0.2)
    pred[:, :, 4:] = 0.9
    for R in (1, 2):
        out = guided_reference(pred, lo, hi, True, R, 0.05)[0]
        assert np.abs(out[:, :32] - 0.2).max() <= 1e-3 * 0.7 and np.abs(out[:, 32:] - 0.9).max() <= 1e-3 * 0.7
