"""Host checks of tiled predictions, no GPU: the four C entry points are declared, bound and exported by both operand
libraries without touching the ABI version or the op kinds; ``mg_tile_plan`` follows the rule it documents, over a sweep, and has the
properties the blend relies on; every entry point refuses bad arguments before any GPU work (no GPU is here: a call that got as far as
a launch would fail differently, so the message proves where it stopped); ``predict_tiled`` refuses what it must before anything is
launched (stand-in pipelines whose engines are namespaces); the command line takes the tile flags for depth and normals only."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import tiles
from marigold_amd.pipeline import MarigoldDepthOutput, MarigoldDepthPipeline, MarigoldIIDPipeline, MarigoldNormalsPipeline, SequenceState
from marigold_amd.schedulers import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mg_tile_plan", "mg_tiles_workspace_bytes", "mg_tile_fit", "mg_tile_blend")
# the op kinds as they were before tiles: the entry points are plain C calls, not kinds
OP_NAMES = {"igemm", "gn_stats", "gn_finalize", "gn_apply", "flash_attn64", "softmax_rows", "gn_slab", "rowgemm", "flash_attn512",
            "sched_step", "linear_small_m", "latent_1x1", "post_nchw", "im2col_small", "conv3x3", "conv3x3_head", "ens_depth_stats",
            "ens_depth_median", "ens_depth_norm", "ens_normals", "resize", "colorize", "eval_depth_ls", "eval_depth_metrics",
            "eval_normals", "memset", "copy", "iidscore_prep", "iidscore_psnr", "iidscore_ssim", "iid_vis", "rgb_prep", "normals_vis",
            "randn", "ens_iid"}
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int mg_tile_plan(int L, int T, int O, int* starts, int cap);" in flat
    assert "long long mg_tiles_workspace_bytes(int n, int th, int tw);" in flat
    grid = "int th, int tw, const int* ystarts, int ny, const int* xstarts, int nx, int Hw, int Ww, "
    assert ("int mg_tile_fit(const float* tiles, " + grid + "const float* guide, int hg, int wg, double* coef, int* flags, void* ws, "
            "long long ws_bytes, void* stream);") in flat
    assert ("int mg_tile_blend(const float* tiles, int C, " + grid + "int oy, int ox, const double* coef_or_null, int normalize, "
            "float* out, void* stream);") in flat
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr) and re.search(r"#define MG_TILE_MAX_PER_AXIS 32\b", hdr)
    assert L.TILE_MAX_PER_AXIS == 32
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btiles\.hip\b", makefile, re.M)
    pi, vp, i = ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int
    for f16 in (False, True):
        lib = L.load(f16)
        for name in NEW:
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_tile_plan.argtypes == [i, i, i, pi, i]
        assert lib.mg_tiles_workspace_bytes.argtypes == [i, i, i] and lib.mg_tiles_workspace_bytes.restype is ctypes.c_longlong
        assert lib.mg_tile_fit.argtypes == [vp, i, i, pi, i, pi, i, i, i, vp, i, i, vp, vp, vp, ctypes.c_longlong, vp]
        assert lib.mg_tile_blend.argtypes == [vp, i, i, i, pi, i, pi, i, i, i, i, i, vp, i, vp, vp]
    assert ctypes.sizeof(L.MgOp) == 360
    assert set(L.OP_NAMES.values()) == OP_NAMES


# ---- mg_tile_plan ------------------------------------------------------------------------------------------------------------------

def _plan_rule(Ln, T, O):
    """The rule of include/marigold_hip.h, restated."""
    if Ln <= T:
        return [0]
    n = -(-(Ln - O) // (T - O))
    return [8 * (i * (Ln - T) // (n - 1) // 8) for i in range(n - 1)] + [Ln - T]


def _c_plan(lib, Ln, T, O, cap=L.TILE_MAX_PER_AXIS):
    starts = (ctypes.c_int * max(cap, 1))(*([-7] * max(cap, 1)))
    n = lib.mg_tile_plan(Ln, T, O, starts, cap)
    return n, list(starts)


@LIBS
def test_tile_plan_sweep_against_the_rule_and_its_properties(f16):
    lib = L.load(f16)
    assert _c_plan(lib, 120, 64, 16)[1][:3] == [0, 24, 56] and _c_plan(lib, 120, 64, 16)[0] == 3
    cases = triple = 0
    for T in (16, 64, 768):
        for O in range(8, T // 2 + 1, 8):
            for Ln in range(8, 6 * T + 1, 8):
                want = _plan_rule(Ln, T, O)
                n, starts = _c_plan(lib, Ln, T, O)
                if len(want) > L.TILE_MAX_PER_AXIS:
                    assert n == -1 and lib.mg_last_error().decode().startswith("mg_tile_plan:"), (Ln, T, O)
                    continue
                assert n == len(want) and starts[:n] == want, (Ln, T, O, n, starts[:n], want)
                assert all(s == -7 for s in starts[n:]), (Ln, T, O)                      # nothing beyond the n entries is written
                ext = min(T, Ln)
                assert starts[0] == 0 and starts[n - 1] == Ln - ext
                assert all(s % 8 == 0 for s in starts[:n]) and all(b > a for a, b in zip(starts, starts[1:n]))
                assert all(a + ext - b >= O for a, b in zip(starts, starts[1:n])), (Ln, T, O, starts[:n])   # consecutive overlap >= O
                covered = np.zeros(Ln, np.int32)
                for s in starts[:n]:
                    covered[s:s + ext] += 1
                assert covered.min() >= 1, (Ln, T, O)
                triple += int(covered.max() >= 3)
                cases += 1
    assert cases > 1000 and triple > 0   # (three tiles over one coordinate do occur: the blend may not assume two)


@LIBS
def test_tile_plan_refusals(f16):
    lib = L.load(f16)

    def refused(args, *words):
        rc = lib.mg_tile_plan(*args)
        msg = lib.mg_last_error().decode()
        assert rc == -1 and msg.startswith("mg_tile_plan:") and all(w in msg for w in words), (args, rc, msg)

    buf = (ctypes.c_int * 40)(*([-7] * 40))
    refused((120, 64, 16, None, 32), "null pointer")
    for Ln, T in ((0, 64), (-8, 64), (12, 64), (120, 60), (120, 0), (121, 64)):
        refused((Ln, T, 16, buf, 32), "multiples of 8")
    refused((120, 64, 0, buf, 32), "overlap")
    refused((120, 64, 4, buf, 32), "overlap")
    refused((120, 64, 12, buf, 32), "overlap")
    refused((120, 64, 40, buf, 32), "half")
    refused((16 * 40, 16, 8, buf, 40), "at most 32")       # n = 79 tiles
    refused((120, 64, 16, buf, 2), "do not fit")           # n = 3 > cap
    refused((120, 64, 16, buf, 0), "do not fit")
    assert list(buf) == [-7] * 40
    assert lib.mg_tile_plan(120, 64, 16, buf, 3) == 3 and list(buf[:4]) == [0, 24, 56, -7]
    with pytest.raises(L.MarigoldHipError, match="mg_tile_plan: the overlap 40 exceeds half"):
        tiles.plan((120, 256), 64, 40)
    p = tiles.plan((120, 256), (64, 128), (16, 32))
    assert p.ystarts == (0, 24, 56) and p.xstarts == (0, 64, 128) and p.tile_hw == (64, 128) and len(p.origins) == 9
    assert p.origins[:4] == ((0, 0), (0, 64), (0, 128), (24, 0))
    assert tiles.plan((64, 128), 128, 32) == ((0,), (0,), (64, 128), ((0, 0),))   # a picture below the tile: one tile of its size


# ---- fit, blend, workspace: the refusals -------------------------------------------------------------------------------------------

def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


@LIBS
def test_fit_blend_and_workspace_refuse_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()                     # stands for every device buffer: no call gets as far as reading it
    p = ctypes.addressof(mem)
    assert p % 16 == 0 or (p + 8) % 16 == 0
    p += p % 16                                        # 16-byte aligned
    ys, xs = _ints(0, 24, 56), _ints(0, 64, 128)

    def refused(fn, args, *words):
        rc = getattr(lib, fn)(*args)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith(fn + ":") and all(w in msg for w in words), (fn, rc, msg)

    # mg_tiles_workspace_bytes
    assert lib.mg_tiles_workspace_bytes(9, 64, 128) == 9 * 2 * 5 * 8 and lib.mg_tiles_workspace_bytes(1, 8, 8) == 40
    assert lib.mg_tiles_workspace_bytes(35, 768, 768) == 35 * 144 * 5 * 8
    for bad in ((0, 64, 128), (-1, 64, 128), (1025, 64, 128), (9, 0, 128), (9, 60, 128), (9, 64, 4), (1, 8192, 8200)):
        rc = lib.mg_tiles_workspace_bytes(*bad)
        assert rc == -1 and lib.mg_last_error().decode().startswith("mg_tiles_workspace_bytes:"), bad

    # mg_tile_fit(tiles, th, tw, ystarts, ny, xstarts, nx, Hw, Ww, guide, hg, wg, coef, flags, ws, ws_bytes, stream)
    def fit_args(**kw):
        a = dict(tiles=p, th=64, tw=128, ys=ys, ny=3, xs=xs, nx=3, Hw=120, Ww=256, guide=p, hg=5, wg=7, coef=p, flags=p, ws=p, ws_bytes=720)
        a.update(kw)
        return tuple(a[k] for k in ("tiles", "th", "tw", "ys", "ny", "xs", "nx", "Hw", "Ww", "guide", "hg", "wg", "coef", "flags", "ws",
                                    "ws_bytes")) + (None,)
    for name in ("tiles", "guide", "coef", "flags", "ws", "ys", "xs"):
        refused("mg_tile_fit", fit_args(**{name: None}), "null pointer")
    refused("mg_tile_fit", fit_args(ny=0), "0 tiles along y")                     # n < 1
    refused("mg_tile_fit", fit_args(nx=33), "33 tiles along x")
    refused("mg_tile_fit", fit_args(th=60), "multiples of 8")
    refused("mg_tile_fit", fit_args(Ww=250), "multiples of 8")
    refused("mg_tile_fit", fit_args(Hw=112), "outside the canvas")                # the last row of tiles ends at 120
    refused("mg_tile_fit", fit_args(xs=_ints(0, 64, 136)), "outside the canvas")
    refused("mg_tile_fit", fit_args(ys=_ints(-8, 24, 56)), "outside the canvas")
    refused("mg_tile_fit", fit_args(hg=0), "guide size")
    refused("mg_tile_fit", fit_args(tiles=p + 4), "16-byte aligned")
    refused("mg_tile_fit", fit_args(ws=p + 8), "workspace must be 16-byte aligned")   # a misaligned workspace
    refused("mg_tile_fit", fit_args(coef=p + 4), "aligned")
    refused("mg_tile_fit", fit_args(ws_bytes=712), "712", "720")                  # a workspace one double short

    # mg_tile_blend(tiles, C, th, tw, ystarts, ny, xstarts, nx, Hw, Ww, oy, ox, coef_or_null, normalize, out, stream)
    def blend_args(**kw):
        a = dict(tiles=p, C=1, th=64, tw=128, ys=ys, ny=3, xs=xs, nx=3, Hw=120, Ww=256, oy=16, ox=32, coef=None, normalize=0, out=p)
        a.update(kw)
        return tuple(a[k] for k in ("tiles", "C", "th", "tw", "ys", "ny", "xs", "nx", "Hw", "Ww", "oy", "ox", "coef", "normalize", "out")) + (None,)
    for name in ("tiles", "out", "ys", "xs"):
        refused("mg_tile_blend", blend_args(**{name: None}), "null pointer")
    for C in (0, 2, 4, -1):
        refused("mg_tile_blend", blend_args(C=C), "channels")                      # C not in {1, 3}
    refused("mg_tile_blend", blend_args(normalize=1), "normalize")                 # normalize needs three channels
    refused("mg_tile_blend", blend_args(C=3, normalize=2), "normalize")
    refused("mg_tile_blend", blend_args(ny=0), "0 tiles along y")
    refused("mg_tile_blend", blend_args(Hw=112), "outside the canvas")
    refused("mg_tile_blend", blend_args(Hw=128), "cover")                          # the tiles end at 120
    refused("mg_tile_blend", blend_args(ys=_ints(8, 24, 56)), "cover")
    refused("mg_tile_blend", blend_args(ys=_ints(0, 20, 56)), "multiple of 8")
    refused("mg_tile_blend", blend_args(ys=_ints(0, 56, 24)), "cover")
    refused("mg_tile_blend", blend_args(xs=_ints(0, 64, 64), Ww=192), "ascending")
    refused("mg_tile_blend", blend_args(xs=_ints(0, 104, 128)), "overlap of at least 32")   # tiles 0 and 1 share 24 columns
    refused("mg_tile_blend", blend_args(oy=0), "overlap")
    refused("mg_tile_blend", blend_args(oy=12), "overlap")
    refused("mg_tile_blend", blend_args(oy=40), "half")
    refused("mg_tile_blend", blend_args(tiles=p + 4), "16-byte aligned")
    refused("mg_tile_blend", blend_args(out=p + 8), "16-byte aligned")
    refused("mg_tile_blend", blend_args(coef=p + 4), "coef")
    assert list(mem) == [0.0] * 64


# ---- predict_tiled: the refusals ---------------------------------------------------------------------------------------------------

def _engine(name, device, launched):
    def boom(*a, **k):
        launched.append(name)
        raise AssertionError(f"{name}: reached a launch")
    return SimpleNamespace(name=name, device=device, replica=boom, config=SimpleNamespace(block_out_channels=(1, 1, 1, 1)),
                           encode_rgb_latent=boom, denoise_program=boom, set_context=boom, f16=False, dtype=torch.bfloat16)


def _stand_in(cls=MarigoldDepthPipeline):
    launched = []
    device = SimpleNamespace(type="cuda")
    kw = dict(default_denoising_steps=2, default_processing_resolution=0, empty_text_embed=torch.zeros(1, 2, 4))
    if cls is MarigoldIIDPipeline:
        unet = _engine("unet", device, launched)
        unet.config = SimpleNamespace(in_channels=12, out_channels=8)
        pipe = cls(unet, _engine("vae", device, launched), DDIMScheduler(), target_properties={"target_names": ["albedo", "material"]}, **kw)
    else:
        pipe = cls(_engine("unet", device, launched), _engine("vae", device, launched), DDIMScheduler(), **kw)
    pipe._preprocess = lambda *a, **k: launched.append("preprocess") or (_ for _ in ()).throw(AssertionError("reached preprocessing"))
    pipe.launched = launched
    return pipe


PICTURE = torch.zeros(1, 3, 128, 256, dtype=torch.uint8)
TILED = dict(tile_size=(64, 128), tile_overlap=(16, 32))


@pytest.mark.parametrize("cls", [MarigoldDepthPipeline, MarigoldNormalsPipeline], ids=["depth", "normals"])
def test_predict_tiled_refuses_before_any_launch(cls):
    pipe = _stand_in(cls)
    with pytest.raises(ValueError, match="predict_tiled: init_latents cannot be combined with tiles"):
        pipe.predict_tiled(PICTURE, init_latents=torch.zeros(1, 4, 8, 16), **TILED)
    with pytest.raises(ValueError, match="predict_tiled: sequence cannot be combined with tiles"):
        pipe.predict_tiled(PICTURE, sequence=SequenceState(), **TILED)
    with pytest.raises(ValueError, match="predict_tiled: images_per_program cannot be combined with tiles"):
        pipe.predict_tiled(PICTURE, images_per_program=2, **TILED)
    with pytest.raises(ValueError, match="predict_tiled: processing_res cannot be combined with tiles"):
        pipe.predict_tiled(PICTURE, processing_res=64, **TILED)
    with pytest.raises(TypeError, match="unexpected keyword arguments \\['colour'\\]"):
        pipe.predict_tiled(PICTURE, colour=1, **TILED)
    with pytest.raises(L.MarigoldHipError, match="mg_tile_plan: the overlap 40 exceeds half"):
        pipe.predict_tiled(PICTURE, tile_size=64, tile_overlap=40)
    with pytest.raises(ValueError, match="4 tile_generators for 9 tiles"):
        pipe.predict_tiled(PICTURE, tile_generators=[None] * 4, **TILED)
    with pytest.raises(TypeError, match="PIL image or a \\[1, 3, H, W\\] tensor"):
        pipe.predict_tiled(np.zeros((128, 256, 3), np.uint8), **TILED)
    pipe._sharded = lambda: True
    with pytest.raises(ValueError, match="predict_tiled is not available on a member-parallel pipeline"):
        pipe.predict_tiled(PICTURE, **TILED)
    assert pipe.launched == []
    # a plan of one tile is the plain call - which starts, in the stand-in, with its preprocessing
    pipe._sharded = lambda: False
    with pytest.raises(AssertionError, match="reached preprocessing"):
        pipe.predict_tiled(torch.zeros(1, 3, 64, 128, dtype=torch.uint8), tile_size=128, tile_overlap=32)


def test_predict_tiled_refuses_the_iid_pipeline():
    pipe = _stand_in(MarigoldIIDPipeline)
    with pytest.raises(ValueError, match="predict_tiled: the intrinsic-image pipeline is not supported"):
        pipe.predict_tiled(PICTURE, **TILED)
    assert pipe.launched == []


def test_the_depth_output_keeps_its_three_fields_and_gains_an_optional_one():
    out = MarigoldDepthOutput(np.zeros((2, 2), np.float32), None, None)
    assert out.degenerate_tiles is None
    assert MarigoldDepthOutput(np.zeros((2, 2), np.float32), None, None, degenerate_tiles=2).degenerate_tiles == 2


# ---- the command line --------------------------------------------------------------------------------------------------------------

class _FakeCliPipe:
    scale_invariant = shift_invariant = True
    default_denoising_steps, default_processing_resolution = 4, 768

    def __init__(self):
        self.calls = []

    def _out(self):
        from PIL import Image
        return MarigoldDepthOutput(np.linspace(0, 1, 48, dtype=np.float32).reshape(6, 8), Image.fromarray(np.zeros((6, 8, 3), np.uint8)), None, 1)

    def map_images(self, images, in_flight=None, generators=None, **kw):
        images = list(images)
        self.calls.append(("map_images", len(images), kw))
        return [self._out() for _ in images]

    def map_video(self, frames, **kw):
        raise AssertionError("map_video")

    def predict_tiled(self, image, **kw):
        self.calls.append(("predict_tiled", image.size, kw))
        return self._out()


def test_cli_tile_flags(tmp_path):
    from PIL import Image
    from marigold_amd import cli
    from marigold_amd.noise import NativeNoise
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    for kind in ("depth", "normals"):
        a = cli.build_parser(kind).parse_args(io)
        assert (a.tile_size, a.tile_overlap, a.tiled_res) == (0, 0, 0)
        a = cli.build_parser(kind).parse_args(io + ["--tile_size", "768", "--tile_overlap", "192", "--tiled_res", "3000"])
        assert (a.tile_size, a.tile_overlap, a.tiled_res) == (768, 192, 3000)
    for flag in ("--tile_size", "--tile_overlap", "--tiled_res"):
        with pytest.raises(SystemExit):
            cli.build_parser("iid").parse_args(io + [flag, "64"])
    inp = tmp_path / "in"
    inp.mkdir()
    for name in ("b.png", "a.png"):
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / name)
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="--tile_size cannot be combined with --sequence"):
        cli.main("depth", base + ["--sequence", "--tile_size", "64"], pipeline=_FakeCliPipe())
    with pytest.raises(ValueError, match="images_per_program"):
        cli.main("depth", base + ["--images_per_program", "2", "--tile_size", "64"], pipeline=_FakeCliPipe())
    with pytest.raises(ValueError, match="need --tile_size"):
        cli.main("depth", base + ["--tile_overlap", "16"], pipeline=_FakeCliPipe())
    with pytest.raises(ValueError, match="multiples of 8"):
        cli.main("normals", base + ["--tile_size", "60"], pipeline=_FakeCliPipe())
    # with the flag: one predict_tiled per file; --processing_res names the guide's resolution
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--tile_size", "64", "--tiled_res", "96", "--processing_res", "32", "--seed", "9", "--maps_in_flight", "2"],
                    pipeline=pipe) == 0
    assert [c[0] for c in pipe.calls] == ["predict_tiled"] * 2 and pipe.calls[0][1] == (8, 6)
    kw = pipe.calls[0][2]
    assert (kw["tile_size"], kw["tile_overlap"], kw["tiled_res"], kw["guide_res"], kw["in_flight"]) == (64, 16, 96, 32, 2)
    assert isinstance(kw["generator"], NativeNoise) and kw["generator"].seed == 9 and "processing_res" not in kw
    assert kw["match_input_res"] is True and kw["color_map"] == "Spectral" and kw["ensemble_size"] == 1
    assert pipe.calls[0][2]["generator"] is not pipe.calls[1][2]["generator"]
    assert (tmp_path / "out" / "depth_npy" / "a_depth.npy").exists() and (tmp_path / "out" / "depth_colored" / "b_depth_colored.png").exists()
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--tile_size", "768", "--tile_overlap", "192"], pipeline=pipe) == 0
    assert pipe.calls[0][2]["tile_overlap"] == 192 and pipe.calls[0][2]["generator"] is None and pipe.calls[0][2]["guide_res"] is None
    # without it nothing changes
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--seed", "7"], pipeline=pipe) == 0
    (name, n, kw), = pipe.calls
    assert (name, n) == ("map_images", 2)
    assert set(kw) == {"denoising_steps", "ensemble_size", "processing_res", "match_input_res", "batch_size", "show_progress_bar",
                       "resample_method", "color_map"}
