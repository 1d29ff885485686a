"""The tile gather (``mg_tile_crop``) and the one-call tiled prediction (``mg_model_predict_tiled``), the part that needs no GPU: the
header, the binding and both built libraries agree on the two entry points and on ``mg_tiled_opts``; the ABI version, ``sizeof(mg_op)``
and the op kinds are what they were; every refusal of either call fires with its documented prefix on a HOST-ONLY model
(``mg_model_load(path, -1)``) - no GPU is here, and the host-only refusal is the LAST check of ``mg_model_predict_tiled``, so a call
that gets that far has passed every other one and a call that is refused earlier proves where it stopped; the example host program
compiles against the header.  tests/test_gpu_tile_crop.py, tests/test_gpu_tiled_uncertainty.py and
tests/test_gpu_predict_tiled_c_host.py run them on the device."""
import ctypes
import os
import re
import subprocess

import pytest

from marigold_amd import _lib as L

from tests import c_hosts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
A = 0x10000   # a fake, 16-byte aligned device address: no call here gets as far as touching it
# (E, H, W, T, K): 0 the guide of a 128 x 256 picture at guide_res 128, 1 tiles K = 2, 2 tiles with E = 3, 3 a guide with E = 3 and
# K = 2, 4 a tile size that is no multiple of 8
CONFIGS = [dict(ensemble_size=1, height=64, width=128, denoising_steps=2, images_per_program=1),
           dict(ensemble_size=1, height=64, width=128, denoising_steps=2, images_per_program=2),
           dict(ensemble_size=3, height=64, width=128, denoising_steps=2, images_per_program=1),
           dict(ensemble_size=3, height=64, width=128, denoising_steps=2, images_per_program=2),
           dict(ensemble_size=1, height=60, width=128, denoising_steps=2, images_per_program=1)]


def _tiny(kind="depth"):
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0)


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    from marigold_amd import image
    d = tmp_path_factory.mktemp("tiled")
    out = {}
    for kind in ("depth", "normals"):
        out[kind] = image.export_model_image(_tiny(kind), str(d / f"{kind}.mgimg"), configs=CONFIGS)["path"]
    out["iid"] = image.export_model_image(_tiny("iid"), str(d / "iid.mgimg"), ensemble_size=1, height=64, width=128)["path"]
    return out


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _error(lib):
    return lib.mg_last_error().decode(errors="replace")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int mg_tile_crop(const uint8_t* src, int hwc, int Hw, int Ww, int th, int tw, const int* ystarts, int ny, const int* xstarts, "
            "int nx, int first, int count, uint8_t* dst, void* stream);") in flat
    assert ("int mg_model_predict_tiled(mg_model* m, const uint8_t* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed, "
            "const mg_tiled_opts* tiled, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null, float* pred_out, "
            "float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null, double* info4_or_null, int* degenerate_or_null, "
            "void* stream);") in flat
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    body = re.search(r"typedef struct mg_tiled_opts \{(.*?)\} mg_tiled_opts;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for names in re.findall(r"\bint\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [n for n, _ in L.MgTiledOpts._fields_] == ["guide_config", "tile_config", "overlap_y", "overlap_x", "tail_config"]
    assert L.MgTiledOpts(1, 2, 8, 8).tail_config == -1
    assert all(t is ctypes.c_int for _, t in L.MgTiledOpts._fields_)
    pi, vp, i = ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_tile_crop", "mg_model_predict_tiled"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_tile_crop.argtypes == [vp, i, i, i, i, i, pi, i, pi, i, i, i, vp, vp]
        assert lib.mg_model_predict_tiled.argtypes == [vp, vp, i, i, i, i, i, ctypes.c_uint64, ctypes.POINTER(L.MgTiledOpts),
                                                       ctypes.POINTER(L.MgPredictOpts), ctypes.POINTER(L.MgOutputOpts)] + [vp] * 7
    assert ctypes.sizeof(L.MgOp) == 360
    assert "ens_iid" in L.OP_NAMES.values() and len(L.OP_NAMES) == 35   # no op kind was added


def test_options_struct_size_and_the_example_compile(tmp_path):
    src = tmp_path / "size.cpp"
    src.write_text('#include <stdio.h>\n#include "marigold_hip.h"\nint main() { printf("%zu %zu %d", sizeof(mg_tiled_opts), sizeof(mg_op), '
                   'MG_ABI_VERSION); return 0; }\n')
    exe = c_hosts.compile_only(src, tmp_path / "size")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(L.MgTiledOpts), ctypes.sizeof(L.MgOp), L.ABI_VERSION] == [20, 360, 4]
    example = os.path.join(ROOT, "examples", "host_tiled.cpp")
    assert "static_assert(sizeof(mg_tiled_opts)" in open(example).read()
    c_hosts.compile_only(example, tmp_path / "host_tiled.o")


# ---- mg_tile_crop's refusals -------------------------------------------------------------------------------------------------------

@LIBS
def test_tile_crop_refusals(f16):
    lib = L.load(f16)
    ok = dict(src=A, hwc=1, Hw=128, Ww=256, th=64, tw=128, ys=[0, 32, 64], xs=[0, 64, 128], first=0, count=9, dst=A + (1 << 20))

    def crop(**kw):
        a = dict(ok, **kw)
        ys, xs = a["ys"], a["xs"]
        ny, nx = a.get("ny", 0 if ys is None else len(ys)), a.get("nx", 0 if xs is None else len(xs))
        rc = lib.mg_tile_crop(a["src"], a["hwc"], a["Hw"], a["Ww"], a["th"], a["tw"], None if ys is None else _ints(ys), ny,
                              None if xs is None else _ints(xs), nx, a["first"], a["count"], a["dst"], None)
        return rc, _error(lib)

    many = [8 * k for k in range(L.TILE_MAX_PER_AXIS + 1)]
    cases = [(dict(src=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(ys=None), "null pointer"), (dict(xs=None), "null pointer"),
             (dict(th=60), "multiples of 8"), (dict(tw=100), "multiples of 8"), (dict(Hw=124), "multiples of 8"), (dict(Ww=252), "multiples of 8"),
             (dict(th=0), "multiples of 8"), (dict(ys=[0, 28, 64]), "no multiple of 8"), (dict(xs=[0, 4, 128]), "no multiple of 8"),
             (dict(ys=[0, 72]), "outside the canvas"), (dict(xs=[-8, 128]), "outside the canvas"), (dict(xs=[0, 136]), "outside the canvas"),
             (dict(first=-1), r"tiles \[-1, -1 \+ 9\)"), (dict(count=0), "tiles"), (dict(first=1), r"tiles \[1, 1 \+ 9\) of a grid of 3 x 3"),
             (dict(first=9, count=1), "of a grid of 3 x 3"), (dict(count=10), "of a grid of 3 x 3"),
             (dict(ny=0), "1 to 32 are supported"), (dict(nx=0), "1 to 32 are supported"),
             (dict(Hw=512, th=8, ys=many), "1 to 32 are supported"), (dict(Ww=512, tw=8, xs=many), "1 to 32 are supported"),
             (dict(Hw=1 << 15, Ww=1 << 14), "canvas of 32768 x 16384 is not supported")]
    for kw, msg in cases:
        rc, err = crop(**kw)
        assert rc != 0 and err.startswith("mg_tile_crop:") and re.search(msg, err), (kw, err)


# ---- mg_model_predict_tiled's refusals ---------------------------------------------------------------------------------------------

def _tiled_call(lib, handle, **kw):
    a = dict(rgb=A, hwc=1, Hin=128, Win=256, guide=0, tile=1, oy=16, ox=32, out=None, pred=A + (1 << 24), unc=None, u16=None, pic=None,
             flags=None, opts=None, tail=-1)
    a.update(kw)
    tiled = None if a["tile"] is None else ctypes.byref(L.MgTiledOpts(a["guide"], a["tile"], a["oy"], a["ox"], a["tail"]))
    out = None if a["out"] is None else ctypes.byref(L.MgOutputOpts(*a["out"]))
    opts = None if a["opts"] is None else ctypes.byref(a["opts"])
    rc = lib.mg_model_predict_tiled(handle, a["rgb"], a["hwc"], a["Hin"], a["Win"], 0, 1, 7, tiled, opts, out, a["pred"], a["unc"], a["u16"],
                                    a["pic"], None, a["flags"], None)
    return rc, _error(lib)


@LIBS
def test_predict_tiled_refusals_on_a_host_only_model(images, f16):
    lib = L.load(f16)
    who = "mg_model_predict_tiled:"
    rc, err = _tiled_call(lib, None)
    assert rc != 0 and err.startswith(who) and "null argument" in err
    depth = lib.mg_model_load(images["depth"].encode(), -1)
    normals = lib.mg_model_load(images["normals"].encode(), -1)
    iid = lib.mg_model_load(images["iid"].encode(), -1)
    assert depth and normals and iid, _error(lib)
    try:
        assert lib.mg_model_select(depth, 2) == 0
        cases = [
            (depth, dict(rgb=None), "null argument"), (depth, dict(pred=None), "null argument"), (depth, dict(tile=None), "null argument"),
            (iid, dict(tile=0), "an intrinsic-image model is not supported"),
            (depth, dict(Hin=124), "124 x 256 must be multiples of 8"), (depth, dict(Win=260), "128 x 260 must be multiples of 8"),
            (depth, dict(Hin=0), "must be multiples of 8"),
            (depth, dict(Hin=64, Win=128), "the plan is ONE tile.*mg_model_predict_out"),
            (depth, dict(tile=5), "tile configuration 5 of 5"), (depth, dict(tile=-1), "tile configuration -1 of 5"),
            (depth, dict(guide=5), "guide configuration 5 of 5"), (depth, dict(guide=-1), "guide configuration -1 of 5"),
            (depth, dict(tile=4), "60 x 128 .* must be multiples of 8"),
            (depth, dict(Hin=56), "64 x 128 exceeds the picture 56 x 256"), (depth, dict(Win=120), "exceeds the picture 128 x 120"),
            (depth, dict(guide=1), "the guide configuration runs 2 pictures per call"),
            (depth, dict(guide=2), "the guide configuration has 3 members, the tile configuration 1"),
            (depth, dict(guide=0, tile=3), "the guide configuration has 1 members, the tile configuration 3"),
            # the tail: 9 tiles in groups of 2 leave one
            (depth, dict(tail=5), "tail configuration 5 of 5"), (depth, dict(tail=-2), "tail configuration -2 of 5"),
            (depth, dict(tail=1), "the tail configuration runs 2 pictures per call, the short last group has 1 tiles"),
            (depth, dict(tail=2), "the tail configuration is of another kind, size .64 x 128. or member count .3."),
            (depth, dict(tail=4), "the tail configuration is of another kind, size .60 x 128."),
            # every plan refusal of mg_tile_plan, in its words behind the prefix
            (depth, dict(oy=0), "mg_tile_plan: the overlap 0 must be a multiple of 8"), (depth, dict(ox=12), "mg_tile_plan: the overlap 12 must be"),
            (depth, dict(oy=40), "mg_tile_plan: the overlap 40 exceeds half the tile length 64"),
            (depth, dict(ox=72), "mg_tile_plan: the overlap 72 exceeds half the tile length 128"),
            # every output-option refusal of mg_model_predict_out, in its words
            (depth, dict(out=(96, 0, 0, None)), "bad output size 96 x 0"), (depth, dict(out=(-1, -1, 0, None)), "bad output size -1 x -1"),
            (depth, dict(out=(96, 192, 3, None)), "out_mode must be 0"),
            (depth, dict(pic=A), "the picture of a depth model needs out_opts.lut256x3"),
            (normals, dict(u16=A), "u16_out and lut256x3 belong to a depth model"),
            (normals, dict(out=(0, 0, 0, A)), "u16_out and lut256x3 belong to a depth model"),
            (normals, dict(opts=L.MgPredictOpts(normals_reduction=2)), "Unrecognized reduction method: 2"),
            (depth, dict(pred=A + 4), "16-byte aligned"), (depth, dict(tile=2, guide=2, unc=A + 8), "16-byte aligned"),
            (depth, dict(flags=A + 2), "aligned to its elements"),
        ]
        for handle, kw, msg in cases:
            rc, err = _tiled_call(lib, handle, **kw)
            assert rc != 0 and err.startswith(who) and re.search(msg, err), (kw, err)
        # more than MG_TILE_MAX_PER_AXIS tiles along x: 8-pixel overlaps of 128-pixel tiles over 4096 pixels make 34
        rc, err = _tiled_call(lib, depth, Win=4096, ox=8)
        assert rc != 0 and err.startswith(who + " mg_tile_plan:") and "at most 32 are supported" in err, err
        # a call that passes every check reaches the last one: the model is host-only.  For normals the guide index is not looked at.
        for handle, kw in ((depth, {}), (depth, dict(tail=0)), (depth, dict(tile=2, guide=2, unc=A, flags=A, out=(96, 192, 1, A), pic=A, u16=A)),
                           (normals, dict(guide=99)), (normals, dict(tile=3, unc=A, pic=A, out=(96, 192, 2, None)))):
            rc, err = _tiled_call(lib, handle, **kw)
            assert rc != 0 and err == who + " a host-only model cannot predict (load it with device >= 0)", (kw, err)
        # no refused call moved the handle off its configuration
        cfg = (ctypes.c_int * 16)()
        assert lib.mg_model_info(depth, cfg) == 0 and cfg[0] == 3 and (cfg[13] or 1) == 1
        assert lib.mg_model_device_bytes(depth) > 0 and lib.mg_model_validate(depth) == 0
    finally:
        for h in (depth, normals, iid):
            lib.mg_model_destroy(h)


def test_python_wrappers_exist_and_refuse_host_tensors():
    import torch
    from marigold_amd import image, tiles
    assert callable(image.ModelImage.predict_tiled)
    plan = tiles.plan((128, 256), (64, 128), (16, 32))
    with pytest.raises(ValueError, match="uint8 CUDA tensor"):
        tiles.crop(torch.zeros(128, 256, 3, dtype=torch.uint8), plan, 0, 9)
