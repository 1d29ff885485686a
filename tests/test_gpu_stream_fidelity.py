"""The stream contract of include/marigold_hip.h on a real MI355X, for every stand-alone call that takes a ``void* stream`` and brings
its own buffers: all of its device work goes to that stream, it returns without waiting for it, two calls in flight on two streams do
not see each other, and two host threads may make such calls at once.  Both operand libraries.

One row per entry point (``ROWS``).  A row builds a ``stream_gate.Call`` from a scene of that entry point's own tests - the smallest
of its ladder that still runs every launch of the chain - and, for the families whose own tests demand bit equality, holds the result
to the restatement those tests use.  tests/stream_gate.py explains the gate.

Part 1  the call behind the gate == the call alone on the side stream == the call alone on the null stream (== the restatement).
Part 2  right after the gated call returns the stream is still busy (``query()`` is False): the call did not wait.
Part 3  two calls behind two gates on two streams, both made before either gate opens: the same entry point on two scenes, and
        every entry point beside one fixed neighbour (``mg_depth_focus``; ``mg_depth_view`` for focus itself).
Part 4  two host threads, a stream each, the whole table once, no gate; and ``mg_last_error`` on the thread that was refused.

The calls the header documents as synchronising (``SYNCHRONISES``) get part 1 only.  tests/test_stream_fidelity_host.py checks on
the CPU that this table names every prototype of the header that ends in ``void* stream)``."""
import ctypes
import functools
import os
import threading

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from tests import stream_gate as G

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The calls that wait for their stream, each with the sentence of include/marigold_hip.h that says so.  mg_ensemble_depth runs behind
# the gate (part 1); the one-call predictions are model programs, which the lane tests of map_images hold to their streams.
SYNCHRONISES = {
    "mg_ensemble_depth": "Synchronises the stream.",
    "mg_model_predict": "Synchronises the stream where mg_ensemble_depth does (depth, B > 1) and nowhere else.",
    "mg_model_predict_out": "Synchronises where mg_ensemble_depth does and nowhere else.",
    "mg_model_predict_many": "Synchronises where mg_ensemble_depth does - once per picture",
    "mg_model_predict_next": "Synchronises where mg_model_predict_out does.",
    "mg_model_predict_tiled": "Synchronises where mg_ensemble_depth does (depth, B > 1: once for the guide and once per tile) and nowhere else.",
}
# Prototypes with a stream that are no row, and why
OUT_OF_SCOPE = {
    "mg_launch": "one op of a model program", "mg_program_run": "model program", "mg_program_run_range": "model program",
    "mg_program_capture": "model program", "mg_conv2d_igemm": "MG_OP_IGEMM: the library's tickets and split-K workspace are single-stream",
    "mg_conv3x3": "one op of a model program (mg_launch under a name)", "mg_model_vae_encode": "model program",
    "mg_model_denoise": "model program", "mg_model_vae_decode": "model program", "mg_model_scratch_fill": "the model's own buffers",
    "mg_model_predict": "model program", "mg_model_predict_iid": "model program", "mg_model_predict_out": "model program",
    "mg_model_predict_many": "model program", "mg_model_predict_tiled": "model program", "mg_event_record": "records an event, no device work",
}


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _np(t):
    return t.detach().cpu().contiguous().numpy()


def _bits16(t):
    """a bf16 / fp16 tensor -> its bits as a numpy int16 array"""
    return _np(t.contiguous().view(torch.int16))


def _pick(seq, variant, what):
    found = [c for c in seq if what(c)]
    assert len(found) > variant, "the ladder lost the scene this row runs"
    return found[variant]


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- the rows: (lib, f16, variant) -> Call.  Variant 0 is the row's scene, variant 1 a second scene of the same ladder --------------

def _focus(lib, f16, variant):
    from tests.focus_scenes import cases
    shape = ((17, 65), (9, 33))[variant]
    c = _pick(cases(), 0, lambda c: c.shape == shape and c.max_radius == 8 and c.gain > 0)
    h, w = c.shape
    n = h * w
    k = G.Call("mg_depth_focus")
    need = lib.mg_depth_focus_workspace_bytes(n)
    fy, fx = c.focus_at if c.focus_at is not None else (-1, -1)
    a = [k.inp(c.d), k.inp(c.colors), int(c.hwc), k.inp(c.mask), k.inp(None if c.coef is None else np.asarray(c.coef, np.float64)), h, w,
         c.z_range[0], c.z_range[1], c.space, c.gain, c.max_radius, fx, fy, 0.0 if c.focus is None else c.focus,
         k.out("rgb", np.uint8, 3 * n), k.out("valid", np.uint8, n), k.out("radius", np.uint16, n), k.out("count", np.int64, 5), k.ws(need), need]
    k.launch = lambda s: lib.mg_depth_focus(*a, s)

    def check(got):
        assert got["count"].tolist() == list(c.want.count) and np.array_equal(got["valid"].reshape(h, w), c.want.valid)
        assert np.array_equal(got["radius"].reshape(h, w), c.want.radius) and np.array_equal(got["rgb"].reshape(c.want.rgb.shape), c.want.rgb)
    k.check = check
    return k


def _view(lib, f16, variant):
    from tests.test_gpu_points import Z_RANGE
    from tests.view_scenes import cases, Z_NEAR
    c = _pick(cases(), 0, lambda c: c.shape == (17, 33) and c.pose_name == ("stereo_right", "turn")[variant])
    assert c.fill > 0 and c.want.count[7] > 0 and c.mask is not None   # holes, and the launch that fills them has work
    coef, edge, hwc = c.opt
    (h, w), (h2, w2) = c.shape, c.size
    n2 = h2 * w2
    pose = np.ascontiguousarray(c.pose, np.float64)
    k = G.Call("mg_depth_view")
    k.alive.append(pose)
    need = lib.mg_depth_view_workspace_bytes(n2)
    a = [k.inp(c.d), k.inp(c.colors), int(hwc), k.inp(c.mask), k.inp(None if coef is None else np.asarray(coef, np.float64)), h, w, *c.K,
         Z_RANGE[0], Z_RANGE[1], edge, pose.ctypes.data, *c.K_out, h2, w2, Z_NEAR, c.fill, k.out("rgb", np.uint8, 3 * n2),
         k.out("depth", np.float32, n2), k.out("valid", np.uint8, n2), k.out("face", np.int32, n2) if c.face else None, k.out("count", np.int64, 8),
         k.ws(need), need]
    k.launch = lambda s: lib.mg_depth_view(*a, s)

    def check(got):
        want = c.want
        assert got["count"].tolist() == list(want.count) and np.array_equal(got["valid"].reshape(h2, w2), want.valid)
        assert not c.face or np.array_equal(got["face"].reshape(h2, w2), want.face)
        assert np.array_equal(got["rgb"].reshape(want.rgb.shape), want.rgb)
        assert np.array_equal(got["depth"].view(np.uint32).reshape(h2, w2), want.depth.view(np.uint32))
    k.check = check
    return k


def _masked_with_coef(cases, variant):
    """a scene with a mask and ``coef`` that keeps something: 7 x 65, and for the second scene 97 x 127 (several chunks)"""
    shape = ((7, 65), (97, 127))[variant]
    return _pick(cases, 0, lambda c: c[1].shape == shape and c[3] is not None and c[5][0] is not None and c[6].count[0] > 0)


def _points(lib, f16, variant):
    from tests.test_gpu_points import _cases, Z_RANGE
    _, d, colors, mask, K, (coef, edge, frame, hwc), want = _masked_with_coef(_cases(), variant)
    h, w = d.shape
    n, cap = h * w, h * w + 3
    k = G.Call("mg_depth_points")
    need = lib.mg_depth_points_workspace_bytes(n)
    a = [k.inp(d), k.inp(colors), int(hwc), k.inp(mask), k.inp(np.asarray(coef, np.float64)), h, w, *K, Z_RANGE[0], Z_RANGE[1], edge,
         L.NORMALS_FRAME[frame], cap, k.out("xyz", np.float32, 3 * cap), k.out("rgb", np.uint8, 3 * cap), k.out("nrm", np.float32, 3 * cap),
         k.out("index", np.int32, cap), k.out("count", np.int64, 2), k.ws(need), need]
    k.launch = lambda s: lib.mg_depth_points(*a, s)

    def check(got):   # (the normals are held to one fp32 step by their own test: here they are held to the call run alone)
        kept, written = want.count
        assert got["count"].tolist() == [kept, written] and written > 0 and np.array_equal(got["index"][:written], want.index)
        assert np.array_equal(got["rgb"][:3 * written].reshape(-1, 3), want.rgb)
        assert np.array_equal(got["xyz"][:3 * written].view(np.uint32).reshape(-1, 3), np.ascontiguousarray(want.xyz).view(np.uint32))
    k.check = check
    return k


def _normals(lib, f16, variant):
    from tests.test_gpu_points import _cases, Z_RANGE
    _, d, _, mask, K, (coef, edge, frame, _), want = _masked_with_coef(_cases(), variant)
    h, w = d.shape
    k = G.Call("mg_depth_normals")
    a = [k.inp(d), k.inp(mask), k.inp(np.asarray(coef, np.float64)), h, w, *K, Z_RANGE[0], Z_RANGE[1], edge, L.NORMALS_FRAME[frame],
         k.out("out", np.float32, 3 * h * w), k.out("valid", np.uint8, h * w)]
    k.launch = lambda s: lib.mg_depth_normals(*a, s)
    k.check = lambda got: np.array_equal(got["valid"].reshape(h, w), want.valid) or pytest.fail("valid differs from the restatement")
    return k


def _mesh(lib, f16, variant):
    from tests.test_gpu_mesh import _cases
    from tests.test_gpu_points import Z_RANGE
    _, d, colors, mask, K, (coef, edge, frame, hwc), want = _masked_with_coef(_cases(), variant)
    h, w = d.shape
    n, cap_v, cap_f = h * w, h * w + 3, 2 * (h - 1) * (w - 1) + 3
    k = G.Call("mg_depth_mesh")
    need = lib.mg_depth_mesh_workspace_bytes(n)
    a = [k.inp(d), k.inp(colors), int(hwc), k.inp(mask), k.inp(np.asarray(coef, np.float64)), h, w, *K, Z_RANGE[0], Z_RANGE[1], edge,
         L.NORMALS_FRAME[frame], cap_v, cap_f, k.out("xyz", np.float32, 3 * cap_v), k.out("rgb", np.uint8, 3 * cap_v),
         k.out("nrm", np.float32, 3 * cap_v), k.out("index", np.int32, cap_v), k.out("faces", np.int32, 3 * cap_f), k.out("count", np.int64, 4),
         k.ws(need), need]
    k.launch = lambda s: lib.mg_depth_mesh(*a, s)

    def check(got):
        V, Vw, F, Fw = want.count
        assert got["count"].tolist() == [V, Vw, F, Fw] and F > 0 and np.array_equal(got["faces"][:3 * Fw].reshape(-1, 3), want.faces)
        assert np.array_equal(got["index"][:Vw], want.index) and np.array_equal(got["rgb"][:3 * Vw].reshape(-1, 3), want.rgb)
        assert np.array_equal(got["xyz"][:3 * Vw].view(np.uint32).reshape(-1, 3), np.ascontiguousarray(want.xyz).view(np.uint32))
    k.check = check
    return k


def _align_fit(lib, f16, variant):
    from tests.test_gpu_align import _scene, CHUNK, DELTA
    n = (CHUNK + 1, 12293)[variant]
    d, ref, mask = _scene(n, True, True)
    k = G.Call("mg_depth_align_fit")
    need = lib.mg_depth_align_workspace_bytes(n)
    a = [k.inp(d), k.inp(ref), k.inp(mask), n, 1, 4, L.ALIGN_START_LS, 1.0, 0.0, DELTA, k.out("coef", np.float64, 2), k.out("flag", np.int32, 1),
         k.ws(need), need]
    k.launch = lambda s: lib.mg_depth_align_fit(*a, s)
    return k


def _align_apply(lib, f16, variant):
    from tests.align_reference import align_apply_reference
    n = (4097, 24 * 40)[variant]
    x = (np.random.default_rng(7).random(n) * 3 - 1).astype(np.float32)
    x[[0, 5, 9, 17, n - 1]] = (np.nan, np.inf, -np.inf, -0.0, np.nan)
    coef = np.array([3.7, -1.2])
    k = G.Call("mg_depth_align_apply")
    a = [k.inp(x), n, k.inp(coef), 1, 0.0, 1.0, k.out("out", np.float32, n)]
    k.launch = lambda s: lib.mg_depth_align_apply(*a, s)

    def check(got):
        want = align_apply_reference(x, coef, True, (0.0, 1.0))
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got["out"]), nan) and _same_bits(got["out"][~nan], want[~nan])
    k.check = check
    return k


def _guided(lib, f16, variant):
    from tests.test_gpu_guided import _case, LADDER
    index = (2, 0)[variant]
    pred, lo, hi, _, _ = _case(index, "random", 2, 0.1)
    (h, w), (H, W) = LADDER[index]
    k = G.Call("mg_guided_upsample")
    a = [k.inp(pred[:3]), 3, h, w, k.inp(lo), k.inp(hi), 1, H, W, 2, 0.1, k.out("out", np.float32, 3 * H * W)]
    k.launch = lambda s: lib.mg_guided_upsample(*a, s)
    return k


def _tile_crop(lib, f16, variant):
    from marigold_amd import tiles as T
    hwc = variant == 0
    canvas, tile, overlap = (24, 40), (16, 16), (8, 8)
    plan = T.plan(canvas, tile, overlap)
    (H, W), (th, tw), n = canvas, plan.tile_hw, len(plan.origins)
    host = torch.randint(0, 256, (H, W, 3) if hwc else (3, H, W), generator=torch.Generator().manual_seed(701), dtype=torch.uint8).numpy()
    ys, xs = list(plan.ystarts), list(plan.xstarts)
    k = G.Call("mg_tile_crop")
    a = [k.inp(host), int(hwc), H, W, th, tw, _ints(ys), len(ys), _ints(xs), len(xs), 0, n, k.out("dst", np.uint8, n * 3 * th * tw)]
    k.launch = lambda s: lib.mg_tile_crop(*a, s)
    want = np.stack([host[y:y + th, x:x + tw] if hwc else host[:, y:y + th, x:x + tw] for y, x in plan.origins])
    k.check = lambda got: _same_bits(got["dst"], want) or pytest.fail("the crop is not the slicing")
    return k


def _tile_fit(lib, f16, variant):
    """a 2 x 2 plan: the first two starts per axis of the fit test's three, its tiles 0, 1, 3 and 4 (a constant tile and one with holes
    among them)"""
    from tests.test_gpu_tiles import _fit_case
    th, tw = ((8, 24), (64, 128))[variant]
    tiles, ys, xs, canvas, guide, _, _ = _fit_case(th, tw, False, (5, 7), seed=107 + variant)
    tiles, ys, xs = tiles[[0, 1, 3, 4]].contiguous(), ys[:2], xs[:2]
    k = G.Call("mg_tile_fit")
    need = lib.mg_tiles_workspace_bytes(4, th, tw)
    a = [k.inp(_np(tiles)), th, tw, _ints(ys), 2, _ints(xs), 2, canvas[0], canvas[1], k.inp(_np(guide)), guide.shape[0], guide.shape[1],
         k.out("coef", np.float64, 8), k.out("flags", np.int32, 4), k.ws(need), need]
    k.launch = lambda s: lib.mg_tile_fit(*a, s)
    return k


def _tile_blend(lib, f16, variant):
    from marigold_amd import tiles as T
    canvas, tile, overlap = (((24, 40), (16, 16), (8, 8)), ((96, 160), (64, 64), (16, 16)))[variant]
    plan = T.plan(canvas, tile, overlap)
    n, (th, tw) = len(plan.origins), plan.tile_hw
    g = torch.Generator().manual_seed(304 - 2 * variant)
    d = torch.rand(n, 1, th, tw, generator=g) * 4 - 1
    coef = np.stack([0.3 + 2.7 * torch.rand(n, generator=g, dtype=torch.float64).numpy(), torch.rand(n, generator=g, dtype=torch.float64).numpy() * 2 - 1],
                    axis=1)
    coef[n // 2, 0] = 0.0
    ys, xs = list(plan.ystarts), list(plan.xstarts)
    k = G.Call("mg_tile_blend")
    a = [k.inp(_np(d)), 1, th, tw, _ints(ys), len(ys), _ints(xs), len(xs), canvas[0], canvas[1], overlap[0], overlap[1], k.inp(coef), 0,
         k.out("out", np.float32, canvas[0] * canvas[1])]
    k.launch = lambda s: lib.mg_tile_blend(*a, s)
    return k


def _rgb_prepare(lib, f16, variant):
    from tests.test_gpu_io_stages import _picture
    src = _picture(33, 47, 80, ("checker", "random")[variant]).numpy()
    k = G.Call("mg_rgb_prepare")
    a = [k.inp(src), 1, 33, 47, k.out("dst", np.float32, 3 * 24 * 34), 0, 24, 34, 1, 1, k.ws(4 * 3 * 33 * 34)]
    k.launch = lambda s: lib.mg_rgb_prepare(*a, s)
    return k


def _resize(lib, f16, variant):
    from tests.test_gpu_resample_ladder import _random
    u8 = variant == 1
    x = _random((3, 33, 47), torch.uint8 if u8 else torch.float32, torch.Generator().manual_seed(21)).numpy()
    k = G.Call("mg_resize")
    a = [k.inp(x), k.out("dst", np.uint8 if u8 else np.float32, 3 * 24 * 34), k.ws(4 * 3 * 33 * 34), 3, 33, 47, 24, 34, 0, int(u8)]
    k.launch = lambda s: lib.mg_resize(*a, s)
    return k


def _lut():
    g = np.random.default_rng(5)
    t = g.integers(0, 256, size=(256, 3), dtype=np.uint8)
    t[:, 0] = g.permutation(256).astype(np.uint8)
    return t


def _depth_stage_restated(x):
    """the numpy lines of the depth output stage (tests/test_gpu_out_stage_kernels.py) -> (clipped, u16, the picture, the NaN mask)"""
    with np.errstate(invalid="ignore"):
        nan, clipped = np.isnan(x), np.clip(x, 0, 1)
        u16 = (clipped * np.float32(65535.0)).astype(np.uint16)
        idx = np.minimum((np.where(nan, np.float32(0), clipped) * np.float32(256.0)).astype(np.int64), 255)
    return clipped, u16, np.where(nan[:, None], np.uint8(0), _lut()[idx]), nan


def _colorize(lib, f16, variant):
    from tests.test_gpu_out_stage_kernels import _depth_input
    n = (37 * 53, 64 * 128)[variant]
    x = _depth_input(n, 3 + variant)
    k = G.Call("mg_colorize")
    a = [k.inp(x), k.inp(_lut()), k.out("out", np.uint8, 3 * n), n, 0.0, 1.0]
    k.launch = lambda s: lib.mg_colorize(*a, s)
    k.check = lambda got: np.array_equal(got["out"].reshape(n, 3), _depth_stage_restated(x)[2]) or pytest.fail("not the numpy picture")
    return k


def _depth_visualize(lib, f16, variant):
    from tests.test_gpu_out_stage_kernels import _depth_input
    n = (64 * 128, 37 * 53)[variant]
    x = _depth_input(n, 5 + variant)
    k = G.Call("mg_depth_visualize")
    a = [k.inp(x), k.inp(_lut()), n, k.out("clipped", np.float32, n), k.out("u16", np.uint16, n), k.out("out", np.uint8, 3 * n)]
    k.launch = lambda s: lib.mg_depth_visualize(*a, s)

    def check(got):
        clipped, u16, picture, nan = _depth_stage_restated(x)
        assert _same_bits(got["clipped"], clipped) and np.array_equal(got["u16"][~nan], u16[~nan]) and not got["u16"][nan].any()
        assert np.array_equal(got["out"].reshape(n, 3), picture)
    k.check = check
    return k


def _normals_finish(lib, f16, variant):
    from tests.test_gpu_out_stage_kernels import _normals_input
    H, W = ((37, 53), (64, 128))[variant]
    x = _normals_input(H * W, 7 + variant)
    k = G.Call("mg_normals_finish")
    a = [k.inp(x), H, W, k.out("clipped", np.float32, 3 * H * W), k.out("out", np.uint8, 3 * H * W)]
    k.launch = lambda s: lib.mg_normals_finish(*a, s)

    def check(got):
        with np.errstate(invalid="ignore"):
            nan, clipped = np.isnan(x), np.clip(x, -1, 1)
            picture = ((clipped + 1) * 127.5).astype(np.uint8)
        out = got["out"].reshape(H * W, 3)
        assert _same_bits(got["clipped"], clipped) and np.array_equal(out.T[~nan], picture[~nan]) and not out.T[nan].any()
    k.check = check
    return k


def _normals_visualize(lib, f16, variant):
    from tests.test_gpu_io_stages import _normals_input, _numpy_picture
    H, W = ((16, 20), (33, 64))[variant]
    x = _normals_input(H, W, 4 + variant).numpy()
    k = G.Call("mg_normals_visualize")
    a = [k.inp(x), H, W, k.out("out", np.uint8, 3 * H * W)]
    k.launch = lambda s: lib.mg_normals_visualize(*a, s)
    k.check = lambda got: _same_bits(got["out"], _numpy_picture(x)) or pytest.fail("not the numpy picture")
    return k


def _iid_visualize(lib, f16, variant):
    from tests.test_gpu_iid_output import _values
    n, H, W = ((3, 33, 65), (1, 11, 13))[variant]
    pred = _values("uniform", (n, H, W), 3300 + variant).numpy()
    k = G.Call("mg_iid_visualize")   # target 0 linear, 1 up to scale, 2 both; the lone target of the second scene both
    a = [k.inp(pred), k.out("out", np.uint8, n * H * W * 3), k.ws(4 * n * L.IID_VIS_PARTS), n, H, W, 0b101 if n == 3 else 1, 0b110 if n == 3 else 1]
    k.launch = lambda s: lib.mg_iid_visualize(*a, s)
    return k


def _randn(lib, f16, variant):
    n = (1023, 4096 + 5)[variant]
    k = G.Call("mg_randn")
    a = [7, 2, 5, n, k.out("dst", np.float32, n), 0]
    k.launch = lambda s: lib.mg_randn(*a, s)

    def check(got):
        """the same op alone (``native_randn``: MG_OP_RANDN on torch's current stream), bit for bit, and the float64 Box-Muller
        restatement at the bound of tests/test_gpu_native_noise.py - the restatement's own libm keeps it from being bit-equal"""
        from marigold_amd import native_randn
        from tests import philox_reference as P
        same_op = native_randn((n,), 7, stream=2, offset=5, device="cuda:0")
        torch.cuda.synchronize()
        assert _same_bits(got["dst"], same_op.cpu().numpy())
        assert np.abs(got["dst"] - P.normals(7, 2, 5, n)).max() <= 1e-5
    k.check = check
    return k


def _latent_carry(lib, f16, variant):
    from tests.test_gpu_sequence import _blend_cpu, _planted
    n = (515, 2 * 4 * 8 * 16 + 1)[variant]
    x0, p0 = _planted(n, 3 + n), _planted(n, 11 + 2 * n)
    k = G.Call("mg_latent_carry")
    a = [k.inout("x", x0.numpy()), k.inp(p0.numpy()), n, 0.1]
    k.launch = lambda s: lib.mg_latent_carry(*a, s)

    def check(got):
        want, x = _blend_cpu(x0, p0, 0.1).numpy(), got["x"].view(np.float32)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(x), nan) and _same_bits(x[~nan], want[~nan])
    k.check = check
    return k


def _sched_step(lib, f16, variant):
    g = torch.Generator().manual_seed(6 + variant)
    x, m, nz = (torch.randn(3, 4, 8, 8, generator=g).numpy() for _ in range(3))
    k = G.Call("mg_sched_step")
    a = [k.inp(x), k.inp(m), k.inp(nz), k.out("out", np.float32, x.size), x.size, 0.7, -0.3, 0.2]
    k.launch = lambda s: lib.mg_sched_step(*a, s)
    return k


def _ensemble_normals(lib, f16, variant):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ensemble_ref.npz"))
    n = gold[("n_e4_in", "n_e10_in")[variant]]
    E, HW = n.shape[0], n.shape[2] * n.shape[3]
    k = G.Call("mg_ensemble_normals")
    a = [k.inp(n.reshape(E, 3, HW).astype(np.float32)), k.out("out", np.float32, 3 * HW), k.out("unc", np.float32, HW), E, HW, 0]
    k.launch = lambda s: lib.mg_ensemble_normals(*a, s)
    return k


def _ensemble_iid(lib, f16, variant):
    from tests import ensemble_bits as EB
    E, n = ((10, 1023), (5, 1280))[variant]
    x, _ = EB.inputs(E, n, False)
    k = G.Call("mg_ensemble_iid")
    a = [k.inp(x), E, n, 0, k.out("pred", np.float32, n), k.out("unc", np.float32, n)]
    k.launch = lambda s: lib.mg_ensemble_iid(*a, s)
    return k


@functools.lru_cache(maxsize=None)
def _eval_inputs():
    from oracle.make_eval_golden import eval_inputs
    return eval_inputs()


def _eval_depth(lib, f16, variant):
    c = _eval_inputs()[("depth_a", "depth_b")[variant]]
    H, W = c["gt"].shape[-2:]
    k = G.Call("mg_eval_depth")
    a = [k.inp(c["rel"].astype(np.float32)), k.inp(c["gt"].astype(np.float32)), k.inp(c["mask"].astype(np.uint8)), H, W, L.EVAL_ALIGN["least_square"],
         0, float("nan"), float("nan"), k.out("out13", np.float64, 13), k.ws(L.EVAL_WS_BYTES)]
    k.launch = lambda s: lib.mg_eval_depth(*a, s)
    return k


def _eval_normals(lib, f16, variant):
    c = _eval_inputs()["normals"]
    pred, gt = (c[key].astype(np.float32).reshape(3, -1) for key in ("pred", "gt"))
    if variant:   # the second scene: the same maps without their last row of pixels' worth
        pred, gt = np.ascontiguousarray(pred[:, :-37]), np.ascontiguousarray(gt[:, :-37])
    HW = pred.shape[1]
    k = G.Call("mg_eval_normals")
    a = [k.inp(pred), k.inp(gt), HW, 1, k.out("out9", np.float64, 9), k.out("err", np.float32, HW), k.ws(L.EVAL_WS_BYTES)]
    k.launch = lambda s: lib.mg_eval_normals(*a, s)
    return k


def _eval_iid(lib, f16, variant):
    from tests.test_gpu_eval_iid import _pair
    shape = ((37, 53), (32, 40))[variant]
    pred, gt, mask = _pair(shape, 7000 + shape[0], True)
    k = G.Call("mg_eval_iid")
    a = [k.inp(pred), k.inp(gt), k.inp(mask.astype(np.uint8)), shape[0], shape[1], 1, L.iid_gamma_mode(None), 3, k.out("out8", np.float64, 8),
         k.ws(L.EVAL_WS_BYTES)]
    k.launch = lambda s: lib.mg_eval_iid(*a, s)
    return k


def _eval_iid_lpips(lib, f16, variant):
    from tests import lpips_cases as C
    case = ((31, 31),) + (("shading", True, 0), ("albedo", True, 1))[variant]
    (H, W), target, _, gamma_mode = case
    p, g, mask = C.case_inputs(*case)
    net = C.net("live")
    net.to(torch.device("cuda", 0))
    need = lib.mg_lpips_workspace_bytes(H, W)
    assert need > 0
    k = G.Call("mg_eval_iid_lpips")
    k.alive.append(net)
    a = [ctypes.byref(net._struct), k.inp(p), k.inp(g), k.inp(mask.astype(np.uint8)), H, W, int(target in C.UP_TO_SCALE), gamma_mode,
         k.out("out8", np.float64, 8), k.ws(L.EVAL_WS_BYTES), k.ws(need), need]
    k.launch = lambda s: lib.mg_eval_iid_lpips(*a, s)
    return k


def _tiny_conv3x3(lib, f16, variant):
    from tests.test_gpu_tiny_vae import _nhwc, _operands
    dt = torch.float16 if f16 else torch.bfloat16
    B, H, W = ((2, 17, 33), (1, 9, 33))[variant]
    x, w, b, r, (Ho, Wo) = _operands(B, H, W, dt, 1000 + variant, True, True, 1, False)
    wd = w.permute(2, 3, 0, 1).reshape(9, 64, 64).contiguous().to(torch.float32).to(dt)
    k = G.Call("mg_tiny_conv3x3")
    a = [k.inp(_bits16(_nhwc(x, dt))), k.const(wd), k.const(b.float()), k.inp(_bits16(_nhwc(r, dt))), k.out("out", np.int16, B * Ho * Wo * 64), B, H, W,
         1, 0, 1]
    k.launch = lambda s: lib.mg_tiny_conv3x3(*a, s)
    return k


@functools.lru_cache(maxsize=None)
def _tiny_vae(f16):
    from marigold_amd.modules import AutoencoderTinyHIP
    from marigold_amd.synthetic import synthetic_tiny_vae_state_dict
    return AutoencoderTinyHIP(synthetic_tiny_vae_state_dict(seed=1234), compute_dtype=torch.float16 if f16 else torch.bfloat16).to("cuda:0")


def _tiny_vae_encode(lib, f16, variant):
    B, H, W = ((1, 15, 11), (1, 8, 8))[variant]
    vae = _tiny_vae(f16)
    rgb = (torch.rand(B, 3, H, W, generator=torch.Generator("cpu").manual_seed(11), dtype=torch.float64) * 2 - 1).float().numpy()
    h, w = vae.latent_hw((H, W))
    need = lib.mg_tiny_vae_workspace_bytes(0, B, H, W)
    assert need > 0
    k = G.Call("mg_tiny_vae_encode")
    a = [ctypes.byref(vae._net), k.inp(rgb), k.out("latent", np.float32, B * 4 * h * w), B, H, W, k.ws(need), need]
    k.launch = lambda s: lib.mg_tiny_vae_encode(*a, s)
    return k


def _tiny_vae_decode(lib, f16, variant):
    B, h, w = ((2, 5, 7), (1, 1, 1))[variant]
    vae = _tiny_vae(f16)
    z = torch.randn(B, 4, h, w, generator=torch.Generator("cpu").manual_seed(12), dtype=torch.float64).float().numpy()
    need = lib.mg_tiny_vae_workspace_bytes(1, B, h, w)
    assert need > 0
    k = G.Call("mg_tiny_vae_decode")
    a = [ctypes.byref(vae._net), k.inp(z), k.out("out", np.float32, B * 64 * h * w), B, h, w, L.POST_DEPTH, k.ws(need), need]
    k.launch = lambda s: lib.mg_tiny_vae_decode(*a, s)
    return k


def _ensemble_depth(lib, f16, variant):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "ensemble_ref.npz"))
    d = gold[("d_e10_in", "d_e3_in")[variant]].astype(np.float32)
    E, H, W = d.shape[0], d.shape[2], d.shape[3]
    k = G.Call("mg_ensemble_depth")
    a = [k.inp(d), E, H, W, 1, 1, 0, 0.02, 50, 1e-6, 1024, k.out("depth", np.float32, H * W), k.out("unc", np.float32, H * W), None]
    k.launch = lambda s: lib.mg_ensemble_depth(*a, s)
    return k


ROWS = {
    "mg_depth_normals": _normals, "mg_depth_points": _points, "mg_depth_mesh": _mesh, "mg_depth_view": _view, "mg_depth_focus": _focus,
    "mg_depth_align_fit": _align_fit, "mg_depth_align_apply": _align_apply, "mg_guided_upsample": _guided,
    "mg_tile_crop": _tile_crop, "mg_tile_fit": _tile_fit, "mg_tile_blend": _tile_blend,
    "mg_rgb_prepare": _rgb_prepare, "mg_resize": _resize,
    "mg_colorize": _colorize, "mg_depth_visualize": _depth_visualize, "mg_normals_finish": _normals_finish,
    "mg_normals_visualize": _normals_visualize, "mg_iid_visualize": _iid_visualize,
    "mg_randn": _randn, "mg_latent_carry": _latent_carry, "mg_sched_step": _sched_step,
    "mg_ensemble_normals": _ensemble_normals, "mg_ensemble_iid": _ensemble_iid,
    "mg_eval_depth": _eval_depth, "mg_eval_normals": _eval_normals, "mg_eval_iid": _eval_iid, "mg_eval_iid_lpips": _eval_iid_lpips,
    "mg_tiny_conv3x3": _tiny_conv3x3, "mg_tiny_vae_encode": _tiny_vae_encode, "mg_tiny_vae_decode": _tiny_vae_decode,
    "mg_ensemble_depth": _ensemble_depth,
}
ASYNC_ROWS = [name for name in ROWS if name not in SYNCHRONISES]
NEIGHBOUR = {name: "mg_depth_focus" for name in ROWS}
NEIGHBOUR["mg_depth_focus"] = "mg_depth_view"


# ---- the session: every call warmed and timed on the default stream, the delay calibrated once ---------------------------------------

def _lib(f16):
    assert torch.cuda.is_available()
    return L.init(0, f16)


@functools.lru_cache(maxsize=None)
def _alone(name, f16, variant):
    """the call run alone on the null stream -> (its result, the host seconds of the warmed-up call); the first run loads the module"""
    call = ROWS[name](_lib(f16), f16, variant)
    G.run_plain(call, None)
    got, seconds = G.run_plain(call, None)
    if call.check is not None:
        call.check(got)
    return got, seconds


@functools.lru_cache(maxsize=None)
def _delay():
    slowest = max((_alone(name, f16, variant)[1], name) for name in ROWS for f16 in (False, True) for variant in (0, 1))
    delay = G.calibrate(slowest[0], _streams()[0])
    print(f"[stream gate] the delay: {delay.kind} x {delay.units} = {delay.ms:.1f} ms on a side stream; the slowest warmed-up host call: "
          f"{slowest[1]} at {delay.slowest_host_ms:.3f} ms")
    assert delay.ms >= G.MIN_DELAY_MS and delay.ms >= G.HOST_FACTOR * delay.slowest_host_ms
    return delay


@functools.lru_cache(maxsize=None)
def _streams():
    return torch.cuda.Stream(), torch.cuda.Stream()


def test_the_delay_outlasts_every_call():
    """warms every call of the table on the default stream (module load and mg_kernel_max_lds stay outside the gate), holds the
    bit-equal families to their restatements, and calibrates the delay; the figures are printed (docs/history/stream_fidelity.md)"""
    delay = _delay()
    assert delay.ms >= G.MIN_DELAY_MS and delay.ms >= G.HOST_FACTOR * delay.slowest_host_ms


# ---- parts 1 and 2 ---------------------------------------------------------------------------------------------------------------

@LIBS
@pytest.mark.parametrize("name", list(ROWS))
def test_all_work_goes_to_the_given_stream_and_the_call_does_not_wait(name, f16):
    delay, (s, _) = _delay(), _streams()
    alone, _ = _alone(name, f16, 0)
    call = ROWS[name](_lib(f16), f16, 0)
    (gated,), (busy,) = G.run_gated([call], [s], delay)
    on_side, _ = G.run_plain(call, s)
    assert G.same(on_side, alone), f"{name}: alone on a side stream differs from alone on the null stream"
    assert G.same(gated, alone), f"{name}: behind the gate differs from the call alone: " \
                                 f"{[key for key in alone if alone[key].tobytes() != gated[key].tobytes()]}"
    if call.check is not None:
        call.check(gated)
    if name not in SYNCHRONISES:
        assert busy, f"{name}: the stream had drained when the call returned - the call waited for it"


# ---- part 3 ----------------------------------------------------------------------------------------------------------------------

@LIBS
@pytest.mark.parametrize("name", ASYNC_ROWS)
def test_two_scenes_of_one_entry_point_in_flight(name, f16):
    delay, streams = _delay(), _streams()
    calls = [ROWS[name](_lib(f16), f16, variant) for variant in (0, 1)]
    got, busy = G.run_gated(calls, streams, delay)
    assert all(busy), f"{name}: a gate had opened before both calls were made"
    for variant in (0, 1):
        assert G.same(got[variant], _alone(name, f16, variant)[0]), f"{name}: scene {variant} differs with another scene in flight"


@LIBS
@pytest.mark.parametrize("name", ASYNC_ROWS)
def test_beside_the_neighbour_in_flight(name, f16):
    delay, streams = _delay(), _streams()
    other = NEIGHBOUR[name]
    calls = [ROWS[name](_lib(f16), f16, 0), ROWS[other](_lib(f16), f16, 1)]
    got, busy = G.run_gated(calls, streams, delay)
    assert all(busy), f"{name}: a gate had opened before both calls were made"
    assert G.same(got[0], _alone(name, f16, 0)[0]), f"{name} differs with {other} in flight"
    assert G.same(got[1], _alone(other, f16, 1)[0]), f"{other} differs with {name} in flight"


# ---- part 4 ----------------------------------------------------------------------------------------------------------------------

def _refused(lib, which):
    """one refusal of the existing refusal tests -> rc; a refusal returns before the first device call.  The message is read later"""
    if which == 0:   # max_radius = 33
        p = 0x10000
        rc = lib.mg_depth_focus(p, p, 1, None, None, 8, 8, 0.0, float("inf"), 0, 1.0, 33, -1, -1, 2.0, p, p, None, p, p, 1 << 20, None)
    else:            # a strength above 1
        rc = lib.mg_latent_carry(0x10000, 0x10000, 16, 1.25, None)
    return rc


@LIBS
def test_two_host_threads(f16):
    _delay()
    lib, streams = _lib(f16), _streams()
    want = {(name, variant): _alone(name, f16, variant)[0] for name in ASYNC_ROWS for variant in (0, 1)}
    calls = {key: ROWS[key[0]](lib, f16, key[1]) for key in want}
    torch.cuda.synchronize()
    failures, messages, start, refused = [], {}, threading.Barrier(2), threading.Barrier(2)

    def work(t):
        try:
            assert lib.mg_init(0) == 0   # (binds this thread to the device)
            start.wait()
            for name in ASYNC_ROWS if t == 0 else reversed(ASYNC_ROWS):
                got, _ = G.run_plain(calls[name, t], streams[t])
                if not G.same(got, want[name, t]):
                    failures.append(f"{name} on thread {t} differs from the call alone")
            # both threads are refused, meet, and only then read: a buffer shared by the threads would hold one message for both
            rc = _refused(lib, t)
            refused.wait()
            messages[t] = (rc, lib.mg_last_error().decode())
        except BaseException as e:   # noqa: BLE001  (an assertion in a thread must fail the test)
            failures.append(f"thread {t}: {e!r}")
            start.abort()
            refused.abort()

    threads = [threading.Thread(target=work, args=(t,)) for t in (0, 1)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not failures, failures
    assert messages[0][0] != 0 and messages[0][1].startswith("mg_depth_focus:") and "max_radius" in messages[0][1], messages[0]
    assert messages[1][0] != 0 and messages[1][1].startswith("mg_latent_carry:"), messages[1]


# ---- the existing runners, given a side stream ------------------------------------------------------------------------------------------

@LIBS
def test_the_existing_runners_on_a_side_stream(f16):
    """the raw runners of the focus, view, points, mesh and align tests take a stream now (this test is their only caller that passes
    one): on a side stream the first four give the restatement's bytes, the fit the bits of the table's row alone"""
    from tests import focus_scenes, test_gpu_align, test_gpu_focus, test_gpu_mesh, test_gpu_points, test_gpu_view, view_scenes
    lib, (s, _) = _lib(f16), _streams()
    c = _pick(focus_scenes.cases(), 0, lambda c: c.shape == (17, 65) and c.max_radius == 8 and c.gain > 0)
    test_gpu_focus._equal(test_gpu_focus._focus(lib, c, stream=s.cuda_stream), c.want, c.name)
    c = _pick(view_scenes.cases(), 0, lambda c: c.shape == (17, 33) and c.pose_name == "stereo_right")
    got = test_gpu_view._view(lib, c, stream=s.cuda_stream)
    assert got["count"].tolist() == list(c.want.count) and np.array_equal(got["rgb"], c.want.rgb) and np.array_equal(got["valid"], c.want.valid)
    name, d, colors, mask, K, opt, want = _masked_with_coef(test_gpu_points._cases(), 0)
    got = test_gpu_points._points(lib, d, colors, mask, K, opt, d.size + 3, stream=s.cuda_stream)
    assert got["count"].tolist() == list(want.count) and test_gpu_points._same_bits(got["xyz"][:want.count[1]], want.xyz)
    _, valid = test_gpu_points._normals(lib, d, mask, K, opt, stream=s.cuda_stream)
    assert np.array_equal(valid, want.valid)
    name, d, colors, mask, K, opt, want = _masked_with_coef(test_gpu_mesh._cases(), 0)
    got = test_gpu_mesh._mesh(lib, d, colors, mask, K, opt, d.size + 3, 2 * (d.shape[0] - 1) * (d.shape[1] - 1) + 3, stream=s.cuda_stream)
    assert got["count"].tolist() == list(want.count) and np.array_equal(got["faces"][:want.count[3]], want.faces)
    d, ref, mask = test_gpu_align._scene(test_gpu_align.CHUNK + 1, True, True)
    coef, flag = torch.empty(2, dtype=torch.float64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.mg_depth_align_workspace_bytes(d.size), dtype=torch.uint8, device="cuda")
    test_gpu_align._fit(lib, *(test_gpu_align._dev(a) for a in (d, ref, mask)), 1, 4, "ls", coef, flag, ws, stream=s.cuda_stream)
    torch.cuda.synchronize()
    alone = _alone("mg_depth_align_fit", f16, 0)[0]
    assert coef.cpu().numpy().tobytes() == alone["coef"].tobytes() and flag.cpu().numpy().tobytes() == alone["flag"].tobytes()
