"""Tiled predictions on a real MI355X: the fit and blend kernels of csrc/tiles.hip against fp64 restatements, on both
operand libraries; an affine recovery through ``tiles.fit`` + ``tiles.blend``; ``predict_tiled`` of the depth and normals pipelines
against the composition it documents, written out by hand; the single-tile case; the refusals.

The bounds.

* FIT.  The restatement samples the guide with ``F.interpolate`` in double and solves every tile with ``numpy.linalg.lstsq``; the
  kernel samples and sums in fp64 too, so the only difference is the order of fp64 sums of fewer than 6e5 terms at 2^-53 each: (s, t)
  within 1e-9 relative to max(1, |value|).  Flags, the exact zeros of the fall-backs, the canaries and the bits of a second run: equality.
  One qualification: over a CONSTANT guide the exact slope of every tile is 0, and the sign of a rounding residue would decide the
  flag; the 1 x 1 guide therefore holds 0.5, a power of two, for which N Sdg = Sd Sg holds exactly in floating point (scaling by a
  power of two commutes with every rounding): the slope is exactly 0 and the tile is flagged by ``s <= 0``.

* BLEND.  Per pixel 32 * 2^-24 * max_i |s_i d_i + t_i| over the covering tiles, against an fp64 restatement that uses the same
  fp32-rounded (s, t).  Derivation: with u = 2^-24 and V = max_i |v_i|, every weight carries 2 roundings (the quotient of the ramp,
  the product wy wx), v_i = fma(s, d, t) one, and each of the at most 9 covering tiles adds one rounding to the running numerator
  (the fma) and one to the running denominator; all weights are positive, so nothing cancels in the denominator and the partial sums
  of the numerator are bounded by V sum w.  Relative to V that is 2 + 1 (a term) + 9 (numerator) + 2 + 9 (denominator, its own
  weights included) + 1 (the quotient) = 24 roundings to first order; 32 leaves room for the second-order terms and is not fitted to
  any measurement.  With ``normalize`` the same bound holds for the unnormalised vector - which the test reconstructs from the
  restatement - and the division by the length (three squares, two sums, a root, a quotient) adds 4 * 2^-24 on a unit vector, plus
  the propagated error of the vector relative to its length.

* The PIPELINE tests are equalities (``np.array_equal``): both sides run the same programs and kernels on the same inputs.

"Tile (8, 8) with O = 8": an overlap of 8 is more than half of an 8-pixel tile, so no plan has two such tiles side by side; the case
is run as what it can be - ONE 8 x 8 tile on an 8 x 8 canvas with O = 8, the smallest call there is - and the smallest overlapping
plan, tiles of 16 with O = 8 = T / 2, where the two ramps of a tile meet, is run beside it.

The models are the tiny synthetic ones of tests/test_gpu_predict_out_c_host.py, two steps."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

pytestmark = pytest.mark.gpu
SEED = (1 << 63) + 31
U = 2.0 ** -24
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {False: L.init(0), True: L.init(0, True)}


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


class _Guarded:
    """A device buffer of ``n`` elements between two canaries of PAD elements (PAD * itemsize is a multiple of 16)."""
    PAD = 16

    def __init__(self, n, dtype, canary):
        self.n, self.canary = n, canary
        self.buf = torch.full((n + 2 * self.PAD,), canary, dtype=dtype, device="cuda")
        self.t = self.buf[self.PAD:self.PAD + n]
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        h = self.buf.cpu()
        return bool((h[:self.PAD] == self.canary).all()) and bool((h[self.PAD + self.n:] == self.canary).all())


# ---- 1. the fit --------------------------------------------------------------------------------------------------------------------

TILE_SHAPES = ((8, 8), (8, 24), (64, 128), (72, 136))
GUIDES = ((1, 1), (5, 7), (64, 128))


def _axis_starts(T, single):
    """n = 1: one tile off the canvas corner; else three starts a quarter tile apart - all three tiles cover T / 2 ... - on a canvas
    rounded up to a multiple of 8"""
    if single:
        return [8], T + 16
    return [0, T // 4, T // 2], -(-(T // 2 + T) // 8) * 8


def _fit_case(th, tw, single, ghw, seed):
    """-> (tiles [n,th,tw] fp32, ystarts, xstarts, canvas, guide fp32, planted: tile index -> kind)"""
    g = torch.Generator().manual_seed(seed)
    ys, Hw = _axis_starts(th, single)
    xs, Ww = _axis_starts(tw, single)
    guide = torch.full(ghw, 0.5) if ghw == (1, 1) else torch.rand(ghw, generator=g)
    full = F.interpolate(guide.double()[None, None], (Hw, Ww), mode="bilinear", align_corners=False)[0, 0]
    tiles, planted = [], {}
    for i, (y0, x0) in enumerate((y, x) for y in ys for x in xs):
        crop = full[y0:y0 + th, x0:x0 + tw]
        s, t = 0.3 + 2.7 * float(torch.rand((), generator=g)), float(torch.rand((), generator=g)) * 2 - 1
        d = ((crop - t) / s + 0.05 * torch.randn(th, tw, generator=g, dtype=torch.float64)).float()
        kind = {1: "constant", 2: "negative", 3: "holes", 4: "empty"}.get(i)
        if kind == "constant":
            d = torch.full((th, tw), 0.375)
        elif kind == "negative":
            d = (-2.0 * crop + 0.25).float() + 0.01 * torch.randn(th, tw, generator=g)
        elif kind == "holes":
            flat = d.view(-1)
            for j, v in enumerate((float("nan"), float("inf"), float("-inf"), float("nan"))):
                flat[(j * 13 + 5) % flat.numel()] = v
        elif kind == "empty":
            d = torch.full((th, tw), float("nan"))
            d[0, 0], d[-1, -1] = float("inf"), float("-inf")
        if kind:
            planted[i] = kind
        tiles.append(d)
    return torch.stack(tiles), ys, xs, (Hw, Ww), guide, planted, full


def _fit_restated(tiles, ys, xs, full):
    """fp64: ``numpy.linalg.lstsq`` per tile over the pixels where the tile and the sampled guide are finite; the degenerate rule of
    include/marigold_hip.h -> (coef [n,2], flags [n])"""
    n, th, tw = tiles.shape
    coef, flags = np.zeros((n, 2)), np.zeros(n, np.int32)
    for i, (y0, x0) in enumerate((y, x) for y in ys for x in xs):
        d = tiles[i].double().numpy().ravel()
        G = full[y0:y0 + th, x0:x0 + tw].numpy().ravel()
        ok = np.isfinite(d) & np.isfinite(G)
        d, G = d[ok], G[ok]
        N = d.size
        degenerate = N < 2 or N * np.sum(d * d) - np.sum(d) ** 2 <= 1e-12 * N * N
        if not degenerate:
            (s, t), *_ = np.linalg.lstsq(np.stack([d, np.ones(N)], axis=1), G, rcond=None)
            degenerate = s <= 1e-12   # (a slope that is 0 up to the solver's rounding: the constant guide, see the module docstring)
        if degenerate:
            s, t = 0.0, (G.mean() if N else 0.0)
        coef[i], flags[i] = (s, t), int(degenerate)
    return coef, flags


def _run_fit(lib, tiles, ys, xs, canvas, guide):
    from marigold_amd import _lib as L, ops as O
    n, th, tw = tiles.shape
    need = lib.mg_tiles_workspace_bytes(n, th, tw)
    assert need == n * -(-th * tw // 4096) * 40
    d_tiles, d_guide = tiles.cuda().contiguous(), guide.cuda().contiguous()
    coef, flags, ws = _Guarded(2 * n, torch.float64, -7.25), _Guarded(n, torch.int32, -77), _Guarded(need // 8, torch.float64, -9.5)
    L.check(lib.mg_tile_fit(d_tiles.data_ptr(), th, tw, _ints(ys), len(ys), _ints(xs), len(xs), canvas[0], canvas[1], d_guide.data_ptr(),
                            guide.shape[0], guide.shape[1], coef.t.data_ptr(), flags.t.data_ptr(), ws.t.data_ptr(), need,
                            O.current_stream_handle()), "mg_tile_fit", lib)
    torch.cuda.synchronize()
    assert coef.intact() and flags.intact() and ws.intact()
    assert torch.equal(d_tiles.cpu().view(torch.int32), tiles.view(torch.int32))   # the tiles are read only
    return coef.t.cpu().clone(), flags.t.cpu().clone()


@LIBS
def test_fit_matches_the_fp64_restatement(libs, f16):
    lib = libs[f16]
    worst = 0.0
    for k, (th, tw) in enumerate(TILE_SHAPES):
        for single in (True, False):
            for ghw in GUIDES:
                tiles, ys, xs, canvas, guide, planted, full = _fit_case(th, tw, single, ghw, seed=100 + 7 * k + len(ghw) * ghw[0] + int(single))
                where = f"tile {th}x{tw} n={tiles.shape[0]} guide {ghw}"
                want_c, want_f = _fit_restated(tiles, ys, xs, full)
                got_c, got_f = _run_fit(lib, tiles, ys, xs, canvas, guide)
                again_c, again_f = _run_fit(lib, tiles, ys, xs, canvas, guide)
                assert torch.equal(got_c.view(torch.int64), again_c.view(torch.int64)) and torch.equal(got_f, again_f), where   # same bits
                got_c, got_f = got_c.numpy().reshape(-1, 2), got_f.numpy()
                assert np.array_equal(got_f, want_f), (where, got_f, want_f)
                err = np.abs(got_c - want_c) / np.maximum(1.0, np.abs(want_c))
                print(f"[tile fit] {where}: max error {err.max():.3e}, flags {got_f.tolist()}")
                worst = max(worst, float(err.max()))
                assert err.max() <= 1e-9, (where, got_c, want_c)
                assert np.all(got_c[want_f == 1, 0] == 0.0), where                      # the fall-back's slope is an exact zero
                if ghw == (1, 1):
                    assert want_f.tolist() == [1] * len(want_f), where                   # a constant guide: every slope is exactly 0
                else:
                    for i, kind in planted.items():
                        assert want_f[i] == (kind != "holes"), (where, i, kind)
                    assert all(want_f[i] == 0 for i in range(len(want_f)) if i not in planted), where
                for i, kind in planted.items():
                    if kind == "empty":
                        assert got_c[i, 0] == 0.0 and got_c[i, 1] == 0.0, where         # no valid pixel: t = 0
    print(f"[tile fit] worst error {worst:.3e}")


# ---- 2. the blend ------------------------------------------------------------------------------------------------------------------

# (canvas, tile size, overlap): triple overlap along both axes (nine tiles over one pixel); one tile; 2 x 3 tiles, every one at a border;
# the smallest call; tiles of 16 with O = T / 2
BLEND_PLANS = (((120, 120), (64, 64), (16, 16)), ((64, 128), (128, 128), (32, 32)), ((96, 160), (64, 64), (16, 16)),
               ((8, 8), (8, 8), (8, 8)), ((24, 40), (16, 16), (8, 8)))


def _ramp(T, O, before, behind):
    u = np.arange(T, dtype=np.float64)
    lo = np.minimum(1.0, (u + 0.5) / O) if before else np.ones(T)
    hi = np.minimum(1.0, (T - u - 0.5) / O) if behind else np.ones(T)
    return np.minimum(lo, hi)


def _blend_restated(tiles, plan, canvas, overlap, coef):
    """fp64, with (s, t) rounded to fp32 first -> (blend [C,H,W], max_i |v_i| per pixel [H,W], number of covering tiles [H,W])"""
    n, C, th, tw = tiles.shape
    num, den = np.zeros((C,) + canvas), np.zeros(canvas)
    vmax, cover = np.zeros(canvas), np.zeros(canvas, np.int32)
    ny, nx = len(plan.ystarts), len(plan.xstarts)
    for i, (y0, x0) in enumerate(plan.origins):
        iy, ix = divmod(i, nx)
        w = np.outer(_ramp(th, overlap[0], iy > 0, iy < ny - 1), _ramp(tw, overlap[1], ix > 0, ix < nx - 1))
        v = tiles[i].double().numpy()
        if coef is not None:
            s, t = np.float32(coef[i, 0]), np.float32(coef[i, 1])
            v = float(s) * v + float(t)
        sl = (slice(y0, y0 + th), slice(x0, x0 + tw))
        num[(slice(None),) + sl] += w * v
        den[sl] += w
        vmax[sl] = np.maximum(vmax[sl], np.abs(v).max(axis=0))
        cover[sl] += 1
    assert den.min() > 0
    return num / den, vmax, cover


def _run_blend(lib, tiles, plan, canvas, overlap, coef, normalize):
    from marigold_amd import _lib as L, ops as O
    n, C, th, tw = tiles.shape
    d_tiles = tiles.cuda().contiguous()
    d_coef = None if coef is None else torch.from_numpy(coef).cuda()
    out = _Guarded(C * canvas[0] * canvas[1], torch.float32, -55.5)
    L.check(lib.mg_tile_blend(d_tiles.data_ptr(), C, th, tw, _ints(plan.ystarts), len(plan.ystarts), _ints(plan.xstarts), len(plan.xstarts),
                              canvas[0], canvas[1], overlap[0], overlap[1], None if d_coef is None else d_coef.data_ptr(), int(normalize),
                              out.t.data_ptr(), O.current_stream_handle()), "mg_tile_blend", lib)
    torch.cuda.synchronize()
    assert out.intact()                                                                  # nothing beyond the canvas is written
    return out.t.cpu().numpy().reshape((C,) + canvas).astype(np.float64)


@LIBS
def test_blend_matches_the_fp64_restatement(libs, f16):
    from marigold_amd import tiles as T
    lib = libs[f16]
    covers = set()
    for k, (canvas, tile, overlap) in enumerate(BLEND_PLANS):
        # (mg_tile_plan refuses O > T / 2 whatever the length: the lone 8 x 8 tile is written out)
        plan = T.TilePlan((0,), (0,), (8, 8), ((0, 0),)) if tile == (8, 8) else T.plan(canvas, tile, overlap)
        n, (th, tw) = len(plan.origins), plan.tile_hw
        g = torch.Generator().manual_seed(300 + k)
        where = f"canvas {canvas} tiles {n} x {th}x{tw} overlap {overlap}"
        # C = 1 with coefficients (a scale in [0.3, 3], a shift in [-1, 1], and a degenerate tile's s = 0)
        d = torch.rand(n, 1, th, tw, generator=g) * 4 - 1
        coef = np.stack([0.3 + 2.7 * torch.rand(n, generator=g, dtype=torch.float64).numpy(),
                         torch.rand(n, generator=g, dtype=torch.float64).numpy() * 2 - 1], axis=1)
        coef[n // 2, 0] = 0.0
        want, vmax, cover = _blend_restated(d, plan, canvas, overlap, coef)
        got = _run_blend(lib, d, plan, canvas, overlap, coef, False)
        ratio = np.abs(got - want)[0] / (32 * U * vmax)
        print(f"[tile blend] {where} C=1: worst error / bound {ratio.max():.3f}, up to {cover.max()} covering tiles")
        assert ratio.max() <= 1.0, where
        covers.add(int(cover.max()))
        # without coefficients the affine map is the identity
        want, vmax, _ = _blend_restated(d, plan, canvas, overlap, None)
        got = _run_blend(lib, d, plan, canvas, overlap, None, False)
        assert (np.abs(got - want)[0] / (32 * U * vmax)).max() <= 1.0, where
        # C = 3 with normalize: vectors around unit length, so that blends stay away from the 1e-6 floor
        v = torch.randn(n, 3, th, tw, generator=g)
        v = v / v.norm(dim=1, keepdim=True) + torch.tensor([0.0, 0.0, 2.0]).view(1, 3, 1, 1)
        want, vmax, _ = _blend_restated(v, plan, canvas, overlap, None)
        raw = _run_blend(lib, v, plan, canvas, overlap, None, False)
        assert (np.abs(raw - want).max(axis=0) / (32 * U * vmax)).max() <= 1.0, where
        length = np.sqrt((want ** 2).sum(axis=0))
        assert length.min() > 0.5
        got = _run_blend(lib, v, plan, canvas, overlap, None, True)
        # |v / |v| - v' / |v'|| <= 2 |v - v'| / |v| per component, to first order; then the division's own roundings
        bound = 2 * np.sqrt(3) * 32 * U * vmax / length + 4 * U
        ratio = np.abs(got - want / length).max(axis=0) / bound
        print(f"[tile blend] {where} C=3 normalize: worst error / bound {ratio.max():.3f}")
        assert ratio.max() <= 1.0, where
        assert np.abs(np.sqrt((got ** 2).sum(axis=0)) - 1).max() <= 4 * U, where
    assert covers == {1, 4, 9}   # the triple overlap met along both axes


@LIBS
def test_blend_propagates_non_finite_values_and_is_continuous_across_seams(libs, f16):
    from marigold_amd import tiles as T
    lib = libs[f16]
    canvas, overlap = (120, 120), (16, 16)
    plan = T.plan(canvas, (64, 64), overlap)
    d = torch.rand(9, 1, 64, 64, generator=torch.Generator().manual_seed(5))
    d[0, 0, 3, 5], d[4, 0, 10, 10], d[8, 0, 60, 60] = float("nan"), float("inf"), float("-inf")
    got = _run_blend(lib, d, plan, canvas, overlap, None, False)[0]
    assert np.isnan(got[3, 5]) and got[24 + 10, 24 + 10] == np.inf and got[56 + 60, 56 + 60] == -np.inf
    assert np.isfinite(got).sum() == got.size - 3
    # two tiles that are the constants 0 and 1, sharing 24 columns with ramps of 16: out = w_b / (w_a + w_b) along x.  A tile enters
    # with the weight 0.5 / O beside a weight of 1 - a step below 0.5 / O - and inside the overlap |d out / dx| = 1 / (O (w_a + w_b))
    # <= 2 / O, because one of two tiles that overlap by at least O weighs 0.5 or more: no step of the size of the tiles' difference
    plan = T.plan((64, 104), (64, 64), overlap)
    assert plan.xstarts == (0, 40) and plan.ystarts == (0,)
    c = torch.stack([torch.zeros(1, 64, 64), torch.ones(1, 64, 64)])
    got = _run_blend(lib, c, plan, (64, 104), overlap, None, False)[0]
    assert np.all(got[:, :40] == 0.0) and np.all(got[:, 64:] == 1.0) and np.all(got == got[:1])
    steps = np.diff(got[0])
    assert steps.min() >= 0.0 and steps.max() <= 2.0 / 16 + 1e-6 and 0 < got[0, 40] <= 0.5 / 16, (steps.max(), got[0, 40])


# ---- 3. affine recovery ------------------------------------------------------------------------------------------------------------

@LIBS
def test_fit_then_blend_recovers_a_map_from_affinely_distorted_crops(libs, f16):
    from marigold_amd import tiles as T
    lib = libs[f16]
    H, W = 128, 256
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing="ij")
    M = (0.5 + 0.3 * torch.sin(5 * xx + 2 * yy) * torch.cos(3 * yy) + 0.15 * xx * yy).float()     # smooth, inside [0.05, 1]
    plan = T.plan((H, W), (64, 128), (16, 32))
    n = len(plan.origins)
    assert n == 9
    g = torch.Generator().manual_seed(77)
    s = 0.3 + 2.7 * torch.rand(n, generator=g, dtype=torch.float64)
    t = torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1
    crops = torch.stack([(M[y0:y0 + 64, x0:x0 + 128].double() - t[i]) / s[i] for i, (y0, x0) in enumerate(plan.origins)]).float()
    coef, flags = T.fit(crops.cuda(), plan.origins, M.cuda(), (H, W), lib=lib)
    out = T.blend(crops.cuda(), plan.origins, (H, W), (16, 32), coef=coef, lib=lib)
    torch.cuda.synchronize()
    assert out.shape == (H, W) and flags.cpu().tolist() == [0] * n
    assert np.abs(coef.cpu().numpy() - np.stack([s.numpy(), t.numpy()], axis=1)).max() <= 1e-6   # (the crops are fp32: 6e-8 of noise each)
    err = np.abs(out.cpu().numpy().astype(np.float64) - M.double().numpy())
    bound = 32 * U * np.abs(M.numpy()) + 1e-6
    print(f"[tile recovery] worst error {err.max():.3e}, worst error / bound {(err / bound).max():.3f}")
    assert (err / bound).max() <= 1.0
    # the wrappers' own checks
    with pytest.raises(ValueError, match="grid"):
        T.fit(crops.cuda(), plan.origins[::-1], M.cuda(), (H, W), lib=lib)
    with pytest.raises(ValueError, match="8 origins for 9 tiles"):
        T.blend(crops.cuda(), plan.origins[:8], (H, W), (16, 32), lib=lib)
    with pytest.raises(ValueError, match="fp32 CUDA tensor"):
        T.blend(crops, plan.origins, (H, W), (16, 32), lib=lib)


# ---- 4. - 6. the pipelines ---------------------------------------------------------------------------------------------------------

PICTURE_HW, TILE, OVERLAP, GUIDE_RES = (128, 256), (64, 128), (16, 32), 128


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind):
    """``_tiny_pipe`` of tests/test_gpu_predict_out_c_host.py."""
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _pil(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _by_hand(pipe, kind, pil, E, tiles_per_program):
    """What ``predict_tiled`` documents, step by step, through the public calls -> (map, picture as an array, flagged tiles | None)"""
    from marigold_amd import NativeNoise, tiles as T
    from marigold_amd.util.image_util import pil_to_tensor
    plan = T.plan(PICTURE_HW, TILE, OVERLAP)
    n, (th, tw) = len(plan.origins), plan.tile_hw
    kw = dict(denoising_steps=2, ensemble_size=E)
    guide = None
    if kind == "depth":
        guide = pipe(pil, processing_res=GUIDE_RES, match_input_res=False, generator=NativeNoise(SEED), **kw).depth_np
        assert guide.shape == (64, 128)
    rgb = pil_to_tensor(pil).unsqueeze(0).cuda()
    crops = [rgb[..., y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0 in plan.origins]
    outs = list(pipe.map_images(crops, in_flight=1, generators=[NativeNoise((SEED + 1 + i) % (1 << 64)) for i in range(n)],
                                images_per_program=tiles_per_program, processing_res=0, match_input_res=False, **kw))
    assert len(outs) == n
    if kind == "depth":
        preds = torch.from_numpy(np.stack([o.depth_np for o in outs])).cuda()
        coef, flags = T.fit(preds, plan.origins, torch.from_numpy(guide).cuda(), PICTURE_HW)
        final = T.blend(preds, plan.origins, PICTURE_HW, OVERLAP, coef=coef)
        final = final.cpu().numpy().clip(0, 1)       # (the working size is the input's: no resize)
        return final, None, int(flags.sum().item())
    preds = torch.from_numpy(np.stack([o.normals_np for o in outs])).cuda()
    final = T.blend(preds, plan.origins, PICTURE_HW, OVERLAP, normalize=True)
    return final.cpu().numpy().clip(-1, 1), None, None


@pytest.mark.parametrize("kind,E", [("depth", 1), ("depth", 3), ("normals", 1)], ids=["depth-E1", "depth-E3", "normals-E1"])
def test_predict_tiled_is_the_documented_composition(kind, E):
    from marigold_amd import NativeNoise
    pipe, pil = _tiny_pipe(kind), _pil(*PICTURE_HW)
    tiled = dict(tile_size=TILE, tile_overlap=OVERLAP, guide_res=GUIDE_RES, denoising_steps=2, ensemble_size=E)
    out = pipe.predict_tiled(pil, in_flight=1, generator=NativeNoise(SEED), **tiled)
    got = out.depth_np if kind == "depth" else out.normals_np
    assert got.shape == ((128, 256) if kind == "depth" else (3, 128, 256)) and got.dtype == np.float32 and np.isfinite(got).all()
    assert out.uncertainty is None
    want, _, flagged = _by_hand(pipe, kind, pil, E, tiles_per_program=8)    # the default: min(9 tiles, 8)
    assert np.array_equal(got, want)
    if kind == "depth":
        assert out.degenerate_tiles == flagged and out.depth_colored.size == (256, 128)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0 and float(got.std()) > 0
    else:
        assert np.abs(np.sqrt((got.astype(np.float64) ** 2).sum(axis=0)) - 1).max() <= 1e-6 and out.normals_img.size == (256, 128)
    picture = np.array(out.depth_colored if kind == "depth" else out.normals_img)
    # two programs in flight, and a second call: the same bits, pictures included
    for in_flight in (2, 1):
        again = pipe.predict_tiled(pil, in_flight=in_flight, generator=NativeNoise(SEED), **tiled)
        assert np.array_equal(again.depth_np if kind == "depth" else again.normals_np, got), in_flight
        assert np.array_equal(np.array(again.depth_colored if kind == "depth" else again.normals_img), picture), in_flight
    if E > 1:
        return
    # another number of tiles per program is the composition with that number
    out3 = pipe.predict_tiled(pil, in_flight=1, tiles_per_program=3, generator=NativeNoise(SEED), **tiled)
    want3, _, _ = _by_hand(pipe, kind, pil, E, tiles_per_program=3)
    assert np.array_equal(out3.depth_np if kind == "depth" else out3.normals_np, want3)
    # explicit tile generators take the place of the documented seeds
    gens = [NativeNoise((SEED + 1 + i) % (1 << 64)) for i in range(9)]
    same = pipe.predict_tiled(pil, in_flight=1, generator=NativeNoise(SEED), tile_generators=gens, **tiled)
    assert np.array_equal(same.depth_np if kind == "depth" else same.normals_np, got)


@pytest.mark.parametrize("kind", ["depth", "normals"])
def test_a_plan_of_one_tile_is_the_plain_call(kind):
    from marigold_amd import NativeNoise
    pipe, pil = _tiny_pipe(kind), _pil(64, 128)
    out = pipe.predict_tiled(pil, tile_size=128, tile_overlap=32, generator=NativeNoise(SEED), denoising_steps=2)
    want = pipe(pil, processing_res=0, generator=NativeNoise(SEED), denoising_steps=2)
    if kind == "depth":
        assert np.array_equal(out.depth_np, want.depth_np) and np.array_equal(np.array(out.depth_colored), np.array(want.depth_colored))
        assert out.degenerate_tiles is None and out.depth_np.shape == (64, 128)
    else:
        assert np.array_equal(out.normals_np, want.normals_np) and np.array_equal(np.array(out.normals_img), np.array(want.normals_img))


def test_predict_tiled_refusals():
    from marigold_amd import SequenceState
    pipe, pil = _tiny_pipe("depth"), _pil(*PICTURE_HW)
    tiled = dict(tile_size=TILE, tile_overlap=OVERLAP)
    with pytest.raises(ValueError, match="predict_tiled: init_latents cannot be combined with tiles"):
        pipe.predict_tiled(pil, init_latents=torch.zeros(1, 4, 8, 16), **tiled)
    with pytest.raises(ValueError, match="predict_tiled: sequence cannot be combined with tiles"):
        pipe.predict_tiled(pil, sequence=SequenceState(), **tiled)
    with pytest.raises(ValueError, match="predict_tiled: images_per_program cannot be combined with tiles"):
        pipe.predict_tiled(pil, images_per_program=2, **tiled)
    pipe.enable_member_parallel()
    try:
        with pytest.raises(ValueError, match="predict_tiled is not available on a member-parallel pipeline"):
            pipe.predict_tiled(pil, **tiled)
    finally:
        pipe._member_parallel = False
    with pytest.raises(ValueError, match="predict_tiled: the intrinsic-image pipeline is not supported"):
        _tiny_pipe("iid").predict_tiled(pil, **tiled)
