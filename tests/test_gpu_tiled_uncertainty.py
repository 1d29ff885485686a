"""The stitched uncertainty of ``predict_tiled`` on a real MI355X, for depth and normals: with ``ensemble_size`` > 1 and
``ensemble_kwargs=dict(output_uncertainty=True)`` the output's ``uncertainty`` equals the composition the docstring documents, written
out by hand through the public calls - the tiles' outputs from ``map_images``, ``tiles.fit`` for the depth's scales, ``tiles.blend``
with ``(s_i, 0)`` (depth) or without coefficients (normals).

Every bound is an equality (``np.array_equal``): both sides run the same programs and kernels on the same bytes.  The geometry is that
of tests/test_gpu_tiles.py - picture 128 x 256, tiles (64, 128), overlap (16, 32), guide_res 128, the tiny synthetic models, two steps."""
import functools

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
SEED = (1 << 63) + 31
PICTURE_HW, TILE, OVERLAP, GUIDE_RES, E = (128, 256), (64, 128), (16, 32), 128, 3
KINDS = pytest.mark.parametrize("kind", ["depth", "normals"])
UNC = dict(output_uncertainty=True)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind):
    """``_tiny_pipe`` of tests/test_gpu_predict_out_c_host.py."""
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    return M.build_synthetic_pipeline(kind, TINY_UNET, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _pil(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _tiled(kind, **kw):
    """One ``predict_tiled`` of the test picture under the documented seeds; ``kw`` over the defaults of this module."""
    from marigold_amd import NativeNoise
    args = dict(tile_size=TILE, tile_overlap=OVERLAP, guide_res=GUIDE_RES, denoising_steps=2, ensemble_size=E, in_flight=1, ensemble_kwargs=UNC)
    args.update(kw)
    return _tiny_pipe(kind).predict_tiled(_pil(*PICTURE_HW), generator=NativeNoise(SEED), **args)


@functools.lru_cache(maxsize=None)
def _with_uncertainty(kind):
    """The output under test (computed once per kind, shared, never modified)."""
    return _tiled(kind)


def _map(kind, out):
    return out.depth_np if kind == "depth" else out.normals_np


def _picture(kind, out):
    return np.array(out.depth_colored if kind == "depth" else out.normals_img)


def _by_hand(kind):
    """The uncertainty ``predict_tiled`` documents, step by step through the public calls -> [128, 256] fp32"""
    from marigold_amd import NativeNoise, tiles as T
    from marigold_amd.util.image_util import pil_to_tensor
    pipe, pil = _tiny_pipe(kind), _pil(*PICTURE_HW)
    plan = T.plan(PICTURE_HW, TILE, OVERLAP)
    n, (th, tw) = len(plan.origins), plan.tile_hw
    kw = dict(denoising_steps=2, ensemble_size=E, ensemble_kwargs=UNC)
    rgb = pil_to_tensor(pil).unsqueeze(0).cuda()
    crops = [rgb[..., y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0 in plan.origins]
    outs = list(pipe.map_images(crops, in_flight=1, generators=[NativeNoise((SEED + 1 + i) % (1 << 64)) for i in range(n)],
                                images_per_program=8, processing_res=0, match_input_res=False, **kw))
    u = torch.from_numpy(np.stack([o.uncertainty for o in outs])).cuda()
    assert u.shape == (n, th, tw) and u.dtype == torch.float32
    if kind == "normals":
        return T.blend(u, plan.origins, PICTURE_HW, OVERLAP).cpu().numpy()
    guide = pipe(pil, processing_res=GUIDE_RES, match_input_res=False, generator=NativeNoise(SEED), **kw).depth_np
    preds = torch.from_numpy(np.stack([o.depth_np for o in outs])).cuda()
    coef, _ = T.fit(preds, plan.origins, torch.from_numpy(guide).cuda(), PICTURE_HW)
    scales = coef.clone()
    scales[:, 1] = 0.0   # (s_i, 0): a tile's uncertainty is in units of its own depth, which the stitch scales by s_i
    return T.blend(u, plan.origins, PICTURE_HW, OVERLAP, coef=scales).cpu().numpy()


@KINDS
def test_uncertainty_is_the_documented_composition(kind):
    out = _with_uncertainty(kind)
    unc = out.uncertainty
    assert isinstance(unc, np.ndarray) and unc.shape == PICTURE_HW and unc.dtype == np.float32
    assert np.isfinite(unc).all() and float(unc.min()) >= 0.0 and float(unc.max()) > 0.0
    want = _by_hand(kind)
    assert np.array_equal(unc, want)


@KINDS
def test_the_switch_changes_nothing_else_and_off_means_none(kind):
    out = _with_uncertainty(kind)
    plain = _tiled(kind, ensemble_kwargs=None)
    assert plain.uncertainty is None
    assert np.array_equal(_map(kind, plain), _map(kind, out)) and np.array_equal(_picture(kind, plain), _picture(kind, out))
    if kind == "depth":
        assert plain.degenerate_tiles == out.degenerate_tiles and out.degenerate_tiles is not None
    assert _tiled(kind, ensemble_kwargs=dict(output_uncertainty=False)).uncertainty is None
    single = _tiled(kind, ensemble_size=1)   # one member: the pipelines return no uncertainty, switch or not
    assert single.uncertainty is None and _map(kind, single).shape[-2:] == PICTURE_HW


@KINDS
def test_a_second_run_and_two_programs_in_flight_give_the_same_bits(kind):
    out = _with_uncertainty(kind)
    for in_flight in (1, 2):
        again = _tiled(kind, in_flight=in_flight)
        assert np.array_equal(again.uncertainty, out.uncertainty), in_flight
        assert np.array_equal(_map(kind, again), _map(kind, out)) and np.array_equal(_picture(kind, again), _picture(kind, out)), in_flight


def test_the_uncertainty_stays_at_the_working_size():
    """Like ``__call__``'s it is never resampled: with ``tiled_res`` the map goes back to the input size, the uncertainty does not."""
    from marigold_amd import NativeNoise
    pipe = _tiny_pipe("normals")
    out = pipe.predict_tiled(_pil(96, 192), tile_size=TILE, tile_overlap=OVERLAP, tiled_res=256, denoising_steps=2, ensemble_size=2, in_flight=1,
                             ensemble_kwargs=UNC, generator=NativeNoise(SEED))
    assert out.normals_np.shape == (3, 96, 192) and out.uncertainty.shape == PICTURE_HW and np.isfinite(out.uncertainty).all()
