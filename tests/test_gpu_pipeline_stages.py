"""The lone call is the composition of its public stages, on a real MI355X: ``pipe(image, init_latents=...)`` of the depth, normals
and intrinsic-image pipelines equals - ``np.array_equal``, uncertainty included - ``_preprocess``, ``single_infer`` over the E members,
the ensembling function of marigold_amd.ensemble for E > 1, ``util.image_util.resize`` to the input size when it is matched, the
read-back and the clip, written out here.  Every other path (lanes, groups, sequences, tiles) is tied to the lone call by its own tests.

Both sides run the same programs and kernels on the same inputs, so the bound is equality.  The tiny synthetic models, a 64 x 128
picture processed at 48 (24 x 48: the resize back really resamples), two steps, fixed initial latents."""
import dataclasses
import functools

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
HW, RES, STEPS = (64, 128), 48, 2


@functools.lru_cache(maxsize=None)
def _pipe(kind):
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    assert torch.cuda.is_available()
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, default_denoising_steps=STEPS, default_processing_resolution=0).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _pil():
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(*HW, seed=5)[0].permute(1, 2, 0).numpy())


def _latents(pipe, E, hw):
    from marigold_amd import synthetic as syn
    h, w = pipe._latent_hw(hw)
    return torch.cat([syn.synthetic_latents(E, h, w, seed=2024 + j) for j in range(pipe._target_latent_channels // 4)], dim=1)


def _by_hand(pipe, kind, E, match_input_res, ensemble_kwargs):
    """-> (prediction, uncertainty | None) as host arrays"""
    from marigold_amd import ensemble as ens
    from marigold_amd.util.image_util import get_tv_resample_method, resize
    resample = get_tv_resample_method("bilinear")
    rgb, input_size = pipe._preprocess(_pil(), RES, resample)
    assert tuple(input_size) == (1, 3) + HW and tuple(rgb.shape[-2:]) == (24, 48)
    preds = pipe.single_infer(rgb.expand(E, -1, -1, -1), STEPS, None, False, _latents(pipe, E, rgb.shape[-2:]))
    uncert = None
    if E > 1:
        if kind == "depth":
            pred, uncert = ens.ensemble_depth(preds, scale_invariant=pipe.scale_invariant, shift_invariant=pipe.shift_invariant,
                                              **ensemble_kwargs)
        else:
            pred, uncert = (ens.ensemble_normals if kind == "normals" else ens.ensemble_iid)(preds, **ensemble_kwargs)
    else:
        pred = preds
    if match_input_res:
        pred = resize(pred, HW, interpolation=resample, antialias=True)
    pred = pred.squeeze().cpu().numpy()
    if kind != "iid":
        pred = pred.clip(*((0, 1) if kind == "depth" else (-1, 1)))
    return pred, None if uncert is None else uncert.squeeze().cpu().numpy()


@pytest.mark.parametrize("match_input_res", [True, False], ids=["input-size", "processed-size"])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("kind", ["depth", "normals", "iid"])
def test_the_lone_call_is_the_composition_of_its_stages(kind, E, match_input_res):
    pipe = _pipe(kind)
    ensemble_kwargs = dict(output_uncertainty=True)
    with torch.no_grad():
        want, want_unc = _by_hand(pipe, kind, E, match_input_res, ensemble_kwargs)
    out = pipe(_pil(), denoising_steps=STEPS, ensemble_size=E, processing_res=RES, match_input_res=match_input_res,
               ensemble_kwargs=ensemble_kwargs, init_latents=_latents(pipe, E, (24, 48)))
    hw = HW if match_input_res else (24, 48)
    if kind == "iid":   # the entries are the 3-channel slices of the prediction, target by target
        got = np.concatenate([e.array for e in out])
        got_unc = None if E == 1 else np.concatenate([e.uncertainty for e in out])
        assert all((e.uncertainty is None) == (E == 1) for e in out)
    else:
        got, got_unc = (out.depth_np, out.uncertainty) if kind == "depth" else (out.normals_np, out.uncertainty)
    assert got.shape == want.shape == ((hw if kind == "depth" else (pipe._pred_channels,) + hw)) and got.dtype == np.float32
    assert np.isfinite(got).all() and float(got.std()) > 0
    assert np.array_equal(got, want)
    assert (got_unc is None) == (E == 1) == (want_unc is None)
    if E > 1:
        assert got_unc.shape == want_unc.shape and np.array_equal(got_unc, want_unc)
