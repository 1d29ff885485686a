"""The intrinsic-image output stage and one-pass validation on a real MI355X: ``iid_visualization_device`` (MG_OP_IID_VIS,
csrc/resize.hip) against the numpy code it replaces on the GPU path (``MarigoldIIDOutput.fill_entry`` run on the CPU tensor),
``MarigoldIIDPipeline.fill_outputs`` against that same numpy code on the same device prediction, and ``validate_iid_main`` against
``infer_main("iid")`` followed by ``eval_main("iid")``.

Bounds.
* A target that is not in linear space takes no transcendental: ``x * 255`` in fp32 and the truncation are exact operations, so its
  picture is bit for bit numpy's.
* A linear target goes through ``powf`` (and an IEEE division when it is up to scale - the same bits as numpy's).  The device's
  ``powf`` and numpy's float32 power may round a result differently by an ulp, which moves a byte only when ``255 x`` lies within
  that ulp of an integer: every differing byte differs by exactly 1, and the share of differing bytes is at most 1e-4 per target.
  numpy's own fp32 path disagrees with an fp64 restatement on 1.7e-6 to 4.0e-6 of the bytes of these value sets at
  3 x 768 x 768 (none on the 1 / 256 grid), so the reference itself sits 25 x inside the cap.
* Out-of-range values: ``astype(uint8)`` keeps the low 8 bits of the truncated int32, and NaN / +-inf / |255 x| >= 2^31 give 0 (what
  cvttss2si leaves in the low byte).  The expected picture is numpy's own on the machine the test runs on; the test first checks
  that this numpy follows the rule on the classes it feeds (negative, above 255, NaN, +inf) - on x86-64 it does, no class is
  restricted.  There a byte that differs by 1 may do so across the wrap (255 <-> 0), so "by exactly 1" is taken modulo 256.
* The scores of ``validate_iid_main`` against ``eval_main``'s: the bounds of tests/test_gpu_eval_iid.py section 8 for the same row -
  PSNR rtol 1e-5 and SSIM ``SSIM_ATOL`` for a target scored as stored, 4 x the movement of the host score under +-2 ulp of its
  gamma'd inputs (``_movement_under_2ulp``, computed on this test's own inputs) for a target that takes a gamma.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch
import yaml

from oracle.make_eval_golden import write_synthetic_datasets
from tests.test_gpu_eval_iid import SSIM_ATOL, _movement_under_2ulp

pytestmark = pytest.mark.gpu

SHARE_CAP = 1e-4
COMBOS = [(False, False), (False, True), (True, False), (True, True)]   # (linear, up_to_scale)
SHAPES = [(1, 11, 13), (3, 33, 65), (2, 128, 96), (3, 768, 768)]
VALUE_SETS = ("uniform", "dark", "grid", "zero", "last_pixel_max")


@pytest.fixture(scope="module")
def IU():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    from marigold_amd.util import image_util
    L.init(0)
    return image_util


def _props(flags):
    names = [f"t{k}" for k in range(len(flags))]
    props = {"target_names": names}
    for name, (linear, up_to_scale) in zip(names, flags):
        props[name] = {"prediction_space": "linear" if linear else "srgb", "up_to_scale": up_to_scale}
    return props


def _host_pictures(pred, flags):
    """``fill_entry`` on the CPU tensor [n,3,H,W] -> uint8 [n,H,W,3]."""
    from marigold_amd.pipeline import MarigoldIIDOutput
    props = _props(flags)
    out = MarigoldIIDOutput(props["target_names"])
    with np.errstate(all="ignore"):   # negative bases, NaN casts: the values numpy returns are the reference, its warnings are not
        for k, name in enumerate(props["target_names"]):
            out.fill_entry(name, pred[k][None], None, props)
    return np.stack([np.asarray(out[name].image) for name in props["target_names"]])


def _check(tag, got, want, flags, wrap=False):
    """Non-linear targets bit for bit; linear targets: every differing byte by exactly 1, at most SHARE_CAP of them."""
    assert got.dtype == np.uint8 and got.shape == want.shape
    for k, (linear, up_to_scale) in enumerate(flags):
        d = np.abs(got[k].astype(np.int32) - want[k].astype(np.int32))
        if wrap:
            d = np.minimum(d, 256 - d)
        share = float((d != 0).mean())
        print(f"[parity] iid picture {tag} target {k} linear={linear} up_to_scale={up_to_scale}: {int((d != 0).sum())} of {d.size} bytes "
              f"differ (share {share:.2e}, cap {SHARE_CAP if linear else 0:.0e}), max difference {int(d.max())}")
        if not linear:
            assert np.array_equal(got[k], want[k]), (tag, k)
        else:
            assert d.max() <= 1 and share <= SHARE_CAP, (tag, k, int(d.max()), share)


def _values(kind, shape, seed):
    n, h, w = shape
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 3, h, w, generator=g)
    if kind == "uniform":
        return u
    if kind == "dark":
        return u ** 4
    if kind == "grid":
        return torch.randint(0, 257, (n, 3, h, w), generator=g).float() / 256.0
    if kind == "zero":      # the 1e-6 floor of the maximum
        return torch.zeros(n, 3, h, w)
    x = u * 0.5             # the maximum is a single value in the last element of every target
    x[:, -1, -1, -1] = 0.9
    return x


# ---- 1. the kernel against the host function ----------------------------------------------------------------------------


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pictures_match_fill_entry(IU, shape):
    n = shape[0]
    for v, kind in enumerate(VALUE_SETS):
        pred = _values(kind, shape, 100 * shape[1] + v)
        dev = pred.cuda()
        for r in range(4):   # every target takes each of the four flag combinations, mixed within one call
            flags = [COMBOS[(k + r) % 4] for k in range(n)]
            got = IU.iid_visualization_device(dev, [f[0] for f in flags], [f[1] for f in flags])
            assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (n, shape[1], shape[2], 3) and got.is_contiguous()
            _check(f"{shape} {kind} rotation {r}", got.cpu().numpy(), _host_pictures(pred, flags), flags)
    # a lone [3,H,W] target, and a view that starts off a 16-byte boundary (the one-pixel-per-lane path at a size the wide one takes)
    one = IU.iid_visualization_device(dev[0], [True], [True])
    assert tuple(one.shape) == (1, shape[1], shape[2], 3)
    flat = torch.empty(pred.numel() + 1, device="cuda")
    flat[1:] = dev.flatten()
    off = flat[1:].view_as(dev)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    flags = [COMBOS[3 - k % 4] for k in range(n)]
    a, b = (IU.iid_visualization_device(t, [f[0] for f in flags], [f[1] for f in flags]) for t in (dev, off))
    assert torch.equal(a, b) and torch.equal(a[0], one[0])


# ---- 2. out-of-range and non-finite inputs ------------------------------------------------------------------------------


def test_numpy_here_keeps_the_low_8_bits():
    """The rule section 2 of the file's docstring relies on, on this machine's numpy (a GPU is not involved)."""
    x = np.array([-0.5, -0.004, 1.5, 1.0039, np.nan, np.inf, 1.0, 0.999999], np.float32)
    with np.errstate(all="ignore"):
        got = (np.tile(x, 1000) * 255).astype(np.uint8)[-x.size:]   # (a long array: the loop numpy runs over an image)
        v = x * np.float32(255)
    want = np.where(np.abs(v) < 2147483648.0, np.trunc(np.where(np.isfinite(v), v, 0)), 0).astype(np.int64) & 0xff
    assert np.array_equal(got, want.astype(np.uint8)), (got, want)


@pytest.mark.parametrize("special", [None, float("nan"), float("inf")], ids=["overshoot", "nan", "inf"])
def test_out_of_range_and_non_finite(IU, special):
    shape = (4, 33, 65)   # the four flag combinations at once: plain, linear and up-to-scale targets
    g = torch.Generator().manual_seed(7)
    pred = torch.rand(shape[0], 3, shape[1], shape[2], generator=g) * 2.0 - 0.5   # [-0.5, 1.5]: bicubic overshoot
    if special is not None:
        pred[:, 1, 17, 31] = special   # one in every target
    want = _host_pictures(pred, COMBOS)
    got = IU.iid_visualization_device(pred.cuda(), [f[0] for f in COMBOS], [f[1] for f in COMBOS]).cpu().numpy()
    _check(f"[-0.5, 1.5] with {special}", got, want, COMBOS, wrap=True)
    assert (want[0] > 200).any() and (want[0, pred[0].permute(1, 2, 0).numpy() < -0.01] > 100).all()   # negative values wrap, they are not clipped
    assert (want[2][(pred[2] < 0).permute(1, 2, 0).numpy()] == 0).all()                                  # a negative base: NaN -> 0
    if special is not None:
        assert got[0, 17, 31, 1] == 0 and got[2, 17, 31, 1] == 0     # NaN -> 0; inf * 255 -> 0
        assert not got[3].any() and not want[3].any()                # an up-to-scale target with a NaN or an inf maximum: all 0
        assert got[2].any() and got[0].any()


# ---- 3. bit reproducibility ----------------------------------------------------------------------------------------------


def test_twenty_calls_the_same_bytes_and_fp16_library(IU):
    from marigold_amd import _lib as L, ops as O
    dev = _values("dark", (3, 768, 768), 31).cuda()
    first = IU.iid_visualization_device(dev, [True] * 3, [True] * 3)
    assert first.any()
    for _ in range(19):
        assert torch.equal(IU.iid_visualization_device(dev, [True] * 3, [True] * 3), first)
    lib16 = L.init(0, True)
    out = torch.full_like(first, 7)
    ws = torch.full((3, L.IID_VIS_PARTS), float("nan"), device="cuda")
    O.launch(O.iid_vis(dev, out, ws, n=3, H=768, W=768, linear=[True] * 3, up_to_scale=[True] * 3), lib=lib16)
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    parts = ws[:, :L.IID_VIS_PARTS].cpu()
    assert torch.equal(parts.max(dim=1).values, dev.cpu().flatten(1).max(dim=1).values)   # every slot of the table is written


# ---- 4. the pipeline -----------------------------------------------------------------------------------------------------


def _tiny_iid(props):
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    n = len(props["target_names"])
    ucfg = dataclasses.replace(TINY_UNET, in_channels=4 + 4 * n, out_channels=4 * n)
    return M.build_synthetic_pipeline("iid", ucfg, TINY_VAE, target_properties=props, default_denoising_steps=2,
                                      default_processing_resolution=0).to("cuda:0")


@pytest.fixture(scope="module")
def pipe2():
    """The two-modality model of test_iid_pipeline_vs_oracle, one target linear and up to scale."""
    assert torch.cuda.is_available()
    return _tiny_iid({"target_names": ["albedo", "shading"], "albedo": {"prediction_space": "srgb"},
                      "shading": {"prediction_space": "linear", "up_to_scale": True}})


def _entries_equal(a, b):
    return all(np.array_equal(a[t].array, b[t].array) and np.array_equal(np.asarray(a[t].image), np.asarray(b[t].image))
               and ((a[t].uncertainty is None and b[t].uncertainty is None) or np.array_equal(a[t].uncertainty, b[t].uncertainty))
               for t in a.target_names)


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("match_input_res", [False, True])
def test_pipeline_entries_against_numpy_fill_entry(pipe2, E, match_input_res):
    from marigold_amd import synthetic as syn
    from marigold_amd.pipeline import MarigoldIIDOutput
    img = syn.synthetic_image(128, 256, seed=3)
    lat0 = torch.randn(E, 8, 8, 16, generator=torch.Generator().manual_seed(70 + E))
    seen = []
    base = pipe2.fill_outputs
    pipe2.fill_outputs = lambda output, final_pred, pred_uncert=None: (seen.append((final_pred, pred_uncert)),
                                                                        base(output, final_pred, pred_uncert))[1]
    try:
        out = pipe2(img, ensemble_size=E, processing_res=128, match_input_res=match_input_res, show_progress_bar=False,
                    init_latents=lat0, ensemble_kwargs=dict(output_uncertainty=True))
    finally:
        del pipe2.fill_outputs
    (final_pred, pred_uncert), = seen
    hw = (128, 256) if match_input_res else (64, 128)
    assert final_pred.is_cuda and tuple(final_pred.shape) == (1, 6) + hw and (pred_uncert is None) == (E == 1)
    ref = MarigoldIIDOutput(pipe2.target_names)   # the same device prediction through the numpy path
    for i, name in enumerate(pipe2.target_names):
        ref.fill_entry(name, final_pred[:, 3 * i:3 * i + 3], None if pred_uncert is None else pred_uncert[:, 3 * i:3 * i + 3],
                       pipe2.target_properties)
    assert out.is_complete
    for i, name in enumerate(pipe2.target_names):
        e, r = out[name], ref[name]
        assert e.array.dtype == r.array.dtype == np.float32 and e.array.shape == r.array.shape == (3,) + hw
        assert e.array.tobytes() == r.array.tobytes()
        if E == 1:
            assert e.uncertainty is None and r.uncertainty is None
        else:
            # (the uncertainty keeps the processing resolution: only the prediction is resized back)
            assert e.uncertainty.dtype == r.uncertainty.dtype and e.uncertainty.shape == r.uncertainty.shape == (3, 64, 128)
            assert e.uncertainty.tobytes() == r.uncertainty.tobytes()
        assert e.image.mode == r.image.mode == "RGB" and e.image.size == r.image.size == hw[::-1]
        flags = [(name == "shading", name == "shading")]
        _check(f"pipeline E={E} match_input_res={match_input_res} {name}", np.asarray(e.image)[None], np.asarray(r.image)[None], flags)
        assert e.device_array.is_cuda and e.device_array.dtype == torch.float32 and tuple(e.device_array.shape) == (3,) + hw
        assert np.array_equal(e.device_array.cpu().numpy(), e.array) and r.device_array is None
    assert np.asarray(out["shading"].image).max() == 255   # normalised to its maximum


def test_map_images_gives_the_lone_outputs(pipe2):
    from marigold_amd import synthetic as syn
    imgs = [syn.synthetic_image(64, 128, seed=s) for s in (1, 2, 3)]
    kw = dict(denoising_steps=2, ensemble_size=2, processing_res=0, show_progress_bar=False, ensemble_kwargs=dict(output_uncertainty=True))
    gens = lambda: [torch.Generator(device="cuda:0").manual_seed(40 + k) for k in range(len(imgs))]   # noqa: E731
    lone = [pipe2(im, generator=g, **kw) for im, g in zip(imgs, gens())]
    flight = list(pipe2.map_images(imgs, in_flight=2, generators=gens(), **kw))
    assert len(flight) == len(lone) == 3
    for a, b in zip(flight, lone):
        assert a.is_complete and _entries_equal(a, b)
        assert all(torch.equal(a[t].device_array, b[t].device_array) for t in a.target_names)
    assert not _entries_equal(lone[0], lone[1])


# ---- 5. validate end to end ------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def pipe3():
    """A tiny lighting model: three targets, UNet 16 -> 12 latent channels."""
    assert torch.cuda.is_available()
    return _tiny_iid({"target_names": ["albedo", "shading", "residual"], "albedo": {"prediction_space": "linear"},
                      "shading": {"prediction_space": "linear", "up_to_scale": True},
                      "residual": {"prediction_space": "linear", "up_to_scale": True}})


@pytest.mark.parametrize("linear", [(), ("shading",)], ids=["srgb", "shading_linear"])
@pytest.mark.parametrize("use_mask", [False, True])
def test_validate_matches_infer_then_eval(pipe3, tmp_path, use_mask, linear):
    from marigold_amd.evaluation import datasets as D, harness as H
    cfgs = write_synthetic_datasets(str(tmp_path))
    cfg_path = tmp_path / "i.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["hypersim_iid"]))
    targets = pipe3.target_names
    base = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path)]
    run = ["--denoise_steps", "2", "--processing_res", "128", "--ensemble_size", "2", "--seed", "5"]
    score = (["--use_mask"] if use_mask else []) + (["--targets_to_eval_in_linear_space"] + list(linear) if linear else [])
    v, p, e = tmp_path / "v", tmp_path / "p", tmp_path / "e"
    assert H.validate_iid_main(base + run + score + ["--output_dir", str(v)], pipeline=pipe3) == 0
    assert H.infer_main("iid", base + run + ["--output_dir", str(p)], pipeline=pipe3) == 0
    assert H.eval_main("iid", base + score + ["--prediction_dir", str(p), "--output_dir", str(e), "--target_names"] + targets) == 0
    files = sorted(os.listdir(p / "ai"))
    assert files == [f"rgb_cam_00_fr0000_{t}.npy" for t in sorted(targets)] and sorted(os.listdir(v / "ai")) == files
    for f in files:
        assert (v / "ai" / f).read_bytes() == (p / "ai" / f).read_bytes(), f
    assert sorted(os.listdir(v / "eval")) == sorted(os.listdir(e)) == ["eval_metrics.txt", "per_sample_metrics.csv"]
    got, want = ((d / "per_sample_metrics.csv").read_text().strip().split("\n") for d in (v / "eval", e))
    assert got[0] == want[0] == "filename," + ",".join(f"{m}_{t}" for t in targets for m in ("psnr", "ssim"))
    assert len(got) == len(want) == 2 and got[1].split(",")[0] == want[1].split(",")[0] == "ai/rgb_cam_00_fr0000.png"
    got, want = ([float(x) for x in row[1].split(",")[1:]] for row in (got, want))
    print(f"[parity] validate use_mask={use_mask} linear={linear}:\n  validate   {got}\n  infer+eval {want}")
    data = D.get_dataset(cfgs["hypersim_iid"], str(tmp_path), D.DatasetMode.EVAL)[0]
    for k, t in enumerate(targets):
        gammas = ([2.2] if t in linear else []) + ([1.0 / 2.2] if t == "albedo" else [])   # Hypersim's three-target albedo rule
        if gammas:
            pr, gt = np.load(p / "ai" / f"rgb_cam_00_fr0000_{t}.npy")[None].astype(np.float32), data[t][None].astype(np.float32)
            for ex in gammas:
                pr, gt = pr ** ex, gt ** ex
            host, moved = _movement_under_2ulp(pr, gt, t, data["mask_" + t] if use_mask else None)
            dev = np.abs(np.array(got[2 * k:2 * k + 2]) - host)
            print(f"[parity]   {t} gamma {gammas}: host moves by {moved[0]:.2e} / {moved[1]:.2e} under +-2 ulp, device differs by {dev[0]:.2e} / {dev[1]:.2e}")
            assert np.array_equal(host, want[2 * k:2 * k + 2])
            assert (dev <= 4 * moved).all(), (t, got, want, moved)
        else:
            np.testing.assert_allclose(got[2 * k], want[2 * k], rtol=1e-5)
            assert abs(got[2 * k + 1] - want[2 * k + 1]) <= SSIM_ATOL
    assert np.isfinite(got).all()
    text = (v / "eval" / "eval_metrics.txt").read_text()
    assert f"of predictions: {v}" in text and "hypersim_iid_synth" in text


def test_validate_scores_only_and_elsewhere(pipe3, tmp_path):
    from marigold_amd.evaluation import harness as H
    cfgs = write_synthetic_datasets(str(tmp_path))
    cfg_path = tmp_path / "i.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["hypersim_iid"]))
    args = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path), "--denoise_steps", "2", "--processing_res", "128",
            "--ensemble_size", "1", "--seed", "5", "--use_mask"]
    assert H.validate_iid_main(args + ["--output_dir", str(tmp_path / "a")], pipeline=pipe3) == 0
    assert H.validate_iid_main(args + ["--output_dir", str(tmp_path / "b"), "--no_save_predictions", "--eval_output_dir",
                                       str(tmp_path / "b_eval"), "--maps_in_flight", "2"], pipeline=pipe3) == 0
    assert os.listdir(tmp_path / "b") == [] and len(os.listdir(tmp_path / "a" / "ai")) == 3
    assert sorted(os.listdir(tmp_path / "b_eval")) == ["eval_metrics.txt", "per_sample_metrics.csv"]
    assert (tmp_path / "b_eval" / "per_sample_metrics.csv").read_bytes() == (tmp_path / "a" / "eval" / "per_sample_metrics.csv").read_bytes()
