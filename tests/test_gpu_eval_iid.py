"""Intrinsic-image scoring on a real MI355X: ``score_iid`` / ``score_iid_sample`` (marigold_amd/evaluation/device.py, the
MG_OP_IIDSCORE_* ops of csrc/evalscore.hip) against the reference's recorded numbers (tests/golden/eval_ref.npz), against an
fp64 restatement of SSIM written here, against the host scorer and through the row ``harness._score_iid`` builds.

Bounds.
* Alignment scale and PSNR: rtol 1e-5 against the golden; the mapped ground truth atol 2e-6 - what tests/test_evaluation.py holds
  the host code to.
* SSIM: 1e-9 absolute against ``_ssim_fp64`` below (torch conv2d in float64 on a reflect-padded CPU tensor, border cropped) and
  against ``metrics.ssim``.  The window moments are fp64 sums of exact products of fp32 values on every side, so the sides
  differ in summation order only: about 121 * 2^-53 / c2 ~ 1e-11 per pixel.  SSIM stays unpinned against torchmetrics, which
  is not available offline: ``_ssim_fp64`` and ``metrics.ssim`` both restate its documented definition (Gaussian 11 x 11, sigma 1.5,
  k1 0.01, k2 0.03, reflect padding, cropped border).
* Quantile: the two order statistics bit for bit np.partition's, the interpolated value within 1 fp32 ulp of np.quantile.
* Gamma modes: device ``powf`` and numpy's float32 power differ by a few ulp, so the target is the host score of numpy-gamma'd
  fp32 inputs and the bound is measured at run time, not chosen: 4 x the largest movement of the host PSNR / SSIM when every
  gamma'd input moves by +-2 fp32 ulp, over seven sign patterns - the four coherent ones (pred and gt each all up or all down:
  a power function that errs to one side) and three random draws.  Measured on the 37 x 53 masked case
  (profiles/eval_iid_device.log), per gamma mode and target the host movement -> bound | device deviation, PSNR in dB / SSIM:
    2.2           albedo   2.83e-06 / 1.90e-07 -> 1.13e-05 / 7.61e-07 | 3.94e-08 / 1.68e-09
    2.2           shading  5.85e-07 / 3.04e-09 -> 2.34e-06 / 1.22e-08 | 3.49e-08 / 8.34e-11
    1 / 2.2       albedo   1.09e-05 / 1.43e-07 -> 4.37e-05 / 5.74e-07 | 2.82e-07 / 4.78e-09
    1 / 2.2       shading  9.10e-07 / 1.13e-09 -> 3.64e-06 / 4.51e-09 | 3.44e-08 / 1.13e-10
    2.2, 1 / 2.2  albedo   5.89e-06 / 2.50e-07 -> 2.36e-05 / 1.00e-06 | 2.52e-07 / 1.07e-08
    2.2, 1 / 2.2  shading  4.39e-07 / 1.87e-09 -> 1.76e-06 / 7.49e-09 | 1.19e-07 / 9.80e-11
"""
import os

import numpy as np
import pytest
import torch

from oracle.make_eval_golden import eval_inputs, write_synthetic_datasets

pytestmark = pytest.mark.gpu

SSIM_ATOL = 1e-9
UP_TO_SCALE = ("shading", "residual")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_ref.npz"))


@pytest.fixture(scope="module")
def iid():
    return eval_inputs()["iid"]


@pytest.fixture(scope="module")
def EV():
    assert torch.cuda.is_available()
    from marigold_amd import evaluation
    return evaluation


def _pair(shape, seed, masked):
    r = np.random.default_rng(seed)
    h, w = shape
    gt = r.uniform(0, 0.7, (3, h, w)).astype(np.float32)
    pred = np.clip(gt * 0.6 + r.normal(0, 0.03, gt.shape), 0, 1).astype(np.float32)
    mask = np.broadcast_to(r.uniform(size=(1, h, w)) > 0.15, gt.shape).copy() if masked else None
    return pred, gt, mask


def _raw(pred, gt, mask, up_to_scale, gamma=None, metrics=3, f16=False):
    """mg_eval_iid itself -> the eight doubles as a CPU tensor."""
    from marigold_amd import _lib as L
    lib = L.init(0, f16)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    m = torch.from_numpy(mask).cuda().view(torch.uint8) if mask is not None else None
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((L.EVAL_WS_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")   # the call owns (and clears) what it needs
    L.check(lib.mg_eval_iid(p.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else None, pred.shape[1], pred.shape[2],
                            int(up_to_scale), L.iid_gamma_mode(gamma), metrics, out.data_ptr(), ws.data_ptr(), None), "mg_eval_iid", lib)
    torch.cuda.synchronize()
    return out.cpu()


def _ssim_fp64(x, y):
    """SSIM of [3,H,W] images, restated independently of the project: one 2-D Gaussian window through conv2d in float64."""
    F = torch.nn.functional
    k = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) / 1.5) ** 2 / 2)
    k = k / k.sum()
    win = torch.outer(k, k)[None, None]

    def blur(a):
        return F.conv2d(F.pad(a[:, None], (5, 5, 5, 5), mode="reflect"), win)[:, 0]
    x, y = torch.from_numpy(np.asarray(x, np.float32)).double(), torch.from_numpy(np.asarray(y, np.float32)).double()
    mx, my = blur(x), blur(y)
    sxx, syy, sxy = blur(x * x) - mx * mx, blur(y * y) - my * my, blur(x * y) - mx * my
    s = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    return float(s[:, 5:-5, 5:-5].mean())


def _mapped_on_host(pred, gt, mask, s, q):
    """The images compute_iid_metric scores for an up-to-scale target, from a given alignment scale and brightness quantile."""
    scale = np.float32(0.0 if q < 1e-4 else 0.8 / q)
    p, g = np.clip(scale * (np.float32(s) * pred), 0, 1), np.clip(scale * gt, 0, 1)
    if mask is not None:
        p, g = np.where(mask, p, 0), np.where(mask, g, 0)
    return p.astype(np.float32), g.astype(np.float32)


# ---- 1. the reference's recorded numbers ----------------------------------------------------------------------------


def test_scale_psnr_and_mapping_match_reference(EV, gold, iid):
    for tag, m in (("nomask", None), ("masked", iid["mask"])):
        alb = EV.score_iid(iid["pred"], iid["gt"], "albedo", m)
        sh = EV.score_iid(iid["pred"], iid["gt"], "shading", m)
        print(f"[iid-parity] {tag}: scale {sh['scale']!r} ref {float(gold[f'iid/scale_{tag}'])!r}; psnr albedo {alb['psnr']!r} ref "
              f"{float(gold[f'iid/psnr_albedo_{tag}'])!r}; psnr shading {sh['psnr']!r} ref {float(gold[f'iid/psnr_shading_{tag}'])!r}")
        np.testing.assert_allclose(sh["scale"], gold[f"iid/scale_{tag}"], rtol=1e-5)
        np.testing.assert_allclose(alb["psnr"], gold[f"iid/psnr_albedo_{tag}"], rtol=1e-5)
        np.testing.assert_allclose(sh["psnr"], gold[f"iid/psnr_shading_{tag}"], rtol=1e-5)
        assert alb["scale"] == 1.0 and np.isnan(alb["quantile"])
        assert alb["n"] == sh["n"] == (iid["gt"].size if m is None else int(m.sum()))
        raw = _raw(iid["pred"], iid["gt"], m, True)
        assert raw[2].item() == sh["scale"] and raw[3].item() == sh["quantile"]
        mapped = np.clip(np.float32(raw[4].item()) * iid["gt"], 0, 1)[None]
        np.testing.assert_allclose(mapped, gold[f"iid/qmap_gt_{tag}"], atol=2e-6)
        # CUDA tensors are used in place
        dev = [torch.from_numpy(a).cuda() for a in (iid["pred"], iid["gt"])] + [None if m is None else torch.from_numpy(m).cuda()]
        assert EV.score_iid(dev[0], dev[1], "shading", dev[2]) == sh
        assert EV.score_iid(iid["pred"][None], iid["gt"][None], "shading", None if m is None else m[None]) == sh


# ---- 2. SSIM against an independent fp64 restatement ---------------------------------------------------------------


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", [(32, 40), (37, 53), (120, 200), (480, 640), (768, 768)])
def test_ssim_matches_fp64_restatement(EV, shape, masked):
    from marigold_amd.evaluation import metrics as M
    pred, gt, mask = _pair(shape, 7000 + shape[0], masked)
    for target in ("albedo", "shading"):
        got = EV.score_iid(pred, gt, target, mask)
        if target in UP_TO_SCALE:
            # the mapping is checked on its own (tests 1 and 4): the restatement scores the images mapped with the device's (s, q)
            np.testing.assert_allclose(got["scale"], M.compute_alignment_scale(pred, gt, mask), rtol=1e-12)
            p, g = _mapped_on_host(pred, gt, mask, got["scale"], got["quantile"])
        else:
            p, g = (pred, gt) if mask is None else (np.where(mask, pred, 0), np.where(mask, gt, 0))
        want, host = _ssim_fp64(p, g), M.ssim(p[None], g[None])
        print(f"[iid-parity] ssim {shape} masked={masked} {target}: device {got['ssim']!r} restatement {want!r} (dev {abs(got['ssim'] - want):.2e}) "
              f"metrics.ssim {host!r} (dev {abs(got['ssim'] - host):.2e})")
        assert abs(got["ssim"] - want) <= SSIM_ATOL
        assert abs(got["ssim"] - host) <= SSIM_ATOL
        # and the whole host function, mapping included
        full = M.compute_iid_metric(pred.copy(), gt.copy(), target, "ssim", mask)
        assert abs(got["ssim"] - full) <= SSIM_ATOL
        np.testing.assert_allclose(got["psnr"], M.compute_iid_metric(pred.copy(), gt.copy(), target, "psnr", mask), rtol=1e-5)
        only = EV.score_iid(pred, gt, target, mask, metrics=("psnr",))
        assert only["psnr"] == got["psnr"] and np.isnan(only["ssim"]) and only["n"] == got["n"]


# ---- 3. closed forms ------------------------------------------------------------------------------------------------


def test_closed_forms(EV):
    pred, gt, _ = _pair((37, 53), 31, False)
    same = EV.score_iid(gt, gt.copy(), "albedo")
    assert abs(same["ssim"] - 1.0) <= 1e-12 and same["psnr"] == float("inf")
    same = EV.score_iid(gt, gt.copy(), "shading")   # s = 1: the mapped images are identical as well
    assert abs(same["ssim"] - 1.0) <= 1e-12 and same["psnr"] == float("inf") and same["scale"] == 1.0
    for a, b in ((0.25, 0.75), (0.1, 0.1000001), (0.9, 0.0)):
        x, y = np.full((3, 40, 48), a, np.float32), np.full((3, 40, 48), b, np.float32)
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        want = (2 * a64 * b64 + 1e-4) / (a64 * a64 + b64 * b64 + 1e-4)
        got = EV.score_iid(x, y, "albedo")
        assert abs(got["ssim"] - want) <= 1e-12, (a, b, got["ssim"], want)
        np.testing.assert_allclose(got["psnr"], 10 * np.log10(1.0 / (a64 - b64) ** 2), rtol=1e-12)
    for shape in ((37, 53), (120, 200)):
        pred, gt, mask = _pair(shape, 32, True)
        ab, ba = EV.score_iid(pred, gt, "albedo", mask), EV.score_iid(gt, pred, "albedo", mask)
        assert np.float64(ab["ssim"]).tobytes() == np.float64(ba["ssim"]).tobytes()
        assert np.float64(ab["psnr"]).tobytes() == np.float64(ba["psnr"]).tobytes()
        assert ab["ssim"] < 0.99


# ---- 4. the quantile is exact -----------------------------------------------------------------------------------------


def _brightness(gt):
    return np.float32(0.3) * gt[0] + np.float32(0.59) * gt[1] + np.float32(0.11) * gt[2]


@pytest.mark.parametrize("n", [1, 2, 10, 11, 1000, 768 * 768])
def test_quantile_order_statistics_are_exact(n):
    from marigold_amd import _lib as L, ops
    L.init(0)
    r = np.random.default_rng(n)
    h, w = (768, 768) if n == 768 * 768 else (32, 40)
    gt = r.uniform(0, 0.7, (3, h, w)).astype(np.float32)
    if n == 1000:   # heavy ties: five distinct grey levels
        gt[:] = r.choice(np.array([0.1, 0.2, 0.3, 0.5, 0.6], np.float32), (1, h, w))
    pred = (gt * np.float32(0.5)).astype(np.float32)
    mask = np.zeros((3, h, w), bool)
    mask.reshape(3, -1)[:, r.permutation(h * w)[:n]] = True
    b = np.sort(_brightness(gt)[mask[0]])
    assert b.size == n
    p, g, m = (torch.from_numpy(a).cuda() for a in (pred, gt, mask))
    out = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.full((L.EVAL_WS_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
    ops.launch(ops.iidscore_prep(p, g, m.view(torch.uint8), out, ws, H=h, W=w))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    pos = np.float32(n - 1) * np.float32(0.9)      # where torch.quantile / np.quantile look on fp32 input
    lo = min(int(np.floor(pos)), n - 1)
    hi = min(lo + 1, n - 1)
    part = np.partition(_brightness(gt)[mask[0]], (lo, hi))
    assert np.float32(out[6]).tobytes() == part[lo].tobytes() == b[lo].tobytes()
    assert np.float32(out[7]).tobytes() == part[hi].tobytes() == b[hi].tobytes()
    want = np.quantile(_brightness(gt)[mask[0]].astype(np.float32), 0.9)
    assert want.dtype == np.float32 and float(np.float32(out[3])) == out[3]
    print(f"[iid-parity] quantile n={n}: device {out[3]!r} numpy {float(want)!r} order statistics {out[6]!r}, {out[7]!r}")
    assert abs(out[3] - float(want)) <= float(np.spacing(want))
    assert out[4] == float(np.float32(0.8 / float(np.float32(out[3]))))
    np.testing.assert_allclose(out[2], 2.0, rtol=1e-12)   # gt = 2 pred


# ---- 5. gamma ---------------------------------------------------------------------------------------------------------


def _host_scores(p, g, target, mask):
    from marigold_amd.evaluation import metrics as M
    return np.array([M.compute_iid_metric(p.copy(), g.copy(), target, m, mask) for m in ("psnr", "ssim")])


def _movement_under_2ulp(p, g, target, mask):
    """How far the host scores move when every (gamma'd, fp32) input moves by +-2 ulp - the precision the inputs carry.  The signs:
    the four coherent patterns (a power function that errs to one side moves a whole image one way) and three random draws."""
    base, worst = _host_scores(p, g, target, mask), np.zeros(2)
    r = np.random.default_rng(900)
    signs = [(np.int32(a), np.int32(b)) for a in (2, -2) for b in (2, -2)]
    signs += [tuple(r.choice(np.array([-2, 2], np.int32), p.shape) for _ in range(2)) for _ in range(3)]
    for sp, sg in signs:
        moved = [(a.view(np.int32) + sgn * (a > 0)).view(np.float32) for a, sgn in ((p, sp), (g, sg))]
        worst = np.maximum(worst, np.abs(_host_scores(moved[0], moved[1], target, mask) - base))
    return base, worst


@pytest.mark.parametrize("gamma", [2.2, 1.0 / 2.2, (2.2, 1.0 / 2.2)])
def test_gamma_modes(EV, gamma):
    pred, gt, mask = _pair((37, 53), 53, True)
    p, g = pred, gt
    for e in (gamma if isinstance(gamma, tuple) else (gamma,)):
        p, g = p ** e, g ** e            # float32 ** Python float: float32, as in harness._score_iid
    assert p.dtype == np.float32
    for target in ("albedo", "shading"):
        want, moved = _movement_under_2ulp(p, g, target, mask)
        bound = 4 * moved
        got = EV.score_iid(pred, gt, target, mask, gamma=gamma)
        dev = np.abs(np.array([got["psnr"], got["ssim"]]) - want)
        print(f"[iid-parity] gamma {gamma} {target}: host psnr / ssim move by {moved[0]:.2e} / {moved[1]:.2e} under +-2 ulp, bound "
              f"{bound[0]:.2e} / {bound[1]:.2e}, device differs by {dev[0]:.2e} / {dev[1]:.2e}")
        assert (moved > 0).all() and (dev <= bound).all()
        assert got != EV.score_iid(pred, gt, target, mask)   # the step is really taken


# ---- 6. degenerate inputs ------------------------------------------------------------------------------------------


def test_degenerate_inputs(EV):
    from marigold_amd import _lib as L
    pred, gt, mask = _pair((37, 53), 61, True)
    for target in ("albedo", "shading"):
        none = EV.score_iid(pred, gt, target, np.zeros_like(mask))
        assert none["n"] == 0 and all(np.isnan(none[k]) for k in ("psnr", "ssim", "scale", "quantile")), none
        assert torch.isnan(_raw(pred, gt, np.zeros_like(mask), target in UP_TO_SCALE)[[0, 1, 2, 3, 4, 6, 7]]).all()
        # garbage under the mask does not leak: the very same scores
        clean = EV.score_iid(pred, gt, target, mask)
        p2, g2 = pred.copy(), gt.copy()
        p2[~mask], g2[~mask] = np.nan, np.nan
        dirty = EV.score_iid(p2, g2, target, mask)
        assert np.isfinite([clean["psnr"], clean["ssim"], clean["scale"]]).all() and clean["n"] == int(mask.sum())
        assert {k: np.float64(v).tobytes() for k, v in dirty.items()} == {k: np.float64(v).tobytes() for k, v in clean.items()}
    dark = np.full_like(gt, 1e-5)
    for m in (None, mask):
        got = EV.score_iid(pred, dark, "shading", m)
        assert got["quantile"] < 1e-4 and got["psnr"] == float("inf") and got["ssim"] == 1.0, got
    small = np.zeros((3, 10, 64), np.float32)
    with pytest.raises(L.MarigoldHipError, match="H, W >= 11 required"):
        EV.score_iid(small, small, "albedo")
    with pytest.raises(NotImplementedError, match="LPIPS"):
        EV.score_iid(pred, gt, "albedo", metrics=("lpips",))
    edge = EV.score_iid(pred[:, :11, :11], gt[:, :11, :11], "albedo")   # one kept value per channel
    np.testing.assert_allclose(edge["ssim"], _ssim_fp64(pred[:, :11, :11], gt[:, :11, :11]), atol=SSIM_ATOL)
    assert EV.score_iid(pred, gt, "albedo", mask)["n"] == int(mask.sum())   # and the scorer still works afterwards


# ---- 7. bit reproducibility --------------------------------------------------------------------------------------------


def test_twenty_calls_the_same_bytes_and_fp16_library():
    pred, gt, mask = _pair((768, 768), 71, True)
    for up in (False, True):
        first = _raw(pred, gt, mask, up, gamma=2.2)
        assert torch.isfinite(first[:2]).all()
        for _ in range(19):
            assert torch.equal(_raw(pred, gt, mask, up, gamma=2.2).view(torch.int64), first.view(torch.int64))
        assert torch.equal(_raw(pred, gt, mask, up, gamma=2.2, f16=True).view(torch.int64), first.view(torch.int64))


# ---- 8. the row of the evaluation program ----------------------------------------------------------------------------


class _Args:
    metrics = ["psnr", "ssim"]


@pytest.mark.parametrize("use_mask", [False, True])
def test_sample_row_matches_the_harness(EV, tmp_path, use_mask):
    from marigold_amd.evaluation import datasets as D, harness as H
    cfgs = write_synthetic_datasets(str(tmp_path))
    dataset = D.get_dataset(cfgs["hypersim_iid"], str(tmp_path), D.DatasetMode.EVAL)
    data = dataset[0]
    r = np.random.default_rng(81)
    targets = ["albedo", "shading", "residual"]
    preds = {t: np.clip(data[t] * r.uniform(0.5, 0.9) + r.normal(0, 0.03, data[t].shape), 0, None).astype(np.float32) for t in targets}
    stem = os.path.join(str(tmp_path), "pred", os.path.splitext(data["rgb_relative_path"])[0])
    os.makedirs(os.path.dirname(stem), exist_ok=True)
    for t in targets:
        np.save(f"{stem}_{t}.npy", preds[t])
    # (a) every target there, none in linear space: the bounds of tests 1 and 2; albedo takes Hypersim's 1 / 2.2, so test 5's
    # (b) shading in linear space (2.2), residual missing
    for linear, missing in (([None], None), (["shading"], "residual")):
        if missing:
            os.remove(f"{stem}_{missing}.npy")
        args = _Args()
        args.prediction_dir, args.target_names, args.use_mask = os.path.join(str(tmp_path), "pred"), targets, use_mask
        args.targets_to_eval_in_linear_space = linear
        label, want = H._score_iid(args, dataset, data, None)
        got = EV.score_iid_sample({t: p for t, p in preds.items() if t != missing}, data, targets, metrics=args.metrics, use_mask=use_mask,
                                  linear_targets=linear, dataset_name=dataset.name)
        print(f"[iid-parity] row use_mask={use_mask} linear={linear} missing={missing}:\n  device {got}\n  host   {want}")
        assert label == data["rgb_relative_path"] and len(got) == len(want) == 6
        assert [v is None for v in got] == [v is None for v in want]
        assert [v is None for v in got] == [False] * 4 + [missing is not None] * 2
        for k, t in enumerate(targets):
            if want[2 * k] is None:
                continue
            gammas = ([2.2] if t in linear else []) + ([1.0 / 2.2] if t == "albedo" else [])
            if gammas:   # the measured bound of test 5, on this target's own inputs
                p, g = preds[t][None], data[t][None].astype(np.float32)
                for e in gammas:
                    p, g = p ** e, g ** e
                base, moved = _movement_under_2ulp(p, g, t, data["mask_" + t] if use_mask else None)
                assert np.array_equal(base, want[2 * k:2 * k + 2])
                assert (np.abs(np.array(got[2 * k:2 * k + 2]) - base) <= 4 * moved).all(), (t, got, want, moved)
            else:
                np.testing.assert_allclose(got[2 * k], want[2 * k], rtol=1e-5)
                assert abs(got[2 * k + 1] - want[2 * k + 1]) <= SSIM_ATOL
