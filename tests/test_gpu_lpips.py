"""LPIPS on a real MI355X: ``score_iid(..., metrics=(..., "lpips"), lpips=net)`` / ``score_iid_sample(..., lpips=net)`` /
``validate_iid_main --lpips_weights`` (evaluation/device.py over mg_eval_iid_lpips, csrc/lpips.hip) against the host function in
float64 (tests/lpips_cases.py), with both synthetic weight sets.

The bound is measured, not chosen.  D is the largest deviation (``lpips_cases.rel_dev``: relative, over the total and the five
tap terms; a tap below 1 % of its case's score is held against 1 % of that score) of the host function in fp32 (torch CPU) from the
same function in fp64 over the cases of the test, taken per weight set; the device has to stay within 8 D on the same cases.  The
factor is not 1 because the device adds its K products (chains of up to 3456 terms) in another order than the CPU's convolution
and D itself scatters from case to case.  D must also lie below a ceiling, so that no degenerate term can inflate it and void the
check.  "live" (every tap above the 1 % floor, all numbers relative): fp32 unit roundoff 2^-24 = 6e-8, a random walk over the
longest K chain (sqrt(3456) = 59) gives 3.5e-6 per layer, and five layers with the norm and the difference behind them about
five times that, 2e-5.  "dead": a position that is nearly switched off has features of the order of sqrt(eps) = 1e-4 left from a
cancelled sum of terms near the bias (0.6), whose absolute roundoff is about 1e-7; f / sqrt(eps + |f|^2) has slope 1 / sqrt(eps)
= 1e4 there, so such a position's contribution is uncertain by about 1e-3 of itself in fp32 on any machine, and a sub-floor tap
made of such positions, held against the floor, can show up to that: 1e-3.  (A wrong eps form moves such a tap by the order of
itself, a share / floor of 0.1 and more; a tail that costs a per cent of a tap above the floor shows as 1e-2: both far above
8 x the ceiling's worst case for the live set and above what the dead set measures.)  The test prints D and the device's figures
(docs/history/lpips_device.md keeps a copy)."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import lpips_cases as C

pytestmark = pytest.mark.gpu

FACTOR = 8.0
D_CEILING = {"live": 2e-5, "dead": 1e-3}


@pytest.fixture(scope="module")
def EV():
    assert torch.cuda.is_available()
    from marigold_amd import evaluation
    return evaluation


def _device_terms(EV, kind, case, f16=False):
    """(terms, result dict) of one case from mg_eval_iid_lpips itself: the eight doubles."""
    from marigold_amd import _lib as L
    from marigold_amd.evaluation import device as DV
    hw, target, masked, gm = case
    p, g, mask = C.case_inputs(*case)
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        lib, ws, stream = DV._setup(dev, f16)
        out, keep = torch.full((16,), 7.0, dtype=torch.float64, device=dev), []
        DV._iid_launch(lib, ws, stream, dev, p, g, mask, target in C.UP_TO_SCALE, C.GAMMA[gm], ("psnr", "lpips"), out[:8], keep,
                       C.net(kind), out[8:])
        v = out.cpu().tolist()
    assert v[9] == 0 and np.isnan(v[15])
    return tuple(v[10:15]), v[8]


@pytest.mark.parametrize("kind", ["live", "dead"])
def test_every_size_against_fp64(EV, kind):
    D, worst, lines = 0.0, 0.0, []
    for case in C.cases():
        want = C.host_terms(kind, *case, True)
        D = max(D, C.rel_dev(C.host_terms(kind, *case, False), want))
    assert 0 < D < D_CEILING[kind], D
    if kind == "live":   # every tap carries more than the floor's share of the score: the whole live set is held relatively
        assert all(min(C.host_terms(kind, *case, True)) > C.TERM_FLOOR * C.total(C.host_terms(kind, *case, True)) for case in C.cases())
    for case in C.cases():
        want = C.host_terms(kind, *case, True)
        got, total = _device_terms(EV, kind, case)
        assert total == C.total(got)   # the total is the terms' sum, in order
        dev = C.rel_dev(got, want)
        worst = max(worst, dev)
        lines.append(f"  {kind} {case}: device {dev:.3e}  host fp32 {C.rel_dev(C.host_terms(kind, *case, False), want):.3e}  lpips {total:.9g}")
    print(f"\nLPIPS {kind}: D = {D:.3e}, bound {FACTOR * D:.3e}, device worst {worst:.3e}\n" + "\n".join(lines))
    assert worst <= FACTOR * D, (worst, D)


def test_dead_positions_occur():
    """The "dead" set must switch whole positions off in the cases the device is held to, or the eps of the channel norm is never
    the only term under the root: every position of the last tap at 31 x 31, some but not all of an image's at 35 x 47."""
    counts = {case: C.dead_positions("dead", case) for case in C.cases() if case[0] in ((31, 31), (35, 47))}
    assert any(all(d == n for d, n in c) for case, c in counts.items() if case[0] == (31, 31))
    assert any(any(0 < d < n for d, n in c) for case, c in counts.items() if case[0] == (35, 47))
    assert all(np.isfinite(C.host_terms("dead", *case, True)).all() for case in counts)


def test_garbage_under_the_mask_and_out_of_range(EV):
    net = C.net("live")
    p, g, mask = C.pair(35, 47, masked=True)
    clean = EV.score_iid(p, g, "shading", mask, metrics=("psnr", "ssim", "lpips"), lpips=net)
    p2, g2 = p.copy(), g.copy()
    p2[~mask], g2[~mask] = np.nan, 1e30
    dirty = EV.score_iid(p2, g2, "shading", mask, metrics=("psnr", "ssim", "lpips"), lpips=net)
    assert np.float64(clean["lpips"]).tobytes() == np.float64(dirty["lpips"]).tobytes() and clean["lpips"] > 0
    assert set(dirty) == {"psnr", "ssim", "scale", "quantile", "n", "lpips"}
    p3 = p.copy()
    idx = np.argwhere(mask)[:3]
    p3[tuple(idx[0])], p3[tuple(idx[1])] = 1.5, np.nan
    g3 = g.copy()
    g3[tuple(idx[2])] = -0.25
    with pytest.raises(ValueError, match=r"lpips: 3 element\(s\) outside \[0, 1\]"):
        EV.score_iid(p3, g3, "albedo", mask, metrics=("lpips",), lpips=net)
    with pytest.raises(ValueError, match=r"lpips: 3 element\(s\) outside \[0, 1\]"):   # the host function counts the same
        from marigold_amd.evaluation import metrics as M
        M.compute_iid_metric(p3[None], g3[None], "albedo", "lpips", mask[None], lpips_net=net)
    with pytest.raises(NotImplementedError, match="LPIPS needs pretrained network weights"):
        EV.score_iid(p, g, "albedo", mask, metrics=("lpips",))
    assert "lpips" not in EV.score_iid(p, g, "albedo", mask, lpips=net)   # only when asked for


def test_sample_row(EV):
    net = C.net("live")
    targets = ["albedo", "shading", "residual"]
    preds, data = {}, {}
    for k, t in enumerate(targets):
        p, g, mask = C.pair(35, 47, seed=k, masked=True)
        preds[t], data[t], data["mask_" + t] = p, g, mask
    preds["residual"] = None
    kw = dict(use_mask=True, linear_targets=("shading",), dataset_name="hypersim_iid")
    row = EV.score_iid_sample(preds, data, targets, lpips=net, **kw)
    plain = EV.score_iid_sample(preds, data, targets, **kw)
    assert len(row) == 9 and len(plain) == 6 and row[6:] == [None] * 3
    assert [row[0], row[1], row[3], row[4]] == plain[:4]   # the other columns are byte-identical to a row without LPIPS
    for k, (t, gamma) in enumerate((("albedo", 1.0 / 2.2), ("shading", 2.2))):
        one = EV.score_iid(preds[t], data[t], t, data["mask_" + t], metrics=("psnr", "ssim", "lpips"), gamma=gamma, lpips=net)
        assert row[3 * k:3 * k + 3] == [one["psnr"], one["ssim"], one["lpips"]]


def test_same_bytes_every_call_and_in_both_libraries(EV):
    case = ((97, 131), "shading", True, 3)
    first = _device_terms(EV, "live", case)
    for _ in range(19):
        assert _device_terms(EV, "live", case) == first
    assert _device_terms(EV, "live", case, f16=True) == first


def test_validate_main_with_lpips_weights(EV, tmp_path):
    """validate_iid_main with a stand-in pipeline (as tests/test_iid_validate_host.py drives it) and --lpips_weights: the lpips_*
    columns are score_iid's.  The synthetic Hypersim sample is 24 x 32, below LPIPS's 31 x 31, so its rasters are rewritten larger."""
    from marigold_amd.evaluation import datasets as DS, harness as H
    from marigold_amd.pipeline import MarigoldIIDOutput
    from oracle.make_eval_golden import write_synthetic_datasets
    cfgs = write_synthetic_datasets(str(tmp_path))
    C.enlarge_iid_sample(tmp_path / cfgs["hypersim_iid"]["dir"])
    cfg_path = tmp_path / "i.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["hypersim_iid"]))
    sample = DS.get_dataset(cfgs["hypersim_iid"], str(tmp_path), DS.DatasetMode.EVAL)[0]
    targets = ["albedo", "shading", "residual"]
    props = {"target_names": targets, "albedo": {"prediction_space": "linear"}, "shading": {"prediction_space": "linear", "up_to_scale": True},
             "residual": {"prediction_space": "srgb", "up_to_scale": True}}
    made = C.noisy_predictions(sample, targets)

    class FakeIID:
        device = "cpu"
        target_names = targets

        def __call__(self, image, **kw):
            o = MarigoldIIDOutput(self.target_names)
            for t in self.target_names:
                o.fill_entry(t, torch.from_numpy(made[t])[None], None, props)
            return o

    a, b = C.write_files(tmp_path)
    argv = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path), "--denoise_steps", "4", "--processing_res", "0",
            "--ensemble_size", "1", "--seed", "1", "--use_mask", "--output_dir", str(tmp_path / "v"), "--no_save_predictions"]
    assert H.validate_iid_main(argv + ["--lpips_weights", a, b], pipeline=FakeIID()) == 0
    rows = (tmp_path / "v" / "eval" / "per_sample_metrics.csv").read_text().strip().split("\n")
    assert rows[0] == "filename," + ",".join(f"{m}_{t}" for t in targets for m in ("psnr", "ssim", "lpips"))
    cells = rows[1].split(",")[1:]
    for k, t in enumerate(targets):
        gamma = 1.0 / 2.2 if t == "albedo" else None   # the Hypersim three-target albedo rule
        one = EV.score_iid(made[t], sample[t], t, sample["mask_" + t], metrics=("psnr", "ssim", "lpips"), gamma=gamma, lpips=C.net("live"))
        assert cells[3 * k:3 * k + 3] == [str(one["psnr"]), str(one["ssim"]), str(one["lpips"])]
