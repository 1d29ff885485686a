"""One-pass validation on a real MI355X: the device scorer (marigold_amd/evaluation/device.py, csrc/evalscore.hip) against the
reference's own numbers (tests/golden/eval_ref.npz, made by its src/util/metric.py and alignment.py), against the host
scorer through the whole preparation, and through ``infer.py --evaluate`` / ``eval.py --on_device``.

Bounds.  The host scorer's own bound against the reference is rtol 2e-6, atol 1e-7 (tests/test_evaluation.py); the device
scorer meets the same for every score that is not built on a logarithm, and the three accuracy counts meet it outright (one
miscounted pixel of <= 19 095 is >= 5e-5).  ``logf`` / ``log10f`` of the device library may differ from numpy's in the last
place; for the three log scores the bound is max(2e-6, 2 x the largest deviation from the golden measured on the three
cases, rounded up to one digit) - profiles/eval_device_parity.log holds the measurement - and may not exceed 2e-5.
"""
import os

import numpy as np
import pytest
import torch

from oracle.make_eval_golden import eval_inputs, write_synthetic_datasets

pytestmark = pytest.mark.gpu

ATOL = 1e-7
RTOL = {"abs_relative_difference": 2e-6, "squared_relative_difference": 2e-6, "rmse_linear": 2e-6,
        "rmse_log": 2e-6, "log10": 2e-6,      # measured <= 8.3e-8 / 9.0e-8 (profiles/eval_device_parity.log): twice that is below the 2e-6 floor
        "delta1_acc": 2e-6, "delta2_acc": 2e-6, "delta3_acc": 2e-6, "i_rmse": 2e-6,
        "silog_rmse": 2e-6}                   # measured <= 1.2e-7
assert max(RTOL.values()) <= 2e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_ref.npz"))


@pytest.fixture(scope="module")
def cases():
    return eval_inputs()


@pytest.fixture(scope="module")
def EV():
    assert torch.cuda.is_available()
    from marigold_amd import evaluation
    from marigold_amd.evaluation import device   # noqa: F401  (the module this file is about)
    return evaluation


def _check(got, want, names, what):
    from marigold_amd.evaluation import metrics as M
    for n, w in zip(names, want):
        g = got[n]
        dev = abs(g - w) / abs(w) if w else abs(g - w)
        print(f"[eval-parity] {what} {n}: device {g!r} reference {float(w)!r} rel.dev {dev:.2e} (rtol {RTOL[n]:.0e})")
    for n, w in zip(names, want):
        np.testing.assert_allclose(got[n], w, rtol=RTOL[n], atol=ATOL, err_msg=f"{what} {n}")
    assert list(got)[:10] == list(M.DEPTH_METRICS)


@pytest.mark.parametrize("key", ["depth_a", "depth_b", "depth_big"])
def test_depth_metrics_match_reference(EV, gold, cases, key):
    from marigold_amd.evaluation import metrics as M
    c = cases[key]
    assert c["pred"].min() >= 0.26   # the 1e-6 floor is a no-op on these cases
    got = EV.score_depth(c["pred"], c["gt"], c["mask"])
    _check(got, gold[f"{key}/metrics_masked"], M.DEPTH_METRICS, f"{key} masked")
    assert got["n"] == int(c["mask"].sum()) and got["scale"] == 1.0 and got["shift"] == 0.0
    for k in (1, 2, 3):   # exact counts
        assert round(got[f"delta{k}_acc"] * got["n"]) == round(float(gold[f"{key}/metrics_masked"][4 + k]) * got["n"])
    names = [n for n in M.DEPTH_METRICS if not n.startswith("delta")]
    full = EV.score_depth(c["pred"], c["gt"], np.ones_like(c["mask"]))
    _check(full, gold[f"{key}/metrics_nomask"], names, f"{key} all pixels")
    # garbage outside the mask must not leak into the scores: the very same bits
    gt, pred = c["gt"].copy(), c["pred"].copy()
    gt[~c["mask"]] = 0
    pred[~c["mask"]] = np.nan
    assert EV.score_depth(pred, gt, c["mask"]) == got
    # CUDA tensors are used in place
    dev = [torch.from_numpy(c[k]).cuda() for k in ("pred", "gt", "mask")]
    assert EV.score_depth(*dev) == got


@pytest.mark.parametrize("key", ["depth_a", "depth_b", "depth_big"])
def test_alignment_matches_reference(EV, gold, cases, key):
    c = cases[key]
    for res in (None, 64):   # (depth_big is 120 x 200: 64 sub-samples its width there)
        got = EV.score_depth(c["rel"], c["gt"], c["mask"], alignment="least_square", alignment_max_res=res)
        print(f"[eval-parity] {key} ls_{res}: device {got['scale']!r}, {got['shift']!r} reference {gold[f'{key}/ls_{res}']}")
        np.testing.assert_allclose([got["scale"], got["shift"]], gold[f"{key}/ls_{res}"], rtol=2e-4)
    got = EV.score_depth(c["rel"], c["gt_holes"], c["mask"], alignment="least_square_disparity")
    np.testing.assert_allclose([got["scale"], got["shift"]], gold[f"{key}/ls_disp"], rtol=2e-4)


def test_alignment_subsampling_index_rule(EV):
    r = np.random.default_rng(4242)
    gt = r.uniform(0.5, 9.5, (37, 53)).astype(np.float32)
    rel = ((gt.max() - gt) / (gt.max() - gt.min()) * 0.9 + 0.05 + r.normal(0, 0.02, gt.shape)).astype(np.float32)
    mask = r.uniform(size=gt.shape) > 0.25
    seen = set()
    for res in (37, 20, None):
        _, s, t = EV.align_depth_least_square(gt, rel, mask, True, res)
        got = EV.score_depth(rel, gt, mask, alignment="least_square", alignment_max_res=res)
        np.testing.assert_allclose([got["scale"], got["shift"]], [float(s[0]), float(t[0])], rtol=1e-6)
        seen.add((got["scale"], got["shift"]))
    assert len(seen) == 3   # the three fits really see different pixels


class _Clip:
    min_depth, max_depth = 0.5, 10.0


def _prepared_inputs(shape, seed):
    r = np.random.default_rng(seed)
    h, w = shape
    gt = (r.uniform(0.3, 12.0, shape) * (1 + 0.3 * np.sin(np.arange(w) / 7.0))).astype(np.float32)
    mask = r.uniform(size=shape) > 0.2
    gt_holes = gt.copy()
    gt_holes[~mask] = 0.0
    metric = np.clip(gt * r.uniform(0.8, 1.25, shape) + r.normal(0, 0.05, shape), 1e-3, None).astype(np.float32)
    rel = ((gt.max() - gt) / (gt.max() - gt.min()) * 0.9 + 0.05 + r.normal(0, 0.01, shape)).astype(np.float32)
    inv = 1.0 / gt
    disp = ((inv - inv.min()) / (inv.max() - inv.min()) * 0.95 + r.normal(0, 0.01, shape)).astype(np.float32)   # some <= 0
    return {None: (metric, gt, mask), "least_square": (rel, gt, mask), "least_square_disparity": (disp, gt_holes, mask)}


@pytest.mark.parametrize("case", ["depth_big", "480x640", "768x768"])
def test_device_scorer_matches_host_scorer_through_the_preparation(EV, cases, case):
    from marigold_amd.evaluation import harness as H, metrics as M
    if case == "depth_big":
        c = cases[case]
        inputs = {None: (c["pred"], c["gt"], c["mask"]), "least_square": (c["rel"], c["gt"], c["mask"]),
                  "least_square_disparity": (c["rel"], c["gt_holes"], c["mask"])}
    else:
        h, w = (int(v) for v in case.split("x"))
        inputs = _prepared_inputs((h, w), 1000 + h)
    for alignment, (pred, gt, mask) in inputs.items():
        for res in (None,) if alignment is None else (None, 320):
            prepared = H.align_and_clip_depth(pred.copy(), gt, mask, _Clip, alignment, res)
            want = [getattr(M, n)(prepared, gt, mask) for n in M.DEPTH_METRICS]
            got = EV.score_depth(pred, gt, mask, alignment=alignment, alignment_max_res=res, min_depth=_Clip.min_depth,
                                 max_depth=_Clip.max_depth)
            _check(got, want, M.DEPTH_METRICS, f"{case} {alignment} max_res={res} vs host")
            assert np.isfinite(want).all() and got["n"] == int(mask.sum())


NORMALS_GOLD = ("mean_angular_error", "median_angular_error", "rmse_angular_error", "sub5_error", "sub7_5_error",
                "sub11_25_error", "sub22_5_error", "sub30_error")


def test_normals_match_reference(EV, gold, cases):
    from marigold_amd.evaluation import metrics as M
    c = cases["normals"]
    for masked in (False, True):
        got, err = EV.score_normals(c["pred"][None], c["gt"][None], masked=masked, return_error_map=True)
        ref = gold[f"normals/err_masked{int(masked)}"]
        assert err.shape == ref.shape and err.dtype == np.float32 and got["n"] == ref.size
        np.testing.assert_allclose(err, ref, atol=2e-2)
        np.testing.assert_allclose([got[n] for n in NORMALS_GOLD], gold[f"normals/metrics_masked{int(masked)}"], atol=0.1)
        assert list(got)[:7] == list(M.NORMALS_METRICS)


def _reductions_agree(EV, pred, gt, masked=True):
    """numpy on the device's own error map must give the device's statistics."""
    got, err = EV.score_normals(pred, gt, masked=masked, return_error_map=True)
    n = err.size
    assert got["n"] == n and n > 0
    e64 = err.astype(np.float64)
    raw = EV.score_normals(pred, gt, masked=masked, rounded=False)
    np.testing.assert_allclose(raw["mean_angular_error"], e64.mean(), rtol=1e-6)
    np.testing.assert_allclose(raw["rmse_angular_error"], np.sqrt((e64 * e64).mean()), rtol=1e-6)
    assert {k: (round(v, 4) if k != "n" else v) for k, v in raw.items()} == got
    assert got["median_angular_error"] == round(float(np.median(err)), 4)
    for name, deg in (("sub5_error", 5), ("sub7_5_error", 7.5), ("sub11_25_error", 11.25), ("sub22_5_error", 22.5), ("sub30_error", 30)):
        assert got[name] == round(100.0 * float(np.sum(err < deg) / n), 4), name
    assert EV.score_normals(pred, gt, masked=masked) == got   # without the map the angles are recomputed: the same bits
    return got


def _tilted(angles_deg, r):
    """gt = random unit vectors, pred = gt rotated by the given angles about an axis orthogonal to it."""
    n = len(angles_deg)
    g = r.normal(size=(3, n))
    g /= np.linalg.norm(g, axis=0)
    o = np.cross(g.T, r.normal(size=(n, 3))).T
    o /= np.linalg.norm(o, axis=0)
    a = np.deg2rad(np.asarray(angles_deg, np.float64))
    return (g * np.cos(a) + o * np.sin(a)).astype(np.float32).reshape(3, 1, n), g.astype(np.float32).reshape(3, 1, n)


def test_normals_reductions_and_exact_median(EV, cases):
    r = np.random.default_rng(99)
    c = cases["normals"]
    _reductions_agree(EV, c["pred"], c["gt"], masked=True)      # n = 2205, odd
    _reductions_agree(EV, c["pred"], c["gt"], masked=False)     # n = 2240, even
    for n in (1, 2, 3, 64, 257, 1000, 1001):
        _reductions_agree(EV, *_tilted(r.uniform(0, 60, n), r))
    # heavy ties: a handful of distinct angles, the two middle ranks in one or in two neighbouring groups
    for n in (4096, 4097):
        _reductions_agree(EV, *_tilted(r.choice([2.0, 6.0, 10.0, 20.0, 25.0, 40.0], n), r))
    p, g = _tilted([10.0] * 500 + [30.0] * 500, r)
    assert abs(_reductions_agree(EV, p, g)["median_angular_error"] - 20.0) < 0.01
    p, g = _tilted([0.0] * 300, r)   # identical vectors: every angle (almost) zero
    _reductions_agree(EV, p, p.copy())
    # a full 768 x 768 map with holes in the ground truth
    g = r.normal(size=(3, 768, 768)).astype(np.float32)
    g /= np.linalg.norm(g, axis=0, keepdims=True)
    p = g + r.normal(0, 0.3, g.shape).astype(np.float32)
    g[:, r.uniform(size=(768, 768)) < 0.1] = 0
    got = _reductions_agree(EV, p, g)
    assert got["n"] < 768 * 768
    # a NaN prediction: NaN mean / median / rmse like numpy, and no fault
    p2 = p.copy()
    p2[:, 5, 5] = np.nan
    g2 = g.copy()
    g2[:, 5, 5] = (0, 0, 1)
    bad = EV.score_normals(p2, g2)
    assert np.isnan(bad["mean_angular_error"]) and np.isnan(bad["median_angular_error"]) and bad["n"] > 0


def test_normals_nothing_to_score(EV):
    p = np.random.default_rng(0).normal(size=(3, 9, 11)).astype(np.float32)
    got, err = EV.score_normals(p, np.zeros_like(p), masked=True, return_error_map=True)
    assert got["n"] == 0 and err.size == 0
    assert all(np.isnan(v) for k, v in got.items() if k != "n")
    # and the scorer still works afterwards
    assert EV.score_normals(p, p.copy())["n"] == 99


def test_ops_are_bit_reproducible(cases):
    from marigold_amd import _lib as L, ops
    L.init(0)
    c = cases["depth_big"]
    h, w = c["gt"].shape
    pred, gt = torch.from_numpy(c["rel"]).cuda(), torch.from_numpy(c["gt_holes"]).cuda()
    mask = torch.from_numpy(c["mask"]).cuda().view(torch.uint8)

    def fresh(n):
        return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    runs = []
    for _ in range(2):
        sums, out, s5, s11 = fresh(5), fresh(13), fresh(512 * 5), fresh(512 * 11)
        ops.launch(ops.eval_depth_ls(pred, gt, mask, sums, s5, H=h, W=w, disparity=True, max_res=64))
        ops.launch(ops.eval_depth_metrics(pred, gt, mask, sums, out, s11, H=h, W=w, disparity=True, min_depth=0.5, max_depth=10.0))
        torch.cuda.synchronize()
        runs.append((sums.cpu(), out.cpu()))
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(*runs))
    n = cases["normals"]
    p, g = (torch.from_numpy(n[k]).cuda().reshape(3, -1) for k in ("pred", "gt"))
    runs = []
    for _ in range(2):
        out, err = fresh(9), torch.full((p.shape[1],), 7.0, dtype=torch.float32, device="cuda")
        ws = torch.full((L.EVAL_WS_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")   # the op owns (and clears) its workspace
        ops.launch(ops.eval_normals(p, g, out, err, ws, HW=p.shape[1], masked=True))
        torch.cuda.synchronize()
        runs.append((out.cpu(), err.cpu()))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))


def test_fp16_library_scores_identically(EV, cases):
    c = cases["depth_big"]
    kw = dict(alignment="least_square_disparity", alignment_max_res=64, min_depth=0.5, max_depth=10.0)
    assert EV.score_depth(c["rel"], c["gt_holes"], c["mask"], f16=True, **kw) == EV.score_depth(c["rel"], c["gt_holes"], c["mask"], **kw)
    n = cases["normals"]
    a, ea = EV.score_normals(n["pred"], n["gt"], return_error_map=True, f16=True)
    b, eb = EV.score_normals(n["pred"], n["gt"], return_error_map=True)
    assert a == b and np.array_equal(ea, eb)


# ---- through the programs ------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def tiny():
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.modules import AutoencoderKLHIP, UNet2DConditionModelHIP
    from marigold_amd.util.host import usable_cores
    torch.set_num_threads(min(16, usable_cores()))
    usd, vsd = syn.synthetic_unet_state_dict(TINY_UNET), syn.synthetic_vae_state_dict(TINY_VAE)
    ctx = syn.synthetic_text_embedding(TINY_UNET.cross_attention_dim)
    eunet = UNet2DConditionModelHIP(usd, TINY_UNET).to("cuda:0")
    eunet.set_context(ctx)
    return dict(eunet=eunet, evae=AutoencoderKLHIP(vsd, TINY_VAE).to("cuda:0"), ctx=ctx)


def _rows(path):
    lines = path.read_text().strip().split("\n")
    return lines[0], [(ln.split(",")[0], [float(v) for v in ln.split(",")[1:]]) for ln in lines[1:]]


def _npy_files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith(".npy"))


def test_infer_evaluate_depth_end_to_end(tiny, tmp_path):
    import yaml
    import marigold_amd as MA
    from marigold_amd.evaluation import harness, metrics as M
    from marigold_amd.schedulers import DDIMScheduler
    cfgs = write_synthetic_datasets(str(tmp_path), as_tar=("nyu",))
    cfg_path = tmp_path / "nyu.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["nyu"]))
    pipe = MA.MarigoldDepthPipeline(tiny["eunet"], tiny["evae"], DDIMScheduler(), scale_invariant=True, shift_invariant=True,
                                    default_denoising_steps=2, default_processing_resolution=128, empty_text_embed=tiny["ctx"])
    base = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path)]
    run = ["--denoise_steps", "2", "--processing_res", "128", "--ensemble_size", "2", "--seed", "11"]
    plain, scored, ev, ev_dev, none = (tmp_path / d for d in ("plain", "scored", "ev", "ev_dev", "none"))
    assert harness.infer_main("depth", base + run + ["--output_dir", str(plain)], pipeline=pipe) == 0
    assert harness.infer_main("depth", base + run + ["--output_dir", str(scored), "--evaluate", "--alignment", "least_square"],
                              pipeline=pipe) == 0
    files = _npy_files(plain)
    assert files == _npy_files(scored) == ["test/kitchen/pred_0003.npy", "test/kitchen/pred_0012.npy"]
    for f in files:   # scoring does not touch the predictions
        assert np.array_equal(np.load(plain / f), np.load(scored / f))
    assert sorted(os.listdir(scored / "eval")) == ["eval_metrics-least_square.txt", "per_sample_metrics.csv"]
    assert harness.eval_main("depth", base + ["--prediction_dir", str(scored), "--output_dir", str(ev), "--alignment",
                                              "least_square"]) == 0
    assert harness.eval_main("depth", base + ["--prediction_dir", str(scored), "--output_dir", str(ev_dev), "--alignment",
                                              "least_square", "--on_device"]) == 0
    head, want = _rows(ev / "per_sample_metrics.csv")
    for other in (scored / "eval", ev_dev):
        head2, got = _rows(other / "per_sample_metrics.csv")
        assert head2 == head == "filename," + ",".join(M.DEPTH_METRICS) and [g[0] for g in got] == [w[0] for w in want] == files
        for (label, g), (_, w) in zip(got, want):
            assert np.isfinite(w).all()
            _check(dict(zip(M.DEPTH_METRICS, g)), w, M.DEPTH_METRICS, f"{os.path.basename(str(other))} {label}")
        a, b = ((d / "eval_metrics-least_square.txt").read_text().split("\n") for d in (other, ev))
        assert a[:6] == b[:6] and len(a) == len(b)   # the same header block; the table holds the (bounded) values
    assert _rows(scored / "eval" / "per_sample_metrics.csv") == _rows(ev_dev / "per_sample_metrics.csv")   # one scorer, the same bits
    # scores only
    assert harness.infer_main("depth", base + run + ["--output_dir", str(none), "--evaluate", "--alignment", "least_square",
                                                     "--no_save_predictions", "--eval_output_dir", str(tmp_path / "elsewhere")],
                              pipeline=pipe) == 0
    assert _npy_files(none) == [] and not (none / "eval").exists()
    assert _rows(tmp_path / "elsewhere" / "per_sample_metrics.csv") == _rows(scored / "eval" / "per_sample_metrics.csv")


def test_infer_evaluate_normals_end_to_end(tiny, tmp_path):
    import yaml
    import marigold_amd as MA
    from marigold_amd.evaluation import harness, metrics as M
    from marigold_amd.schedulers import DDIMScheduler
    cfgs = write_synthetic_datasets(str(tmp_path))
    cfg_path = tmp_path / "n.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["nyu_normals"]))
    pipe = MA.MarigoldNormalsPipeline(unet=tiny["eunet"], vae=tiny["evae"], scheduler=DDIMScheduler(), empty_text_embed=tiny["ctx"],
                                      default_denoising_steps=2, default_processing_resolution=0)
    base = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path)]
    run = ["--denoise_steps", "2", "--processing_res", "0", "--ensemble_size", "2", "--seed", "3"]
    plain, scored, ev, ev_dev, none = (tmp_path / d for d in ("plain", "scored", "ev", "ev_dev", "none"))
    assert harness.infer_main("normals", base + run + ["--output_dir", str(plain)], pipeline=pipe) == 0
    assert harness.infer_main("normals", base + run + ["--output_dir", str(scored), "--evaluate"], pipeline=pipe) == 0
    assert _npy_files(plain) == _npy_files(scored) == ["x/img.npy"]
    assert np.array_equal(np.load(plain / "x" / "img.npy"), np.load(scored / "x" / "img.npy"))
    assert harness.eval_main("normals", base + ["--prediction_dir", str(scored), "--output_dir", str(ev)]) == 0
    assert harness.eval_main("normals", base + ["--prediction_dir", str(scored), "--output_dir", str(ev_dev), "--on_device"]) == 0
    head, want = _rows(ev / "per_sample_metrics.csv")
    for other in (scored / "eval", ev_dev):
        head2, got = _rows(other / "per_sample_metrics.csv")
        assert head2 == head == "filename," + ",".join(M.NORMALS_METRICS) and [g[0] for g in got] == [w[0] for w in want] == ["x/img.png"]
        # angles from acosf on the device vs numpy's arccos: the host test's bound on the statistics
        np.testing.assert_allclose(got[0][1], want[0][1], atol=0.1)
        assert (other / "eval_metrics.txt").exists()
    assert _rows(scored / "eval" / "per_sample_metrics.csv") == _rows(ev_dev / "per_sample_metrics.csv")
    assert harness.infer_main("normals", base + run + ["--output_dir", str(none), "--evaluate", "--no_save_predictions"],
                              pipeline=pipe) == 0
    assert _npy_files(none) == [] and (none / "eval" / "per_sample_metrics.csv").exists()
