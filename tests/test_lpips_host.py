"""LPIPS without a GPU: the weight loader, the definition on the host (``metrics.lpips``), ``compute_iid_metric(..., "lpips")``,
``eval_main("iid", ... --lpips_weights)`` and the argument checks of ``mg_eval_iid_lpips`` in both libraries (they come before the
first device call).  The weights are synthetic (tests/lpips_cases.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from marigold_amd import _lib as L
from marigold_amd.evaluation import LpipsNet, harness as H, metrics as M
from tests import lpips_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the loader -------------------------------------------------------------------------------------------------------------


def test_loader_round_trip_and_errors(tmp_path):
    a, b = C.write_files(tmp_path, "live")
    backbone, lin = C.state_dicts("live")
    net = LpipsNet.from_files(a, b)
    for l, layer in enumerate(C.BACKBONE_LAYERS):
        assert torch.equal(net.conv_w[l], backbone[f"features.{layer}.weight"]) and net.conv_w[l].dtype == torch.float32
        assert torch.equal(net.conv_b[l], backbone[f"features.{layer}.bias"])
        assert torch.equal(net.lin_w[l], lin[f"lin{l}.model.1.weight"])
    assert any(k.startswith("classifier.") for k in backbone)   # present in the file, ignored by the loader
    same = LpipsNet.from_state_dicts({k: v for k, v in backbone.items() if not k.startswith("classifier.")}, lin)
    assert all(torch.equal(x, y) for x, y in zip(same.conv_w + same.conv_b + same.lin_w, net.conv_w + net.conv_b + net.lin_w))
    missing = {k: v for k, v in backbone.items() if k != "features.6.bias"}
    with pytest.raises(ValueError, match=r"'features\.6\.bias' is missing"):
        LpipsNet.from_state_dicts(missing, lin)
    with pytest.raises(ValueError, match=r"'lin3\.model\.1\.weight' is missing"):
        LpipsNet.from_state_dicts(backbone, {k: v for k, v in lin.items() if k != "lin3.model.1.weight"})
    wrong = dict(backbone)
    wrong["features.3.weight"] = torch.zeros(192, 64, 3, 3)
    with pytest.raises(ValueError, match=r"'features\.3\.weight'.*\(192, 64, 3, 3\).*\(192, 64, 5, 5\)"):
        LpipsNet.from_state_dicts(wrong, lin)
    wrong_lin = dict(lin)
    wrong_lin["lin0.model.1.weight"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"'lin0\.model\.1\.weight'"):
        LpipsNet.from_state_dicts(backbone, wrong_lin)
    with pytest.raises(ValueError, match="needs a GPU"):
        net.to("cpu")


# ---- the definition ---------------------------------------------------------------------------------------------------------


def _features_by_unfold(image, net):
    """Steps 1-3 restated in fp64 without conv2d / max_pool2d: explicit zero padding, F.unfold patches, one matmul per layer."""
    x = torch.as_tensor(image, dtype=torch.float64).reshape(1, 3, *image.shape[-2:])
    x = ((2 * x - 1) - torch.tensor(M.LPIPS_SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(M.LPIPS_SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    taps = []
    for l, (cin, cout, k, stride, pad) in enumerate(M.LPIPS_CONVS):
        if M.LPIPS_POOL_BEFORE[l]:
            h, w = x.shape[-2:]
            ho, wo = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            x = F.unfold(x, 3, stride=2).reshape(1, x.shape[1], 9, ho, wo).amax(dim=2)
        h, w = x.shape[-2:]
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        padded = torch.zeros(1, cin, h + 2 * pad, w + 2 * pad, dtype=torch.float64)
        padded[:, :, pad:pad + h, pad:pad + w] = x
        cols = F.unfold(padded, k, stride=stride)[0]   # [cin * k * k, ho * wo], rows (ci, ky, kx)
        y = net.conv_w[l].to(torch.float64).reshape(cout, -1) @ cols + net.conv_b[l].to(torch.float64)[:, None]
        x = y.clamp_min(0).reshape(1, cout, ho, wo)
        taps.append(x)
    return taps


@pytest.mark.parametrize("hw", [(31, 31), (35, 47)])
def test_geometry_against_unfold(hw):
    net = C.net("live")
    p, g, _ = C.pair(*hw)
    got, want = M.lpips_features(p[None], net, torch.float64), _features_by_unfold(p, net)
    sizes = [tuple(t.shape[-2:]) for t in got]
    assert sizes == ([(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)] if hw == (31, 31) else [(8, 11), (3, 5), (1, 2), (1, 2), (1, 2)])
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    # the whole score from the restated features
    terms = []
    for l, (a, b) in enumerate(zip(want, _features_by_unfold(g, net))):
        ua, ub = (t / (M.LPIPS_NORM_EPS + (t * t).sum(1, keepdim=True)).sqrt() for t in (a, b))
        terms.append(float((net.lin_w[l].to(torch.float64) * (ua - ub) ** 2).sum(1).mean()))
    ref = M.lpips(p[None], g[None], net, torch.float64)
    assert abs(sum(terms) - ref) <= 1e-12 * ref and ref > 0


def test_identity_symmetry_and_dead_positions():
    for kind in ("live", "dead"):
        net = C.net(kind)
        p, g, _ = C.pair(35, 47)
        assert M.lpips(p[None], p[None], net) == 0.0 and M.lpips(g[None], g[None], net, torch.float64) == 0.0
        for dtype in (torch.float32, torch.float64):
            assert M.lpips(p[None], g[None], net, dtype) == M.lpips(g[None], p[None], net, dtype)
    # the "dead" set switches whole positions off: all of layer 5 at 31 x 31, some at 35 x 47; each contributes exactly 0
    net = C.net("dead")
    p, g, _ = C.pair(31, 31)
    f5p, f5g = (M.lpips_features(x[None], net, torch.float64)[4] for x in (p, g))
    assert float(f5p.abs().sum()) == 0 and float(f5g.abs().sum()) == 0
    terms = M.lpips_terms(p[None], g[None], net, torch.float64)
    assert terms[4] == 0.0 and all(np.isfinite(terms)) and terms[0] > 0
    # among the device test's cases: one image partly dead at 35 x 47 (asserted, not trusted), and the unit vectors stay finite
    counts = {case: C.dead_positions("dead", case) for case in C.cases() if case[0] == (35, 47)}
    partly = [case for case, c in counts.items() if any(0 < d < n for d, n in c)]
    assert partly and any(all(d == n for d, n in c) for c in counts.values())
    pp, gg, mask = C.case_inputs(*partly[0])
    ps, gs = C.scored_images(C.gamma_np(pp, partly[0][3]), C.gamma_np(gg, partly[0][3]), partly[0][1], mask)
    for x in (ps, gs):
        f5 = M.lpips_features(x, net, torch.float64)[4]
        dead = f5.abs().sum(1) == 0
        unit = M._lpips_unit(f5)
        assert torch.isfinite(unit).all() and float(unit[:, :, dead[0]].abs().sum()) == 0
    assert all(np.isfinite(C.host_terms("dead", *partly[0], f64)).all() for f64 in (False, True))
    p, g, _ = C.pair(35, 47)
    with pytest.raises(ValueError, match="H, W >= 31"):
        M.lpips(p[None, :, :30], g[None, :, :30], net)


# ---- compute_iid_metric -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("target", ["albedo", "shading"])
def test_compute_iid_metric(target):
    net = C.net("live")
    p, g, mask = C.pair(35, 47, masked=True)
    for m in (None, mask):
        ps, gs = C.scored_images(p, g, target, m)
        assert ps.shape == (1, 3, 35, 47) and (m is None or (float(np.abs(ps[~m[None]]).sum()) == 0 and float(np.abs(gs[~m[None]]).sum()) == 0))
        want = M.lpips(ps, gs, net)
        assert M.compute_iid_metric(p[None], g[None], target, "lpips", None if m is None else m[None], lpips_net=net) == want
        assert M.compute_iid_metric(p, g, target, "lpips", m, lpips_net=net) == want
    with pytest.raises(NotImplementedError, match="LPIPS needs pretrained network weights"):
        M.compute_iid_metric(p[None], g[None], target, "lpips", mask[None])
    # garbage: refused outside the mask, unseen under it
    inside, outside = tuple(np.argwhere(mask)[0]), tuple(np.argwhere(~mask)[0])
    clean = M.compute_iid_metric(p, g, "albedo", "lpips", mask, lpips_net=net)
    for value in (1.5, np.nan):
        bad = p.copy()
        bad[inside] = value
        with pytest.raises(ValueError, match=r"lpips: 1 element\(s\) outside \[0, 1\]"):
            M.compute_iid_metric(bad, g, "albedo", "lpips", mask, lpips_net=net)
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            M.compute_iid_metric(bad, g, "albedo", "lpips", None, lpips_net=net)
        hidden = p.copy()
        hidden[outside] = value
        assert M.compute_iid_metric(hidden, g, "albedo", "lpips", mask, lpips_net=net) == clean


def test_pinned_against_torchmetrics(golden_dir):
    """Consumes tests/golden/lpips_ref.npz (tools/pin_lpips_against_torchmetrics.py: image pairs and torchmetrics' values) together with
    the pretrained files named by MARIGOLD_LPIPS_BACKBONE / MARIGOLD_LPIPS_LIN; without them the definition stays unpinned."""
    path = os.path.join(golden_dir, "lpips_ref.npz")
    files = os.environ.get("MARIGOLD_LPIPS_BACKBONE"), os.environ.get("MARIGOLD_LPIPS_LIN")
    if not os.path.exists(path) or not all(files):
        pytest.skip("LPIPS UNPINNED against torchmetrics: tests/golden/lpips_ref.npz (tools/pin_lpips_against_torchmetrics.py) or the "
                    "pretrained files (MARIGOLD_LPIPS_BACKBONE, MARIGOLD_LPIPS_LIN) are not here; metrics.lpips restates the definition")
    ref = np.load(path)
    net = LpipsNet.from_files(*files)
    for h, w in ref["sizes"]:
        got = M.lpips(ref[f"pred_{h}x{w}"][None], ref[f"gt_{h}x{w}"][None], net)
        assert abs(got - float(ref[f"lpips_{h}x{w}"])) <= 1e-5 * float(ref[f"lpips_{h}x{w}"])   # fp32 against fp32: summation order


# ---- the command line -------------------------------------------------------------------------------------------------------


def test_eval_main_with_lpips_weights(tmp_path):
    """The synthetic Hypersim sample of ``write_synthetic_datasets`` is 24 x 32, below LPIPS's 31 x 31: its rasters are rewritten
    larger (same files, names and distributions) before anything is scored."""
    from marigold_amd.evaluation import datasets as DS
    from oracle.make_eval_golden import write_synthetic_datasets
    cfgs = write_synthetic_datasets(str(tmp_path))
    C.enlarge_iid_sample(tmp_path / cfgs["hypersim_iid"]["dir"])
    cfg_path = tmp_path / "i.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["hypersim_iid"]))
    sample = DS.get_dataset(cfgs["hypersim_iid"], str(tmp_path), DS.DatasetMode.EVAL)[0]
    targets = ["albedo", "shading", "residual"]
    preds = tmp_path / "p" / "ai"
    os.makedirs(preds)
    made = C.noisy_predictions(sample, targets)
    for t in targets:
        np.save(preds / f"rgb_cam_00_fr0000_{t}.npy", made[t])
    a, b = C.write_files(tmp_path)
    argv = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path), "--prediction_dir", str(tmp_path / "p"), "--use_mask",
            "--target_names"] + targets
    assert H.eval_main("iid", argv + ["--output_dir", str(tmp_path / "with"), "--lpips_weights", a, b]) == 0
    assert H.eval_main("iid", argv + ["--output_dir", str(tmp_path / "without")]) == 0
    rows = (tmp_path / "with" / "per_sample_metrics.csv").read_text().strip().split("\n")
    assert rows[0] == "filename,psnr_albedo,ssim_albedo,lpips_albedo,psnr_shading,ssim_shading,lpips_shading,psnr_residual,ssim_residual,lpips_residual"
    cells = rows[1].split(",")[1:]
    net = C.net("live")
    for k, t in enumerate(targets):
        p, g = made[t][None], sample[t][None].astype(np.float32)
        if t == "albedo":   # the Hypersim three-target rule of script/iid/eval.py
            p, g = p ** (1.0 / 2.2), g ** (1.0 / 2.2)
        want = [M.compute_iid_metric(p.copy(), g.copy(), t, m, sample["mask_" + t], **({"lpips_net": net} if m == "lpips" else {}))
                for m in ("psnr", "ssim", "lpips")]
        assert cells[3 * k:3 * k + 3] == [str(v) for v in want] and 0 < want[2] < 1
    # without the flag: the files of a run that knows nothing of LPIPS (the columns and values the flag leaves alone are the same text)
    plain = (tmp_path / "without" / "per_sample_metrics.csv").read_text().strip().split("\n")
    assert plain[0] == "filename,psnr_albedo,ssim_albedo,psnr_shading,ssim_shading,psnr_residual,ssim_residual"
    assert plain[1].split(",")[1:] == [c for i, c in enumerate(cells) if i % 3 != 2]
    assert "lpips_albedo" not in (tmp_path / "without" / "eval_metrics.txt").read_text()
    # ... and whole, byte for byte, the two files as the writer made them before the flag existed, restated here from the scores:
    # one row of str() values under the psnr / ssim header, and the tabulated averages (one sample: the values themselves)
    from tabulate import tabulate
    names = [f"{m}_{t}" for t in targets for m in ("psnr", "ssim")]
    values = []
    for t in targets:
        p, g = made[t][None], sample[t][None].astype(np.float32)
        if t == "albedo":
            p, g = p ** (1.0 / 2.2), g ** (1.0 / 2.2)
        values += [M.compute_iid_metric(p.copy(), g.copy(), t, m, sample["mask_" + t]) for m in ("psnr", "ssim")]
    assert sorted(os.listdir(tmp_path / "without")) == ["eval_metrics.txt", "per_sample_metrics.csv"]
    assert (tmp_path / "without" / "per_sample_metrics.csv").read_bytes() == \
        ("filename," + ",".join(names) + "\n" + "ai/rgb_cam_00_fr0000.png," + ",".join(str(v) for v in values) + "\n").encode()
    assert (tmp_path / "without" / "eval_metrics.txt").read_bytes() == \
        (f"Evaluation metrics:\n    of predictions: {tmp_path / 'p'}\n    on dataset: hypersim_iid_synth\n"
         f"    with samples in: {cfgs['hypersim_iid']['filenames']}\n" + tabulate([names, [0.0 + v for v in values]])).encode()
    assert "lpips_residual" in (tmp_path / "with" / "eval_metrics.txt").read_text()
    # the parsers: the flag takes two paths, --metrics keeps its choices
    assert H.eval_parser("iid").parse_args(argv + ["--output_dir", "o"]).lpips_weights is None
    assert H.validate_iid_parser().parse_args(["--dataset_config", "c", "--base_data_dir", "d", "--output_dir", "o", "--denoise_steps", "4", "--processing_res", "0",
                                               "--ensemble_size", "1", "--lpips_weights", "x", "y"]).lpips_weights == ["x", "y"]
    for flags in (["--lpips_weights", "x"], ["--metrics", "lpips"]):
        with pytest.raises(SystemExit):
            H.eval_parser("iid").parse_args(argv + ["--output_dir", "o"] + flags)


# ---- the C contract ---------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("f16", [False, True])
def test_c_contract_without_a_gpu(f16):
    lib = L.load(f16)
    sizes = [lib.mg_lpips_workspace_bytes(h, w) for h, w in ((31, 31), (31, 64), (64, 80), (231, 300), (768, 1024))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert lib.mg_lpips_workspace_bytes(30, 64) == -1 and b"H, W >= 31" in lib.mg_last_error()
    header = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    assert header.index("int mg_eval_iid(") < header.index("long long mg_lpips_workspace_bytes(") < header.index("int mg_eval_iid_lpips(")
    a = 0x100000
    net = L.MgLpipsNet()
    for l in range(5):
        net.conv_w[l], net.conv_b[l], net.lin_w[l] = a, a, a
    need = lib.mg_lpips_workspace_bytes(31, 64)

    def call(net_=net, pred=a, gt=a, h=31, w=64, out=a, eval_ws=a, act=a, nbytes=need):
        return lib.mg_eval_iid_lpips(ctypes.byref(net_) if net_ is not None else None, pred, gt, None, h, w, 1, 0, out, eval_ws, act, nbytes, None)

    hollow = L.MgLpipsNet()
    for kw, msg in ((dict(net_=None), "null pointer"), (dict(pred=None), "null pointer"), (dict(gt=None), "null pointer"),
                    (dict(out=None), "null pointer"), (dict(eval_ws=None), "null pointer"), (dict(act=None), "null pointer"),
                    (dict(net_=hollow), "null pointer in the network"), (dict(h=30), "H, W >= 31"), (dict(h=64, w=30), "H, W >= 31"),
                    (dict(out=a + 4), "8-byte aligned"), (dict(pred=a + 2), "4-byte aligned"), (dict(act=a + 8), "16-byte aligned"),
                    (dict(nbytes=need - 1), "activation workspace too small")):
        assert call(**kw) == 2, kw
        assert msg in lib.mg_last_error().decode(), (kw, lib.mg_last_error())
