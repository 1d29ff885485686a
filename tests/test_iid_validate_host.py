"""Intrinsic images, the parts of the device output stage and of one-pass validation that need no GPU: the new op kind in the
header, the binding and both libraries, its contract through the library's dry run, the parser of ``validate_iid_main``, the
refusals that stay (``infer_main("iid") --evaluate``, ``eval_parser("iid") --on_device``), the numpy path of
``MarigoldIIDOutput.fill_entry`` behind a host pipeline, and the loop ``validate_iid_main`` shares with ``infer_main`` driven by a
stand-in pipeline with the device scorer replaced by the host scorer."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

from marigold_amd import _lib as L, ops, opstats
from marigold_amd.evaluation import harness as H
from marigold_amd.pipeline import MarigoldIIDOutput, MarigoldIIDPipeline
from oracle.make_eval_golden import write_synthetic_datasets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = {"target_names": ["albedo", "shading", "residual"], "albedo": {"prediction_space": "linear"},
         "shading": {"prediction_space": "linear", "up_to_scale": True},
         "residual": {"prediction_space": "srgb", "up_to_scale": True}}
REQ = ["--dataset_config", "c.yaml", "--base_data_dir", "d", "--output_dir", "o", "--denoise_steps", "4", "--processing_res", "0",
       "--ensemble_size", "1"]


# ---- the op ---------------------------------------------------------------------------------------------------------------


def test_op_kind_in_header_binding_and_opstats():
    header = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    every = [int(n) for n in re.findall(r"^\s*MG_OP_\w+ = (\d+)", header, flags=re.M)]
    assert len(every) == len(set(every))
    assert int(re.search(r"MG_OP_IID_VIS = (\d+)", header).group(1)) == L.OP_IID_VIS == max(every)   # appended: the next free number
    assert L.OP_NAMES[L.OP_IID_VIS] == "iid_vis"
    assert int(re.search(r"#define MG_IID_VIS_PARTS (\d+)", header).group(1)) == L.IID_VIS_PARTS
    assert re.search(r"#define MG_ABI_VERSION 4\b", header) and L.ABI_VERSION == 4   # additive: no version bump
    a = 0x10000
    op = ops.iid_vis(a, a, a, n=3, H=768, W=768, linear=[True, True, False], up_to_scale=[True, False, True])
    raw = ops.Raw(op)
    assert (raw.n, raw.h, raw.w, raw.linear_bits, raw.up_to_scale_bits) == (3, 768, 768, 0b011, 0b101)
    cls, flops, byts = opstats.op_cost(op)
    assert cls == "resize" and flops == 0
    assert byts == 3 * 768 * 768 * (3 * 5 + 4)   # fp32 in, one byte out per element; one target is read twice (its maximum)
    with pytest.raises(ValueError, match="flags"):
        ops.iid_vis(a, a, a, n=2, H=8, W=8, linear=[True], up_to_scale=[True, False])


def test_op_contract_dry_run_in_both_libraries():
    a = 0x10000
    for f16 in (False, True):
        seq = ops.OpSeq("iid_vis", f16=f16)
        seq.add(ops.iid_vis(a, a, a, n=3, H=768, W=768, linear=[True] * 3, up_to_scale=[True] * 3))
        seq.add(ops.iid_vis(a + 4, a + 1, None, n=1, H=11, W=13, linear=[True], up_to_scale=[False]))   # no maximum: no workspace
        seq.add(ops.iid_vis(a, a, None, n=2, H=1, W=1, linear=[False, False], up_to_scale=[True, True]))
        seq.validate()
        stray = ops.iid_vis(a, a, a, n=2, H=8, W=8, linear=[True, False], up_to_scale=[False, False])
        ops.Raw(stray).linear_bits = 0b100
        for op, msg in ((ops.iid_vis(a, a, None, n=1, H=8, W=8, linear=[True], up_to_scale=[True]), "workspace"),
                        (ops.iid_vis(a, a, a + 2, n=1, H=8, W=8, linear=[True], up_to_scale=[True]), "workspace"),
                        (ops.iid_vis(None, a, a, n=1, H=8, W=8, linear=[False], up_to_scale=[False]), "null"),
                        (ops.iid_vis(a, None, a, n=1, H=8, W=8, linear=[False], up_to_scale=[False]), "null"),
                        (ops.iid_vis(a + 2, a, a, n=1, H=8, W=8, linear=[False], up_to_scale=[False]), "4-byte aligned"),
                        (ops.iid_vis(a, a, a, n=1, H=0, W=8, linear=[False], up_to_scale=[False]), "bad size"),
                        (ops.iid_vis(a, a, a, n=17, H=8, W=8, linear=[False] * 17, up_to_scale=[False] * 17), "1 to 16 targets"),
                        (stray, "beyond")):
            s = ops.OpSeq("bad", f16=f16)
            s.add(op)
            with pytest.raises(L.MarigoldHipError, match=msg):
                s.validate()


def test_device_wrapper_refuses_host_tensors():
    from marigold_amd.util.image_util import iid_visualization_device
    with pytest.raises(AssertionError, match="fp32 CUDA"):
        iid_visualization_device(torch.zeros(1, 3, 4, 4), [False], [False])


# ---- the numpy path stays ------------------------------------------------------------------------------------------------


def _entry_as_before(pred, unc, name):
    """``fill_entry`` before the device stage existed, restated: (array, uint8 HWC picture, uncertainty)."""
    array = pred.squeeze().cpu().numpy()
    vis = array
    if PROPS[name].get("prediction_space", "srgb") == "linear":
        if PROPS[name].get("up_to_scale", False):
            vis = vis / max(vis.max(), 1e-6)
        vis = vis ** (1 / 2.2)
    return array, np.moveaxis((vis * 255).astype(np.uint8), 0, -1), None if unc is None else unc.squeeze().cpu().numpy()


@pytest.mark.parametrize("with_uncertainty", [False, True])
def test_host_prediction_goes_through_fill_entry_unchanged(with_uncertainty):
    g = torch.Generator().manual_seed(5)
    pred = torch.rand(1, 9, 12, 20, generator=g)
    unc = torch.rand(1, 9, 12, 20, generator=g) if with_uncertainty else None
    stand_in = SimpleNamespace(target_names=PROPS["target_names"], target_properties=PROPS, n_targets=3)
    out = MarigoldIIDOutput(PROPS["target_names"])
    MarigoldIIDPipeline.fill_outputs(stand_in, out, pred, unc)
    assert out.is_complete
    for i, name in enumerate(PROPS["target_names"]):
        array, picture, u = _entry_as_before(pred[:, 3 * i:3 * i + 3], None if unc is None else unc[:, 3 * i:3 * i + 3], name)
        e = out[name]
        assert e.array.dtype == np.float32 and e.array.shape == (3, 12, 20) and np.array_equal(e.array, array)
        assert isinstance(e.image, Image.Image) and e.image.mode == "RGB" and np.array_equal(np.asarray(e.image), picture)
        assert (e.uncertainty is None) if u is None else np.array_equal(e.uncertainty, u)
        assert e.device_array is None
    direct = MarigoldIIDOutput(PROPS["target_names"])
    direct.fill_entry("shading", pred[:, 3:6], None, PROPS)
    assert np.array_equal(np.asarray(direct["shading"].image), np.asarray(out["shading"].image)) and not direct.is_complete
    with pytest.raises(RuntimeError, match="already filled"):
        direct.fill_entry("shading", pred[:, 3:6], None, PROPS)
    with pytest.raises(KeyError, match="Unknown entry name"):
        direct.fill_entry("depth", pred[:, 3:6], None, PROPS)


# ---- the program ---------------------------------------------------------------------------------------------------------


def test_validate_parser():
    a = H.validate_iid_parser().parse_args(REQ)
    assert (a.checkpoint, a.half_precision, a.resample_method, a.seed, a.yes, a.maps_in_flight, a.images_per_program) == \
        ("prs-eth/marigold-iid-appearance-v1-1", False, "bilinear", None, False, 0, 1)
    assert (a.no_save_predictions, a.eval_output_dir, a.use_mask, a.targets_to_eval_in_linear_space, a.metrics) == \
        (False, None, False, [None], ["psnr", "ssim"])
    a = H.validate_iid_parser().parse_args(REQ + ["--fp16", "--seed", "3", "--yes", "--maps_in_flight", "2", "--images_per_program", "2",
                                                  "--no_save_predictions", "--eval_output_dir", "e", "--use_mask", "--resample_method", "bicubic",
                                                  "--targets_to_eval_in_linear_space", "shading", "residual", "--metrics", "psnr"])
    assert (a.half_precision, a.seed, a.yes, a.maps_in_flight, a.images_per_program, a.no_save_predictions, a.eval_output_dir, a.use_mask,
            a.resample_method, a.targets_to_eval_in_linear_space, a.metrics) == \
        (True, 3, True, 2, 2, True, "e", True, "bicubic", ["shading", "residual"], ["psnr"])
    # the targets are the pipeline's, the output keeps the input's resolution, and scoring is what the program is for
    for flag in (["--target_names", "albedo"], ["--output_processing_res"], ["--evaluate"], ["--on_device"], ["--metrics", "lpips"]):
        with pytest.raises(SystemExit):
            H.validate_iid_parser().parse_args(REQ + flag)
    # the scoring flags are eval_parser's own
    e = H.eval_parser("iid").parse_args(["--prediction_dir", "p"] + REQ[:6])
    assert (e.use_mask, e.targets_to_eval_in_linear_space, e.metrics, e.target_names) == (False, [None], ["psnr", "ssim"], ["albedo", "material"])


def test_the_cli_flags_still_exclude_iid(tmp_path):
    req = ["--dataset_config", str(tmp_path / "none.yaml"), "--base_data_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"),
           "--denoise_steps", "4", "--processing_res", "0", "--ensemble_size", "1"]
    with pytest.raises(ValueError, match="--evaluate scores depth and normals only: the IID metrics"):
        H.infer_main("iid", req + ["--evaluate"], pipeline=object())
    assert not (tmp_path / "o").exists()
    with pytest.raises(SystemExit):
        H.eval_parser("iid").parse_args(["--prediction_dir", "p"] + req[:6] + ["--on_device"])
    assert not hasattr(H.eval_parser("iid").parse_args(["--prediction_dir", "p"] + req[:6]), "on_device")


def test_linear_target_must_be_a_target(tmp_path):
    req = ["--dataset_config", str(tmp_path / "none.yaml"), "--base_data_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"),
           "--denoise_steps", "4", "--processing_res", "0", "--ensemble_size", "1"]
    pipe = SimpleNamespace(target_names=["albedo", "material"])
    with pytest.raises(ValueError, match=r"'shading' specified in targets_to_eval_in_linear_space does not belong to the predicted "
                                         r"targets: target_names=\['albedo', 'material'\]"):
        H.validate_iid_main(req + ["--targets_to_eval_in_linear_space", "shading"], pipeline=pipe)
    assert not (tmp_path / "o").exists()   # refused before anything is written
    with pytest.raises(ValueError, match="--images_per_program must be >= 1"):
        H.validate_iid_main(req + ["--images_per_program", "0"], pipeline=pipe)


def test_validate_loop_with_a_stand_in_pipeline(tmp_path, monkeypatch):
    """``validate_iid_main`` end to end on the host: a stand-in pipeline, the device scorer replaced by the host row
    (``harness._score_iid`` on the same arrays) - so its files must be those of ``infer_main`` + ``eval_main``, byte for byte."""
    from marigold_amd.evaluation import datasets as D, device as DV
    cfgs = write_synthetic_datasets(str(tmp_path))
    cfg_path = tmp_path / "i.yaml"
    cfg_path.write_text(yaml.safe_dump(cfgs["hypersim_iid"]))
    sample = D.get_dataset(cfgs["hypersim_iid"], str(tmp_path), D.DatasetMode.EVAL)[0]
    targets = PROPS["target_names"]
    calls = []

    class FakeIID:
        device = "cpu"
        target_names = targets

        def __call__(self, image, **kw):
            calls.append(kw)
            o = MarigoldIIDOutput(self.target_names)
            for t in self.target_names:
                o.fill_entry(t, torch.from_numpy(np.nan_to_num(sample[t]) * (0.5 if t != "albedo" else 0.9))[None], None, PROPS)
            return o

    def host_row(preds, data, target_names, *, metrics, use_mask, linear_targets, dataset_name, **kw):
        assert all(isinstance(preds[t], np.ndarray) for t in target_names)   # no device_array on a host pipeline: the arrays themselves
        stem = tmp_path / "row" / os.path.splitext(data["rgb_relative_path"])[0]
        os.makedirs(stem.parent, exist_ok=True)
        for t in target_names:
            np.save(f"{stem}_{t}.npy", preds[t])
        args = SimpleNamespace(prediction_dir=str(tmp_path / "row"), target_names=list(target_names), metrics=list(metrics),
                               use_mask=use_mask, targets_to_eval_in_linear_space=list(linear_targets))
        return H._score_iid(args, SimpleNamespace(name=dataset_name), data, None)[1]
    monkeypatch.setattr(DV, "score_iid_sample", host_row)
    base = ["--dataset_config", str(cfg_path), "--base_data_dir", str(tmp_path)]
    run = ["--denoise_steps", "4", "--processing_res", "0", "--ensemble_size", "1", "--seed", "1"]
    score = ["--use_mask", "--targets_to_eval_in_linear_space", "shading"]
    assert H.validate_iid_main(base + run + score + ["--output_dir", str(tmp_path / "v")], pipeline=FakeIID()) == 0
    assert calls[-1]["match_input_res"] is True and calls[-1]["denoising_steps"] == 4 and "color_map" not in calls[-1]
    assert H.infer_main("iid", base + run + ["--output_dir", str(tmp_path / "p")], pipeline=FakeIID()) == 0
    assert H.eval_main("iid", base + score + ["--prediction_dir", str(tmp_path / "p"), "--output_dir", str(tmp_path / "e"),
                                              "--target_names"] + targets) == 0
    names = sorted(os.listdir(tmp_path / "p" / "ai"))
    assert names == [f"rgb_cam_00_fr0000_{t}.npy" for t in sorted(targets)] and sorted(os.listdir(tmp_path / "v" / "ai")) == names
    for f in names:
        assert (tmp_path / "v" / "ai" / f).read_bytes() == (tmp_path / "p" / "ai" / f).read_bytes()
    assert sorted(os.listdir(tmp_path / "v" / "eval")) == sorted(os.listdir(tmp_path / "e")) == ["eval_metrics.txt", "per_sample_metrics.csv"]
    got, want = ((d / "per_sample_metrics.csv").read_text() for d in (tmp_path / "v" / "eval", tmp_path / "e"))
    assert got == want and got.startswith("filename,psnr_albedo,ssim_albedo,psnr_shading,ssim_shading,psnr_residual,ssim_residual\nai/rgb_cam_00_fr0000.png,")
    assert (tmp_path / "v" / "eval" / "eval_metrics.txt").read_text() == \
        (tmp_path / "e" / "eval_metrics.txt").read_text().replace(str(tmp_path / "p"), str(tmp_path / "v"))
    # scores only, somewhere else
    assert H.validate_iid_main(base + run + ["--output_dir", str(tmp_path / "w"), "--no_save_predictions", "--eval_output_dir",
                                             str(tmp_path / "w_eval"), "--metrics", "psnr"], pipeline=FakeIID()) == 0
    assert os.listdir(tmp_path / "w") == [] and sorted(os.listdir(tmp_path / "w_eval")) == ["eval_metrics.txt", "per_sample_metrics.csv"]
    assert (tmp_path / "w_eval" / "per_sample_metrics.csv").read_text().startswith("filename,psnr_albedo,psnr_shading,psnr_residual\n")
    launcher = open(os.path.join(ROOT, "script", "iid", "validate.py")).read()
    assert "validate_iid_main" in launcher and len(launcher.strip().split("\n")) == 11
