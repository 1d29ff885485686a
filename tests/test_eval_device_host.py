"""One-pass validation, the parts that need no GPU: the C ABI of the device scorer (header, binding, library), the op
contracts through the library's dry run, the new flags of the infer / eval programs and the writer they share."""
import ctypes
import os
import re

import numpy as np
import pytest
from tabulate import tabulate

from marigold_amd import _lib as L, ops
from marigold_amd.evaluation import harness as H, metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_eval_depth", "mg_eval_normals")


def test_abi_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in L.EXPORTS
        for f16 in (False, True):
            assert hasattr(L.load(f16), name), (name, f16)
    kinds = dict(re.findall(r"(MG_OP_EVAL_\w+) = (\d+)", header))
    assert kinds == {"MG_OP_EVAL_DEPTH_LS": "26", "MG_OP_EVAL_DEPTH_METRICS": "27", "MG_OP_EVAL_NORMALS": "28"}
    assert (L.OP_EVAL_DEPTH_LS, L.OP_EVAL_DEPTH_METRICS, L.OP_EVAL_NORMALS) == (26, 27, 28)
    assert int(re.search(r"#define MG_EVAL_WS_BYTES \((\d+) \* 1024\)", header).group(1)) * 1024 == L.EVAL_WS_BYTES
    assert re.search(r"#define MG_ABI_VERSION 4\b", header) and L.ABI_VERSION == 4   # additive: no version bump
    assert "evalscore.hip" in open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()


def test_fit_width_is_the_host_downscale():
    from marigold_amd.evaluation.alignment import _nearest_downscale
    for (h, w), res in (((37, 53), 37), ((37, 53), 20), ((120, 200), 64), ((480, 640), 320), ((768, 768), 500)):
        factor = float(np.min(res / np.array((h, w))))
        ow, inv = ops.eval_fit_width(h, w, res)
        cols = _nearest_downscale(np.arange(w)[None], factor)[0]
        assert ow == cols.size and inv == float(np.float32(1.0 / factor))
        got = np.minimum(np.floor(np.arange(ow, dtype=np.float32) * np.float32(inv)), w - 1).astype(np.int64)
        assert np.array_equal(got, cols)
    assert ops.eval_fit_width(37, 53, 64) == (0, 0.0) and ops.eval_fit_width(37, 53, None) == (0, 0.0)


def test_op_contracts_dry_run():
    """mg_program_validate runs each launcher's checks without touching a device."""
    a = 0x10000   # fake, aligned device addresses
    seq = ops.OpSeq("eval")
    seq.add(ops.eval_depth_ls(a, a, a, a, a, H=120, W=200, disparity=True, max_res=64))
    seq.add(ops.eval_depth_metrics(a, a, a, a, a, a, H=120, W=200, min_depth=1e-3, max_depth=float("inf")))
    seq.add(ops.eval_depth_metrics(a, a, a, None, a, a, H=120, W=200))
    seq.add(ops.eval_normals(a, a, a, None, a, HW=40 * 56))
    seq.add(ops.eval_normals(None, None, a, None, a, HW=0))
    seq.validate()
    bad = ops.eval_depth_ls(a, a, a, a, a, H=120, W=200)
    ops.Raw(bad).fit_w = 201   # sub-sampled width beyond the map's
    for op, msg in ((bad, "sub-sampled width"), (ops.eval_depth_ls(a, a, a, a + 4, a, H=8, W=8), "aligned"),
                    (ops.eval_depth_metrics(a, a, None, None, a, a, H=8, W=8), "null"),
                    (ops.eval_normals(a, a, a, None, None, HW=8), "null"),
                    (ops.eval_depth_metrics(a, a, a, None, a, a, H=0, W=8), "bad size")):
        s = ops.OpSeq("bad")
        s.add(op)
        with pytest.raises(L.MarigoldHipError, match=msg):
            s.validate()
    lib = L.load()
    assert lib.mg_eval_depth(a, a, a, 8, 8, 7, 0, ctypes.c_double(0), ctypes.c_double(1), a, a, None) != 0
    assert b"alignment" in lib.mg_last_error()


def test_flags():
    req = ["--dataset_config", "c.yaml", "--base_data_dir", "d", "--output_dir", "o", "--denoise_steps", "4",
           "--processing_res", "0", "--ensemble_size", "1"]
    a = H.infer_parser("depth").parse_args(req)
    assert (a.evaluate, a.eval_output_dir, a.no_save_predictions, a.alignment, a.alignment_max_res) == (False, None, False, None, None)
    a = H.infer_parser("depth").parse_args(req + ["--evaluate", "--alignment", "least_square_disparity", "--alignment_max_res", "320",
                                                  "--eval_output_dir", "e", "--no_save_predictions"])
    assert (a.evaluate, a.eval_output_dir, a.no_save_predictions, a.alignment, a.alignment_max_res) == \
        (True, "e", True, "least_square_disparity", 320)
    with pytest.raises(SystemExit):
        H.infer_parser("depth").parse_args(req + ["--alignment", "median"])
    n = H.infer_parser("normals").parse_args(req + ["--evaluate"])
    assert n.evaluate and not hasattr(n, "alignment")
    ereq = ["--prediction_dir", "p", "--dataset_config", "c.yaml", "--base_data_dir", "d", "--output_dir", "o"]
    assert H.eval_parser("depth").parse_args(ereq).on_device is False
    assert H.eval_parser("depth").parse_args(ereq + ["--on_device"]).on_device is True
    assert H.eval_parser("normals").parse_args(ereq + ["--on_device"]).on_device is True
    with pytest.raises(SystemExit):
        H.eval_parser("iid").parse_args(ereq + ["--on_device"])
    from marigold_amd import cli
    for parser in (H.infer_parser("depth"), cli.build_parser("depth")):   # the default is 3 for small ensembles
        text = " ".join(parser.format_help().split())
        assert "default (2)" not in text and "else 2" in text


def test_evaluate_rejects_iid_and_unsaved_unscored_runs(tmp_path):
    req = ["--dataset_config", str(tmp_path / "none.yaml"), "--base_data_dir", str(tmp_path), "--output_dir", str(tmp_path / "o"),
           "--denoise_steps", "4", "--processing_res", "0", "--ensemble_size", "1"]
    with pytest.raises(ValueError, match="--evaluate scores depth and normals only"):
        H.infer_main("iid", req + ["--evaluate"], pipeline=object())
    with pytest.raises(ValueError, match="--no_save_predictions without --evaluate"):
        H.infer_main("depth", req + ["--no_save_predictions"], pipeline=object())
    assert not (tmp_path / "o").exists()   # rejected before anything is written


class _Dataset:
    disp_name, filename_ls_path, min_depth, max_depth = "nyu_synth", "/data/split.txt", 1e-3, 10.0


def _files_as_eval_main_wrote_them(kind, out, prediction_dir, names, rows, alignment):
    """The tail of eval_main before the writer was factored out, restated: what the files must hold, byte for byte."""
    os.makedirs(out, exist_ok=True)
    tracker = M.MetricTracker(*names)
    with open(os.path.join(out, "per_sample_metrics.csv"), "w+") as f:
        f.write("filename," + ",".join(names) + "\n")
        for scored in rows:
            if scored is None:
                continue
            label, values = scored
            for n, v in zip(names, values):
                if v is not None:
                    tracker.update(n, v)
            f.write(label + "," + ",".join("" if v is None else str(v) for v in values) + "\n")
    text = (f"Evaluation metrics:\n    of predictions: {prediction_dir}\n    on dataset: {_Dataset.disp_name}\n"
            f"    with samples in: {_Dataset.filename_ls_path}\n")
    if kind == "depth":
        text += f"min_depth = {_Dataset.min_depth}\nmax_depth = {_Dataset.max_depth}\n"
    result = tracker.result()
    text += tabulate([list(result.keys()), list(result.values())])
    name = "eval_metrics" + (f"-{alignment}" if kind == "depth" and alignment else "") + ".txt"
    with open(os.path.join(out, name), "w+") as f:
        f.write(text)
    return name


@pytest.mark.parametrize("kind,alignment", [("depth", "least_square"), ("depth", None), ("normals", None), ("iid", None)])
def test_shared_writer_is_byte_identical(tmp_path, kind, alignment):
    r = np.random.default_rng(5)
    names = {"depth": list(M.DEPTH_METRICS), "normals": list(M.NORMALS_METRICS), "iid": ["psnr_albedo", "ssim_albedo"]}[kind]
    rows = [(f"test/kitchen/pred_{i:04d}.npy", [float(v) for v in r.uniform(0, 3, len(names))]) for i in range(4)]
    rows.insert(2, None)                                   # a missing prediction
    rows[3] = (rows[3][0], [None] + rows[3][1][1:])        # an empty cell (iid: a missing target)
    rows[1] = (rows[1][0], [round(v, 4) for v in rows[1][1]])
    name = _files_as_eval_main_wrote_them(kind, str(tmp_path / "want"), "/p/pred", names, rows, alignment)
    path = H._write_eval_files(kind, str(tmp_path / "got"), _Dataset, "/p/pred", names, iter(rows), alignment)
    assert os.path.basename(path) == name
    assert sorted(os.listdir(tmp_path / "got")) == sorted(os.listdir(tmp_path / "want")) == sorted(["per_sample_metrics.csv", name])
    for f in ("per_sample_metrics.csv", name):
        assert (tmp_path / "got" / f).read_bytes() == (tmp_path / "want" / f).read_bytes()
    assert (tmp_path / "got" / "per_sample_metrics.csv").read_text().startswith("filename," + ",".join(names) + "\n")
