"""The two benchmark programs of the reference, per task (depth / normals / iid):

* ``infer_main``  - script/<task>/infer.py: run the pipeline over a dataset split and write one ``.npy``
  prediction per image under ``<output_dir>/<scene dirs of the rgb path>/``;
* ``eval_main``   - script/<task>/eval.py: read those predictions back, align (depth), score against
  the ground truth, write ``per_sample_metrics.csv`` and ``eval_metrics[-<alignment>].txt``.

Flags, file names and the text formats are the reference's.  What differs is the plumbing: samples are
decoded one image ahead on a host thread and predictions are written behind the GPU (the reference's
DataLoader(batch_size=1, num_workers=0) serialises decode -> predict -> save), and the scores are numpy
(see metrics.py).  Inference only runs on an MI355X - there is no CPU path.

One-pass validation (depth, normals): ``infer_main --evaluate`` scores every image on the GPU as it leaves the engine
(device.py; the reference's validation loop, src/trainer/marigold_depth_trainer.py:510-601) and writes the files of
``eval_main`` under ``--eval_output_dir``; ``eval_main --on_device`` runs the same scorer on read-back files.

One-pass validation (iid): ``validate_iid_main`` (script/iid/validate.py) - the reference's IID validation loop
(src/trainer/marigold_iid_trainer.py, ``validate``): every prediction is scored where the pipeline left it on the GPU
(``IIDEntry.device_array``, device.score_iid_sample) and the files of ``eval_main("iid")`` are written.  It is a program of its
own: ``infer_main("iid") --evaluate`` and ``eval_main("iid") --on_device`` keep refusing, as they always have.
"""
import argparse
import logging
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image
from tabulate import tabulate

from . import metrics as M
from .alignment import align_depth_least_square, depth2disparity, disparity2depth
from .datasets import DatasetMode, get_dataset, get_pred_name, load_dataset_config

_DEFAULT_CKPT = {"depth": "prs-eth/marigold-depth-v1-1", "normals": "prs-eth/marigold-normals-v1-1",
                 "iid": "prs-eth/marigold-iid-appearance-v1-1"}
_TASK = {"depth": "Monocular Depth Estimation", "normals": "Surface Normals Estimation",
         "iid": "Intrinsic Image Decomposition"}


def seed_all(seed=0):
    """src/util/seeding.py:31-39 (the engine itself draws from the per-image generator only)."""
    import random
    import torch
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


# ---- inference over a dataset ------------------------------------------------------------------------


def _model_arguments(p, kind):
    p.add_argument("--checkpoint", type=str, default=_DEFAULT_CKPT[kind], help="Checkpoint path or hub name.")
    p.add_argument("--dataset_config", type=str, required=True, help="Path to the config file of the evaluation dataset.")
    p.add_argument("--base_data_dir", type=str, required=True, help="Base path to the datasets.")
    p.add_argument("--output_dir", type=str, required=True, help="Output directory.")
    p.add_argument("--denoise_steps", type=int, required=True, help="Diffusion denoising steps.")
    p.add_argument("--processing_res", type=int, required=True,
                   help="Resolution the input is resized to before estimation; 0 = native.")
    p.add_argument("--ensemble_size", type=int, required=True, help="Number of predictions to be ensembled.")
    p.add_argument("--half_precision", "--fp16", action="store_true", help="Load the 16-bit weight variant.")
    p.add_argument("--tiny_vae", type=str, default=None, metavar="DIR",
                   help="Folder of a diffusers AutoencoderTiny: the pipeline encodes and decodes with it in place of the checkpoint's VAE.")


def _run_arguments(p):
    p.add_argument("--resample_method", choices=["bilinear", "bicubic", "nearest"], default="bilinear")
    p.add_argument("--seed", type=int, default=None, help="Reproducibility seed; None = time-seeded.")
    p.add_argument("--yes", action="store_true", help="Do not ask before writing into an existing output dir.")
    p.add_argument("--maps_in_flight", type=int, default=0,
                   help="Images on the GPU at a time (independent maps on concurrent HIP streams; results do not depend on it); "
                        "0 = the engine's default (maps_in_flight_for: 3 lanes while a program holds 8 members or fewer on this GPU, else 2).")
    p.add_argument("--images_per_program", type=int, default=1,
                   help="Consecutive images of one processed size that share one denoising program (their members batched); "
                        "1 = one image per program.")


def infer_parser(kind):
    p = argparse.ArgumentParser(description=f"Marigold : {_TASK[kind]} : Dataset Inference")
    _model_arguments(p, kind)
    p.add_argument("--output_processing_res", action="store_true",
                   help="Output at the processing resolution instead of resizing back to the input resolution.")
    _run_arguments(p)
    p.add_argument("--evaluate", action="store_true",
                   help="Score every prediction on the GPU as it is produced and write per_sample_metrics.csv and "
                        "eval_metrics[-<alignment>].txt like eval.py (depth and normals).")
    p.add_argument("--eval_output_dir", type=str, default=None, help="Where --evaluate writes; default <output_dir>/eval.")
    p.add_argument("--no_save_predictions", action="store_true", help="With --evaluate: do not write the .npy predictions.")
    if kind == "depth":
        _alignment_arguments(p)
    return p


def _iid_scoring_arguments(p, target_names=False):
    p.add_argument("--use_mask", action="store_true", help="Evaluate only in the masked region.")
    if target_names:
        p.add_argument("--target_names", nargs="+", default=["albedo", "material"], type=str,
                       help="A list of predicted targets to evaluate.")
    p.add_argument("--targets_to_eval_in_linear_space", nargs="*", default=[None], type=str,
                   help="Targets to evaluate in linear space (as opposed to sRGB by default).")
    p.add_argument("--metrics", nargs="+", default=["psnr", "ssim"], choices=["psnr", "ssim"],
                   help="(LPIPS of the reference needs pretrained network weights: give them with --lpips_weights)")
    p.add_argument("--lpips_weights", nargs=2, default=None, metavar=("BACKBONE", "LIN"), type=str,
                   help="Score LPIPS too, after each target's --metrics columns: the torchvision AlexNet state dict and the "
                        "lpips 'lin' layers' state dict (two .pth files; nothing is downloaded).")


def validate_iid_parser():
    """The flags of ``infer_parser("iid")`` that apply to a scored run (the output keeps the input's resolution: the ground
    truth has it) and the scoring flags of ``eval_parser("iid")``; the targets are the pipeline's."""
    p = argparse.ArgumentParser(description=f"Marigold : {_TASK['iid']} : One-Pass Validation")
    _model_arguments(p, "iid")
    _run_arguments(p)
    p.add_argument("--eval_output_dir", type=str, default=None, help="Where the metric files go; default <output_dir>/eval.")
    p.add_argument("--no_save_predictions", action="store_true", help="Do not write the .npy predictions.")
    _iid_scoring_arguments(p)
    return p


def _alignment_arguments(p):
    p.add_argument("--alignment", choices=[None, "least_square", "least_square_disparity"], default=None,
                   help="Method to estimate scale and shift between predictions and ground truth.")
    p.add_argument("--alignment_max_res", type=int, default=None, help="Max operating resolution used for LS alignment")


def _confirm_existing(directory, assume_yes):
    """script/depth/infer.py:165-183: ask before re-using an output folder."""
    while os.path.exists(directory) and not assume_yes:
        answer = input(f"The directory '{directory}' already exists. Are you sure to continue? (y/n): ").strip().lower()
        if answer == "y":
            return True
        if answer == "n":
            print("Exiting...")
            return False
        print("Invalid input. Please enter 'y' (for Yes) or 'n' (for No).")
    return True


def _pipeline_input(kind, sample):
    if kind == "iid":   # float [0,1] -> uint8 by truncation (marigold/util/image_util.py:137-141)
        return (sample["rgb"] * 255.0).astype(np.uint8)
    return sample["rgb_int"].astype(np.uint8)


def _prediction_files(kind, dataset, pipeline, rgb_rel, out):
    """[(relative file name, array)] of one pipeline output (depth infer.py:268-281, normals infer.py:258-270,
    iid infer.py:270-287)."""
    folder, base = os.path.dirname(rgb_rel), os.path.basename(rgb_rel)
    stem = os.path.splitext(base)[0]
    if kind == "depth":
        return [(os.path.join(folder, get_pred_name(base, dataset.name_mode, suffix=".npy")), out.depth_np)]
    if kind == "normals":
        return [(os.path.join(folder, stem + ".npy"), out.normals_np)]
    return [(os.path.join(folder, f"{stem}_{t}.npy"), out[t].array) for t in pipeline.target_names]


def _save_npy(path, arr):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    if os.path.exists(path):
        logging.warning(f"Existing file: '{path}' will be overwritten")
    np.save(path, arr)


def _load_pipeline(kind, args, pipeline):
    """The injected ``pipeline``, or the checkpoint of ``args`` on the GPU."""
    import torch
    if pipeline is None:
        pipeline = _checkpoint_pipeline(kind, args)
    if getattr(args, "tiny_vae", None):
        from ..cli import apply_tiny_vae
        apply_tiny_vae(pipeline, args.tiny_vae, args.half_precision)
    return pipeline


def _checkpoint_pipeline(kind, args):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: the Marigold HIP engine has no CPU fallback")
    import marigold_amd as MA
    cls = {"depth": MA.MarigoldDepthPipeline, "normals": MA.MarigoldNormalsPipeline,
           "iid": MA.MarigoldIIDPipeline}[kind]
    pipeline = cls.from_pretrained(args.checkpoint, variant="fp16" if args.half_precision else None,
                                   torch_dtype=torch.float16 if args.half_precision else torch.float32)
    return pipeline.to("cuda")


def _open_run(kind, args, mode):
    """Seed, output folder and dataset of a run over a dataset -> (seed, dataset), or None when the user keeps the folder."""
    logging.info(f"Inference settings: checkpoint = `{args.checkpoint}`, with denoise_steps = {args.denoise_steps}, "
                 f"ensemble_size = {args.ensemble_size}, processing resolution = {args.processing_res}, "
                 f"seed = {args.seed}; dataset config = `{args.dataset_config}`.")
    seed = int(time.time()) if args.seed is None else args.seed
    seed_all(seed)
    if not _confirm_existing(args.output_dir, args.yes):
        return None
    os.makedirs(args.output_dir, exist_ok=True)
    logging.info(f"output dir = {args.output_dir}")
    dataset = get_dataset(load_dataset_config(args.dataset_config), args.base_data_dir, mode)
    if dataset.spec.kind != kind:
        raise AssertionError(f"'{dataset.name}' is a {dataset.spec.kind} dataset, not {kind}")
    return seed, dataset


def _predict_dataset(kind, args, dataset, pipeline, seed, match_input_res, save=True, consume=None, score=None):
    """The loop ``infer_main`` and ``validate_iid_main`` share: samples decoded one image ahead on a reader thread, up to
    ``--maps_in_flight`` images on the GPU (``map_images``), predictions saved behind the GPU on writer threads.  ``score(sample,
    output, files)`` -> one ``(label, values)`` row per image, in input order; ``consume`` takes the iterator of those rows
    (the metric writer) while the loop runs."""
    import torch
    device = getattr(pipeline, "device", "cpu")
    n = len(dataset)
    t0 = time.perf_counter()
    kw = dict(denoising_steps=args.denoise_steps, ensemble_size=args.ensemble_size,
              processing_res=args.processing_res, match_input_res=match_input_res, batch_size=0,
              show_progress_bar=False, resample_method=args.resample_method)
    if kind == "depth":
        kw["color_map"] = None

    def generator_of():   # a fresh generator per image, seeded alike (script/depth/infer.py:186-190)
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        return g
    with ThreadPoolExecutor(max_workers=1) as reader, ThreadPoolExecutor(max_workers=2) as writer:
        samples = []   # in input order; the engine asks for the next image when a lane is free, results come back in order

        def images():
            pending = reader.submit(dataset.__getitem__, 0) if n else None
            for i in range(n):
                sample = pending.result()
                pending = reader.submit(dataset.__getitem__, i + 1) if i + 1 < n else None
                samples.append(sample)
                yield Image.fromarray(np.moveaxis(_pipeline_input(kind, sample), 0, -1))
        if hasattr(pipeline, "map_images"):   # the engine: up to --maps_in_flight images on the GPU at a time
            if args.images_per_program > 1:
                kw["images_per_program"] = args.images_per_program
            outs = pipeline.map_images(images(), in_flight=args.maps_in_flight or None, generators=(generator_of() for _ in range(n)), **kw)
        else:                                 # an object with the reference pipeline's call surface only
            outs = (pipeline(im, generator=generator_of(), **kw) for im in images())
        writes = []

        def results():   # saves each output behind the GPU; with a scorer yields its row
            for i, out in enumerate(outs):
                files = _prediction_files(kind, dataset, pipeline, samples[i]["rgb_relative_path"], out)
                if save:
                    for rel, arr in files:
                        writes.append(writer.submit(_save_npy, os.path.join(args.output_dir, rel), arr))
                if score is not None:
                    yield score(samples[i], out, files)
                samples[i] = None
        if consume is not None:
            consume(results())
        else:
            for _ in results():
                pass
        for w in writes:
            w.result()
    dt = time.perf_counter() - t0
    logging.info(f"{_TASK[kind]} inference on {dataset.disp_name}: {n} images in {dt:.1f} s "
                 f"({n / max(dt, 1e-9):.2f} img/s)")


def infer_main(kind, argv=None, pipeline=None) -> int:
    """``pipeline`` lets tests inject a ready pipeline object; otherwise the checkpoint is loaded onto the GPU."""
    logging.basicConfig(level=logging.INFO)
    args = infer_parser(kind).parse_args(argv)
    if args.ensemble_size > 15:
        logging.warning("Running with large ensemble size will be slow.")
    match_input_res = not args.output_processing_res
    if 0 == args.processing_res and match_input_res is False:
        logging.warning("Processing at native resolution without resizing output might NOT lead to exactly the "
                        "same resolution, due to the padding and pooling properties of conv layers.")
    if args.images_per_program < 1:
        raise ValueError(f"--images_per_program must be >= 1 (got {args.images_per_program})")
    if args.evaluate and kind == "iid":
        raise ValueError("--evaluate scores depth and normals only: the IID metrics (SSIM, quantile mapping) run on the host, "
                         "use script/iid/eval.py on the written predictions")
    if args.no_save_predictions and not args.evaluate:
        raise ValueError("--no_save_predictions without --evaluate would compute predictions and keep none of them")
    run = _open_run(kind, args, DatasetMode.EVAL if args.evaluate else DatasetMode.RGB_ONLY)   # (EVAL samples carry rgb_int + the ground truth)
    if run is None:
        return 0
    seed, dataset = run
    pipeline = _load_pipeline(kind, args, pipeline)
    if not args.evaluate:
        _predict_dataset(kind, args, dataset, pipeline, seed, match_input_res)
        return 0
    names = list(M.DEPTH_METRICS if kind == "depth" else M.NORMALS_METRICS)
    _predict_dataset(kind, args, dataset, pipeline, seed, match_input_res, save=not args.no_save_predictions,
                     score=lambda sample, out, files: _score_on_device(kind, args, dataset, sample, files[0][1], names),
                     consume=lambda rows: _write_eval_files(kind, args.eval_output_dir or os.path.join(args.output_dir, "eval"), dataset,
                                                            args.output_dir, names, rows, getattr(args, "alignment", None)))
    return 0


def _linear_targets(linear, target_names):
    """``--targets_to_eval_in_linear_space`` checked against the targets (script/iid/eval.py:96-103)."""
    for t in linear:
        if t is not None and t not in target_names:
            raise ValueError(f"'{t}' specified in targets_to_eval_in_linear_space does not belong to the "
                             f"predicted targets: target_names={target_names}")
    return linear


def validate_iid_main(argv=None, pipeline=None) -> int:
    """Predict and score an IID dataset in one pass: ``infer_main("iid")``'s run with every output scored on the GPU where the
    pipeline left it (``IIDEntry.device_array``: no upload of a prediction, one read-back of the scores per sample), and the
    ``per_sample_metrics.csv`` / ``eval_metrics.txt`` of ``eval_main("iid")`` written under ``--eval_output_dir``.  The targets are
    ``pipeline.target_names``."""
    from . import device as DV
    logging.basicConfig(level=logging.INFO)
    args = validate_iid_parser().parse_args(argv)
    if args.ensemble_size > 15:
        logging.warning("Running with large ensemble size will be slow.")
    if args.images_per_program < 1:
        raise ValueError(f"--images_per_program must be >= 1 (got {args.images_per_program})")
    pipeline = _load_pipeline("iid", args, pipeline)
    targets = list(pipeline.target_names)
    linear = _linear_targets(args.targets_to_eval_in_linear_space, targets)
    run = _open_run("iid", args, DatasetMode.EVAL)
    if run is None:
        return 0
    seed, dataset = run
    names = _iid_column_names(targets, args)
    extra = {}
    if args.lpips_weights:
        from .lpips_net import LpipsNet
        extra["lpips"] = LpipsNet.from_files(*args.lpips_weights)

    def score(sample, out, files):
        preds = {t: out[t].device_array if out[t].device_array is not None else out[t].array for t in targets}
        return sample["rgb_relative_path"], DV.score_iid_sample(preds, sample, targets, metrics=args.metrics, use_mask=args.use_mask,
                                                                 linear_targets=linear, dataset_name=dataset.name, **extra)
    _predict_dataset("iid", args, dataset, pipeline, seed, True, save=not args.no_save_predictions, score=score,
                     consume=lambda rows: _write_eval_files("iid", args.eval_output_dir or os.path.join(args.output_dir, "eval"), dataset,
                                                            args.output_dir, names, rows))
    return 0


# ---- evaluation ------------------------------------------------------------------------------------------


def eval_parser(kind):
    p = argparse.ArgumentParser(description=f"Marigold : {_TASK[kind]} : Metrics Evaluation")
    p.add_argument("--prediction_dir", type=str, required=True, help="Directory with predictions obtained from inference.")
    p.add_argument("--dataset_config", type=str, required=True, help="Path to the config file of the evaluation dataset.")
    p.add_argument("--base_data_dir", type=str, required=True, help="Base path to the datasets.")
    p.add_argument("--output_dir", type=str, required=True, help="Output directory.")
    if kind == "depth":
        _alignment_arguments(p)
    elif kind == "normals":
        p.add_argument("--use_mask", action="store_true", help="Evaluate only in the masked region.")
    else:
        _iid_scoring_arguments(p, target_names=True)
    p.add_argument("--no_cuda", action="store_true", help="(reference flag; scoring runs on the host here)")
    if kind != "iid":
        p.add_argument("--on_device", action="store_true",
                       help="Score on the GPU with the scorer of infer.py --evaluate (evaluation/device.py) instead of numpy.")
    return p


def align_and_clip_depth(depth_pred, depth_raw, valid_mask, dataset, alignment=None, alignment_max_res=None):
    """The per-sample preparation of script/depth/eval.py:176-212."""
    if alignment == "least_square":
        depth_pred, _, _ = align_depth_least_square(depth_raw, depth_pred, valid_mask, True, alignment_max_res)
    elif alignment == "least_square_disparity":
        gt_disp, gt_pos = depth2disparity(depth_raw, return_mask=True)
        ok = valid_mask & gt_pos & (depth_pred > 0)
        disp, _, _ = align_depth_least_square(gt_disp, depth_pred, ok, True, alignment_max_res)
        depth_pred = disparity2depth(np.clip(disp, a_min=1e-3, a_max=None))   # avoid 0 disparity
    depth_pred = np.clip(depth_pred, a_min=dataset.min_depth, a_max=dataset.max_depth)
    return np.clip(depth_pred, a_min=1e-6, a_max=None)


def _score_on_device(kind, args, dataset, data, pred, names):
    """(label, values) of one prediction from the GPU scorer: the rows ``_score_depth`` / ``_score_normals`` compute in numpy."""
    from . import device as DV
    rgb_name = data["rgb_relative_path"]
    if kind == "depth":
        label = os.path.join(os.path.dirname(rgb_name), get_pred_name(os.path.basename(rgb_name), dataset.name_mode, suffix=".npy"))
        res = DV.score_depth(pred, data["depth_raw_linear"].squeeze(), data["valid_mask_raw"].squeeze(), alignment=args.alignment,
                             alignment_max_res=args.alignment_max_res, min_depth=dataset.min_depth, max_depth=dataset.max_depth)
    else:
        label, res = rgb_name, DV.score_normals(pred, data["normals"], masked=True)
    return label, [res[n] for n in names]


def _score_depth(args, dataset, data, names):
    rgb_name = data["rgb_relative_path"]
    pred_name = os.path.join(os.path.dirname(rgb_name),
                             get_pred_name(os.path.basename(rgb_name), dataset.name_mode, suffix=".npy"))
    path = os.path.join(args.prediction_dir, pred_name)
    if not os.path.exists(path):
        logging.warning(f"Can't find prediction: {path}")
        return None
    if args.on_device:
        return _score_on_device("depth", args, dataset, data, np.load(path).astype(np.float32), names)
    gt, valid = data["depth_raw_linear"].squeeze(), data["valid_mask_raw"].squeeze()
    pred = align_and_clip_depth(np.load(path).astype(np.float32), gt, valid, dataset, args.alignment,
                                args.alignment_max_res)
    return pred_name, [getattr(M, n)(pred, gt, valid) for n in names]


def _score_normals(args, dataset, data, names):
    rgb_name = data["rgb_relative_path"]
    path = os.path.join(args.prediction_dir, os.path.splitext(rgb_name)[0] + ".npy")
    if not os.path.exists(path):
        logging.warning(f"Can't find prediction: {path}")
        return None
    if args.on_device:
        return _score_on_device("normals", args, dataset, data, np.load(path).astype(np.float32), names)
    err = M.compute_cosine_error(np.load(path).astype(np.float32), data["normals"], masked=True)
    return rgb_name, [getattr(M, n)(err) for n in names]


def _iid_column_names(targets, args):
    """Per target: the --metrics columns, then LPIPS when its weights were given (the reference's order: psnr, ssim, lpips)."""
    metrics = list(args.metrics) + (["lpips"] if getattr(args, "lpips_weights", None) else [])
    return [f"{m}_{t}" for t in targets for m in metrics]


def _score_iid(args, dataset, data, names):
    rgb_name = data["rgb_relative_path"]
    net = getattr(args, "lpips_net", None)
    metrics = list(args.metrics) + (["lpips"] if net is not None else [])
    stem = os.path.join(args.prediction_dir, os.path.splitext(rgb_name)[0])
    values = []
    for target in args.target_names:
        path = f"{stem}_{target}.npy"
        if not os.path.exists(path):
            # keep the columns aligned with `names` (metric-major per target): a missing target leaves empty cells
            # and is not counted in the averages (the reference updates its tracker by metric name too)
            logging.warning(f"Can't find prediction: {path}")
            values += [None] * len(metrics)
            continue
        pred, gt = np.load(path)[None].astype(np.float32), data[target][None].astype(np.float32)
        if target in args.targets_to_eval_in_linear_space:
            pred, gt = pred ** 2.2, gt ** 2.2
        if "hypersim" in dataset.name and len(args.target_names) == 3 and target == "albedo":
            pred, gt = pred ** (1.0 / 2.2), gt ** (1.0 / 2.2)
        mask = data["mask_" + target] if args.use_mask else None
        values += [M.compute_iid_metric(pred.copy(), gt.copy(), target, m, mask, **({"lpips_net": net} if m == "lpips" else {}))
                   for m in metrics]
    return rgb_name, values


def eval_main(kind, argv=None) -> int:
    logging.basicConfig(level=logging.INFO)
    args = eval_parser(kind).parse_args(argv)
    os.makedirs(args.output_dir, exist_ok=True)
    dataset = get_dataset(load_dataset_config(args.dataset_config), args.base_data_dir, DatasetMode.EVAL)
    if kind == "depth":
        names, score = list(M.DEPTH_METRICS), _score_depth
    elif kind == "normals":
        names, score = list(M.NORMALS_METRICS), _score_normals
    else:
        _linear_targets(args.targets_to_eval_in_linear_space, args.target_names)
        names, score = _iid_column_names(args.target_names, args), _score_iid
        if args.lpips_weights:
            from .lpips_net import LpipsNet
            args.lpips_net = LpipsNet.from_files(*args.lpips_weights)
    _write_eval_files(kind, args.output_dir, dataset, args.prediction_dir, names,
                      (score(args, dataset, data, names) for data in dataset), getattr(args, "alignment", None))
    return 0


def _write_eval_files(kind, output_dir, dataset, prediction_dir, names, scored, alignment=None):
    """``per_sample_metrics.csv`` and ``eval_metrics[-<alignment>].txt`` (script/depth/eval.py:139-245) from ``scored``, an
    iterable of ``(label, values)`` rows (None = prediction missing; a None value = an empty cell that is not averaged).
    The rows are written as they arrive.  Shared by ``eval_main`` and ``infer_main --evaluate``."""
    os.makedirs(output_dir, exist_ok=True)
    tracker = M.MetricTracker(*names)
    per_sample = os.path.join(output_dir, "per_sample_metrics.csv")
    with open(per_sample, "w+") as f:
        f.write("filename," + ",".join(names) + "\n")
        for row in scored:
            if row is None:
                continue
            label, values = row
            assert len(values) == len(names)
            for n, v in zip(names, values):
                if v is not None:
                    tracker.update(n, v)
            f.write(label + "," + ",".join("" if v is None else str(v) for v in values) + "\n")
    text = (f"Evaluation metrics:\n    of predictions: {prediction_dir}\n    on dataset: {dataset.disp_name}\n"
            f"    with samples in: {dataset.filename_ls_path}\n")
    if kind == "depth":
        text += f"min_depth = {dataset.min_depth}\nmax_depth = {dataset.max_depth}\n"
    result = tracker.result()
    text += tabulate([list(result.keys()), list(result.values())])
    name = "eval_metrics" + (f"-{alignment}" if kind == "depth" and alignment else "") + ".txt"
    with open(os.path.join(output_dir, name), "w+") as f:
        f.write(text)
    logging.info(f"Evaluation metrics saved to {os.path.join(output_dir, name)}")
    return os.path.join(output_dir, name)
