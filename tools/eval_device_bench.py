#!/usr/bin/env python
"""The device scorer (marigold_amd/evaluation/device.py) measured: its deviation from the reference's numbers, its cost per
image beside the host scorer's, and what one-pass validation buys the dataset protocol.

    python tools/eval_device_bench.py parity      # per case and score: relative deviation from tests/golden/eval_ref.npz
    python tools/eval_device_bench.py scorer      # ms per image: host align + clip + ten scores | device score_depth (upload + sync)
    python tools/eval_device_bench.py protocol    # images/s at 768 x 768, E = 1, T = 4 / 10, --images_per_program 8:
                                                  # infer | infer then eval | infer --evaluate --no_save_predictions

``protocol`` writes a synthetic ScanNet-layout split (16-bit PNG depth) into a temporary folder and runs the programs of
evaluation/harness.py on the full architecture with synthetic weights; every variant runs once to warm up, then timed.
"""
import argparse
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parity():
    from marigold_amd.evaluation import metrics as M, score_depth
    from oracle.make_eval_golden import eval_inputs
    gold = np.load(os.path.join(ROOT, "tests", "golden", "eval_ref.npz"))
    cases = eval_inputs()
    worst = {}
    for key in ("depth_a", "depth_b", "depth_big"):
        c = cases[key]
        for tag, mask, names in (("masked", c["mask"], M.DEPTH_METRICS),
                                 ("nomask", np.ones_like(c["mask"]), [n for n in M.DEPTH_METRICS if not n.startswith("delta")])):
            got = score_depth(c["pred"], c["gt"], mask)
            host = [getattr(M, n)(c["pred"], c["gt"], mask) for n in names]
            for n, w, h in zip(names, gold[f"{key}/metrics_{tag}"], host):
                dev, hdev = abs(got[n] - w) / abs(w), abs(h - w) / abs(w)
                worst[n] = max(worst.get(n, 0.0), dev)
                print(f"{key:9s} {tag:6s} n={got['n']:6d} {n:27s} device {got[n]:.12g} reference {float(w):.12g} "
                      f"rel.dev device {dev:.2e} host {hdev:.2e}")
    print("largest relative deviation of the device scorer from the reference, per score:")
    for n in M.DEPTH_METRICS:
        print(f"  {n:27s} {worst[n]:.2e}")


def _median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def scorer(reps):
    import torch
    from marigold_amd.evaluation import harness as H, metrics as M, score_depth, score_normals

    class Clip:
        min_depth, max_depth = 1e-3, 10.0
    r = np.random.default_rng(1)
    for h, w in ((480, 640), (768, 768)):
        gt = r.uniform(0.3, 12.0, (h, w)).astype(np.float32)
        mask = r.uniform(size=(h, w)) > 0.2
        rel = ((gt.max() - gt) / (gt.max() - gt.min()) * 0.9 + 0.05 + r.normal(0, 0.01, (h, w))).astype(np.float32)

        def host():
            p = H.align_and_clip_depth(rel, gt, mask, Clip, "least_square", None)
            return [getattr(M, n)(p, gt, mask) for n in M.DEPTH_METRICS]

        def device():
            return score_depth(rel, gt, mask, alignment="least_square", min_depth=Clip.min_depth, max_depth=Clip.max_depth)
        dgt, dmask = torch.from_numpy(gt).cuda(), torch.from_numpy(mask).cuda()

        def device_gt_resident():
            return score_depth(rel, dgt, dmask, alignment="least_square", min_depth=Clip.min_depth, max_depth=Clip.max_depth)
        for name, fn in (("host  align_and_clip_depth + ten scores (numpy, one thread)", host),
                         ("device score_depth, numpy pred / gt / mask (3 uploads + sync)", device),
                         ("device score_depth, numpy pred, gt / mask resident", device_gt_resident)):
            med, best = _median_ms(fn, reps)
            print(f"depth   {h}x{w} least_square  {name:62s} median {med:7.3f} ms  min {best:7.3f} ms", flush=True)
        g = r.normal(size=(3, h, w)).astype(np.float32)
        p = g + r.normal(0, 0.3, g.shape).astype(np.float32)

        def nhost():
            e = M.compute_cosine_error(p, g, masked=True)
            return [getattr(M, n)(e) for n in M.NORMALS_METRICS]
        for name, fn in (("host  compute_cosine_error + seven scores", nhost), ("device score_normals, numpy pred / gt", lambda: score_normals(p, g))):
            med, best = _median_ms(fn, reps)
            print(f"normals {h}x{w}               {name:62s} median {med:7.3f} ms  min {best:7.3f} ms", flush=True)


def _png(a, mode=None):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(a, mode).save(b, format="PNG", compress_level=1)
    return b.getvalue()


def protocol(images, res):
    import yaml
    import marigold_amd as MA
    from marigold_amd.evaluation import harness as H
    pipe = MA.build_synthetic_pipeline("depth", default_processing_resolution=0).to("cuda:0")
    r = np.random.default_rng(3)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "scannet", "s"))
        lines = []
        for i in range(images):
            for name, data in ((f"color_{i}.png", _png(r.integers(0, 256, (res, res, 3)).astype(np.uint8))),
                               (f"depth_{i}.png", _png(r.integers(0, 12000, (res, res)).astype(np.uint16)))):
                with open(os.path.join(tmp, "scannet", "s", name), "wb") as f:
                    f.write(data)
            lines.append(f"s/color_{i}.png s/depth_{i}.png")
        split = os.path.join(tmp, "split.txt")
        with open(split, "w") as f:
            f.write("\n".join(lines) + "\n")
        cfg = os.path.join(tmp, "scannet.yaml")
        with open(cfg, "w") as f:
            yaml.safe_dump(dict(name="scannet_depth", disp_name="scannet_synth", dir="scannet", filenames=split), f)
        base = ["--dataset_config", cfg, "--base_data_dir", tmp]
        for T in (4, 10):
            run = base + ["--denoise_steps", str(T), "--processing_res", "0", "--ensemble_size", "1", "--seed", "1",
                          "--images_per_program", "8", "--yes"]
            out = os.path.join(tmp, f"pred_T{T}")

            def infer():
                H.infer_main("depth", run + ["--output_dir", out], pipeline=pipe)

            def evaluate():
                H.eval_main("depth", base + ["--prediction_dir", out, "--output_dir", os.path.join(tmp, f"ev_T{T}"),
                                             "--alignment", "least_square"])

            def one_pass():
                H.infer_main("depth", run + ["--output_dir", os.path.join(tmp, f"one_T{T}"), "--evaluate", "--alignment",
                                             "least_square", "--no_save_predictions"], pipeline=pipe)
            t = {}
            for name, fn in (("infer", infer), ("eval", evaluate), ("one_pass", one_pass)):
                fn()   # warm-up: programs built, files in the page cache
                t0 = time.perf_counter()
                fn()
                t[name] = time.perf_counter() - t0
            print(f"{res}x{res} E=1 T={T:2d} images_per_program=8, {images} images (wall clock, PNG decode included):\n"
                  f"  infer (writes .npy)                          {t['infer']:6.2f} s  {images / t['infer']:6.2f} images/s\n"
                  f"  eval (host scorer, reads .npy)               {t['eval']:6.2f} s  {t['eval'] / images * 1e3:6.2f} ms/image\n"
                  f"  infer then eval                              {t['infer'] + t['eval']:6.2f} s  {images / (t['infer'] + t['eval']):6.2f} images/s\n"
                  f"  infer --evaluate --no_save_predictions       {t['one_pass']:6.2f} s  {images / t['one_pass']:6.2f} images/s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["parity", "scorer", "protocol"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--res", type=int, default=768)
    a = ap.parse_args()
    {"parity": parity, "scorer": lambda: scorer(a.reps), "protocol": lambda: protocol(a.images, a.res)}[a.what]()
