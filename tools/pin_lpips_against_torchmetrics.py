#!/usr/bin/env python
"""Pin ``evaluation.metrics.lpips`` against torchmetrics itself - ONE command, on a machine where ``import torchmetrics`` works
and the two pretrained files are at hand (neither is true where this project is built, so the definition in ``metrics.lpips`` is
restated from knowledge of ``LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True)`` and stays unpinned until this
has run).

    python tools/pin_lpips_against_torchmetrics.py BACKBONE.pth LIN.pth

BACKBONE: torchvision's AlexNet state dict (alexnet-owt-*.pth); LIN: the lpips package's lin layers for AlexNet (weights/v0.1/alex.pth,
which torchmetrics ships as well).  The script builds torchmetrics' metric with the pretrained weights it finds itself - the same
two files - and ``LpipsNet`` from the given paths, scores seeded image pairs with both, prints the differences and writes tests/golden/lpips_ref.npz: the pairs' sizes and seeds, small image pairs
themselves and torchmetrics' values - inputs and values only, no weights.  tests/test_lpips_host.py consumes the file when it is
present together with the two weight files named by MARIGOLD_LPIPS_BACKBONE / MARIGOLD_LPIPS_LIN, and says "unpinned" otherwise.
If the values differ, the constants to correct are the named ones at the top of the LPIPS section of evaluation/metrics.py.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((31, 31), (35, 47), (64, 80), (97, 131))


def pair(h, w):
    r = np.random.default_rng(1000 * h + w)
    g = r.uniform(0, 1, (3, h, w)).astype(np.float32)
    return np.clip(g + 0.1 * r.normal(size=g.shape), 0, 1).astype(np.float32), g


def main(backbone_path, lin_path, out_path):
    from torchmetrics.image import LearnedPerceptualImagePatchSimilarity
    from marigold_amd.evaluation import LpipsNet, metrics as M
    net = LpipsNet.from_files(backbone_path, lin_path)
    metric = LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True)   # its own pretrained weights: the same two files
    store, worst = {}, 0.0
    for h, w in SIZES:
        p, g = pair(h, w)
        with torch.no_grad():
            ref = float(metric(torch.from_numpy(p)[None], torch.from_numpy(g)[None]))
            metric.reset()
        ours = M.lpips(p[None], g[None], net)
        worst = max(worst, abs(ours - ref) / abs(ref))
        print(f"{h} x {w}: torchmetrics {ref:.9g}  metrics.lpips {ours:.9g}  relative difference {abs(ours - ref) / abs(ref):.3e}")
        store[f"pred_{h}x{w}"], store[f"gt_{h}x{w}"], store[f"lpips_{h}x{w}"] = p, g, np.float64(ref)
    store["sizes"] = np.asarray(SIZES)
    np.savez_compressed(out_path, **store)
    print(f"worst relative difference {worst:.3e}; wrote {out_path} ({os.path.getsize(out_path)} bytes)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("backbone")
    ap.add_argument("lin")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lpips_ref.npz"))
    a = ap.parse_args()
    main(a.backbone, a.lin, a.out)
