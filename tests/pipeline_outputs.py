"""Digests of what the pipelines return on the GPU, to compare two trees over the same built libraries.  A plain helper module (not
collected), with a ``__main__``:

    python -m tests.pipeline_outputs --dump FILE      one line per output array or picture: ``name sha256 shape dtype``

A fixed matrix on the tiny synthetic models (tests/test_gpu_tiles.py::_tiny_pipe), 64 x 128 synthetic pictures, two steps, the
library's own noise generator (``NativeNoise`` seeds only - nothing depends on torch's generator): the lone call of the three kinds
over ensemble size, processing resolution and ``match_input_res``; depth with and without a colour map, with uncertainty, with the LCM
scheduler, with the members in two batches; ``map_images`` and ``map_video`` over lanes and images per program; ``predict_tiled``.
Two trees that compute the same write byte-identical files.  No digest is kept in the repository: any kernel change moves them."""
import argparse
import dataclasses
import hashlib

import numpy as np
import torch
from PIL import Image

SEED = (1 << 63) + 31
KINDS = ("depth", "normals", "iid")


def _tiny_pipe(kind, scheduler=None):
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=scheduler, default_denoising_steps=2,
                                      default_processing_resolution=0).to("cuda:0")


def _pil(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).numpy())


def _line(name, value):
    if value is None:
        return f"{name} none - -"
    a = np.ascontiguousarray(np.asarray(value))
    return f"{name} {hashlib.sha256(a.tobytes()).hexdigest()} {'x'.join(map(str, a.shape)) or 'scalar'} {a.dtype}"


def _lines(name, out):
    """Every array and picture of one output."""
    if hasattr(out, "depth_np"):
        fields = [("depth_np", out.depth_np), ("depth_colored", out.depth_colored), ("uncertainty", out.uncertainty),
                  ("degenerate_tiles", out.degenerate_tiles)]
    elif hasattr(out, "normals_np"):
        fields = [("normals_np", out.normals_np), ("normals_img", out.normals_img), ("uncertainty", out.uncertainty)]
    else:
        fields = [(f"{e.name}.{f}", getattr(e, f)) for e in out for f in ("array", "image", "uncertainty")]
    return [_line(f"{name}/{f}", v) for f, v in fields]


def matrix():
    """-> the lines of the dump, in a fixed order"""
    from marigold_amd import NativeNoise
    from marigold_amd.schedulers import LCMScheduler
    lines = []
    pil = _pil(64, 128)
    pipes = {kind: _tiny_pipe(kind) for kind in KINDS}

    def call(name, pipe, **kw):
        lines.extend(_lines(name, pipe(pil, generator=NativeNoise(SEED), **kw)))

    for kind, pipe in pipes.items():
        for E in (1, 3):
            for res in (0, 48):
                for match in (True, False):
                    call(f"{kind}/E={E}/res={res}/match={int(match)}", pipe, ensemble_size=E, processing_res=res, match_input_res=match)
        call(f"{kind}/E=3/batch_size=2", pipe, ensemble_size=3, batch_size=2)
        call(f"{kind}/E=3/res=48/uncertainty", pipe, ensemble_size=3, processing_res=48, ensemble_kwargs=dict(output_uncertainty=True))
    depth = pipes["depth"]
    for cmap in ("Spectral", None):
        call(f"depth/E=1/color_map={cmap}", depth, color_map=cmap)
        call(f"depth/E=3/res=48/color_map={cmap}", depth, ensemble_size=3, processing_res=48, color_map=cmap)
    lcm = _tiny_pipe("depth", LCMScheduler())
    for E in (1, 3):
        call(f"depth-lcm/E={E}", lcm, ensemble_size=E)
    call("depth-lcm/E=3/batch_size=2", lcm, ensemble_size=3, batch_size=2)

    pictures = [_pil(64, 128, seed=10 + i) for i in range(3)] + [_pil(48, 96, seed=10 + i) for i in (3, 4)]   # a change of size
    frames = [_pil(64, 128, seed=20 + i) for i in range(4)]
    for kind, pipe in pipes.items():
        for E in (1, 2):
            for lanes in (1, 3):
                for k in (1, 2):
                    outs = pipe.map_images(pictures, in_flight=lanes, images_per_program=k, ensemble_size=E,
                                           generators=[NativeNoise(SEED + 1 + i) for i in range(5)])
                    for i, out in enumerate(outs):
                        lines.extend(_lines(f"map_images/{kind}/E={E}/in_flight={lanes}/per_program={k}/{i}", out))
                outs = pipe.map_video(frames, in_flight=lanes, ensemble_size=E, generators=[NativeNoise(SEED + 7 + i) for i in range(4)])
                for i, out in enumerate(outs):
                    lines.extend(_lines(f"map_video/{kind}/E={E}/in_flight={lanes}/{i}", out))

    large = _pil(128, 256)
    for kind in ("depth", "normals"):
        for E in (1, 2):
            for match in (True, False):
                out = pipes[kind].predict_tiled(large, tile_size=(64, 128), tile_overlap=(16, 32), guide_res=128,tiled_res=0 if match else 192,
                                                match_input_res=match, ensemble_size=E, generator=NativeNoise(SEED))
                lines.extend(_lines(f"predict_tiled/{kind}/E={E}/match={int(match)}", out))
        out = pipes[kind].predict_tiled(pil, tile_size=128, tile_overlap=32, generator=NativeNoise(SEED))
        lines.extend(_lines(f"predict_tiled/{kind}/one-tile", out))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", required=True, metavar="FILE")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    lines = matrix()
    with open(args.dump, "w") as f:
        f.write("\n".join(lines) + "\n")
    import marigold_amd.pipeline
    print(f"{len(lines)} lines -> {args.dump} (pipelines of {marigold_amd.pipeline.__file__})")


if __name__ == "__main__":
    main()
