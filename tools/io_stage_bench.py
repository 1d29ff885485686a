#!/usr/bin/env python
"""Times the device I/O stages on the GPU box against the host code they replace on a CUDA pipeline, alternating, on the same
seeded data.

* input: ``_preprocess`` of a PIL image through MG_OP_RGB_PREP (``device_io_stages = True``) and through the host branch (``False``:
  ``pil_to_tensor``, the device resample where the size changes, torch's normalisation, the range assert).  Host clock around work
  that ends where ``single_infer`` starts computing: the normalised image on the device (the host branch's upload included) and the
  stream drained.  The time inside ``_preprocess`` alone is reported too - what a lane thread spends before it hands over.
* normals output: ``MarigoldNormalsPipeline._tail`` (``_finish``'s end) of a CUDA prediction through MG_OP_NORMALS_VIS and through the numpy lines; host
  clock around work that ends in the read-backs.
* the launches alone by device events.

Shapes: 768 x 768 (no resample) and 375 x 1242 -> 231 x 768 (bilinear).  The first line of the log is the box's calibration
(``mg_clock_probe``: shader clock and matrix rate under load).  Needs an MI355X.

    python tools/io_stage_bench.py [--rounds 200] [--log profiles/io_stages.log]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

WARM = 5


def _stat(v):
    return f"{statistics.median(v):7.3f}  ({min(v):.3f} - {max(v):.3f})"


def _alternate(rounds, pairs):
    """pairs: [(label, fn)] -> {label: [ms]}; fn() does the work and returns when it is complete."""
    times = {label: [] for label, _ in pairs}
    for r in range(rounds + WARM):
        for label, fn in pairs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARM:
                times[label].append(dt)
    return times


def _events(rounds, fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for r in range(rounds + WARM):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        if r >= WARM:
            out.append(ev[0].elapsed_time(ev[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--log", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("no MI355X visible: nothing to measure")
    from marigold_amd import _lib as L
    from marigold_amd.pipeline import MarigoldNormalsPipeline, _MarigoldPipelineBase
    from marigold_amd.util.image_util import InterpolationMode, normals_visualization_device, prepare_rgb_device
    from marigold_amd.util.host import usable_cores
    torch.set_num_threads(min(16, usable_cores()))
    lib = L.init(0)
    mhz, tflops = ctypes.c_double(), ctypes.c_double()
    L.check(lib.mg_clock_probe(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 0, ctypes.byref(mhz), ctypes.byref(tflops)),
            "mg_clock_probe", lib)
    lines = [f"calibration of this box (mg_clock_probe, random operands): shader clock {mhz.value:.0f} MHz under matrix load, "
             f"{tflops.value:.0f} TFLOP/s bf16 MFMA chain; torch {torch.__version__}, {usable_cores()} usable host cores, "
             f"{torch.get_num_threads()} torch threads",
             f"{args.rounds} alternating rounds after {WARM} warm-up rounds; ms, median (min - max)"]
    dev = torch.device("cuda:0")

    def stand_in(on):
        s = SimpleNamespace(device=dev, io_dtype=torch.float32, device_io_stages=on)
        s._preprocess_device = lambda *a: _MarigoldPipelineBase._preprocess_device(s, *a)
        return s
    g = torch.Generator().manual_seed(0)
    for (h, w), res in (((768, 768), 0), ((375, 1242), 768)):
        pil = Image.fromarray(torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy())
        inside = {True: [], False: []}

        def prep(on, pil=pil, res=res, inside=inside):
            t0 = time.perf_counter()
            rgb, _ = _MarigoldPipelineBase._preprocess(stand_in(on), pil, res, InterpolationMode.BILINEAR)
            inside[on].append((time.perf_counter() - t0) * 1e3)
            rgb = rgb.to(dev)
            torch.cuda.synchronize()
            return rgb
        t = _alternate(args.rounds, [("host branch", lambda: prep(False)), ("device stage", lambda: prep(True))])
        same = torch.equal(prep(False), prep(True))
        u8 = torch.from_numpy(np.array(pil)).to(dev)
        size = None if res == 0 else (231, 768)
        kernel = _events(args.rounds, lambda: prepare_rgb_device(u8, size, InterpolationMode.BILINEAR, torch.float32, True))
        lines.append(f"input stage, PIL {h} x {w}" + (f" -> {size[0]} x {size[1]} (bilinear)" if size else " (same size)") + ":")
        lines.append(f"  {'host branch, to device':32s} {_stat(t['host branch'])}")
        lines.append(f"  {'device stage, to device':32s} {_stat(t['device stage'])}")
        lines.append(f"  {'host branch, in _preprocess':32s} {_stat(inside[False][WARM:args.rounds + WARM])}")
        lines.append(f"  {'device stage, in _preprocess':32s} {_stat(inside[True][WARM:args.rounds + WARM])}")
        lines.append(f"  {'MG_OP_RGB_PREP launches':32s} {_stat(kernel)}   (device events, picture already on the device)")
        lines.append(f"  results identical: {same}")
    for h, w in ((768, 768), (375, 1242)):
        pred = torch.nn.functional.normalize(torch.randn(1, 3, h, w, generator=g), dim=1).to(dev)

        def finish(on, pred=pred):
            return MarigoldNormalsPipeline._tail(SimpleNamespace(device_io_stages=on), pred, None)
        t = _alternate(args.rounds, [("numpy", lambda: finish(False)), ("device", lambda: finish(True))])
        a, b = finish(False), finish(True)
        same = np.array_equal(a.normals_np, b.normals_np) and np.array_equal(np.asarray(a.normals_img), np.asarray(b.normals_img))
        kernel = _events(args.rounds, lambda: normals_visualization_device(pred[0]))
        lines.append(f"normals output, 3 x {h} x {w}, _finish to its read-backs:")
        lines.append(f"  {'numpy lines':32s} {_stat(t['numpy'])}")
        lines.append(f"  {'device stage':32s} {_stat(t['device'])}")
        lines.append(f"  {'MG_OP_NORMALS_VIS launch':32s} {_stat(kernel)}   (device events)")
        lines.append(f"  results identical: {same}")
    text = "\n".join(lines)
    print(text)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
