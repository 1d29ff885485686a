#!/usr/bin/env python
"""Pictures per second of the one-call C prediction (``mg_model_predict_out``) through 1, 2 and 3 handles driven at the same time,
each from its own host thread on its own stream: depth, 768 x 768, E = 1, T = 10 on the full architecture with synthetic weights.

Two ways of getting the handles alternate within one session on one box:

    replicas   one image of one configuration (``export_model_image(configs=[...])``), loaded once; lanes 2 and 3 are
               ``mg_model_replica`` handles over the same device-resident weights
    loaded     the single-configuration image of the same shape, loaded once per lane (every lane uploads its own weights):
               what a host did before replicas existed

Both images are exported to --dir (a few GB each, removed once loaded) and driven through ctypes, which releases the interpreter lock
for the length of a call: what a C host with a thread per lane does.  A visit of (way, lanes) starts the lanes' threads behind a
barrier; every thread makes --calls calls, each ending in a synchronise of its stream, the picture resident in HBM and the outputs
left on the device; the visit's rate is lanes x calls / wall time from the barrier to the last thread's end.  One warm-up visit per
(way, lanes), then --rounds rounds over all of them; the median rate of a (way, lanes) over the rounds is reported, with the
library's own accounting of the memory each way holds.  The box calibration of bench.py comes first.

    python tools/predict_lanes_bench.py
    python tools/predict_lanes_bench.py --lanes 1,2 --steps 4 --rounds 3
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JOIN_S = 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=str, default="1,2,3", help="handles driven at the same time, comma separated")
    ap.add_argument("--res", type=int, default=768)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ensemble", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6, help="timed calls per lane per visit")
    ap.add_argument("--dir", type=str, default=None, help="where the model images are written (default: a temporary directory)")
    ap.add_argument("--no-calibration", action="store_true")
    args = ap.parse_args()
    import torch
    import marigold_amd as M
    from marigold_amd import image, synthetic as syn
    lanes = [int(v) for v in args.lanes.split(",")]
    nmax = max(lanes)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pipe = M.build_synthetic_pipeline("depth", default_processing_resolution=0).to(dev)   # binds the library to the device
    if not args.no_calibration:
        from bench import calibration
        print("calibration " + json.dumps(calibration(dev)), flush=True)
    res, E, T = args.res, args.ensemble, args.steps
    hwc = [syn.synthetic_image(res, res, seed=s).to(dev)[0].permute(1, 2, 0).contiguous() for s in range(nmax)]   # uint8 [H,W,3]
    one = dict(ensemble_size=E, height=res, width=res, denoising_steps=T)
    handles = {}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, "configs.mgimg")
        t0 = time.perf_counter()
        info = image.export_model_image(pipe, path, configs=[one])
        parent = image.ModelImage(path)
        os.remove(path)
        handles["replicas"] = [parent] + [parent.replica() for _ in range(nmax - 1)]
        print(f"replicas: image of {info['file_bytes'] / 1e9:.2f} GB exported, loaded once and replicated {nmax - 1} time(s) in "
              f"{time.perf_counter() - t0:.1f} s; shared {parent.shared_bytes / 1e9:.2f} GB once, private {parent.device_bytes / 1e9:.2f} GB per handle, "
              f"{(parent.shared_bytes + sum(h.device_bytes for h in handles['replicas'])) / 1e9:.2f} GB in all", flush=True)
        path = os.path.join(d, "single.mgimg")
        t0 = time.perf_counter()
        info = image.export_model_image(pipe, path, **one)
        handles["loaded"] = [image.ModelImage(path) for _ in range(nmax)]
        os.remove(path)
        print(f"loaded: image of {info['file_bytes'] / 1e9:.2f} GB exported and loaded {nmax} time(s) in {time.perf_counter() - t0:.1f} s; "
              f"{handles['loaded'][0].device_bytes / 1e9:.2f} GB per handle, {sum(h.device_bytes for h in handles['loaded']) / 1e9:.2f} GB in all", flush=True)
    streams = [torch.cuda.Stream(dev) for _ in range(nmax)]

    def visit(way, n, calls):
        barrier, errors, ends = threading.Barrier(n + 1), [], [0.0] * n

        def lane(i):
            try:
                torch.cuda.set_device(dev)
                with torch.cuda.stream(streams[i]):
                    barrier.wait()
                    for c in range(calls):
                        handles[way][i].predict_out(hwc[i], 1000 + i)
                        streams[i].synchronize()
                ends[i] = time.perf_counter()
            except Exception as e:   # noqa: BLE001
                errors.append(e)
                barrier.abort()
        threads = [threading.Thread(target=lane, args=(i,), daemon=True) for i in range(n)]
        for t in threads:
            t.start()
        barrier.wait()
        t0 = time.perf_counter()
        for t in threads:
            t.join(JOIN_S)
            if t.is_alive():
                raise RuntimeError(f"{way}, {n} lanes: a lane did not finish within {JOIN_S} s")
        if errors:
            raise errors[0]
        return n * calls / (max(ends) - t0)

    rows = [(way, n) for n in lanes for way in ("replicas", "loaded")]
    rates = {r: [] for r in rows}
    for r in rows:
        visit(r[0], r[1], 2)
    for _ in range(args.rounds):
        for r in rows:
            rates[r].append(visit(r[0], r[1], args.calls))
    for r in rows:
        v = rates[r]
        med = statistics.median(v)
        print(f"{r[0]:9s} lanes={r[1]} E={E} T={T} {res}x{res}  {med:7.2f} pictures/s  {1e3 / med:7.2f} ms/picture  "
              f"(min {min(v):.2f}, max {max(v):.2f}, {len(v)} visits of {r[1] * args.calls} calls)", flush=True)
    for hs in handles.values():
        for h in reversed(hs):
            h.close()


if __name__ == "__main__":
    main()
