"""Depth to 3D behind the depth pipeline, on a real MI355X with the smallest synthetic checkpoint, E = 1, T = 1: ``pipe(image)``
followed by ``depth_to_points`` with the picture's colours is the restatement (tests/points_reference.py) applied to ``out.depth_np``;
and ``script/depth/run.py --save_points`` - through ``cli.main`` - writes under ``--maps_in_flight 2`` the file the serial call
writes, which is the file ``depth_to_points(...).write_ply`` writes for the same call made by hand."""
import functools
import os

import numpy as np
import pytest
import torch

from tests.pipeline_outputs import _pil, _tiny_pipe
from tests.points_reference import points_reference

pytestmark = pytest.mark.gpu
NEAR, FAR, EDGE, FOV = 2.0, 6.0, 0.25, 55.0   # (a wide edge rule: the synthetic checkpoint's maps are rough)


@functools.lru_cache(maxsize=None)
def _pipe():
    assert torch.cuda.is_available()
    return _tiny_pipe("depth")


def _ulps(got, want):
    def ordered(a):
        i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(got) - ordered(want))


def test_the_pipeline_s_map_as_a_cloud_is_the_restatement():
    from marigold_amd import NativeNoise, depth_to_normals, depth_to_points, intrinsics_from_fov
    pipe, pil = _pipe(), _pil(48, 64)
    out = pipe(pil, denoising_steps=1, ensemble_size=1, processing_res=0, generator=NativeNoise(11), show_progress_bar=False)
    depth = out.depth_np
    assert depth.shape == (48, 64) and depth.dtype == np.float32 and depth.max() > depth.min()
    picture = np.array(pil.convert("RGB"))
    K = intrinsics_from_fov(48, 64, FOV)
    dev = torch.from_numpy(depth).cuda()
    cloud = depth_to_points(dev, K, colors=torch.from_numpy(picture).cuda(), coef=(FAR - NEAR, NEAR), edge_rel=EDGE, normals=True, index=True).to_host()
    want = points_reference(depth, tuple(K), colors=picture, coef=(FAR - NEAR, NEAR), edge_rel=EDGE)
    assert (cloud.kept, cloud.written) == want.count and cloud.written <= depth.size
    assert np.array_equal(cloud.index, want.index) and np.array_equal(cloud.rgb, want.rgb)
    assert np.array_equal(cloud.xyz.view(np.uint32), want.xyz.view(np.uint32))
    assert _ulps(cloud.normals, want.nrm).max(initial=0) <= 1
    normals, valid = depth_to_normals(dev, K, coef=(FAR - NEAR, NEAR), edge_rel=EDGE)
    dense = points_reference(depth, tuple(K), coef=(FAR - NEAR, NEAR), edge_rel=EDGE, frame="marigold")
    everything = depth_to_points(dev, K, coef=(FAR - NEAR, NEAR)).to_host()   # no edge rule: every pixel of a map in [0, 1] is kept
    assert everything.written == depth.size and np.array_equal(everything.xyz[:, 2], (depth.astype(np.float64) * (FAR - NEAR) + NEAR).astype(np.float32).reshape(-1))
    assert np.array_equal(valid.cpu().numpy(), dense.valid != 0) and _ulps(normals.cpu().numpy(), dense.dense).max() <= 1


def test_the_command_line_writes_the_same_cloud_with_two_maps_in_flight(tmp_path):
    from marigold_amd import cli, depth_to_points, intrinsics_from_fov
    pipe = _pipe()
    inp = tmp_path / "in"
    inp.mkdir()
    pils = {"a": _pil(48, 64, seed=1), "b": _pil(48, 64, seed=2), "c": _pil(40, 72, seed=3)}
    for name, pil in pils.items():
        pil.save(inp / f"{name}.png")
    common = ["--input_rgb_dir", str(inp), "--denoise_steps", "1", "--ensemble_size", "1", "--processing_res", "0", "--seed", "5", "--save_points",
              "--fov_deg", str(FOV), "--points_near", str(NEAR), "--points_far", str(FAR), "--points_edge_rel", str(EDGE), "--points_normals"]
    files = {}
    for lanes in (1, 2):
        out = tmp_path / f"out{lanes}"
        assert cli.main("depth", common + ["--output_dir", str(out), "--maps_in_flight", str(lanes)], pipeline=pipe) == 0
        assert sorted(os.listdir(out / "depth_points")) == ["a_points.ply", "b_points.ply", "c_points.ply"]
        files[lanes] = {n: open(out / "depth_points" / f"{n}_points.ply", "rb").read() for n in pils}
    assert files[1] == files[2]
    # the same call by hand
    from PIL import Image
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    pil = Image.open(inp / "c.png")
    res = pipe(pil, denoising_steps=1, ensemble_size=1, processing_res=0, match_input_res=True, batch_size=0, show_progress_bar=False,
               resample_method="bilinear", color_map="Spectral", generator=g)
    cloud = depth_to_points(torch.from_numpy(res.depth_np).cuda(), intrinsics_from_fov(40, 72, FOV),
                            colors=torch.from_numpy(np.array(pil.convert("RGB"))).cuda().permute(2, 0, 1).contiguous(), coef=(FAR - NEAR, NEAR),
                            edge_rel=EDGE, normals=True)
    cloud.write_ply(tmp_path / "hand.ply")
    assert open(tmp_path / "hand.ply", "rb").read() == files[1]["c"]
