"""examples/host_mesh.cpp on a real MI355X: a fresh process without Python - model image, picture bytes, seed, camera, near and far in; a
PLY out - writes, byte for byte, the file ``depth_to_mesh(...).write_ply`` writes for
``pipe(image, generator=NativeNoise(seed), match_input_res=False)`` with the picture's colours resampled to the map's size."""
import functools
import subprocess

import numpy as np
import pytest
import torch

from tests import c_hosts
from tests.pipeline_outputs import _pil, _tiny_pipe

pytestmark = pytest.mark.gpu
SEED = (1 << 63) + 47


@functools.lru_cache(maxsize=None)
def _pipe():
    assert torch.cuda.is_available()
    return _tiny_pipe("depth")


@pytest.fixture(scope="module")
def host_mesh(tmp_path_factory):
    return c_hosts.build_example("host_mesh", tmp_path_factory.mktemp("host_mesh"))


@pytest.mark.parametrize("size,normals,edge", [((96, 192), 1, 0.25), ((64, 128), 0, 0.0)], ids=["resampled-normals", "own-size"])
def test_c_host_mesh(host_mesh, tmp_path, size, normals, edge):
    """a 64 x 128 model image; a 96 x 192 picture, which ``processing_res=128`` brings to that size by itself, and a picture of that size"""
    from marigold_amd import NativeNoise, depth_to_mesh, image, intrinsics_from_fov, read_mesh_ply, scale_intrinsics
    from marigold_amd.util.image_util import InterpolationMode, resize
    pipe, pil = _pipe(), _pil(*size)
    model, raw, ply, ours = (str(tmp_path / n) for n in ("model.mgimg", "image.u8", "c.ply", "py.ply"))
    image.export_model_image(pipe, model, ensemble_size=1, height=64, width=128)
    np.asarray(pil).tofile(raw)
    fov, near, far = 63.5, 1.5, 7.25
    args = [host_mesh, model, raw, str(size[0]), str(size[1]), str(SEED), repr(fov), repr(near), repr(far), repr(edge), str(normals), ply]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[mesh C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = pipe(pil, processing_res=128, match_input_res=False, generator=NativeNoise(SEED), show_progress_bar=False)
    assert out.depth_np.shape == (64, 128)
    K = intrinsics_from_fov(size[0], size[1], fov)
    planes = torch.from_numpy(np.array(pil.convert("RGB"))).cuda().permute(2, 0, 1).contiguous()
    if size != (64, 128):
        K = scale_intrinsics(K, size, (64, 128))
        planes = resize(planes, (64, 128), InterpolationMode.BILINEAR, antialias=True)
    depth_to_mesh(torch.from_numpy(out.depth_np).cuda(), K, colors=planes.contiguous(), coef=(far - near, near), edge_rel=edge,
                  normals=bool(normals)).write_ply(ours)
    assert open(ply, "rb").read() == open(ours, "rb").read()
    mesh = read_mesh_ply(ply)
    assert (mesh.normals is not None) == bool(normals) and mesh.faces.min(initial=0) >= 0 and mesh.faces.max(initial=0) < mesh.vertices_written
    if edge == 0.0:
        assert mesh.vertices_written == 64 * 128 and mesh.faces_written == 2 * 63 * 127
    else:
        assert mesh.vertices_written <= 64 * 128 and mesh.faces_written <= 2 * 63 * 127
