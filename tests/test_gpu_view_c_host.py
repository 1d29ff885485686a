"""examples/host_view.cpp on a real MI355X: a fresh process without Python - model image, picture bytes, seed, camera, near and far,
baseline and fill in; a PPM out - writes, byte for byte, the two pictures of ``stereo_pair(...)`` side by side for
``pipe(image, generator=NativeNoise(seed), match_input_res=False)``, drawn with the picture's own colours."""
import functools
import subprocess

import numpy as np
import pytest
import torch

from tests import c_hosts
from tests.pipeline_outputs import _pil, _tiny_pipe

pytestmark = pytest.mark.gpu
SEED = (1 << 63) + 53


@functools.lru_cache(maxsize=None)
def _pipe():
    assert torch.cuda.is_available()
    return _tiny_pipe("depth")


@pytest.fixture(scope="module")
def host_view(tmp_path_factory):
    return c_hosts.build_example("host_view", tmp_path_factory.mktemp("host_view"))


def test_c_host_view(host_view, tmp_path):
    """the tiny model's 64 x 128 image and a picture of that size"""
    from marigold_amd import NativeNoise, image, intrinsics_from_fov, stereo_pair
    from marigold_amd.view import write_ppm
    size = (64, 128)
    pipe, pil = _pipe(), _pil(*size)
    model, raw, ppm, ours = (str(tmp_path / n) for n in ("model.mgimg", "image.u8", "c.ppm", "py.ppm"))
    image.export_model_image(pipe, model, ensemble_size=1, height=64, width=128)
    np.asarray(pil).tofile(raw)
    fov, near, far, edge, baseline, fill = 63.5, 1.5, 7.25, 0.25, 0.4, 5
    args = [host_view, model, raw, str(size[0]), str(size[1]), str(SEED), repr(fov), repr(near), repr(far), repr(edge), repr(baseline), str(fill), ppm]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[view C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = pipe(pil, processing_res=128, match_input_res=False, generator=NativeNoise(SEED), show_progress_bar=False)
    assert out.depth_np.shape == size
    planes = torch.from_numpy(np.array(pil.convert("RGB"))).cuda().permute(2, 0, 1).contiguous()
    pair = [eye.to_host() for eye in stereo_pair(torch.from_numpy(out.depth_np).cuda(), intrinsics_from_fov(*size, fov), planes, baseline,
                                                 coef=(far - near, near), edge_rel=edge, fill_radius=fill)]
    write_ppm(ours, np.concatenate([eye.rgb for eye in pair], axis=1))
    got = open(ppm, "rb").read()
    assert got == open(ours, "rb").read() and got.startswith(b"P6\n256 64\n255\n") and len(got) == 14 + 3 * 64 * 256
    for eye in pair:   # something was drawn and something filled, and the two eyes differ
        assert eye.count["drawn"] > 0 and eye.count["covered"] == (eye.valid == 1).sum() > 0 and eye.count["filled"] == (eye.valid == 2).sum() > 0
    assert not np.array_equal(pair[0].rgb, pair[1].rgb)
