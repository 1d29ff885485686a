"""examples/host_focus.cpp on a real MI355X: a fresh process without Python - model image, picture bytes, seed, camera, near and far, a
focus pixel, an aperture and the largest radius in; a PPM out - writes, byte for byte, the picture of ``refocus(...)`` for
``pipe(image, generator=NativeNoise(seed), match_input_res=False)``, made from the picture's own colours."""
import functools
import subprocess

import numpy as np
import pytest
import torch

from tests import c_hosts
from tests.pipeline_outputs import _pil, _tiny_pipe

pytestmark = pytest.mark.gpu
SEED = (1 << 63) + 59


@functools.lru_cache(maxsize=None)
def _pipe():
    assert torch.cuda.is_available()
    return _tiny_pipe("depth")


@pytest.fixture(scope="module")
def host_focus(tmp_path_factory):
    return c_hosts.build_example("host_focus", tmp_path_factory.mktemp("host_focus"))


def test_c_host_focus(host_focus, tmp_path):
    """the tiny model's 64 x 128 image and a picture of that size"""
    from marigold_amd import NativeNoise, image, intrinsics_from_fov, refocus
    size = (64, 128)
    pipe, pil = _pipe(), _pil(*size)
    model, raw, ppm, ours = (str(tmp_path / n) for n in ("model.mgimg", "image.u8", "c.ppm", "py.ppm"))
    image.export_model_image(pipe, model, ensemble_size=1, height=64, width=128)
    np.asarray(pil).tofile(raw)
    fov, near, far, focus_at, aperture, max_radius = 63.5, 1.5, 7.25, (40, 100), 0.75, 12
    args = [host_focus, model, raw, str(size[0]), str(size[1]), str(SEED), repr(fov), repr(near), repr(far), str(focus_at[0]), str(focus_at[1]),
            repr(aperture), str(max_radius), ppm]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[focus C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    out = pipe(pil, processing_res=128, match_input_res=False, generator=NativeNoise(SEED), show_progress_bar=False)
    assert out.depth_np.shape == size
    planes = torch.from_numpy(np.array(pil.convert("RGB"))).cuda().permute(2, 0, 1).contiguous()
    shot = refocus(torch.from_numpy(out.depth_np).cuda(), planes, focus_at=focus_at, K=intrinsics_from_fov(*size, fov), aperture=aperture,
                   max_radius=max_radius, coef=(far - near, near)).to_host()
    shot.write_ppm(ours)
    got = open(ppm, "rb").read()
    assert got == open(ours, "rb").read() and got.startswith(b"P6\n128 64\n255\n") and len(got) == 14 + 3 * 64 * 128
    # the focus was good, something stayed sharp, something was blurred, and the picture changed
    assert shot.count["bad_focus"] == 0 and shot.count["usable"] == 64 * 128 and shot.count["sharp"] > 0
    assert shot.count["contributions"] > 2 * shot.count["usable"] and not np.array_equal(shot.rgb, np.array(pil.convert("RGB")))
