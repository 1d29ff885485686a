"""``guided_upsample=`` of the three pipelines on a real MI355X: the call against a composition written out here - the pipeline's own
device prediction at the processed size, ``marigold_amd.guided.guided_upsample`` against the input picture's bytes, the kind's tail -
bit for bit; the keyword left at its default changes nothing; ``map_images`` (with ``images_per_program``) and ``map_video`` carry it;
every refusal; and examples/host_guided.cpp, a fresh process, writes the arrays the pipeline returns.

The bound is equality everywhere: both sides run the same kernels on the same inputs in the same order.  The models are the tiny
synthetic ones of tests/pipeline_outputs.py, two steps; pictures of 64 x 128 processed at 24 x 48, so the enlargement is 8/3 per side."""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import c_hosts
from tests.pipeline_outputs import _lines, _pil, _tiny_pipe

pytestmark = pytest.mark.gpu
SEED = (1 << 63) + 47
RES = 48
KINDS = ("depth", "normals", "iid")


@functools.lru_cache(maxsize=None)
def _pipe(kind):
    assert torch.cuda.is_available()
    return _tiny_pipe(kind)


def _noise(seed=SEED):
    from marigold_amd import NativeNoise
    return NativeNoise(seed)


def _same(a, b, what):
    la, lb = _lines(what, a), _lines(what, b)
    assert la == lb, [(x, y) for x, y in zip(la, lb) if x != y][:3]


def _composed(pipe, pil, guided, seed=SEED, **kw):
    """The call's definition, step by step: the unclipped ensembled prediction on the device at the processed size (the pipeline's own
    call with ``match_input_res=False``, stopped in front of its tail), enlarged against the picture's bytes, then the kind's tail."""
    from marigold_amd.guided import guided_upsample
    finish = {a: kw[a] for a in pipe._finish_args if a in kw}
    dev = copy.copy(pipe)
    dev._tail = lambda final_pred, pred_uncert, **_: (final_pred, pred_uncert)
    low, unc = dev(pil, match_input_res=False, generator=_noise(seed), **kw)
    assert low.is_cuda and low.dtype == torch.float32 and tuple(low.shape[-2:]) == (24, 48)
    u8 = torch.from_numpy(np.array(pil.convert("RGB"))).to(low.device)
    up = guided_upsample(low.reshape((-1,) + tuple(low.shape[-2:])), u8, **guided)
    assert tuple(up.shape[-2:]) == (pil.height, pil.width)
    return pipe._tail(up.reshape(tuple(low.shape[:-2]) + tuple(up.shape[-2:])), unc, **finish)


CALLS = [("depth", 1, None), ("depth", 3, dict(output_uncertainty=True)), ("normals", 1, None), ("normals", 3, dict(output_uncertainty=True)),
         ("iid", 1, None), ("iid", 2, None)]


@pytest.mark.parametrize("kind,E,ens", CALLS, ids=[f"{k}-E{e}" for k, e, _ in CALLS])
def test_the_call_is_the_composition(kind, E, ens):
    pipe, pil = _pipe(kind), _pil(64, 128)
    kw = dict(ensemble_size=E, processing_res=RES, ensemble_kwargs=ens, show_progress_bar=False)
    got = pipe(pil, guided_upsample=True, generator=_noise(), **kw)
    _same(got, _composed(pipe, pil, dict(radius=2, sigma=0.1), **kw), f"{kind}/E={E}")
    got = pipe(pil, guided_upsample=dict(radius=3, sigma=0.03), generator=_noise(), **kw)
    _same(got, _composed(pipe, pil, dict(radius=3, sigma=0.03), **kw), f"{kind}/E={E}/radius=3")
    plain = pipe(pil, generator=_noise(), **kw)
    assert _lines("x", got)[0] != _lines("x", plain)[0]   # it is not the bilinear enlargement
    if E > 1 and ens:   # the uncertainty is not resampled, with or without the keyword
        unc = got.uncertainty
        assert unc is not None and unc.shape[-2:] == (24, 48) and np.array_equal(unc, plain.uncertainty)
    # a uint8 [1, 3, H, W] tensor on the host or on the device: the same picture, the same output
    chw = torch.from_numpy(np.array(pil.convert("RGB"))).permute(2, 0, 1)[None].contiguous()
    for image in (chw, chw.cuda()):
        _same(pipe(image, guided_upsample=dict(radius=3, sigma=0.03), generator=_noise(), **kw), got, f"{kind}/E={E}/tensor")


@pytest.mark.parametrize("kind", KINDS)
def test_the_default_keyword_changes_nothing(kind):
    pipe, pil = _pipe(kind), _pil(64, 128)
    for kw in (dict(processing_res=RES), dict(processing_res=RES, match_input_res=False), dict(processing_res=0, ensemble_size=2)):
        plain = pipe(pil, generator=_noise(), show_progress_bar=False, **kw)
        for off in (None, False):
            _same(pipe(pil, guided_upsample=off, generator=_noise(), show_progress_bar=False, **kw), plain, f"{kind}/{kw}")


@pytest.mark.parametrize("kind", KINDS)
def test_map_images_and_map_video_carry_the_keyword(kind):
    pipe = _pipe(kind)
    guided = dict(radius=1, sigma=0.2)
    kw = dict(processing_res=RES, guided_upsample=guided, show_progress_bar=False)
    pictures = [_pil(64, 128, seed=10 + i) for i in range(3)]
    alone = [pipe(p, generator=_noise(SEED + 1 + i), **kw) for i, p in enumerate(pictures)]
    for lanes in (1, 2):
        outs = list(pipe.map_images(pictures, in_flight=lanes, generators=[_noise(SEED + 1 + i) for i in range(3)], **kw))
        for i, (a, b) in enumerate(zip(alone, outs)):
            _same(b, a, f"map_images/{kind}/in_flight={lanes}/{i}")
    # two images per program: each image's members ride in a larger batch, whose arithmetic the enlargement does not touch - the output
    # is the composition over that program's own device prediction, and the lone call's wherever the program's prediction is the lone one's
    outs = list(pipe.map_images(pictures, in_flight=1, images_per_program=2, generators=[_noise(SEED + 1 + i) for i in range(3)], **kw))
    dev = copy.copy(pipe)
    dev._tail = lambda final_pred, pred_uncert, **_: (final_pred, pred_uncert)
    lows = list(dev.map_images(pictures, in_flight=1, images_per_program=2, generators=[_noise(SEED + 1 + i) for i in range(3)],
                               processing_res=RES, match_input_res=False, show_progress_bar=False))
    from marigold_amd.guided import guided_upsample
    for i, (out, (low, unc), pil) in enumerate(zip(outs, lows, pictures)):
        u8 = torch.from_numpy(np.array(pil.convert("RGB"))).cuda()
        up = guided_upsample(low.reshape((-1,) + tuple(low.shape[-2:])), u8, **guided)
        _same(out, pipe._tail(up.reshape(tuple(low.shape[:-2]) + tuple(up.shape[-2:])), unc), f"map_images/{kind}/per_program=2/{i}")
        la, lb = _lines("x", out), _lines("x", alone[i])
        print(f"[guided] {kind} images_per_program=2 image {i}: {'the lone call, bit for bit' if la == lb else 'differs from the lone call'}")
        _same(out, alone[i], f"map_images/{kind}/per_program=2 against the lone call/{i}")
    # a sequence: the serial loop map_video stands for
    from marigold_amd import SequenceState
    frames = [_pil(64, 128, seed=20 + i) for i in range(3)]
    state = SequenceState(0.1)
    serial = [pipe(f, sequence=state, generator=_noise(SEED + 7 + i), **kw) for i, f in enumerate(frames)]
    for lanes in (1, 2):
        outs = list(pipe.map_video(frames, in_flight=lanes, generators=[_noise(SEED + 7 + i) for i in range(3)], **kw))
        for i, (a, b) in enumerate(zip(serial, outs)):
            _same(b, a, f"map_video/{kind}/in_flight={lanes}/{i}")


@pytest.mark.parametrize("kind", KINDS)
def test_refusals(kind):
    import marigold_amd as M
    pipe, pil = _pipe(kind), _pil(64, 128)
    with pytest.raises(ValueError, match="match_input_res=False"):
        pipe(pil, guided_upsample=True, match_input_res=False)
    for image in (torch.rand(1, 3, 64, 128) * 255, torch.zeros(3, 64, 128, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="PIL image or a uint8"):
            pipe(image, guided_upsample=True)
    with pytest.raises(ValueError, match="radius"):
        pipe(pil, guided_upsample=dict(radius=0))
    with pytest.raises(ValueError, match="sigma"):
        pipe(pil, guided_upsample=dict(sigma=-1))
    with pytest.raises(ValueError, match="match_input_res=False"):
        list(pipe.map_images([pil, pil], images_per_program=2, guided_upsample=True, match_input_res=False))
    view = copy.copy(pipe)
    view._member_parallel = True
    with pytest.raises(ValueError, match="member-parallel"):
        view(pil, guided_upsample=True)
    view = copy.copy(pipe)
    view.device_io_stages = False
    with pytest.raises(ValueError, match="CUDA pipeline"):
        view(pil, guided_upsample=True)
    if kind != "iid":
        with pytest.raises(ValueError, match="predict_tiled: guided_upsample cannot be combined with tiles"):
            pipe.predict_tiled(_pil(128, 256), tile_size=(64, 128), tile_overlap=(16, 32), guided_upsample=True)
    # the function itself: shapes and dtypes of device tensors
    pred, pic = torch.zeros(3, 5, 7, device="cuda"), torch.zeros(16, 24, 3, dtype=torch.uint8, device="cuda")
    for bad_pred in (torch.zeros(17, 5, 7, device="cuda"), torch.zeros(1, 3, 5, 7, device="cuda"), pred.double(), pred.cpu()):
        with pytest.raises(ValueError, match="guided_upsample: "):
            M.guided_upsample(bad_pred, pic)
    for bad_pic in (pic.float(), pic.cpu(), torch.zeros(16, 24, 4, dtype=torch.uint8, device="cuda"), torch.zeros(2, 3, 16, 24, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError, match="guided_upsample: the picture"):
            M.guided_upsample(pred, bad_pic)
    with pytest.raises(ValueError, match="hwc"):
        M.guided_upsample(pred, pic, hwc=False)
    assert tuple(M.guided_upsample(pred, pic).shape) == (3, 16, 24) and tuple(M.guided_upsample(pred[0], pic.permute(2, 0, 1)[None].contiguous()).shape) == (16, 24)


# ---- the C host ----------------------------------------------------------------------------------------------------------------

def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


@pytest.fixture(scope="module")
def host_guided(tmp_path_factory):
    return c_hosts.build_example("host_guided", tmp_path_factory.mktemp("host_guided"))


@pytest.mark.parametrize("kind,radius,sigma", [("depth", 2, 0.1), ("normals", 3, 0.05)], ids=["depth", "normals"])
def test_c_host_guided(host_guided, tmp_path, kind, radius, sigma):
    """examples/host_guided.cpp in a fresh process on a 96 x 192 picture and a 64 x 128 model image: the files it writes against the
    pipeline's call with ``processing_res=128`` (which brings that picture to 64 x 128 by itself)."""
    from marigold_amd import image
    pipe, size = _pipe(kind), (96, 192)
    pil = _pil(*size)
    model, raw, prefix, lut_path = (str(tmp_path / n) for n in ("model.mgimg", "image.u8", "out", "spectral.lut"))
    image.export_model_image(pipe, model, ensemble_size=1, height=64, width=128)
    np.asarray(pil).tofile(raw)
    image.export_color_table("Spectral", lut_path)
    args = [host_guided, model, raw, str(size[0]), str(size[1]), str(SEED), prefix, str(radius), repr(sigma)] + ([lut_path] if kind == "depth" else [])
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[guided C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ref = pipe(pil, processing_res=128, guided_upsample=dict(radius=radius, sigma=sigma), generator=_noise(), show_progress_bar=False)
    C = 1 if kind == "depth" else 3
    pred = np.fromfile(prefix + ".f32", dtype=np.float32).reshape((C,) + size)
    pic = _pnm(prefix + ".ppm", b"P6", size[0], size[1], 255, np.uint8, 3)
    if kind == "depth":
        assert np.array_equal(pred[0], ref.depth_np) and np.array_equal(pic, np.asarray(ref.depth_colored))
        u16 = _pnm(prefix + ".pgm", b"P5", size[0], size[1], 65535, ">u2", 1).astype(np.uint16)
        assert np.array_equal(u16, (ref.depth_np * 65535.0).astype(np.uint16)) and u16.max() > u16.min()
    else:
        assert np.array_equal(pred, ref.normals_np) and np.array_equal(pic, np.asarray(ref.normals_img))
        assert not os.path.exists(prefix + ".pgm")
