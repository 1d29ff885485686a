"""``align=`` of the depth pipeline and ``map_video(align=...)`` on a real MI355X: the call against a composition written out here - the
pipeline's own device prediction at the processed size, ``marigold_amd.align_depth`` against the reference the state should hold, the
depth tail - bit for bit; frame 0 and ``align=None`` against the call without a state; ``map_video`` over one, two and three lanes
against the serial loop; a reset state against a fresh one; every refusal; and examples/host_align.cpp, a fresh process, writes the
arrays and pictures the pipeline returns.

The bound is equality everywhere: both sides run the same kernels on the same inputs in the same order.  The models are the tiny
synthetic ones of tests/pipeline_outputs.py, two steps; five frames of 64 x 128 processed at 24 x 48."""
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
SEED = (1 << 63) + 53
RES = 48
FRAMES = 5
UNC = dict(output_uncertainty=True)


@functools.lru_cache(maxsize=None)
def _pipe(kind="depth"):
    assert torch.cuda.is_available()
    return _tiny_pipe(kind)


def _video(h, w, count, seed):
    """One scene with a block that moves across it - consecutive frames resemble each other, as a video's do"""
    from PIL import Image
    base, other = np.asarray(_pil(h, w, seed=seed)), np.asarray(_pil(h, w, seed=seed + 1))
    frames = []
    for k in range(count):
        a = base.copy()
        x0 = (w // 16) * (1 + 2 * k)
        a[h // 4:h // 2, x0:x0 + w // 8] = other[h // 4:h // 2, x0:x0 + w // 8]
        frames.append(Image.fromarray(a))
    return tuple(frames)


@functools.lru_cache(maxsize=None)
def _frames(h=64, w=128):
    return _video(h, w, FRAMES, 30)


def _noise(k=0):
    from marigold_amd import NativeNoise
    return NativeNoise(SEED + k)


def _same(a, b, what):
    la, lb = _lines(what, a), _lines(what, b)
    assert la == lb, [(x, y) for x, y in zip(la, lb) if x != y][:3]
    for x, y in ((a.align_coef, b.align_coef), (a.align_flag, b.align_flag)):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), what


def _composed(pipe, frames, settings, **kw):
    """The serial loop's definition, step by step: per frame the unclipped ensembled prediction on the device at the processed size (the
    pipeline's own call with ``match_input_res=False``, stopped in front of its tail), fitted to the reference with ``align_depth`` from
    (1, 0) and replaced by s * pred + t, the uncertainty by s times itself; then the enlargement and the depth tail.
    -> [(output, coef, flag)]"""
    from marigold_amd import align
    from marigold_amd.util.image_util import get_tv_resample_method, resize
    dev = copy.copy(pipe)
    dev._tail = lambda final_pred, pred_uncert, **_: (final_pred, pred_uncert)
    fit = {k: v for k, v in settings.items() if k != "reference"}
    ref, outs = None, []
    for k, pil in enumerate(frames):
        low, unc = dev(pil, match_input_res=False, generator=_noise(k), **kw)
        assert low.is_cuda and low.dtype == torch.float32 and tuple(low.shape[-2:]) == (24, 48)
        if k == 0:
            aligned, coef, flag = low, torch.tensor([1.0, 0.0], dtype=torch.float64, device=low.device), torch.zeros(1, dtype=torch.int32, device=low.device)
        else:
            aligned, coef, flag = align.align_depth(low, ref, start=(1.0, 0.0), **fit)
            if unc is not None:
                unc = align.apply(unc, coef, use_shift=False)
        if k == 0 or settings.get("reference", "previous") == "previous":
            ref = aligned.clone()
        up = resize(aligned, (pil.height, pil.width), interpolation=get_tv_resample_method("bilinear"), antialias=True)
        outs.append((pipe._tail(up, unc), coef, flag))
    return outs


@pytest.mark.parametrize("E,ens", [(1, None), (3, UNC)], ids=["E1", "E3-uncertainty"])
@pytest.mark.parametrize("reference", ["previous", "first"])
def test_the_call_is_the_composition(E, ens, reference):
    from marigold_amd import DepthAlignState
    pipe, frames = _pipe(), _frames()
    kw = dict(ensemble_size=E, processing_res=RES, ensemble_kwargs=ens, show_progress_bar=False)
    settings = dict(iters=3, delta=0.08, reference=reference)
    state = DepthAlignState(**settings)
    got = []
    for k, f in enumerate(frames):
        got.append(pipe(f, align=state, generator=_noise(k), **kw))
        assert state.frames == k + 1 and state.coef is got[-1].align_coef and state.flag is got[-1].align_flag
        assert tuple(state.reference_map.shape) == (24, 48)
    want = _composed(pipe, frames, settings, **kw)
    plain = [pipe(f, generator=_noise(k), **kw) for k, f in enumerate(frames)]
    for k, (g, (w, coef, flag)) in enumerate(zip(got, want)):
        assert _lines(k, g) == _lines(k, w), (k, [(x, y) for x, y in zip(_lines(k, g), _lines(k, w)) if x != y][:3])
        assert torch.equal(g.align_coef, coef) and torch.equal(g.align_flag, flag) and g.align_coef.is_cuda and g.align_flag.dtype == torch.int32
        assert (g.uncertainty is not None) == (ens is not None)
    # frame 0 is the call without a state, bit for bit, with the identity for a fit
    assert _lines(0, got[0]) == _lines(0, plain[0]) and got[0].align_coef.tolist() == [1.0, 0.0] and got[0].align_flag.item() == 0
    assert plain[0].align_coef is None and plain[0].align_flag is None
    # the later frames were fitted: they moved, their flags are clear, and the uncertainty is s times the plain one
    flags = [g.align_flag.item() for g in got]
    print(f"[align pipeline] E={E} {reference}: s, t = {[tuple(round(v, 4) for v in g.align_coef.tolist()) for g in got]}, flags {flags}")
    assert flags[0] == 0 and 0 in flags[1:]
    assert any(_lines(k, got[k])[0] != _lines(k, plain[k])[0] for k in range(1, FRAMES))
    if ens is not None:
        for k in range(1, FRAMES):
            s = got[k].align_coef[0].item()
            assert np.array_equal(got[k].uncertainty, (plain[k].uncertainty.astype(np.float64) * s).astype(np.float32))


def test_first_and_previous_differ_only_in_what_they_were_fitted_to():
    from marigold_amd import DepthAlignState
    pipe, frames = _pipe(), _frames()
    kw = dict(processing_res=RES, match_input_res=False, show_progress_bar=False)
    a, b = DepthAlignState(reference="previous"), DepthAlignState(reference="first")
    first = None
    for k, f in enumerate(frames[:3]):
        x, y = pipe(f, align=a, generator=_noise(k), **kw), pipe(f, align=b, generator=_noise(k), **kw)
        if k == 0:
            first = b.reference_map.clone()
        if k <= 1:   # both were fitted to frame 0
            _same(x, y, f"frame {k}")
        assert torch.equal(b.reference_map, first)                       # "first" keeps frame 0's map
        assert np.array_equal(a.reference_map.cpu().numpy().clip(0, 1), x.depth_np)   # "previous" holds this frame's aligned map, unclipped
    assert not torch.equal(a.reference_map, first)


def test_align_none_changes_no_bit():
    pipe, pil = _pipe(), _frames()[0]
    for kw in (dict(processing_res=RES), dict(processing_res=RES, match_input_res=False), dict(processing_res=0, ensemble_size=2, ensemble_kwargs=UNC),
               dict(processing_res=RES, guided_upsample=True)):
        plain = pipe(pil, generator=_noise(), show_progress_bar=False, **kw)
        _same(pipe(pil, align=None, generator=_noise(), show_progress_bar=False, **kw), plain, str(kw))
        assert plain.align_coef is None and plain.align_flag is None


@pytest.mark.parametrize("extra", [dict(), dict(guided_upsample=True), dict(match_input_res=False), dict(ensemble_size=2, ensemble_kwargs=UNC)],
                         ids=["plain", "guided", "processed-size", "E2-uncertainty"])
def test_map_video_is_the_serial_loop(extra):
    from marigold_amd import DepthAlignState, SequenceState
    pipe, frames = _pipe(), _frames()
    kw = dict(processing_res=RES, show_progress_bar=False, **extra)
    settings = dict(iters=2, delta=0.1, reference="previous")
    seq, state = SequenceState(0.2), DepthAlignState(**settings)
    serial = [pipe(f, sequence=seq, align=state, generator=_noise(k), **kw) for k, f in enumerate(frames)]
    assert all(o.align_coef is not None for o in serial) and any(o.align_coef.tolist() != [1.0, 0.0] for o in serial[1:])
    for lanes in (1, 2, 3):
        outs = list(pipe.map_video(frames, strength=0.2, in_flight=lanes, align=settings, generators=[_noise(k) for k in range(FRAMES)], **kw))
        assert len(outs) == FRAMES
        for k, (a, b) in enumerate(zip(serial, outs)):
            _same(b, a, f"map_video/in_flight={lanes}/{k}")
    # align=True: the defaults; off: map_video as it was
    seq, state = SequenceState(0.2), DepthAlignState()
    serial = [pipe(f, sequence=seq, align=state, generator=_noise(k), **kw) for k, f in enumerate(frames[:3])]
    for a, b in zip(serial, pipe.map_video(frames[:3], strength=0.2, in_flight=2, align=True, generators=[_noise(k) for k in range(3)], **kw)):
        _same(b, a, "map_video/align=True")
    seq = SequenceState(0.2)
    serial = [pipe(f, sequence=seq, generator=_noise(k), **kw) for k, f in enumerate(frames[:3])]
    for off in (None, False):
        for a, b in zip(serial, pipe.map_video(frames[:3], strength=0.2, in_flight=2, align=off, generators=[_noise(k) for k in range(3)], **kw)):
            _same(b, a, f"map_video/align={off}")
            assert b.align_coef is None


def test_a_reset_state_runs_like_a_fresh_one():
    from marigold_amd import DepthAlignState
    pipe, frames = _pipe(), _frames()
    kw = dict(processing_res=RES, show_progress_bar=False)
    state = DepthAlignState()
    for k, f in enumerate(frames[:3]):
        pipe(f, align=state, generator=_noise(k), **kw)
    state.reset()
    assert state.frames == 0 and state.reference_map is None and state.coef is None and state.flag is None
    got = [pipe(f, align=state, generator=_noise(40 + k), **kw) for k, f in enumerate(frames[3:])]
    fresh = DepthAlignState()
    want = [pipe(f, align=fresh, generator=_noise(40 + k), **kw) for k, f in enumerate(frames[3:])]
    for k, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"after reset/{k}")
    # after a reset the state takes another processed size too
    state.reset()
    assert pipe(frames[0], align=state, generator=_noise(), processing_res=0, show_progress_bar=False).depth_np.shape == (64, 128)
    assert tuple(state.reference_map.shape) == (64, 128)


def test_a_degenerate_frame_passes_unchanged_and_becomes_the_reference():
    from marigold_amd import DepthAlignState
    pipe, frames = _pipe(), _frames()
    kw = dict(processing_res=RES, match_input_res=False, show_progress_bar=False)
    state = DepthAlignState()
    pipe(frames[0], align=state, generator=_noise(), **kw)
    state.reference_map.fill_(float("nan"))   # nothing to fit to: the next frame's fit is degenerate
    plain = pipe(frames[1], generator=_noise(1), **kw)
    out = pipe(frames[1], align=state, generator=_noise(1), **kw)
    assert out.align_flag.item() == 1 and out.align_coef.tolist() == [1.0, 0.0]
    assert np.array_equal(out.depth_np, plain.depth_np) and np.array_equal(np.asarray(out.depth_colored), np.asarray(plain.depth_colored))
    assert np.array_equal(state.reference_map.cpu().numpy().clip(0, 1), plain.depth_np) and state.frames == 2
    pipe(frames[2], align=state, generator=_noise(2), **kw)
    assert state.frames == 3


def test_refusals():
    from marigold_amd import DepthAlignState
    pipe, pil = _pipe(), _frames()[0]
    for kind in ("normals", "iid"):
        other = _pipe(kind)
        with pytest.raises(ValueError, match="no such ambiguity"):
            other(pil, align=DepthAlignState())
        with pytest.raises(ValueError, match="no such ambiguity"):
            other.map_video([pil], align=True)
    with pytest.raises(TypeError, match="DepthAlignState"):
        pipe(pil, align=True)
    state = DepthAlignState()
    pipe(pil, align=state, generator=_noise(), processing_res=RES, show_progress_bar=False)
    with pytest.raises(ValueError, match="reset"):
        pipe(pil, align=state, processing_res=0)
    assert state.frames == 1
    view = copy.copy(pipe)
    view._member_parallel = True
    with pytest.raises(ValueError, match="member-parallel"):
        view(pil, align=DepthAlignState())
    with pytest.raises(ValueError, match="predict_tiled: align cannot be combined with tiles"):
        pipe.predict_tiled(_pil(128, 256), tile_size=(64, 128), tile_overlap=(16, 32), align=DepthAlignState())
    with pytest.raises(ValueError, match="map_images: align"):
        pipe.map_images([pil, pil], align=DepthAlignState())
    with pytest.raises(ValueError, match="map_video: align"):
        pipe.map_video([pil], align=DepthAlignState())
    with pytest.raises(ValueError, match="delta"):
        pipe.map_video([pil], align=dict(delta=-1))


# ---- the C host ----------------------------------------------------------------------------------------------------------------

def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


@pytest.fixture(scope="module")
def host_align(tmp_path_factory):
    return c_hosts.build_example("host_align", tmp_path_factory.mktemp("host_align"))


@pytest.mark.parametrize("size,E,reference", [((96, 192), 1, "previous"), ((64, 128), 2, "first")], ids=["E1-enlarged-previous", "E2-uncertainty-first"])
def test_c_host_align(host_align, tmp_path, size, E, reference):
    """examples/host_align.cpp in a fresh process on a 64 x 128 model image: the files it writes against ``map_video(align=...)`` with
    ``processing_res=128`` (which brings a 96 x 192 frame to 64 x 128 by itself)."""
    from marigold_amd import image
    pipe = _pipe()
    frames = list(_video(size[0], size[1], 3, 60))
    strength, delta, iters = 0.25, 0.07, 3
    model, prefix, lut_path = (str(tmp_path / n) for n in ("model.mgimg", "out", "spectral.lut"))
    image.export_model_image(pipe, model, ensemble_size=E, height=64, width=128)
    image.export_color_table("Spectral", lut_path)
    args = []
    for k, f in enumerate(frames):
        raw = str(tmp_path / f"frame{k}.u8")
        np.asarray(f).tofile(raw)
        args += [raw, str(SEED + k)]
    args = [host_align, model, str(size[0]), str(size[1]), repr(strength), repr(delta), str(iters), reference, prefix, lut_path, "--"] + args
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[align C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ref = list(pipe.map_video(frames, strength=strength, in_flight=1, align=dict(delta=delta, iters=iters, reference=reference),
                              generators=[_noise(k) for k in range(3)], processing_res=128, ensemble_size=E,
                              ensemble_kwargs=UNC if E > 1 else None, show_progress_bar=False))
    for k, want in enumerate(ref):
        pre = f"{prefix}.{k}"
        pred = np.fromfile(pre + ".f32", dtype=np.float32).reshape(size)
        coef = np.fromfile(pre + ".coef", dtype=np.float64)
        pic = _pnm(pre + ".ppm", b"P6", size[0], size[1], 255, np.uint8, 3)
        u16 = _pnm(pre + ".pgm", b"P5", size[0], size[1], 65535, ">u2", 1).astype(np.uint16)
        assert np.array_equal(pred, want.depth_np), k
        assert np.array_equal(pic, np.asarray(want.depth_colored)), k
        assert np.array_equal(u16, (want.depth_np * 65535.0).astype(np.uint16)) and u16.max() > u16.min()
        assert coef[:2].tolist() == want.align_coef.tolist() and int(coef[2]) == want.align_flag.item(), k
        assert os.path.exists(pre + ".unc.f32") == (E > 1)
        if E > 1:
            assert np.array_equal(np.fromfile(pre + ".unc.f32", dtype=np.float32).reshape(64, 128), want.uncertainty), k
    assert any(o.align_flag.item() == 0 and o.align_coef.tolist() != [1.0, 0.0] for o in ref[1:])
