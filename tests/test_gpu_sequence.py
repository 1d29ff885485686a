"""Image sequences on a real MI355X: the carry kernel against torch's bits, ``sequence=`` against ``init_latents``,
``map_video`` lanes against the serial loop, ``mg_model_predict_next`` from a C host (examples/host_sequence.cpp, a fresh process) and
through ctypes against ``map_video``, and a reset state against a fresh one.

Every bound is equality: both sides run the same programs on the same rows, and the blend is defined to torch's bits - ``(x * a) +
(prev * b)`` in fp32 on the CPU with ``b = fp32(strength)``, ``a = fp32(1 - b)``: two rounded products, one rounded sum.  One
qualification, for the kernel test only: IEEE 754 fixes WHERE a NaN comes out, not its sign or payload, and the host's choice is the
host CPU's (x86 makes the NaN of inf * 0 with the sign bit set, the GPU without).  So the comparison is bitwise -
``.view(torch.int32)`` - on every element that is not a NaN, the infinities and signed zeros included, and "a NaN exactly where the
reference has one" on the rest.

The models are the tiny synthetic ones of tests/test_gpu_predict_out_c_host.py: 64 x 128, two DDIM steps, four LCM steps."""
import dataclasses
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image

from tests import c_hosts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HW = (64, 128)
SEED = (1 << 63) + 21


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {False: L.init(0), True: L.init(0, True)}


def _coefficients(strength):
    """(a, b) as 0-dim fp32 tensors: b = fp32(strength), a = fp32(1 - double(b)) - what ``mg_latent_carry`` computes."""
    b = np.float32(strength)
    return torch.tensor(np.float32(1.0 - float(b))), torch.tensor(b)


def _blend_cpu(x, prev, strength):
    a, b = _coefficients(strength)
    return (x.cpu() * a) + (prev.cpu() * b)


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------

SIZES = (1, 3, 4, 5, 511, 512, 515, 2 * 4 * 8 * 16 + 1)
PAD = 8   # floats of canary on either side; 32 bytes, so the offset alone decides the 16-byte alignment


def _planted(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    specials = (float("nan"), float("inf"), float("-inf"), -0.0)
    for j, s in enumerate(specials):   # spread over the vector; a short vector gets as many as fit
        if n > j:
            v[(j * 37 + seed) % n] = s
    return v


@pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
def test_latent_carry_kernel_rounds_like_torch_and_stays_in_bounds(libs, f16):
    lib = libs[f16]
    from marigold_amd import _lib as L, ops as O
    nan_bits_differ = 0
    for n in SIZES:
        for off_x in (0, 1):
            for off_p in (0, 1):
                x0, p0 = _planted(n, 3 + n), _planted(n, 11 + 2 * n)
                if n >= 4:   # the products that make a NaN out of finite-or-infinite operands: inf * 0 at strength 0 and 1
                    assert torch.isinf(x0).any() and torch.isinf(p0).any()
                for strength in (0.0, 0.1, 0.5, 1.0):
                    bx = torch.full((n + 2 * PAD + 1,), 7.5, device="cuda")
                    bp = torch.full((n + 2 * PAD + 1,), -3.25, device="cuda")
                    assert bx.data_ptr() % 16 == 0 and bp.data_ptr() % 16 == 0
                    x, p = bx[PAD + off_x:PAD + off_x + n], bp[PAD + off_p:PAD + off_p + n]
                    assert x.data_ptr() % 16 == 4 * off_x and p.data_ptr() % 16 == 4 * off_p
                    x.copy_(x0)
                    p.copy_(p0)
                    L.check(lib.mg_latent_carry(x.data_ptr(), p.data_ptr(), n, strength, O.current_stream_handle()), "mg_latent_carry", lib)
                    torch.cuda.synchronize()
                    want = _blend_cpu(x0, p0, strength)
                    got = x.cpu()
                    nan = torch.isnan(want)
                    where = f"n={n} x+{off_x} prev+{off_p} strength={strength}"
                    assert torch.equal(torch.isnan(got), nan), where
                    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32)), where
                    nan_bits_differ += int((got[nan].view(torch.int32) != want[nan].view(torch.int32)).sum())
                    if strength in (0.0, 1.0) and n >= 4:
                        assert int(nan.sum()) >= 2, where   # the planted NaN and an inf * 0
                    hx, hp = bx.cpu(), bp.cpu()
                    assert bool((hx[:PAD + off_x] == 7.5).all()) and bool((hx[PAD + off_x + n:] == 7.5).all()), where   # the canaries
                    assert bool((hp[:PAD + off_p] == -3.25).all()) and bool((hp[PAD + off_p + n:] == -3.25).all()), where
                    kept = hp[PAD + off_p:PAD + off_p + n]
                    assert torch.equal(kept.view(torch.int32), p0.view(torch.int32)), where   # prev is read only
    print(f"[latent carry] NaNs whose sign or payload differs from the host's: {nan_bits_differ}")


def test_latent_carry_refusals_launch_nothing(libs):
    lib = libs[False]
    from marigold_amd import ops as O
    x = torch.full((16,), 2.0, device="cuda")
    for args in ((x.data_ptr(), x.data_ptr(), -4, 0.1), (None, x.data_ptr(), 4, 0.1), (x.data_ptr(), None, 4, 0.1),
                 (x.data_ptr(), x.data_ptr(), 16, 1.25), (x.data_ptr(), x.data_ptr(), 16, float("nan"))):
        assert lib.mg_latent_carry(*args, O.current_stream_handle()) != 0 and lib.mg_last_error().decode().startswith("mg_latent_carry:")
    assert lib.mg_latent_carry(x.data_ptr(), x.data_ptr(), 0, 0.5, O.current_stream_handle()) == 0
    torch.cuda.synchronize()
    assert bool((x == 2.0).all())


# ---- the tiny pipelines ------------------------------------------------------------------------------------------------------------

def _make_pipe(kind, lcm=False, f16=False):
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.schedulers import LCMScheduler
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=LCMScheduler() if lcm else None, default_denoising_steps=4 if lcm else 2,
                                      default_processing_resolution=0, compute_dtype=torch.float16 if f16 else None).to("cuda:0")


_tiny_pipe = functools.lru_cache(maxsize=None)(_make_pipe)


@functools.lru_cache(maxsize=None)
def _pil(seed):
    from marigold_amd import synthetic as syn
    return Image.fromarray(syn.synthetic_image(HW[0], HW[1], seed=seed)[0].permute(1, 2, 0).numpy())


def _arrays(kind, out):
    """Everything an output holds, as numpy arrays (None where it holds none)."""
    if kind == "depth":
        return [out.depth_np, np.asarray(out.depth_colored), out.uncertainty]
    if kind == "normals":
        return [out.normals_np, np.asarray(out.normals_img), out.uncertainty]
    return [a for e in out for a in (e.array, np.asarray(e.image), e.uncertainty)]


def _same(kind, a, b):
    xs, ys = _arrays(kind, a), _arrays(kind, b)
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and np.isfinite(x).all() and np.array_equal(x, y)


def _differs(kind, a, b):
    return not np.array_equal(_arrays(kind, a)[0], _arrays(kind, b)[0])


def _generator(native, seed):
    import marigold_amd as M
    return M.NativeNoise(seed) if native else torch.Generator(device="cuda:0").manual_seed(seed & 0xffff)


# ---- 2. sequence= against init_latents ---------------------------------------------------------------------------------------------

#        id                  kind      E  lcm    batch  f16    native noise
CASES = [("depth-E1",        "depth",   1, False, 0,     False, False),
         ("depth-E2",        "depth",   2, False, 0,     False, True),
         ("normals-E3",      "normals", 3, False, 0,     False, False),
         ("iid-E1",          "iid",     1, False, 0,     False, True),
         ("depth-lcm",       "depth",   1, True,  0,     False, True),
         ("depth-E3-batch2", "depth",   3, False, 2,     False, False),
         ("depth-fp16",      "depth",   2, False, 0,     True,  True)]


@pytest.mark.parametrize("name,kind,E,lcm,batch,f16,native", CASES, ids=[c[0] for c in CASES])
def test_sequence_equals_init_latents(libs, name, kind, E, lcm, batch, f16, native):
    import marigold_amd as M
    pipe = _tiny_pipe(kind, lcm, f16)
    steps = 4 if lcm else 2
    kw = dict(denoising_steps=steps, ensemble_size=E, processing_res=0, batch_size=batch, show_progress_bar=False,
              ensemble_kwargs=dict(output_uncertainty=True) if kind != "iid" else None)
    f0, f1 = _pil(5), _pil(6)
    h, w = pipe._latent_hw(HW)
    shape = (E, pipe._target_latent_channels, h, w)
    # frame 0: the plain call
    state = M.SequenceState(strength=0.1)
    plain0 = pipe(f0, generator=_generator(native, SEED), **kw)
    first = pipe(f0, generator=_generator(native, SEED), sequence=state, **kw)
    _same(kind, first, plain0)
    assert state.frames == 1 and state.latent.dtype == torch.float32 and state.latent.is_cuda and tuple(state.latent.shape) == shape
    # ... and the state holds the denoising program's x (with batch_size < E: the last batch's rows)
    bs = batch or E
    last = E - ((E - 1) // bs) * bs
    prog = pipe.unet.denoise_program(last, h, w, pipe.scheduler, steps)
    assert tuple(prog.x.shape) == (last,) + shape[1:] and torch.equal(state.latent[E - last:], prog.x)
    latent0 = state.latent.clone()
    # frame 1: init_latents = the blend of the draw the generator gives and the carried latent, made on the CPU
    g = _generator(native, SEED + 1)
    z = torch.cat([pipe._randn((min(bs, E - i),) + shape[1:], g) for i in range(0, E, bs)]) if not lcm else pipe._randn(shape, g)
    assert not lcm or (batch == 0 and native and g.next_stream == 1)   # the LCM step noises follow on streams 1, 2, 3
    init = _blend_cpu(z, latent0, 0.1).to("cuda:0")
    want1 = pipe(f1, generator=g, init_latents=init, **kw)
    got1 = pipe(f1, generator=_generator(native, SEED + 1), sequence=state, **kw)
    _same(kind, got1, want1)
    assert state.frames == 2 and not torch.equal(state.latent, latent0)
    # the carry is live: at strength 0.5 frame 1 is another map than without a state
    strong = M.SequenceState(strength=0.5)
    pipe(f0, generator=_generator(native, SEED), sequence=strong, **kw)
    assert torch.equal(strong.latent, latent0)
    carried = pipe(f1, generator=_generator(native, SEED + 1), sequence=strong, **kw)
    alone = pipe(f1, generator=_generator(native, SEED + 1), **kw)
    assert _differs(kind, carried, alone) and _differs(kind, carried, got1)
    # a state of another shape is refused before anything runs; the state stays as it was
    with pytest.raises(ValueError, match="reset"):
        pipe(f1, sequence=strong, **dict(kw, ensemble_size=E + 1))
    assert strong.frames == 2


# ---- 3. map_video lanes ------------------------------------------------------------------------------------------------------------

VIDEO = (5, 6, 5, 7, 7, 6, 5)   # seven frames from three distinct pictures


@functools.lru_cache(maxsize=None)
def _serial_video(kind, E):
    """The serial ``sequence=`` loop (computed once per case, shared, never modified)."""
    import marigold_amd as M
    pipe = _tiny_pipe(kind)
    state = M.SequenceState(strength=0.5)
    return [pipe(_pil(p), sequence=state, generator=M.NativeNoise(SEED + k), denoising_steps=2, ensemble_size=E, processing_res=0,
                 show_progress_bar=False) for k, p in enumerate(VIDEO)]


@pytest.mark.parametrize("kind,E", [("depth", 1), ("normals", 2)], ids=["depth-E1", "normals-E2"])
@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_map_video_lanes_equal_the_serial_loop(libs, kind, E, in_flight):
    import marigold_amd as M
    pipe = _tiny_pipe(kind)
    want = _serial_video(kind, E)
    assert _differs(kind, want[0], want[2]) and _differs(kind, want[3], want[4])   # the same picture, another map: the carry and the seed
    for _ in range(2):   # twice on the same pipeline: the lanes, their streams and the allocator's blocks are reused
        outs = list(pipe.map_video((_pil(p) for p in VIDEO), strength=0.5, in_flight=in_flight,
                                   generators=(M.NativeNoise(SEED + k) for k in range(len(VIDEO))), denoising_steps=2, ensemble_size=E,
                                   processing_res=0, show_progress_bar=False))
        assert len(outs) == len(VIDEO)
        for got, ref in zip(outs, want):
            _same(kind, got, ref)
    assert len(pipe._lanes) >= (in_flight if in_flight > 1 else 0)


# ---- 4. the C host and ModelImage.predict_next -------------------------------------------------------------------------------------

HOST_VIDEO = (5, 6, 6, 7)
HOST_SEEDS = tuple(SEED + 100 + k for k in range(4))
STRENGTH = 0.25


@pytest.fixture(scope="module")
def models(libs, tmp_path_factory):
    """depth: ONE image of three configurations - E = 1; E = 1 with two steps' worth of another size; K = 2 - normals E = 2, iid E = 1."""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("sequence")
    paths = {k: str(d / f"{k}.mgimg") for k in ("depth", "normals", "iid")}
    image.export_model_image(_tiny_pipe("depth"), paths["depth"], configs=[dict(ensemble_size=1, height=64, width=128),
                                                                          dict(ensemble_size=2, height=64, width=128),
                                                                          dict(ensemble_size=1, height=64, width=128, images_per_program=2)])
    image.export_model_image(_tiny_pipe("normals"), paths["normals"], ensemble_size=2, height=64, width=128)
    image.export_model_image(_tiny_pipe("iid"), paths["iid"], ensemble_size=1, height=64, width=128)
    return paths


@pytest.fixture(scope="module")
def table():
    from marigold_amd.util.image_util import colormap_lut_u8
    return colormap_lut_u8("Spectral")


@functools.lru_cache(maxsize=None)
def _video_reference(kind, E, pictures=HOST_VIDEO, seeds=HOST_SEEDS):
    import marigold_amd as M
    return list(_tiny_pipe(kind).map_video([_pil(p) for p in pictures], strength=STRENGTH, generators=[M.NativeNoise(s) for s in seeds],
                                           in_flight=1, match_input_res=True, denoising_steps=2, ensemble_size=E, processing_res=0,
                                           ensemble_kwargs=dict(output_uncertainty=True), show_progress_bar=False))


def _check_frame(kind, E, got, ref):
    """(pred, unc, u16, picture) as numpy against the pipeline's output."""
    pred, unc, u16, pic = got
    want, want_pic, want_unc = _arrays(kind, ref)
    want = want[None] if kind == "depth" else want
    assert np.isfinite(want).all() and np.array_equal(pred, want)
    assert np.array_equal(pic, want_pic)
    if E > 1:
        assert np.array_equal(unc, want_unc)
    else:
        assert unc is None and want_unc is None
    if kind == "depth":
        assert np.array_equal(u16, (ref.depth_np * 65535.0).astype(np.uint16)) and u16.max() > u16.min()


def _next(mi, kind, picture, seed, lut, strength=STRENGTH, call="predict_next"):
    u8 = torch.from_numpy(np.array(_pil(picture))).cuda()
    kw = dict(out_size=HW, lut=lut if kind == "depth" else None, u16=kind == "depth", picture=True)
    out = mi.predict_next(u8, seed, strength, **kw) if call == "predict_next" else mi.predict_out(u8, seed, **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out[:4])


@pytest.mark.parametrize("kind,E", [("depth", 1), ("normals", 2)], ids=["depth-E1", "normals-E2"])
def test_predict_next_matches_map_video(libs, models, table, kind, E):
    from marigold_amd import image
    lut = torch.from_numpy(table).cuda()
    ref = _video_reference(kind, E)
    assert _differs(kind, ref[1], ref[2])   # the same picture twice in a row: the carry and the seed make another map
    mi = image.ModelImage(models[kind])
    try:
        base = mi.device_bytes
        for k, (p, s) in enumerate(zip(HOST_VIDEO, HOST_SEEDS)):
            _check_frame(kind, E, _next(mi, kind, p, s, lut), ref[k])
        # the handle counts its carried buffer: the x slot, E x 4 x 8 x 16 fp32 (the temporaries of the outputs aside: none at this size)
        assert mi.device_bytes - base == E * 4 * 8 * 16 * 4
        # seq_reset, then a call: mg_model_predict_out's bits - and the first frame's again
        mi.seq_reset()
        after_reset = _next(mi, kind, HOST_VIDEO[0], HOST_SEEDS[0], lut)
        plain = _next(mi, kind, HOST_VIDEO[0], HOST_SEEDS[0], lut, call="predict_out")
        for a, b in zip(after_reset, plain):
            assert (a is None and b is None) or np.array_equal(a, b)
        _check_frame(kind, E, after_reset, ref[0])
        # predict_out in between neither reads nor changes the state: the sequence goes on where it was
        _check_frame(kind, E, _next(mi, kind, HOST_VIDEO[1], HOST_SEEDS[1], lut), ref[1])
    finally:
        mi.close()


def test_select_resets_the_carry_and_a_replica_has_its_own(libs, models, table):
    from marigold_amd import image
    lut = torch.from_numpy(table).cuda()
    ref = _video_reference("depth", 1)
    mi = image.ModelImage(models["depth"])
    rep = None
    try:
        assert len(mi.configs) == 3 and mi.selected == 0
        for k in range(2):
            _check_frame("depth", 1, _next(mi, "depth", HOST_VIDEO[k], HOST_SEEDS[k], lut), ref[k])
        # a replica starts empty and runs a sequence of its own; the parent's goes on undisturbed
        rep = mi.replica()
        _check_frame("depth", 1, _next(rep, "depth", HOST_VIDEO[0], HOST_SEEDS[0], lut), ref[0])
        _check_frame("depth", 1, _next(mi, "depth", HOST_VIDEO[2], HOST_SEEDS[2], lut), ref[2])
        _check_frame("depth", 1, _next(rep, "depth", HOST_VIDEO[1], HOST_SEEDS[1], lut), ref[1])
        _check_frame("depth", 1, _next(mi, "depth", HOST_VIDEO[3], HOST_SEEDS[3], lut), ref[3])
        # to another configuration (E = 2: a sequence there) and back: nothing is carried over either way
        ref2 = _video_reference("depth", 2)
        mi.select(1)
        for k in range(2):
            _check_frame("depth", 2, _next(mi, "depth", HOST_VIDEO[k], HOST_SEEDS[k], lut), ref2[k])
        mi.select(0)
        _check_frame("depth", 1, _next(mi, "depth", HOST_VIDEO[0], HOST_SEEDS[0], lut), ref[0])
        _check_frame("depth", 1, _next(mi, "depth", HOST_VIDEO[1], HOST_SEEDS[1], lut), ref[1])
    finally:
        if rep is not None:
            rep.close()
        mi.close()


def test_predict_next_refusals(libs, models):
    """A K = 2 configuration, an intrinsic-image model and a bad strength are refused before anything is launched."""
    from marigold_amd import image, ops as O
    lib = libs[False]
    u8 = torch.from_numpy(np.array(_pil(5))).cuda()
    out = torch.full((3, 64, 128), -3.0, device="cuda")

    def refused(mi, strength, *words):
        rc = lib.mg_model_predict_next(mi.handle, u8.data_ptr(), 1, 64, 128, 0, 0, 1, None, None, out.data_ptr(), None, None, None, None,
                                       O.current_stream_handle(), strength)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_next:") and all(w in msg for w in words), msg

    mi = image.ModelImage(models["depth"])
    try:
        refused(mi, 1.5, "strength")
        refused(mi, float("nan"), "strength")
        mi.select(2)
        refused(mi, 0.1, "2 pictures per call")
    finally:
        mi.close()
    mi = image.ModelImage(models["iid"])
    try:
        refused(mi, 0.1, "intrinsic-image")
    finally:
        mi.close()
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())


def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


@pytest.fixture(scope="module")
def host_sequence(tmp_path_factory):
    """examples/host_sequence.cpp, built as the ``host_picture`` fixture of tests/test_gpu_predict_out_c_host.py builds its example."""
    return c_hosts.build_example("host_sequence", tmp_path_factory.mktemp("host_sequence"))


@pytest.mark.parametrize("kind,E", [("depth", 1), ("normals", 2)], ids=["depth-E1", "normals-E2"])
def test_c_host_sequence(libs, models, host_sequence, tmp_path, kind, E):
    """examples/host_sequence.cpp in a fresh process, one mg_model_predict_next per frame: the files it writes, read back."""
    from marigold_amd import image
    prefix, lut_path = str(tmp_path / "out"), str(tmp_path / "spectral.lut")
    image.export_color_table("Spectral", lut_path)
    frames = []
    for k, (p, s) in enumerate(zip(HOST_VIDEO, HOST_SEEDS)):
        raw = str(tmp_path / f"frame{k}.u8")
        np.asarray(_pil(p)).tofile(raw)
        frames += [raw, str(s)]
    args = [host_sequence, models[kind], "64", "128", str(STRENGTH), prefix] + ([lut_path] if kind == "depth" else []) + ["--"] + frames
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[sequence C host] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    ref = _video_reference(kind, E)
    C = 1 if kind == "depth" else 3
    for k in range(len(HOST_VIDEO)):
        pre = f"{prefix}.{k}"
        pred = np.fromfile(pre + ".f32", dtype=np.float32).reshape((C,) + HW)
        unc = np.fromfile(pre + ".unc.f32", dtype=np.float32).reshape(HW) if E > 1 else None
        assert os.path.exists(pre + ".unc.f32") == (E > 1) and os.path.exists(pre + ".pgm") == (kind == "depth")
        u16 = _pnm(pre + ".pgm", b"P5", HW[0], HW[1], 65535, ">u2", 1).astype(np.uint16) if kind == "depth" else None
        pic = _pnm(pre + ".ppm", b"P6", HW[0], HW[1], 255, np.uint8, 3)
        _check_frame(kind, E, (pred, unc, u16, pic), ref[k])


# ---- 5. a stale carry --------------------------------------------------------------------------------------------------------------

def test_a_reset_state_runs_like_a_fresh_one(libs, models, table):
    """Sequence A, reset, sequence B: B is what a freshly built pipeline / a freshly loaded model gives for B."""
    import marigold_amd as M
    from marigold_amd import image
    A, B = (5, 6, 7), (7, 5)
    kw = dict(denoising_steps=2, ensemble_size=2, processing_res=0, show_progress_bar=False)
    pipe = _tiny_pipe("depth")
    state = M.SequenceState(strength=0.5)
    for k, p in enumerate(A):
        pipe(_pil(p), sequence=state, generator=M.NativeNoise(SEED + k), **kw)
    state.reset()
    assert state.latent is None and state.frames == 0
    got = [pipe(_pil(p), sequence=state, generator=M.NativeNoise(SEED + 50 + k), **kw) for k, p in enumerate(B)]
    fresh_pipe, fresh = _make_pipe("depth"), M.SequenceState(strength=0.5)
    want = [fresh_pipe(_pil(p), sequence=fresh, generator=M.NativeNoise(SEED + 50 + k), **kw) for k, p in enumerate(B)]
    for a, b in zip(got, want):
        _same("depth", a, b)
    assert _differs("depth", got[1], pipe(_pil(B[1]), generator=M.NativeNoise(SEED + 51), **kw))   # B's second frame does carry
    # the C handle
    lut = torch.from_numpy(table).cuda()
    mi, fresh_mi = image.ModelImage(models["normals"]), None
    try:
        for k, p in enumerate(A):
            _next(mi, "normals", p, SEED + k, lut)
        mi.seq_reset()
        got = [_next(mi, "normals", p, SEED + 50 + k, lut) for k, p in enumerate(B)]
        fresh_mi = image.ModelImage(models["normals"])
        want = [_next(fresh_mi, "normals", p, SEED + 50 + k, lut) for k, p in enumerate(B)]
        for a, b in zip(got, want):
            for x, y in zip(a, b):
                assert (x is None and y is None) or np.array_equal(x, y)
        alone = _next(fresh_mi, "normals", B[1], SEED + 51, lut, call="predict_out")
        assert not np.array_equal(alone[0], got[1][0])
    finally:
        mi.close()
        if fresh_mi is not None:
            fresh_mi.close()
