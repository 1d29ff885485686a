"""Host checks of depth alignment, no GPU: the three C entry points are declared, bound and exported by both operand
libraries without touching the ABI version or the op kinds; the fit and the apply refuse bad arguments before any GPU work (no GPU is
here: a call that got as far as a launch would fail differently, so the message proves where it stopped); ``DepthAlignState`` and
``align_depth`` check their arguments; ``align=`` and ``map_video(align=)`` refuse what they must before anything is launched
(stand-in pipelines whose engines are namespaces) and leave a call without them untouched; with several lanes the align stage takes
turns in frame order on a turnstile of its own; the command line hands the flags on; the C host example compiles; and the numpy
restatement the GPU tests are measured against is robust where plain least squares is not."""
import contextlib
import ctypes
import os
import re
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L
from marigold_amd import align
from marigold_amd.align import DepthAlignState, align_depth
from marigold_amd.pipeline import MarigoldDepthOutput, MarigoldDepthPipeline, MarigoldIIDPipeline, MarigoldNormalsPipeline
from marigold_amd.schedulers import DDIMScheduler
from tests import c_hosts
from tests.align_reference import align_apply_reference, align_fit_reference, robustness_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
CAP = 20.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "#define MG_ALIGN_MAX_ITERS 32" in hdr and "enum { MG_ALIGN_START_GIVEN = 0, MG_ALIGN_START_LS = 1 };" in flat
    assert "long long mg_depth_align_workspace_bytes(long long n);" in flat
    assert ("int mg_depth_align_fit(const float* d, const float* ref, const unsigned char* mask_or_null, long long n, int fit_shift, int iters, "
            "int start_mode, double s_start, double t_start, double delta, double* coef, int* flag, void* ws, long long ws_bytes, "
            "void* stream);") in flat
    assert ("int mg_depth_align_apply(const float* x, long long n, const double* coef, int use_shift, float clip_lo, float clip_hi, "
            "float* out, void* stream);") in flat
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    makefile = open(os.path.join(ROOT, "marigold_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\balign\.hip\b", makefile, re.M)
    assert re.search(r"^FLAGS_align\s*:=\s*-ffp-contract=off\s*$", makefile, re.M)
    vp, i, ll, dbl, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_depth_align_workspace_bytes", "mg_depth_align_fit", "mg_depth_align_apply"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_depth_align_workspace_bytes.argtypes == [ll] and lib.mg_depth_align_workspace_bytes.restype is ll
        assert lib.mg_depth_align_fit.argtypes == [vp, vp, vp, ll, i, i, i, dbl, dbl, dbl, vp, vp, vp, ll, vp]
        assert lib.mg_depth_align_apply.argtypes == [vp, ll, vp, i, f, f, vp, vp]
    assert (L.ALIGN_MAX_ITERS, L.ALIGN_START_GIVEN, L.ALIGN_START_LS) == (32, 0, 1)
    assert ctypes.sizeof(L.MgOp) == 360
    assert "align" not in " ".join(L.OP_NAMES.values())   # plain C calls, no op kind
    import marigold_amd
    assert marigold_amd.align_depth is align_depth and marigold_amd.DepthAlignState is DepthAlignState


@LIBS
def test_workspace_bytes(f16):
    lib = L.load(f16)
    for n in (0, -1, -(1 << 40), (1 << 30) + 1):
        assert lib.mg_depth_align_workspace_bytes(n) == -1
        assert lib.mg_last_error().decode().startswith("mg_depth_align_workspace_bytes:")
    sizes = [1, 2, 63, 64, 65, 4095, 4096, 4097, 12293, 768 * 768, 1 << 24, 1 << 30]
    got = [lib.mg_depth_align_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 8 == 0 for b in got) and got == sorted(got) and got[0] < got[-1]


@LIBS
def test_the_fit_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()                      # stands for every device buffer: no call gets as far as reading it
    p = (ctypes.addressof(mem) + 15) // 16 * 16
    need = lib.mg_depth_align_workspace_bytes(100)
    names = ("d", "ref", "mask", "n", "fit_shift", "iters", "start_mode", "s_start", "t_start", "delta", "coef", "flag", "ws", "ws_bytes")

    def refused(*words, **kw):
        a = dict(d=p, ref=p, mask=None, n=100, fit_shift=1, iters=4, start_mode=0, s_start=1.0, t_start=0.0, delta=0.05, coef=p, flag=p, ws=p,
                 ws_bytes=need)
        a.update(kw)
        rc = lib.mg_depth_align_fit(*(a[k] for k in names), None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_depth_align_fit:") and all(w in msg for w in words), (kw, rc, msg)

    for n in (0, -5, (1 << 30) + 1):
        refused("pixels", n=n)
    for name in ("d", "ref", "coef", "flag", "ws"):
        refused("null pointer", **{name: None})
    refused("workspace holds", ws_bytes=need - 1)
    refused("workspace holds", ws_bytes=0)
    refused("16-byte aligned", ws=p + 8)
    refused("aligned to their elements", d=p + 2)
    refused("aligned to their elements", coef=p + 4)
    for iters in (-1, 33):
        refused("iterations", iters=iters)
    for mode in (-1, 2):
        refused("start mode", start_mode=mode)
    for delta in (0.0, -0.05, float("nan"), float("inf")):
        refused("delta", delta=delta)
    for bad in (dict(s_start=float("nan")), dict(t_start=float("inf")), dict(s_start=float("-inf"))):
        refused("start values", **bad)
    assert list(mem) == [0.0] * 64


@LIBS
def test_the_apply_refuses_bad_arguments_before_any_gpu_work(f16):
    lib = L.load(f16)
    mem = (ctypes.c_double * 64)()
    p = (ctypes.addressof(mem) + 15) // 16 * 16

    def refused(*words, **kw):
        a = dict(x=p, n=100, coef=p, use_shift=1, lo=0.0, hi=1.0, out=p)
        a.update(kw)
        rc = lib.mg_depth_align_apply(*(a[k] for k in ("x", "n", "coef", "use_shift", "lo", "hi", "out")), None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_depth_align_apply:") and all(w in msg for w in words), (kw, rc, msg)

    for n in (0, -1, (1 << 30) + 1):
        refused("elements", n=n)
    for name in ("x", "coef", "out"):
        refused("null pointer", **{name: None})
    refused("aligned to their elements", x=p + 1)
    refused("aligned to their elements", out=p + 2)
    refused("aligned to their elements", coef=p + 4)
    assert list(mem) == [0.0] * 64


# ---- marigold_amd.align ------------------------------------------------------------------------------------------------------------

def test_the_state_s_arguments():
    st = DepthAlignState()
    assert (st.iters, st.delta, st.reference, st.fit_shift) == (4, 0.05, "previous", True) == (align.DEFAULT_ITERS, align.DEFAULT_DELTA, "previous", True)
    assert st.reference_map is None and st.coef is None and st.flag is None and st.frames == 0
    st = DepthAlignState(iters=0, delta=2, reference="first", fit_shift=False)
    assert (st.iters, st.delta, st.reference, st.fit_shift) == (0, 2.0, "first", False)
    st.frames, st._sig, st.reference_map = 3, ((8, 8), "cuda"), object()
    st.reset()
    assert st.frames == 0 and st._sig is None and st.reference_map is None
    for bad in (dict(iters=-1), dict(iters=33), dict(iters=1.5), dict(iters=True), dict(delta=0), dict(delta=-1.0), dict(delta=float("nan")),
                dict(delta=float("inf")), dict(delta="0.05"), dict(reference="last"), dict(reference=None)):
        with pytest.raises(ValueError, match="DepthAlignState"):
            DepthAlignState(**bad)
    assert align.settings(None) is None and align.settings(False) is None
    assert isinstance(align.settings(True), DepthAlignState) and align.settings(dict(iters=2, reference="first")).reference == "first"
    for bad in (dict(strength=1), 3, "yes", dict(iters=99)):
        with pytest.raises(ValueError):
            align.settings(bad)


def test_align_depth_refuses_what_is_not_a_pair_of_device_maps():
    for pred in (np.zeros((5, 7), np.float32), torch.zeros(5, 7), torch.zeros(5, 7, dtype=torch.float64)):
        with pytest.raises(ValueError, match="align_depth: pred must be a non-empty fp32 CUDA tensor"):
            align_depth(pred, pred)
    assert "start=\"ls\"" in align_depth.__doc__ and "mask" in align_depth.__doc__   # the sparse-anchor use is shown
    for start in ("median", (1.0,), (float("nan"), 0.0), 3):
        with pytest.raises(ValueError, match="start"):
            align._check_start("align_depth", start)
    assert align._check_start("align_depth", "ls")[0] == L.ALIGN_START_LS and align._check_start("align_depth", (2, 0.5)) == (L.ALIGN_START_GIVEN, 2.0, 0.5)


# ---- the pipelines' keyword: the refusals ------------------------------------------------------------------------------------------

def _engine(name, device, launched):
    def boom(*a, **k):
        launched.append(name)
        raise AssertionError(f"{name}: reached a launch")
    return SimpleNamespace(name=name, device=device, replica=boom, config=SimpleNamespace(block_out_channels=(1, 1, 1, 1)),
                           encode_rgb_latent=boom, denoise_program=boom, set_context=boom, f16=False, dtype=torch.bfloat16)


def _stand_in(cls, device_type="cuda"):
    launched = []
    device = SimpleNamespace(type=device_type)
    kw = dict(default_denoising_steps=2, default_processing_resolution=0, empty_text_embed=torch.zeros(1, 2, 4))
    if cls is MarigoldIIDPipeline:
        unet = _engine("unet", device, launched)
        unet.config = SimpleNamespace(in_channels=12, out_channels=8)
        pipe = cls(unet, _engine("vae", device, launched), DDIMScheduler(), target_properties={"target_names": ["albedo", "material"]}, **kw)
    else:
        pipe = cls(_engine("unet", device, launched), _engine("vae", device, launched), DDIMScheduler(), **kw)

    def reached(name):
        def stop(*a, **k):
            launched.append(name)
            raise AssertionError(f"reached {name}")
        return stop
    pipe._preprocess, pipe._preprocess_device = reached("preprocessing"), reached("preprocessing")
    pipe.launched = launched
    return pipe


PICTURE = torch.zeros(1, 3, 128, 256, dtype=torch.uint8)


@pytest.mark.parametrize("cls", [MarigoldNormalsPipeline, MarigoldIIDPipeline], ids=["normals", "iid"])
def test_the_other_kinds_refuse_the_keyword(cls):
    pipe = _stand_in(cls)
    with pytest.raises(ValueError, match="no such ambiguity"):
        pipe(PICTURE, align=DepthAlignState())
    with pytest.raises(ValueError, match="no such ambiguity"):
        pipe.map_video([PICTURE], align=True)
    assert pipe.launched == []
    with pytest.raises(AssertionError, match="reached preprocessing"):   # without it the call goes on as ever
        pipe(PICTURE, align=None)


def test_the_depth_pipeline_refuses_before_any_launch():
    pipe = _stand_in(MarigoldDepthPipeline)
    with pytest.raises(TypeError, match="DepthAlignState"):
        pipe(PICTURE, align=True)
    # a state that holds a reference of another processed size (the stand-in VAE halves three times: 128 x 256 decodes to 128 x 256)
    st = DepthAlignState()
    st.frames, st._sig = 1, ((64, 256), pipe.device)
    with pytest.raises(ValueError, match="reset"):
        pipe(PICTURE, align=st)
    assert st.frames == 1
    with pytest.raises(ValueError, match="needs a CUDA pipeline"):
        _stand_in(MarigoldDepthPipeline, "cpu")(PICTURE, align=DepthAlignState())
    with pytest.raises(ValueError, match="needs a CUDA pipeline"):
        _stand_in(MarigoldDepthPipeline, "cpu").map_video([PICTURE], align=True)
    with pytest.raises(ValueError, match="predict_tiled: align cannot be combined with tiles"):
        pipe.predict_tiled(PICTURE, tile_size=(64, 128), tile_overlap=(16, 32), align=DepthAlignState())
    with pytest.raises(ValueError, match="map_images: align"):
        pipe.map_images([PICTURE], align=DepthAlignState())
    with pytest.raises(ValueError, match="map_video: align is True or a dict"):
        pipe.map_video([PICTURE], align=DepthAlignState())
    with pytest.raises(ValueError, match="unknown keys"):
        pipe.map_video([PICTURE], align=dict(sigma=1))
    with pytest.raises(ValueError, match="DepthAlignState: iters"):
        pipe.map_video([PICTURE], align=dict(iters=40))
    pipe._sharded = lambda: True
    with pytest.raises(ValueError, match="align is not available on a member-parallel pipeline"):
        pipe(PICTURE, align=DepthAlignState())
    with pytest.raises(ValueError, match="member-parallel"):
        pipe.map_video([PICTURE], align=True)
    pipe._sharded = lambda: False
    pipe._member_parallel = True
    with pytest.raises(ValueError, match="align is not available on a member-parallel pipeline"):
        pipe(PICTURE, align=DepthAlignState())
    pipe._member_parallel = False
    assert pipe.launched == []
    # accepted, the call goes on - in the stand-in, to its preprocessing; so does a call without the keyword
    st = DepthAlignState()
    st.frames, st._sig = 1, ((128, 256), pipe.device)
    for kw in (dict(align=st), dict(align=DepthAlignState()), dict(align=None), dict()):
        with pytest.raises(AssertionError, match="reached preprocessing"):
            pipe(PICTURE, **kw)


def test_align_none_leaves_the_call_path_untouched():
    """Without a state ``_finish`` touches nothing of the alignment: no library is loaded for it, no turn is looked at, and the output
    carries no fit."""
    pipe = _stand_in(MarigoldDepthPipeline)
    seen = {}

    def tail(final_pred, pred_uncert, **finish):
        seen["pred"] = final_pred
        return MarigoldDepthOutput(final_pred.numpy(), None, None)
    pipe._tail = tail
    pipe._align_turn = "never looked at"
    pred = torch.rand(1, 1, 6, 8)
    out = pipe._finish(pred, (1, 3, 6, 8), 1, False, None, None)
    assert seen["pred"] is pred and out.align_coef is None and out.align_flag is None
    assert MarigoldDepthOutput(np.zeros((2, 2), np.float32), None, None).align_coef is None


# ---- map_video(align=...) over stand-in lanes --------------------------------------------------------------------------------------

SLEEP_MS = (9, 2, 6, 1, 8, 3, 5)


def _capped(fn):
    box = {}

    def target():
        try:
            box["result"] = fn()
        except BaseException as e:  # noqa: BLE001
            box["error"] = e
    t = threading.Thread(target=target, daemon=True)
    t.start()
    t.join(CAP)
    assert not t.is_alive(), f"deadlock: still running after {CAP} s"
    if "error" in box:
        raise box["error"]
    return box.get("result")


class _VideoStandIn(MarigoldDepthPipeline):
    """A call sleeps (its encode), takes its frame's denoise turn, hands it on, sleeps (its decode), takes its frame's ALIGN turn - reads
    the state, writes it - hands that on and returns what it saw."""

    def __init__(self, fail_at=None):
        device = SimpleNamespace(type="cuda")

        def engine(name):
            return SimpleNamespace(name=name, device=device, replica=lambda: engine(name + "'"), config=SimpleNamespace(block_out_channels=(1,)))
        super().__init__(engine("unet"), engine("vae"), DDIMScheduler(), default_denoising_steps=2, default_processing_resolution=0,
                         empty_text_embed=torch.zeros(1, 2, 4))
        self.fail_at, self.denoised, self.aligned, self.refused = fail_at, [], [], []

    def _lane_stream(self):
        return None

    def _lane_contexts(self, streams):
        return [contextlib.nullcontext() for _ in streams], lambda: None

    def __call__(self, image, sequence=None, generator=None, align=None, **kw):
        k = int(image[0, 0, 0, 0])
        time.sleep(SLEEP_MS[k % 7] / 1000.0)
        turn, aturn = self._sequence_turn, self._align_turn
        try:
            if turn is not None:
                turn[0].wait(turn[1], timeout=CAP)
            self.denoised.append(k)
            sequence.frames += 1
            if turn is not None:
                turn[0].done(turn[1])
            time.sleep(SLEEP_MS[(k + 3) % 7] / 1000.0)
            if k == self.fail_at:
                time.sleep(0.02)   # the later frames are at the align turnstile by now
                raise OSError(f"frame {k} failed")
            if aturn is not None:
                aturn[0].wait(aturn[1], timeout=CAP)
        except RuntimeError:
            self.refused.append(k)
            raise
        seen = align.frames
        self.aligned.append(k)
        align.frames += 1
        if aturn is not None:
            aturn[0].done(aturn[1])
        return (k, seen, align, aturn is not None and aturn[1], turn is not None and turn[0] is not aturn[0])


def _frames(n, hw=(64, 128)):
    for k in range(n):
        yield torch.full((1, 3) + hw, k, dtype=torch.uint8)


@pytest.mark.parametrize("n_lanes", [1, 2, 3])
def test_map_video_orders_the_align_stage_on_a_turnstile_of_its_own(n_lanes):
    def scenario():
        before = set(threading.enumerate())
        pipe = _VideoStandIn()
        outs = list(pipe.map_video(_frames(7), in_flight=n_lanes, align=dict(iters=2, reference="first")))
        assert [o[0] for o in outs] == list(range(7)) and [o[1] for o in outs] == list(range(7))   # frame k aligned after k frames
        assert pipe.denoised == list(range(7)) and pipe.aligned == list(range(7))
        states = {id(o[2]) for o in outs}
        assert len(states) == 1 and isinstance(outs[0][2], DepthAlignState) and (outs[0][2].iters, outs[0][2].reference) == (2, "first")
        if n_lanes == 1:
            assert all(o[3] is False for o in outs)
        else:
            assert [o[3] for o in outs] == list(range(7)) and all(o[4] for o in outs)   # two turnstiles, not one
        assert "_align_turn" not in vars(pipe) and pipe._align_turn is None   # the turns sat on per-call views
        # one state per call
        again = list(pipe.map_video(_frames(2), in_flight=1, align=True))
        assert again[0][2] is not outs[0][2] and [o[1] for o in again] == [0, 1]
        assert [t for t in threading.enumerate() if t not in before and t is not threading.current_thread()] == []
    _capped(scenario)


def test_a_frame_that_fails_before_its_align_turn_aborts_both_turnstiles():
    def scenario():
        before = set(threading.enumerate())
        pipe = _VideoStandIn(fail_at=1)
        got = []
        with pytest.raises(OSError, match="frame 1 failed"):
            for out in pipe.map_video(_frames(7), in_flight=3, align=True):
                got.append(out[0])
        assert got == [0] and pipe.aligned == [0]
        assert pipe.refused and all(k > 1 for k in pipe.refused)   # the lanes at a turnstile raised; no cap ran out
        assert [t for t in threading.enumerate() if t not in before and t is not threading.current_thread()] == []
    _capped(scenario)


# ---- the command line --------------------------------------------------------------------------------------------------------------

class _FakeCliPipe:
    scale_invariant = shift_invariant = True
    default_denoising_steps, default_processing_resolution = 4, 768
    target_names = ["albedo"]

    def __init__(self):
        self.calls = []

    def _out(self):
        from PIL import Image
        return MarigoldDepthOutput(np.linspace(0, 1, 48, dtype=np.float32).reshape(6, 8), Image.fromarray(np.zeros((6, 8, 3), np.uint8)), None)

    def map_images(self, images, in_flight=None, generators=None, **kw):
        images = list(images)
        self.calls.append(("map_images", len(images), kw))
        return [self._out() for _ in images]

    def map_video(self, frames, strength=0.1, in_flight=None, generators=None, **kw):
        frames = list(frames)
        self.calls.append(("map_video", len(frames), kw))
        return [self._out() for _ in frames]


def test_cli_sequence_align_flags(tmp_path, capsys):
    from PIL import Image
    from marigold_amd import cli
    io = ["--input_rgb_dir", "i", "--output_dir", "o"]
    a = cli.build_parser("depth").parse_args(io)
    assert (a.sequence_align, a.align_delta, a.align_iters, a.align_reference) == (False, 0.05, 4, "previous")
    inp = tmp_path / "in"
    inp.mkdir()
    for name in ("b.png", "a.png"):
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / name)
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    # without the flag no keyword is passed, whatever the other three say
    for extra in (["--sequence"], ["--sequence", "--align_delta", "0.2", "--align_iters", "1", "--align_reference", "first"]):
        pipe = _FakeCliPipe()
        assert cli.main("depth", base + extra, pipeline=pipe) == 0
        assert pipe.calls[0][0] == "map_video" and "align" not in pipe.calls[0][2]
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--sequence", "--sequence_align"], pipeline=pipe) == 0
    assert pipe.calls[0][:2] == ("map_video", 2) and pipe.calls[0][2]["align"] == dict(iters=4, delta=0.05, reference="previous")
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--sequence", "--sequence_align", "--align_delta", "0.2", "--align_iters", "0", "--align_reference", "first"],
                    pipeline=pipe) == 0
    assert pipe.calls[0][2]["align"] == dict(iters=0, delta=0.2, reference="first")
    # refused with an argparse error: without --sequence, with settings the state refuses, and on the other kinds' scripts
    for kind, extra, word in (("depth", ["--sequence_align"], "needs --sequence"),
                              ("depth", ["--sequence", "--sequence_align", "--align_iters", "40"], "iters"),
                              ("depth", ["--sequence", "--sequence_align", "--align_delta", "0"], "delta"),
                              ("depth", ["--sequence", "--sequence_align", "--align_reference", "last"], "invalid choice"),
                              ("normals", ["--sequence", "--sequence_align"], "unrecognized arguments"),
                              ("iid", ["--sequence", "--sequence_align"], "unrecognized arguments"),
                              ("normals", ["--sequence", "--align_delta", "0.1"], "unrecognized arguments")):
        pipe = _FakeCliPipe()
        with pytest.raises(SystemExit) as e:
            cli.main(kind, base + extra, pipeline=pipe)
        assert e.value.code == 2 and word in capsys.readouterr().err and pipe.calls == []


def test_the_launchers_are_untouched_and_reach_the_flags():
    for kind in ("depth", "normals", "iid"):
        src = open(os.path.join(ROOT, "script", kind, "run.py")).read()
        assert "align" not in src and "cli" in src


# ---- the C host example ------------------------------------------------------------------------------------------------------------

def test_the_c_host_example_compiles(tmp_path):
    c_hosts.compile_only(os.path.join(ROOT, "examples", "host_align.cpp"), tmp_path / "host_align.o")
    assert os.path.getsize(tmp_path / "host_align.o") > 0
    assert "host_align" in open(os.path.join(ROOT, "README.md")).read()


# ---- the restatement's own properties ----------------------------------------------------------------------------------------------

def test_the_restatement_is_robust_where_least_squares_is_not():
    d, ref, s_true = robustness_scene()
    s, t, flag = align_fit_reference(d, ref, iters=4, start=(1.0, 0.0), delta=0.05)
    assert flag == 0 and abs(s - s_true) <= 0.03
    s_ls, _, flag = align_fit_reference(d, ref, iters=0)
    assert flag == 0 and abs(s_ls - s_true) > 0.2
    # the undisturbed scene: both recover it
    d2 = d.copy()
    d2[:len(d) // 5] = ((ref[:len(d) // 5].astype(np.float64) - 0.07) / 0.8).astype(np.float32)
    for iters in (0, 4):
        s, t, flag = align_fit_reference(d2, ref, iters=iters)
        assert flag == 0 and abs(s - 0.8) <= 0.005 and abs(t - 0.07) <= 0.005


def test_the_restatement_s_rules():
    g = np.random.default_rng(5)
    ref = g.random(200).astype(np.float32)
    d = ((ref - 0.1) / 2).astype(np.float32)
    # exact data: every mode recovers (2, 0.1); pixels that are masked or not finite do not count
    for kw in (dict(iters=0), dict(iters=3), dict(iters=2, start="ls"), dict(iters=8, start=(5.0, -1.0), delta=10.0)):
        s, t, flag = align_fit_reference(d, ref, **kw)
        assert flag == 0 and abs(s - 2) <= 1e-5 and abs(t - 0.1) <= 1e-5, kw
    bad_d, bad_ref, mask = d.copy(), ref.copy(), np.ones(200, np.uint8)
    bad_d[3], bad_d[4], bad_ref[5], bad_ref[6] = np.nan, np.inf, -np.inf, np.nan
    bad_d[7], mask[7] = 1e6, 0
    keep = np.ones(200, bool)
    keep[3:8] = False
    assert align_fit_reference(bad_d, bad_ref, mask, iters=0) == align_fit_reference(d[keep], ref[keep], iters=0)
    # without the shift: s = Sdg / Sdd, t = 0
    s, t, flag = align_fit_reference(d, 3 * d, fit_shift=False, iters=2)
    assert flag == 0 and t == 0.0 and abs(s - 3) <= 1e-6
    # degenerate: constant d, one pixel, everything masked, a slope <= 0, an all-NaN reference
    for name, dd, rr, mm in (("constant", np.full(50, 0.3), ref[:50], None), ("one pixel", d[:1], ref[:1], None),
                             ("masked", d, ref, np.zeros(200, np.uint8)), ("negative", d, -d, None), ("nan", d, np.full(200, np.nan), None)):
        for kw in (dict(iters=0), dict(iters=4), dict(iters=4, start="ls"), dict(iters=4, fit_shift=False)):
            if name == "constant" and not kw.get("fit_shift", True):
                continue   # (a constant d is no obstacle to a fit of the scale alone)
            assert align_fit_reference(dd, rr, mm, **kw) == (1.0, 0.0, 1), (name, kw)
    # the apply: fp64 product and sum, one rounding, the clamp keeps NaN
    x = np.array([0.25, -1.0, np.nan, np.inf, -np.inf, 3.0], np.float32)
    out = align_apply_reference(x, (2.0, 0.5), clip=(0.0, 1.0))
    assert out.dtype == np.float32 and np.array_equal(out, np.array([1.0, 0.0, np.nan, 1.0, 0.0, 1.0], np.float32), equal_nan=True)
    assert np.array_equal(align_apply_reference(x, (2.0, 0.5), use_shift=False), (x * 2).astype(np.float32), equal_nan=True)
    assert np.array_equal(align_apply_reference(x, (1.0, 0.0)), x, equal_nan=True)
