"""Host checks of image sequences, no GPU: the three C entry points are declared, bound and exported by both operand
libraries without touching the ABI version or the op kinds; ``mg_latent_carry`` refuses bad arguments before any GPU work;
``sequence=`` and ``map_video`` refuse what they must before anything is launched (stand-in pipelines whose engines are
namespaces); ``--sequence`` reaches ``map_video`` with one ``NativeNoise(seed + k)`` per frame and leaves the plain command line on
``map_images``; a frame that fails in one lane of ``map_video`` still lets the earlier frame out, aborts the turnstile and leaves
no thread.  Every wait carries ``CAP`` seconds: a cap against deadlock, not a measurement."""
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
from marigold_amd.pipeline import (MarigoldDepthOutput, MarigoldDepthPipeline, MarigoldIIDPipeline, MarigoldNormalsPipeline,
                                   SequenceState)
from marigold_amd.schedulers import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 20.0
# the op kinds as they were before sequences: the carry kernel is a plain C call, not a kind
OP_NAMES = {"igemm", "gn_stats", "gn_finalize", "gn_apply", "flash_attn64", "softmax_rows", "gn_slab", "rowgemm", "flash_attn512",
            "sched_step", "linear_small_m", "latent_1x1", "post_nchw", "im2col_small", "conv3x3", "conv3x3_head", "ens_depth_stats",
            "ens_depth_median", "ens_depth_norm", "ens_normals", "resize", "colorize", "eval_depth_ls", "eval_depth_metrics",
            "eval_normals", "memset", "copy", "iidscore_prep", "iidscore_psnr", "iidscore_ssim", "iid_vis", "rgb_prep", "normals_vis",
            "randn", "ens_iid"}


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


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------

def test_prototypes_bindings_and_exports():
    hdr = open(os.path.join(ROOT, "include", "marigold_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int mg_latent_carry(float* x, const float* prev, int64_t n, float strength, void* stream);" in flat
    assert "int mg_model_seq_reset(mg_model* m);" in flat
    out = re.search(r"int mg_model_predict_out\((.*?)\);", flat).group(1)
    nxt = re.search(r"int mg_model_predict_next\((.*?)\);", flat).group(1)
    assert nxt == out + ", float strength"   # exactly mg_model_predict_out's arguments, then the strength
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr)
    for f16 in (False, True):
        lib = L.load(f16)
        for name in ("mg_latent_carry", "mg_model_seq_reset", "mg_model_predict_next"):
            assert name in L.EXPORTS and hasattr(lib, name)
        assert lib.mg_abi_version() == 4 == L.ABI_VERSION
        assert lib.mg_model_predict_next.argtypes == lib.mg_model_predict_out.argtypes + [ctypes.c_float]
        assert lib.mg_latent_carry.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]
    assert ctypes.sizeof(L.MgOp) == 360
    assert set(L.OP_NAMES.values()) == OP_NAMES


@pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
def test_latent_carry_refuses_bad_arguments_before_any_gpu_work(f16):
    """No GPU is here: a call that got as far as a launch would fail differently, so the message proves where it stopped."""
    lib = L.load(f16)
    buf = (ctypes.c_float * 8)()
    x = ctypes.addressof(buf)

    def refused(args, *words):
        rc = lib.mg_latent_carry(*args, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_latent_carry:") and all(w in msg for w in words), (rc, msg)

    refused((x, x, -1, 0.1), "-1")
    refused((None, x, 4, 0.1), "null pointer")
    refused((x, None, 4, 0.1), "null pointer")
    for bad in (-0.25, 1.5, float("nan"), float("inf")):
        refused((x, x, 4, bad), "strength", "[0, 1]")
        refused((x, x, 0, bad), "strength")     # the strength is checked whatever n is
    assert lib.mg_latent_carry(None, None, 0, 0.5, None) == 0   # n == 0: a no-op, pointers and all
    assert lib.mg_latent_carry(x, x, 0, 0.0, None) == 0 and lib.mg_latent_carry(x, x, 0, 1.0, None) == 0
    assert list(buf) == [0.0] * 8


def test_sequence_calls_refuse_a_null_model():
    lib = L.load()
    assert lib.mg_model_seq_reset(None) != 0 and b"mg_model_seq_reset" in lib.mg_last_error()
    assert lib.mg_model_predict_next(None, None, 1, 8, 8, 0, 0, 0, None, None, None, None, None, None, None, None, 0.1) != 0
    assert lib.mg_last_error().decode().startswith("mg_model_predict_next:")


# ---- SequenceState, sequence=, map_video: the refusals -----------------------------------------------------------------------------

def _engine(name, device, launched):
    """An engine stand-in: anything a launch would need raises and is recorded."""
    def replica():
        return _engine(name + "'", device, launched)

    def boom(*a, **k):
        launched.append(name)
        raise AssertionError(f"{name}: reached a launch")
    vae_cfg = SimpleNamespace(block_out_channels=(1, 1, 1, 1))
    return SimpleNamespace(name=name, device=device, replica=replica, config=vae_cfg, encode_rgb_latent=boom, denoise_program=boom,
                           set_context=boom, f16=False, dtype=torch.bfloat16)


def _stand_in(cls=MarigoldDepthPipeline, **kw):
    launched = []
    device = SimpleNamespace(type="cuda")
    if cls is MarigoldIIDPipeline:
        unet = _engine("unet", device, launched)
        unet.config = SimpleNamespace(in_channels=12, out_channels=8)
        pipe = cls(unet, _engine("vae", device, launched), DDIMScheduler(), default_denoising_steps=2, default_processing_resolution=0,
                   empty_text_embed=torch.zeros(1, 2, 4), target_properties={"target_names": ["albedo", "material"]})
    else:
        pipe = cls(_engine("unet", device, launched), _engine("vae", device, launched), DDIMScheduler(), default_denoising_steps=2,
                   default_processing_resolution=0, empty_text_embed=torch.zeros(1, 2, 4), **kw)
    pipe._preprocess = lambda *a, **k: launched.append("preprocess") or (_ for _ in ()).throw(AssertionError("reached preprocessing"))
    pipe.launched = launched
    return pipe


FRAME = torch.zeros(1, 3, 64, 128, dtype=torch.uint8)


def test_sequence_state_surface():
    st = SequenceState()
    assert st.strength == 0.1 and st.latent is None and st.frames == 0
    assert SequenceState(strength=0.5).strength == 0.5 and SequenceState(0).strength == 0.0 and SequenceState(1).strength == 1.0
    for bad in (-0.1, 1.01, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            SequenceState(bad)
    st.latent, st.frames, st._sig = torch.zeros(1, 4, 8, 16), 3, ("depth", (1, 4, 8, 16), "dev")
    st.reset()
    assert st.latent is None and st.frames == 0 and st._sig is None
    import marigold_amd
    assert marigold_amd.SequenceState is SequenceState


@pytest.mark.parametrize("cls", [MarigoldDepthPipeline, MarigoldNormalsPipeline, MarigoldIIDPipeline], ids=["depth", "normals", "iid"])
def test_call_refuses_before_any_launch(cls):
    pipe = _stand_in(cls)
    C = 8 if cls is MarigoldIIDPipeline else 4
    with pytest.raises(ValueError, match="init_latents"):
        pipe(FRAME, sequence=SequenceState(), init_latents=torch.zeros(1, C, 8, 16))
    # a state that carries another shape: another processed size, another E, another kind
    dev = pipe.device
    for sig in ((pipe._kind, (1, C, 8, 8), dev), (pipe._kind, (2, C, 8, 16), dev), ("other", (1, C, 8, 16), dev)):
        st = SequenceState()
        st.latent, st.frames, st._sig = torch.zeros(sig[1]), 1, sig
        with pytest.raises(ValueError, match="reset"):
            pipe(FRAME, sequence=st)
        assert st.frames == 1
    pipe._sharded = lambda: True
    with pytest.raises(ValueError, match="member-parallel"):
        pipe(FRAME, sequence=SequenceState())
    with pytest.raises(TypeError, match="SequenceState"):
        _stand_in(cls)(FRAME, sequence=object())
    assert pipe.launched == []
    # the matching state goes on - into the stand-in's preprocessing, which is where a real call starts its GPU work
    st = SequenceState()
    st.latent, st.frames, st._sig = torch.zeros(1, C, 8, 16), 1, (pipe._kind, (1, C, 8, 16), dev)
    pipe._sharded = lambda: False
    with pytest.raises(AssertionError, match="reached preprocessing"):
        pipe(FRAME, sequence=st)


def test_map_video_refusals():
    pipe = _stand_in()
    frames = [FRAME] * 3
    with pytest.raises(ValueError, match="images_per_program"):
        pipe.map_video(frames, images_per_program=2)
    with pytest.raises(ValueError, match="init_latents"):
        pipe.map_video(frames, init_latents=torch.zeros(1, 4, 8, 16))
    with pytest.raises(ValueError, match="generators"):
        pipe.map_video(frames, in_flight=2, generator=torch.Generator())
    with pytest.raises(ValueError, match="in_flight"):
        pipe.map_video(frames, in_flight=0)
    with pytest.raises(ValueError, match="strength"):
        pipe.map_video(frames, strength=2.0)
    with pytest.raises(ValueError, match="2 generators for 3 frames"):
        pipe.map_video(frames, generators=[None, None])
    pipe._sharded = lambda: True
    with pytest.raises(ValueError, match="member-parallel"):
        pipe.map_video(frames)
    assert pipe.launched == []


# ---- map_video over stand-in lanes -------------------------------------------------------------------------------------------------

SLEEP_MS = (9, 2, 6, 1, 8, 3, 5)


class _VideoStandIn(MarigoldDepthPipeline):
    """``_SettingsStandIn`` of tests/test_lanes_host.py for sequences: a call sleeps (its encode), takes its frame's turn, 'denoises' -
    reads the state, writes it - hands the turn on, sleeps again (its decode) and returns what it saw."""

    def __init__(self, fail_at=None):
        device = SimpleNamespace(type="cuda")

        def engine(name):
            return SimpleNamespace(name=name, device=device, replica=lambda: engine(name + "'"), config=SimpleNamespace(block_out_channels=(1,)))
        super().__init__(engine("unet"), engine("vae"), DDIMScheduler(), default_denoising_steps=2, default_processing_resolution=0,
                         empty_text_embed=torch.zeros(1, 2, 4))
        self.fail_at, self.order, self.refused = fail_at, [], []

    def _lane_stream(self):
        return None

    def _lane_contexts(self, streams):
        return [contextlib.nullcontext() for _ in streams], lambda: None

    def __call__(self, image, sequence=None, generator=None, **kw):
        k = int(image[0, 0, 0, 0])
        time.sleep(SLEEP_MS[k % 7] / 1000.0)
        turn = self._sequence_turn
        if turn is not None:
            try:
                turn[0].wait(turn[1], timeout=CAP)
            except RuntimeError:
                self.refused.append(k)
                raise
        if k == self.fail_at:
            time.sleep(0.02)   # the later frames are at the turnstile by now
            raise OSError(f"frame {k} failed")
        seen = sequence.frames
        self.order.append(k)
        sequence.frames += 1
        if turn is not None:
            turn[0].done(turn[1])
        time.sleep(SLEEP_MS[(k + 3) % 7] / 1000.0)
        return (k, seen, generator, turn is not None and turn[1], self.unet.name)


def _frames(n, hw=(64, 128)):
    for k in range(n):
        yield torch.full((1, 3) + hw, k, dtype=torch.uint8)


@pytest.mark.parametrize("n_lanes", [1, 2, 3])
def test_map_video_orders_the_denoise_stage_and_keeps_input_order(n_lanes):
    def scenario():
        before = set(threading.enumerate())
        pipe = _VideoStandIn()
        pulled = []

        def lazy():
            for f in _frames(7):
                pulled.append(len(pulled))
                yield f
        gen = pipe.map_video(lazy(), strength=0.5, in_flight=n_lanes, generators=(f"g{k}" for k in range(7)), ensemble_size=1)
        assert pulled == []   # nothing is consumed before the first output is asked for
        first = next(gen)
        assert len(pulled) <= 1 + n_lanes   # consumed lazily: at most one frame per lane ahead of the caller
        outs = [first] + list(gen)
        assert [o[0] for o in outs] == list(range(7)) and [o[1] for o in outs] == list(range(7))   # frame k saw k frames before it
        assert [o[2] for o in outs] == [f"g{k}" for k in range(7)]
        assert pipe.order == list(range(7))
        if n_lanes == 1:
            assert all(o[3] is False for o in outs) and "_sequence_turn" not in vars(pipe)
        else:
            assert [o[3] for o in outs] == list(range(7)) and len({o[4] for o in outs}) > 1
            assert "_sequence_turn" not in vars(pipe) and pipe._sequence_turn is None   # the turns sat on per-call views
        assert [t for t in threading.enumerate() if t not in before and t is not threading.current_thread()] == []
    _capped(scenario)


def test_a_frame_that_fails_in_a_lane_lets_the_earlier_frame_out_and_aborts_the_turnstile():
    def scenario():
        before = set(threading.enumerate())
        pipe = _VideoStandIn(fail_at=1)
        got = []
        with pytest.raises(OSError, match="frame 1 failed"):
            for out in pipe.map_video(_frames(7), in_flight=3):
                got.append(out[0])
        assert got == [0] and pipe.order == [0]
        assert pipe.refused and all(k > 1 for k in pipe.refused)   # the lanes at the turnstile raised; no cap ran out
        assert [t for t in threading.enumerate() if t not in before and t is not threading.current_thread()] == []
    _capped(scenario)


def test_map_video_refuses_a_frame_of_another_processed_size_and_too_few_generators():
    def scenario():
        pipe = _VideoStandIn()

        def frames():
            yield from _frames(2)
            yield torch.full((1, 3, 64, 96), 2, dtype=torch.uint8)
        got = []
        with pytest.raises(ValueError, match="processed size"):
            for out in pipe.map_video(frames(), in_flight=2):
                got.append(out[0])
        assert got == [0, 1]
        got = []
        with pytest.raises(ValueError, match="fewer generators"):
            for out in pipe.map_video(_frames(3), in_flight=1, generators=iter(["a", "b"])):
                got.append(out[0])
        assert got == [0, 1]
    _capped(scenario)


# ---- the command line --------------------------------------------------------------------------------------------------------------

class _FakeCliPipe:
    scale_invariant = shift_invariant = True
    default_denoising_steps, default_processing_resolution = 4, 768

    def __init__(self):
        self.calls = []

    def _out(self):
        from PIL import Image
        return MarigoldDepthOutput(np.linspace(0, 1, 48, dtype=np.float32).reshape(6, 8), Image.fromarray(np.zeros((6, 8, 3), np.uint8)), None)

    def map_images(self, images, in_flight=None, generators=None, **kw):
        images, generators = list(images), list(generators)
        self.calls.append(("map_images", len(images), in_flight, generators, kw))
        return [self._out() for _ in images]

    def map_video(self, frames, strength=0.1, in_flight=None, generators=None, **kw):
        frames, generators = list(frames), list(generators)
        self.calls.append(("map_video", len(frames), strength, in_flight, generators, kw))
        return [self._out() for _ in frames]


def test_cli_sequence_runs_map_video_with_native_seeds(tmp_path):
    from PIL import Image
    from marigold_amd import cli
    from marigold_amd.noise import NativeNoise
    a = cli.build_parser("depth").parse_args(["--input_rgb_dir", "i", "--output_dir", "o"])
    assert a.sequence is False and a.carry_strength == 0.1
    inp = tmp_path / "in"
    inp.mkdir()
    for name in ("f002.png", "f000.png", "f001.png"):
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / name)
    base = ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out")]
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--sequence", "--seed", "40", "--carry_strength", "0.25", "--maps_in_flight", "2"], pipeline=pipe) == 0
    (name, n, strength, in_flight, gens, kw), = pipe.calls
    assert (name, n, strength, in_flight) == ("map_video", 3, 0.25, 2)
    assert all(isinstance(g, NativeNoise) for g in gens) and [g.seed for g in gens] == [40, 41, 42] and all(g.next_stream == 0 for g in gens)
    assert kw["ensemble_size"] == 1 and kw["match_input_res"] is True and kw["color_map"] == "Spectral" and "images_per_program" not in kw
    for k in range(3):   # the usual per-frame files
        assert (tmp_path / "out" / "depth_npy" / f"f00{k}_depth.npy").exists() and (tmp_path / "out" / "depth_bw" / f"f00{k}_depth.png").exists()
    # defaults: the recipe's strength, the engine's lane count, no generators without a seed
    pipe = _FakeCliPipe()
    assert cli.main("depth", base + ["--sequence"], pipeline=pipe) == 0
    assert pipe.calls[0][:4] == ("map_video", 3, 0.1, None) and pipe.calls[0][4] == [None] * 3
    with pytest.raises(ValueError, match="images_per_program"):
        cli.main("depth", base + ["--sequence", "--images_per_program", "2"], pipeline=_FakeCliPipe())


def test_cli_without_sequence_sees_map_images_as_before(tmp_path):
    from PIL import Image
    from marigold_amd import cli
    inp = tmp_path / "in"
    inp.mkdir()
    for name in ("b.png", "a.png"):
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(inp / name)
    pipe = _FakeCliPipe()
    assert cli.main("depth", ["--input_rgb_dir", str(inp), "--output_dir", str(tmp_path / "out"), "--seed", "7", "--carry_strength", "0.9"],
                    pipeline=pipe) == 0
    (name, n, in_flight, gens, kw), = pipe.calls
    assert (name, n, in_flight) == ("map_images", 2, None)
    assert all(isinstance(g, torch.Generator) and g.initial_seed() == 7 for g in gens)
    assert set(kw) == {"denoising_steps", "ensemble_size", "processing_res", "match_input_res", "batch_size", "show_progress_bar",
                       "resample_method", "color_map"}
