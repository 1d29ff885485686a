"""``MarigoldDepthPipeline`` / ``MarigoldNormalsPipeline`` with the reference's call surface
(marigold/marigold_depth_pipeline.py:154-338, marigold/marigold_normals_pipeline.py:139-308):
same arguments, defaults, asserts / exceptions / warnings and output containers, on top of the
MI355X engine (HIP programs for VAE encode, the whole T-step denoising loop, VAE decode and the
ensembling).  Differences that are deliberate and documented in DESIGN.md:

* the image is VAE-encoded once per call, not once per ensemble member (the reference encodes E
  identical copies, :258 / :427);
* all members of a batch run through one native denoising program (no per-step Python);
* optional member parallelism over the GPUs of a node (``enable_member_parallel``): members are
  sharded over ranks and collected with ONE gather (RCCL over xGMI) before aggregation;
* ``init_latents`` (extension) lets callers supply the initial noise for parity runs;
* ``generator=NativeNoise(seed)`` (extension) draws the noise with the library's own generator (noise.py), as a C host does;
* ``map_images(images_per_program=k)`` (extension) runs the members of up to k same-size images in one program;
* ``sequence=SequenceState()`` / ``map_video`` (extension) carry each frame's denoised latent into the next frame's initial noise
  (DESIGN.md 6c);
* ``align=DepthAlignState()`` / ``map_video(align=True)`` (extension, depth) fit every frame's map, scale and shift, robustly to the
  frame before on the device, so that the range stops changing from frame to frame (align.py);
* ``predict_tiled`` (extension) cuts a large picture into overlapping tiles of the training size, predicts them through
  ``map_images`` and stitches them on the device (tiles.py).
"""
import contextlib
import copy
import functools
import logging
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch
from PIL import Image

from . import _lib as L
from . import dist as mdist
from . import ops as O
from . import tiles as tiling
from .align import DepthAlignState, settings as align_settings
from .ensemble import ensemble_depth, ensemble_iid, ensemble_normals
from .guided import guided_upsample, settings as guided_settings
from .lanes import Turnstile as _Turnstile, Turnstiles as _Turnstiles, run_lanes
from .modules import AutoencoderKLHIP, UNet2DConditionModelHIP
from .noise import NativeNoise
from .schedulers import DDIMScheduler, LCMScheduler
from .util.batchsize import find_batch_size
from .util.image_util import (chw2hwc, colorize_depth_device, colorize_depth_maps, get_tv_resample_method,
                              iid_visualization_device, max_res_size, normals_visualization_device, pil_to_tensor,
                              prepare_rgb_device, resize, resize_max_res)


@dataclass
class MarigoldDepthOutput:
    """depth_np [H,W] in [0,1]; depth_colored PIL RGB | None; uncertainty [H,W] | None
    (reference :60-75).  ``degenerate_tiles`` (extension): None, or - from ``predict_tiled`` - how many tiles could not be fitted to
    the guide (constant, no valid pixel, a slope <= 0) and were replaced by the guide's mean over them.  ``align_coef`` / ``align_flag``
    (extension): None, or - from a call with ``align=`` - the DEVICE tensors of the frame's fit, fp64 [2] (s, t) and int32 [1]
    (1: degenerate, the frame passed unchanged); reading them is the caller's choice."""
    depth_np: np.ndarray
    depth_colored: Union[None, Image.Image]
    uncertainty: Union[None, np.ndarray]
    degenerate_tiles: Optional[int] = None
    align_coef: Optional[torch.Tensor] = None
    align_flag: Optional[torch.Tensor] = None


@dataclass
class MarigoldNormalsOutput:
    """normals_np [3,H,W] unit vectors in [-1,1]; normals_img PIL; uncertainty | None
    (normals reference :59-74)."""
    normals_np: np.ndarray
    normals_img: Image.Image
    uncertainty: Union[None, np.ndarray]


class SequenceState:
    """What a sequence of frames carries from one call to the next (``pipe(frame, sequence=state)``, ``map_video``): the denoised
    latent of the frame before.  Frame k starts from ``(1 - strength) * noise + strength * latent`` (``mg_latent_carry``); the first
    frame of a state starts from the noise alone, bit for bit the call without a state.

    ``latent``: None, or the fp32 device tensor [E, C, h, w] of the last frame's members - the state's own memory, one of the two
    buffers it writes in turn: valid until the frame after next is predicted (clone it to keep it).  ``frames``: how many frames
    have been predicted.  ``reset()`` starts a new sequence.

    Buffer lifetime: frame k reads buffer (k - 1) % 2 and writes buffer k % 2 on the stream it runs on, and records an event
    behind its write; frame k + 1, on whichever stream, makes its stream wait for that event first.  Every access is therefore
    ordered by the chain of events, and the buffers are never returned to torch's allocator while the state is in use."""

    def __init__(self, strength=0.1):
        strength = float(strength)
        if not 0.0 <= strength <= 1.0:
            raise ValueError(f"SequenceState: strength must be in [0, 1] (got {strength})")
        self.strength = strength
        self.latent = None
        self.frames = 0
        self._sig = None             # (pipeline kind, shape of the latent, device): what the next frame must match
        self._ring = [None, None]
        self._event = None           # recorded behind the last frame's copy into its buffer (kept over a reset: the buffers are reused)

    def reset(self):
        self.latent, self.frames, self._sig = None, 0, None

    def _check(self, sig):
        if self._sig is not None and self._sig != sig:
            raise ValueError(f"sequence: the state carries a {self._sig[0]} latent of shape {tuple(self._sig[1])} on {self._sig[2]}, this "
                             f"frame needs a {sig[0]} latent of shape {tuple(sig[1])} on {sig[2]} (reset() starts a new sequence)")


class _FrameCarry:
    """One frame's turn on a ``SequenceState``, around the denoising programs of its members (``single_infer``): ``blend`` before a
    program runs, ``keep`` after it.  The first ``blend`` takes the frame's turn (``map_video`` lanes) and makes the stream wait for
    the event of the frame before; the last ``keep`` records this frame's event and hands the turn on.  Nothing here waits on the
    host for the GPU."""

    def __init__(self, state, sig, lib, turn=None):
        self.state, self.sig, self.lib, self.turn = state, sig, lib, turn
        self.new = None

    def _enter(self):
        st = self.state
        if self.turn is not None:
            self.turn[0].wait(self.turn[1])
        st._check(self.sig)
        stream = torch.cuda.current_stream(self.sig[2])
        if st._event is not None:
            stream.wait_event(st._event)
        slot = st.frames % 2
        buf = st._ring[slot]
        if buf is None or tuple(buf.shape) != tuple(self.sig[1]) or buf.device != self.sig[2]:
            buf = st._ring[slot] = torch.empty(tuple(self.sig[1]), dtype=torch.float32, device=self.sig[2])
        buf.record_stream(stream)   # (should the state be dropped with work of this stream still queued)
        self.new = buf

    def blend(self, x, rows):
        if self.new is None:
            self._enter()
        prev = self.state.latent
        if prev is not None:
            prev.record_stream(torch.cuda.current_stream(self.sig[2]))
            part = prev[rows]
            L.check(self.lib.mg_latent_carry(x.data_ptr(), part.data_ptr(), x.numel(), self.state.strength, O.current_stream_handle()),
                    "mg_latent_carry", self.lib)

    def keep(self, x, rows, last):
        self.new[rows].copy_(x)
        if last:
            st = self.state
            st.latent, st._sig, st.frames = self.new, self.sig, st.frames + 1
            st._event = torch.cuda.Event()
            st._event.record(torch.cuda.current_stream(self.sig[2]))
            if self.turn is not None:
                self.turn[0].done(self.turn[1])


@contextlib.contextmanager
def _on_stream(device, stream, caller):
    """``with`` this in a lane's thread: its work goes to the lane's HIP stream, behind what the caller has queued on its own."""
    torch.cuda.set_device(device)
    stream.wait_stream(caller)   # inputs the caller produced on its stream
    with torch.cuda.stream(stream):
        yield


class _MarigoldPipelineBase:
    latent_scale_factor = 0.18215
    _kind = "depth"
    _ckpt_hint = "prs-eth/marigold-depth-v1-1"
    _target_latent_channels = 4    # latent channels the UNet predicts (4 per modality)
    _pred_channels = 1             # channels of one decoded prediction
    _gather_turn = None            # (turnstile, map index): set only on the per-call view a lane of map_images runs on
    _sequence_turn = None          # (turnstile, frame index): likewise, on the view a lane of map_video runs on
    _align_turn = None             # (turnstile, frame index): likewise, for the align stage of map_video(align=...)

    def __init__(self, unet: UNet2DConditionModelHIP, vae: AutoencoderKLHIP,
                 scheduler: Union[DDIMScheduler, LCMScheduler], text_encoder=None, tokenizer=None,
                 scale_invariant: Optional[bool] = True, shift_invariant: Optional[bool] = True,
                 default_denoising_steps: Optional[int] = None,
                 default_processing_resolution: Optional[int] = None, empty_text_embed=None):
        self.unet, self.vae, self.scheduler = unet, vae, scheduler
        self.text_encoder, self.tokenizer = text_encoder, tokenizer
        self.scale_invariant = scale_invariant
        self.shift_invariant = shift_invariant
        self.default_denoising_steps = default_denoising_steps
        self.default_processing_resolution = default_processing_resolution
        self.config = dict(scale_invariant=scale_invariant, shift_invariant=shift_invariant,
                           default_denoising_steps=default_denoising_steps,
                           default_processing_resolution=default_processing_resolution)
        self.empty_text_embed = empty_text_embed
        self._member_group = None
        self._member_parallel = False
        self._member_root = None
        self._member_force = False
        self._lanes = []   # map_images' lanes: (unet and vae engine, stream)

    # ---- diffusers.DiffusionPipeline surface the callers use ---------------------------------
    @property
    def device(self):
        return self.unet.device

    @property
    def dtype(self):
        """Compute dtype of the engine (bf16 operands, fp32 accumulation)."""
        return self.unet.dtype

    # Tensors at the pipeline boundary - the normalised image, the initial latents, the LCM per-step noise, the
    # predictions - are fp32 like the reference's default pipeline (script/depth/run.py:203-215 loads fp32 unless
    # --fp16); the engine's boundary convolutions convert them on the fly, so nothing is rounded to bf16 on the way in.
    io_dtype = torch.float32
    # The reference draws the initial latents and the LCM per-step noise in the MODEL dtype (:430-435:
    # ``torch.randn(..., dtype=self.dtype, generator=generator)``): a pipeline loaded with
    # ``from_pretrained(torch_dtype=torch.float16 | torch.bfloat16)`` (script/depth/run.py:203-214, ``--fp16``) consumes the
    # generator as 16-bit draws - a different random stream from the fp32 one.  ``noise_dtype`` reproduces that choice:
    # fp32 by default (the reference's default load), the caller's ``torch_dtype`` when one was given; the draws are
    # widened to fp32 on their way into the engine's latent buffers (exact for both 16-bit types).
    noise_dtype = torch.float32

    def _randn(self, shape, generator):
        if isinstance(generator, NativeNoise):   # the library's generator: the next stream of its seed, fp32 rounded to io_dtype in the store
            return generator.randn(shape, dtype=self.io_dtype, device=self.device)
        return torch.randn(tuple(shape), device=self.device, dtype=self.noise_dtype, generator=generator).to(self.io_dtype)

    def to(self, device):
        self.unet.to(device)
        self.vae.to(device)
        self._lanes = []   # engine replicas of map_images belong to the device they were made on
        return self

    def set_vae(self, vae):
        """Swap the pipeline's autoencoder (``AutoencoderKLHIP`` or ``AutoencoderTinyHIP``, e.g. from ``checkpoint.load_tiny_vae``)
        for one with the UNet's operand type; it is moved to the pipeline's device.  The cached lanes of ``map_images`` hold
        replicas of the old one and are dropped."""
        if vae.dtype != self.unet.dtype:
            raise ValueError(f"set_vae: the VAE computes on {vae.dtype}, the UNet on {self.unet.dtype}")
        if self.unet.device.type == "cuda" and vae.device != self.unet.device:
            vae.to(self.unet.device)
        self.vae = vae
        self._lanes = []
        return self

    @classmethod
    def from_pretrained(cls, path, variant=None, torch_dtype=None, **kw):
        from .checkpoint import load_pipeline
        return load_pipeline(cls, path, variant=variant, torch_dtype=torch_dtype, **kw)

    def enable_xformers_memory_efficient_attention(self):
        """No-op: the engine's attention is already a fused flash kernel (run.py:217-220)."""

    def set_progress_bar_config(self, **kw):
        pass

    def enable_member_parallel(self, group=None, root=None, force_collective=False):
        """Shard ensemble members over the ranks of ``group`` (torch.distributed; RCCL on GPUs).  ``force_collective``:
        take the sharded path - full-E noise draw sliced by member, ONE gather - even in a group of one rank (the RCCL
        path on a single GPU; results are those of the plain path bit for bit)."""
        self._member_group = group
        self._member_parallel = True
        self._member_root = root
        self._member_force = bool(force_collective) and mdist.is_on(group)

    def _sharded(self):
        return self._member_parallel and (mdist.world_size(self._member_group) > 1 or self._member_force)

    # ---- maps in flight ----------------------------------------------------------------------
    # The reference's scripts call the pipeline image by image (script/depth/run.py:231-262, script/depth/infer.py): every map waits
    # for the one before it.  One map alone leaves the MI355X partly idle wherever a launch is a single lockstep round of workgroups
    # whose HBM-bound epilogues follow their K loops, has a part-filled last round, or is a host-driven chain (the alignment
    # optimiser's ~80 evaluations per map): a SECOND, independent map on another HIP stream fills those holes (DESIGN.md section 6b;
    # tools/inflight_bench.py: +9 % maps/s at E = 10, every map bit-identical to the one-at-a-time result).  288 GB of HBM hold the
    # second set of workspaces (23 GB at 768 x 768, E = 10) many times over; the weights are shared.
    # A GPU that holds eight members or fewer (small ensembles, the shards of the member-parallel path) has more and longer holes
    # per map - its launches are single part-filled rounds - and takes a THIRD lane: same box, interleaved
    # (profiles/r6_inflight_by_ensemble.log) E = 1 / 2 / 3 / 5 / 6 / 8: 51.4 / 77.5 / 100.6 / 146.5 / 172.6 / 211.8 ms per map with two
    # lanes, 45.0 / 70.3 / 95.0 / 143.1 / 165.7 / 208.2 with three (a fourth: 48.4 / 70.7 / 94.2 / 142.4); at E = 10 the third lane
    # buys 0.4-0.5 %.
    default_maps_in_flight = 2
    small_ensemble_maps_in_flight = 3
    small_ensemble_members = 8

    def maps_in_flight_for(self, ensemble_size: int = 1) -> int:
        """The lane count ``map_images`` uses when the caller names none: by the members THIS GPU runs per map (the ensemble
        divided over the ranks of a member-parallel pipeline)."""
        world = mdist.world_size(self._member_group) if self._sharded() else 1
        local = -(-max(1, int(ensemble_size)) // max(1, world))
        return self.small_ensemble_maps_in_flight if local <= self.small_ensemble_members else self.default_maps_in_flight

    def _view(self, unet, vae):
        """A shallow copy of this pipeline as it is now, over the given engines and with a scheduler object of its own."""
        v = copy.copy(self)
        v.unet, v.vae, v.scheduler, v._lanes = unet, vae, copy.deepcopy(self.scheduler), []
        return v

    def replicate(self):
        """Another pipeline over the same device-resident weights: engine replicas (own workspaces, programs, launch-private
        state) and its own scheduler object - what a caller's second thread runs a map on."""
        return self._view(self.unet.replica(), self.vae.replica())

    def _lane_resources(self, n):
        """The first n lanes, (engines, stream) each: lane 0 over the pipeline's own unet / vae engines, the others over
        replicas.  All that ``map_images`` keeps between calls: the pipelines its lanes run on are views made per call."""
        while len(self._lanes) < n:
            unet, vae = (self.unet.replica(), self.vae.replica()) if self._lanes else (self.unet, self.vae)
            self._lanes.append((SimpleNamespace(unet=unet, vae=vae), self._lane_stream()))
        return self._lanes[:n]

    def _lane_stream(self):
        return torch.cuda.Stream(device=self.device)

    def _lane_contexts(self, streams):
        """-> (a context per lane, for its thread; what the caller calls once they are all left)"""
        caller = torch.cuda.current_stream(self.device)
        return [_on_stream(self.device, s, caller) for s in streams], lambda: [caller.wait_stream(s) for s in streams]

    def map_images(self, images, in_flight: Optional[int] = None, generators=None, images_per_program: int = 1,
                   **call_kwargs):
        """``(pipe(image, **call_kwargs) for image in images)`` with up to ``in_flight`` maps on the GPU at a time (default
        ``maps_in_flight_for(ensemble_size)``; 1 = one after the other on the caller's stream).  A generator: outputs come in input order
        as they complete, and ``images`` (any iterable) is consumed as lanes become free, at most one group per lane ahead of the caller.  ``generators``: one
        ``torch.Generator`` (or ``NativeNoise``, or None) per image - with several maps in flight a single shared generator would be consumed in
        completion order, so ``generator=`` is refused; every map is then bit-identical to what ``pipe(image, generator=g)``
        returns on its own.  Member-parallel pipelines (several ranks): every rank must call this with the same images and
        ``in_flight``; the lanes then issue their gathers strictly in map order, one at a time (``_Turnstile``), so the collective
        sequence is the same on every rank whichever lane finishes first.

        ``images_per_program`` = k > 1: up to k consecutive images of the same processed size share one VAE-encode program, one
        denoising program of k x ensemble_size members and one decode program (a change of size starts a new group); each image's
        noise is drawn from its own generator exactly as its lone call draws it, and each image gets the output its lone call
        returns, up to the arithmetic of the larger batch.  ``in_flight`` then counts programs (default
        ``maps_in_flight_for(k * ensemble_size)``).  Not with ``init_latents``, a shared ``generator`` or several ranks.  With
        ``batch_size=0`` a program holds at most 64 members at 768 x 768 (``find_batch_size``; more run as several programs of whole
        images); each lane keeps workspaces for its program's members."""
        k = int(images_per_program)
        if k < 1:
            raise ValueError(f"images_per_program must be >= 1 (got {images_per_program})")
        if call_kwargs.get("align") is not None:
            raise ValueError("map_images: align orders consecutive frames; use map_video(align=...) or call the pipeline frame by frame")
        if k > 1:
            if call_kwargs.get("init_latents") is not None:
                raise ValueError("map_images: init_latents cannot be combined with images_per_program > 1")
            if call_kwargs.get("generator") is not None:
                raise ValueError("map_images: pass `generators` (one per image) instead of a shared `generator` when "
                                 "images_per_program > 1")
            if self._sharded():
                raise ValueError("map_images: images_per_program > 1 is not available on a member-parallel pipeline")
        n = self._lane_count("map_images", "image", images, generators, in_flight,
                             functools.partial(self.maps_in_flight_for, k * call_kwargs.get("ensemble_size", 1)), k, call_kwargs)
        pairs = self._paired("map_images", "image", iter(images), None if generators is None else iter(generators))

        def groups():
            """[(image, generator)]: up to k consecutive images of one processed size"""
            group, size = [], None
            for image, g in pairs:
                image_size = self._processed_size(image, call_kwargs.get("processing_res")) if k > 1 else None
                if group and image_size != size:   # this image opens the next group
                    yield group
                    group = []
                group.append((image, g))
                size = image_size
                if len(group) == k:
                    yield group
                    group = []
            if group:
                yield group

        def run_one(pipe, group, index, turnstile):
            """-> the outputs of the group's images, in order"""
            kw = dict(call_kwargs)
            if len(group) > 1:
                return pipe._call_group([im for im, _ in group], None if generators is None else [g for _, g in group], kw)
            image, g = group[0]
            if generators is not None:
                kw["generator"] = g
            if turnstile is not None:
                pipe._gather_turn = (turnstile, index)   # on this call's view of the lane
            return [pipe(image, **kw)]

        return self._drive_lanes(groups(), n, self._sharded(), run_one)   # (a turnstile: the gathers, map by map)

    def _lane_count(self, caller, noun, items, generators, in_flight, default, per_lane, call_kwargs):
        """The checks ``map_images`` and ``map_video`` make of their arguments at the call -> the number of lanes.  ``default()``: the
        count when the caller names none; ``per_lane``: how many items a lane takes at a time."""
        n = default() if in_flight is None else int(in_flight)
        if n < 1:
            raise ValueError(f"in_flight must be >= 1 (got {in_flight})")
        if generators is not None and hasattr(items, "__len__") and hasattr(generators, "__len__") and len(items) != len(generators):
            raise ValueError(f"{len(generators)} generators for {len(items)} {noun}s")
        if hasattr(items, "__len__"):
            n = min(n, max(1, -(-len(items) // per_lane)))
        if self.device.type != "cuda":
            n = 1
        if n > 1 and call_kwargs.get("generator") is not None:
            raise ValueError(f"{caller}: pass `generators` (one per {noun}) instead of a shared `generator` when in_flight > 1")
        return n

    @staticmethod
    def _paired(caller, noun, items, generators):
        """(item, its generator | None) for every item; the two iterators advance together."""
        for item in items:
            g = None if generators is None else next(generators, StopIteration)
            if g is StopIteration:
                raise ValueError(f"{caller}: fewer generators than {noun}s")
            yield item, g

    def _drive_lanes(self, groups, n, ordered, run_one):
        """A generator over the outputs of ``run_one(view, group, k, turnstile)`` for group k = 0, 1 ... of the iterator ``groups``, on
        ``n`` lanes (``run_lanes``).  ``view``: the pipeline the lane runs on; ``turnstile``: with several lanes and ``ordered``, the
        ``Turnstile`` a stage of the calls passes in the order of k, else None; ``ordered`` = 2, 3 ...: that many stages, a
        ``Turnstiles`` with one turnstile each, which fail together."""
        take = functools.partial(next, enumerate(groups), None)   # -> (index, group) | None; one lane at a time (run_lanes)
        views, contexts, leave, turnstile = [self], [contextlib.nullcontext()], lambda: None, None   # one lane: inline, on this very object
        if n > 1:
            if self.empty_text_embed is None:
                self.encode_empty_text()   # what a lone call would write back to the pipeline
            lanes = self._lane_resources(n)
            views = [self._view(e.unet, e.vae) for e, _ in lanes]   # lane 0 too: no lane works on the caller's object
            contexts, leave = self._lane_contexts([stream for _, stream in lanes])
            turnstile = None if not ordered else _Turnstile() if ordered is True else _Turnstiles(_Turnstile() for _ in range(ordered))
        try:
            yield from run_lanes(contexts, take, lambda lane, group, k: run_one(views[lane], group, k, turnstile), turnstile)
        finally:
            leave()

    @staticmethod
    def _input_hw(image):
        """(height, width) of a PIL image or an image tensor."""
        if isinstance(image, Image.Image):
            return image.height, image.width
        if isinstance(image, torch.Tensor):
            return tuple(image.shape[-2:])
        raise TypeError(f"Unknown input type: {type(image) = }")

    def _processed_size(self, image, processing_res):
        """(height, width) ``_preprocess`` gives ``image``, without resampling it."""
        hw = self._input_hw(image)
        if processing_res is None:
            processing_res = self.default_processing_resolution
        return max_res_size(hw, processing_res) if processing_res > 0 else hw

    # ---- image sequences ---------------------------------------------------------------------
    # Frame k of a sequence starts from 0.9 noise + 0.1 x (denoised latent of frame k - 1) - the recipe Marigold's authors give for
    # frame-by-frame video - so consecutive maps stop flickering with the noise draw.  Only the DENOISE stage of frame k depends on
    # frame k - 1: preprocessing and the VAE encode run ahead of it, decode / ensemble / output stage beside the next frame's
    # denoise.
    def _frame_carry(self, sequence, init_latents, input_image, processing_res, ensemble_size):
        """``__call__``'s check of ``sequence=``, before anything is launched -> the frame's ``_FrameCarry`` | None."""
        if sequence is None:
            return None
        if not isinstance(sequence, SequenceState):
            raise TypeError(f"sequence must be a SequenceState (got {type(sequence).__name__})")
        if init_latents is not None:
            raise ValueError("sequence and init_latents cannot be combined: the sequence decides the initial latents")
        if self._sharded():
            raise ValueError("sequence is not available on a member-parallel pipeline")
        h, w = self._latent_hw(self._processed_size(input_image, processing_res))
        sig = (self._kind, (int(ensemble_size), self._target_latent_channels, h, w), self.device)
        sequence._check(sig)
        return _FrameCarry(sequence, sig, L.load(bool(getattr(self.unet, "f16", False))), self._sequence_turn)

    def frames_in_flight_for(self, ensemble_size: int = 1) -> int:
        """The lane count ``map_video`` uses when the caller names none: ``map_images``' - at 768 x 768, E = 1, three lanes beat one by
        more than the spread of alternated runs at T = 1, 4 and 10 (13.6 against 17.5, 32.3 against 35.2, 68.0 against 70.8 ms per frame;
        tools/sequence_bench.py, profiles/sequence_768.log)."""
        return self.maps_in_flight_for(ensemble_size)

    def map_video(self, frames, strength: float = 0.1, in_flight: Optional[int] = None, generators=None, align=None, **call_kwargs):
        """``state = SequenceState(strength); (pipe(frame, sequence=state, generator=g, **call_kwargs) for frame, g in zip(frames,
        generators))`` - consecutive frames of one sequence, each started from the frame before (``SequenceState``) - with up to
        ``in_flight`` frames on the GPU at a time (default ``frames_in_flight_for(ensemble_size)``).  A generator with ``map_images``'
        contract: outputs in input order, ``frames`` consumed lazily, one entry of ``generators`` per frame, a shared ``generator=``
        refused when ``in_flight > 1``.  Every output is, bit for bit, what the serial loop returns: with several lanes only the
        denoise stage takes turns (a ``Turnstile``, frame by frame; its GPU work is ordered by events, nothing waits on the host),
        while a frame's preprocessing and encode run ahead of its turn and its decode, ensemble and output stage behind it.
        Refused: ``images_per_program``, ``init_latents``, member-parallel pipelines, a frame whose processed size differs from the
        first frame's.

        ``align`` (depth only): ``True`` or a dict with ``iters``, ``delta``, ``reference`` and / or ``fit_shift`` - one
        ``DepthAlignState`` for this call, ``pipe(frame, sequence=state, align=align_state, ...)`` per frame: every frame's map is fitted,
        scale and shift, to the aligned map of the frame before (or the first frame's).  With several lanes the align stage takes turns
        in frame order too, on a turnstile of its own; the outputs stay the serial loop's bit for bit."""
        if isinstance(align, DepthAlignState):
            raise ValueError("map_video: align is True or a dict of settings; the call keeps a DepthAlignState of its own")
        align_state = align_settings(align)
        if align_state is not None:
            self._align_plan(align_state, None, None)   # (the kind and the device: refused before anything is drawn or launched)
        for name in ("images_per_program", "init_latents", "sequence"):
            if call_kwargs.get(name) is not None:
                raise ValueError(f"map_video: {name} cannot be combined with a sequence of frames")
            call_kwargs.pop(name, None)
        if self._sharded():
            raise ValueError("map_video: a sequence is not available on a member-parallel pipeline")
        state = SequenceState(strength)
        n = self._lane_count("map_video", "frame", frames, generators, in_flight,
                             functools.partial(self.frames_in_flight_for, call_kwargs.get("ensemble_size", 1)), 1, call_kwargs)
        pairs = self._paired("map_video", "frame", iter(frames), None if generators is None else iter(generators))

        def items():
            """[(frame, generator)], one frame each, all of the first frame's processed size"""
            size = None
            for k, (image, g) in enumerate(pairs):
                image_size = self._processed_size(image, call_kwargs.get("processing_res"))
                if size is not None and image_size != size:
                    raise ValueError(f"map_video: frame {k} has the processed size {image_size}, the sequence began with {size}")
                size = image_size
                yield [(image, g)]

        def run_one(pipe, group, index, turnstile):
            kw = dict(call_kwargs)
            image, g = group[0]
            if generators is not None:
                kw["generator"] = g
            if align_state is not None:
                kw["align"] = align_state
            if turnstile is not None:   # on this call's view of the lane
                pipe._sequence_turn = (turnstile if align_state is None else turnstile[0], index)
                pipe._align_turn = None if align_state is None else (turnstile[1], index)
            return [pipe(image, sequence=state, **kw)]

        # (a turnstile: the denoise stages, frame by frame; with align a second one: the align stages)
        return self._drive_lanes(items(), n, True if align_state is None else 2, run_one)

    # ---- large pictures: tiles ---------------------------------------------------------------
    # A picture far above the training size is cut into overlapping tiles of that size on a grid (tiles.plan); the tiles are
    # same-size images, i.e. the workload of map_images(images_per_program=k) and its lanes.  Their predictions stay on the device
    # (``_device_out``), depth tiles are fitted - scale and shift each - to one ordinary low-resolution prediction of the whole picture
    # (tiles.fit), and the tiles are blended with feathered weights over the full-size canvas (tiles.blend).  DESIGN.md 6e.
    _device_out = False            # True only on the view predict_tiled predicts on: _finish stops in front of its read-back tail
    _device_out_uncertainty = False   # on that view: _finish hands back the pair (prediction, uncertainty | None), both on the device

    _clip_range = (0, 1)           # of a finished prediction

    def _finish(self, target_preds, input_size, ensemble_size, match_input_res, resample, ensemble_kwargs, guided=None, align=None,
                **finish):
        """``__call__``'s tail: the members of one image -> its output (``_tail``: the kind's pictures, read-backs and clip).  On the
        view ``predict_tiled`` predicts on it stops in front of ``_tail``: -> the clipped prediction on the device, [H,W] or [3,H,W]
        (the clip is the one ``_tail`` applies on the host) - or, where the view asks for it (``_device_out_uncertainty``), the pair of
        that prediction and the ensemble's uncertainty, [H,W] fp32 on the device, None without one.  ``guided``: None, or what
        ``_guided_plan`` and ``_preprocess`` left for the edge-guided enlargement that then takes the resize's place -
        (radius, sigma, the input picture's bytes on the device, whether they are HWC).  ``align``: None, or the frame's
        ``DepthAlignState`` (``_align_plan``): after the ensemble and before the enlargement the prediction is fitted to the state's
        reference and replaced by ``s * pred + t``, unclipped, the uncertainty by ``s`` times itself; the output carries the fit."""
        if target_preds is None:  # member-parallel non-root rank with a rooted gather
            return self._empty_output()
        if ensemble_size > 1:
            final_pred, pred_uncert = self._ensemble(target_preds, ensemble_kwargs)
        else:
            final_pred, pred_uncert = target_preds, None
        fitted = None
        if align is not None:
            final_pred, pred_uncert, *fitted = align._step(final_pred, pred_uncert, L.load(bool(getattr(self.unet, "f16", False))),
                                                           self._align_turn)
        if guided is not None:
            radius, sigma, picture, hwc = guided
            lead = final_pred.shape[:-2]
            final_pred = guided_upsample(final_pred.float().reshape((-1,) + tuple(final_pred.shape[-2:])), picture, radius, sigma, hwc,
                                         lib=L.load(bool(getattr(self.unet, "f16", False))))
            final_pred = final_pred.reshape(tuple(lead) + tuple(final_pred.shape[-2:]))
        elif match_input_res:
            final_pred = resize(final_pred, input_size[-2:], interpolation=resample, antialias=True)
        if self._device_out:
            final_pred = final_pred.squeeze().float().clamp(*self._clip_range)
            if self._device_out_uncertainty:
                return final_pred, None if pred_uncert is None else pred_uncert.squeeze().float()
            return final_pred
        out = self._tail(final_pred, pred_uncert, **finish)
        if fitted is not None:
            out.align_coef, out.align_flag = fitted
        return out

    @torch.no_grad()
    def predict_tiled(self, image, tile_size=768, tile_overlap=192, tiled_res: int = 0, guide_res: Optional[int] = None,
                      tiles_per_program: Optional[int] = None, in_flight: Optional[int] = None, generator=None, tile_generators=None,
                      **call_kwargs):
        """The prediction of a LARGE picture from overlapping tiles, stitched on the device -> the output ``__call__`` returns.

        The working size is the input's - or ``max_res_size(hw, tiled_res)`` when ``tiled_res`` > 0 - with each side floored to a
        multiple of 8; the picture is resampled to it (``resample_method``) where it differs.  ``tiles.plan(working size, tile_size,
        tile_overlap)`` places the tiles (``tile_size`` / ``tile_overlap``: an int or (h, w), multiples of 8; the overlap is the
        minimum, at most half a tile).  A plan of ONE tile returns exactly ``pipe(image, processing_res=tiled_res,
        generator=generator, **call_kwargs)`` and runs no guide.  Otherwise:

        * depth only - the GUIDE: the ordinary prediction ``pipe(image, processing_res=guide_res, match_input_res=False,
          generator=generator, ...)`` (``guide_res`` None: the pipeline's default processing resolution), ensembled like any call;
        * the TILES: crops of the working picture, taken on the device (an 8-bit picture is cropped as uint8 CUDA tensors), go through
          ``map_images(crops, images_per_program=tiles_per_program, in_flight=in_flight, generators=..., processing_res=0,
          match_input_res=False, ...)``; ``tiles_per_program`` defaults to min(number of tiles, 8); with ``ensemble_size`` > 1 every
          tile is ensembled on its own; no prediction is read back;
        * the STITCH: depth - ``tiles.fit`` against the guide, then ``tiles.blend`` with the fitted scale and shift of every tile;
          normals - ``tiles.blend(normalize=True)``; then ``__call__``'s tail: the resize to the input size when ``match_input_res``,
          the clip, the coloured depth / normals picture.

        Noise.  Tile i (row-major) draws from ``tile_generators[i]`` when given.  Else with ``generator=NativeNoise(seed)`` the guide
        draws from ``generator`` and tile i from ``NativeNoise((seed + 1 + i) mod 2^64)``: the result does not depend on
        ``in_flight`` or ``tiles_per_program`` beyond the arithmetic of the batch.  A ``torch.Generator`` is consumed by the guide
        first and then tile by tile in row-major order, with ONE program in flight (``in_flight`` is taken as 1).  ``generator=None``:
        randomised, as in ``__call__``.

        Uncertainty.  With ``ensemble_size`` > 1 and ``ensemble_kwargs=dict(output_uncertainty=True)`` - the switch ``__call__``
        honours - ``uncertainty`` is an [Hw, Ww] fp32 array at the WORKING size (like ``__call__``'s it is never resampled to the input
        size); in every other case it is None.  Every tile's uncertainty u_i comes from the tile's own ensemble and stays on the device
        beside its prediction.  Normals: ``tiles.blend(u, ...)``, the feathered mean of the tiles' uncertainties.  Depth: u_i is in units
        of the tile's normalised depth and the stitched depth is s_i d_i + t_i, so the tile contributes s_i u_i:
        ``tiles.blend(u, ..., coef=[(s_i, 0)])`` with the s_i of the depth's fit.  A degenerate tile has s_i = 0 and therefore
        contributes 0 with its weight - where only such a tile covers a pixel the uncertainty there is 0, which says nothing about the
        prediction; ``degenerate_tiles`` reports how many there are.  The guide's uncertainty is not used.

        A depth output carries ``degenerate_tiles``, the number of tiles ``tiles.fit`` flagged.  Refused: the intrinsic-image pipeline,
        member-parallel pipelines, ``init_latents``, ``sequence``, ``images_per_program``, ``guided_upsample``, ``align`` and
        ``processing_res`` (``tiled_res`` and ``guide_res`` take its place)."""
        if self._kind not in ("depth", "normals"):
            raise ValueError("predict_tiled: the intrinsic-image pipeline is not supported (depth and normals only)")
        if self._member_parallel or self._sharded():
            raise ValueError("predict_tiled is not available on a member-parallel pipeline")
        for name in ("init_latents", "sequence", "images_per_program", "processing_res", "guided_upsample", "align"):
            if call_kwargs.get(name) is not None:
                raise ValueError(f"predict_tiled: {name} cannot be combined with tiles")
            call_kwargs.pop(name, None)
        unknown = set(call_kwargs) - set(self._call_args) - set(self._finish_args)
        if unknown:
            raise TypeError(f"predict_tiled() got unexpected keyword arguments {sorted(unknown)}")
        tiled_res = int(tiled_res)
        if tiled_res < 0:
            raise ValueError(f"predict_tiled: tiled_res must be >= 0 (got {tiled_res})")
        if not isinstance(image, Image.Image) and \
                not (isinstance(image, torch.Tensor) and image.dim() == 4 and tuple(image.shape[:2]) == (1, 3)):
            raise TypeError(f"predict_tiled: the image must be a PIL image or a [1, 3, H, W] tensor (got {type(image).__name__})")
        hw = self._input_hw(image)
        work_hw = tuple(d // 8 * 8 for d in (max_res_size(hw, tiled_res) if tiled_res > 0 else hw))
        plan = tiling.plan(work_hw, tile_size, tile_overlap)   # (refuses bad sizes: nothing has been launched)
        n = len(plan.origins)
        if tile_generators is not None:
            tile_generators = list(tile_generators)
            if len(tile_generators) != n:
                raise ValueError(f"predict_tiled: {len(tile_generators)} tile_generators for {n} tiles")
        if n == 1:
            return self(image, processing_res=tiled_res, generator=generator, **call_kwargs)
        if tiles_per_program is None:
            tiles_per_program = min(n, 8)
        if tile_generators is None and generator is not None:
            if isinstance(generator, NativeNoise):
                tile_generators = [NativeNoise((generator.seed + 1 + i) & ((1 << 64) - 1)) for i in range(n)]
            else:
                tile_generators, in_flight = [generator] * n, 1   # one stream of draws: guide, then tile by tile
        match_input_res = call_kwargs.pop("match_input_res", True)
        resample = get_tv_resample_method(call_kwargs.get("resample_method", "bilinear"))
        finish = {a: call_kwargs.pop(a) for a in self._finish_args if a in call_kwargs}
        if self.empty_text_embed is None:
            self.encode_empty_text()
        dev = copy.copy(self)   # shares engines, scheduler and lanes with this pipeline; its calls stop in front of the read-back
        dev._device_out = True
        with_unc = call_kwargs.get("ensemble_size", 1) > 1 and bool((call_kwargs.get("ensemble_kwargs") or {}).get("output_uncertainty"))

        # the working picture on the device, [1,3,H,W] in the input's number format
        rgb = pil_to_tensor(image.convert("RGB")).unsqueeze(0) if isinstance(image, Image.Image) else image
        input_size = rgb.shape
        rgb = rgb.to(self.device)
        if work_hw != hw:
            rgb = resize(rgb, work_hw, interpolation=resample, antialias=True)
        th, tw = plan.tile_hw
        crops = [rgb[..., y0:y0 + th, x0:x0 + tw].contiguous() for y0, x0 in plan.origins]

        coef = flags = None
        if self._kind == "depth":
            guide = dev(image, processing_res=guide_res, match_input_res=False, generator=generator, **call_kwargs)   # [hg,wg]
        dev._device_out_uncertainty = with_unc   # (the guide above handed back its prediction alone; the tiles hand back pairs)
        preds = list(dev.map_images(crops, in_flight=in_flight, generators=tile_generators, images_per_program=tiles_per_program,
                                    processing_res=0, match_input_res=False, **call_kwargs))
        uncert = None
        if with_unc:
            preds, uncert = [p for p, _ in preds], torch.stack([u for _, u in preds]).reshape(n, th, tw)
        preds = torch.stack(preds).reshape(n, self._pred_channels, th, tw)
        overlap = tiling._pair(tile_overlap, "tile_overlap")
        if self._kind == "depth":
            coef, flags = tiling.fit(preds[:, 0], plan.origins, guide, work_hw)
            final_pred = tiling.blend(preds, plan.origins, work_hw, overlap, coef=coef)
            if with_unc:   # s_i u_i: the scale of the fit without its shift
                uncert = tiling.blend(uncert, plan.origins, work_hw, overlap, coef=torch.stack([coef[:, 0], torch.zeros_like(coef[:, 0])], dim=1))
        else:
            final_pred = tiling.blend(preds, plan.origins, work_hw, overlap, normalize=True)
            if with_unc:
                uncert = tiling.blend(uncert, plan.origins, work_hw, overlap)
        final_pred = final_pred.unsqueeze(0)
        if match_input_res:
            final_pred = resize(final_pred, input_size[-2:], interpolation=resample, antialias=True)
        out = self._tail(final_pred, uncert, **finish)
        if flags is not None:
            out.degenerate_tiles = int(flags.sum().item())
        return out

    # ---- reference methods -------------------------------------------------------------------
    def _check_inference_step(self, n_step: int) -> None:
        assert n_step >= 1
        if isinstance(self.scheduler, DDIMScheduler):
            if "trailing" != self.scheduler.config.timestep_spacing:
                logging.warning(
                    f"The loaded `DDIMScheduler` is configured with `timestep_spacing="
                    f'"{self.scheduler.config.timestep_spacing}"`; the recommended setting is `"trailing"`. '
                    f"This change is backward-compatible and yields better results. "
                    f"Consider using `{self._ckpt_hint}` for the best experience.")
            else:
                if n_step > 10:
                    logging.warning(
                        f"Setting too many denoising steps ({n_step}) may degrade the prediction; consider "
                        f"relying on the default values.")
            if not self.scheduler.config.rescale_betas_zero_snr:
                logging.warning(
                    f"The loaded `DDIMScheduler` is configured with `rescale_betas_zero_snr="
                    f"{self.scheduler.config.rescale_betas_zero_snr}`; the recommended setting is True. "
                    f"Consider using `{self._ckpt_hint}` for the best experience.")
        elif isinstance(self.scheduler, LCMScheduler):
            self._lcm_policy(n_step)
        else:
            raise RuntimeError(f"Unsupported scheduler type: {type(self.scheduler)}")

    def encode_empty_text(self):
        """CLIP("") with padding="do_not_pad" -> [1,2,D]; constant per checkpoint, computed once on
        the host (reference :381-394)."""
        if self.tokenizer is None or self.text_encoder is None:
            raise RuntimeError("no text encoder/tokenizer and no precomputed empty_text_embed")
        text_inputs = self.tokenizer("", padding="do_not_pad", max_length=self.tokenizer.model_max_length,
                                     truncation=True, return_tensors="pt")
        with torch.no_grad():
            self.empty_text_embed = self.text_encoder(text_inputs.input_ids)[0].to(self.dtype)

    def encode_rgb(self, rgb_in: torch.Tensor) -> torch.Tensor:
        return self.vae.encode_rgb_latent(rgb_in)

    @torch.no_grad()
    def single_infer(self, rgb_in: torch.Tensor, num_inference_steps: int,
                     generator: Union[torch.Generator, None], show_pbar: bool = False,
                     init_latents: Optional[torch.Tensor] = None,
                     step_noises: Optional[torch.Tensor] = None, rgb_members: Optional[int] = None, carry=None) -> torch.Tensor:
        """One batched prediction (reference :396-477).  rgb_in [B,3,h,w] in [-1,1]; identical
        (expanded) rows are encoded once.  ``rgb_members`` = m: rgb_in holds B distinct images and the batch is their
        B x m members, image-major (one encode program of B images, one denoising program of B m members).
        ``carry`` = (a ``_FrameCarry``, the rows of the sequence's latent these B members are, whether this is the frame's last batch)."""
        device = self.device
        B = rgb_in.shape[0] if rgb_members is None else rgb_in.shape[0] * rgb_members
        shared = rgb_members is None and (B == 1 or rgb_in.stride(0) == 0)
        rgb_in = (rgb_in[:1] if shared else rgb_in).to(device)
        rgb_latent = self.encode_rgb(rgb_in)                       # [1|B|B/m,4,h,w] fp32
        h, w = rgb_latent.shape[-2:]
        if init_latents is None:
            target_latent = self._randn((B, self._target_latent_channels, h, w), generator)
        else:
            target_latent = init_latents.to(device)
        if self.empty_text_embed is None:
            self.encode_empty_text()
        self.unet.set_context(self.empty_text_embed)
        prog = self.unet.denoise_program(B, h, w, self.scheduler, num_inference_steps,
                                         rgb_broadcast=shared, rgb_members=rgb_members)
        prog.rgb_latent.copy_(rgb_latent)
        prog.x.copy_(target_latent)
        for k, nz in enumerate(prog.noises):  # LCM consumes the generator once per non-final step (:466-468)
            if step_noises is not None:
                nz.copy_(step_noises[k])
            else:
                nz.copy_(self._randn(nz.shape, generator))
        if carry is not None:
            carry[0].blend(prog.x, carry[1])
        prog.run()
        if carry is not None:
            carry[0].keep(prog.x, carry[1], carry[2])
        return self._decode(prog.x)

    def _step_noise_count(self, denoising_steps):
        """How many per-step noises the scheduler, set to ``denoising_steps`` steps here, has a program draw."""
        self.scheduler.set_timesteps(denoising_steps)
        return sum(bool(self.scheduler.needs_noise(i)) for i in range(denoising_steps))

    def _predict_members(self, rgb_norm, ensemble_size, denoising_steps, batch_size, generator,
                         init_latents, carry=None):
        """All E members of one image -> [E,C,h,w] (on every rank when member-parallel).  ``carry``: the frame's ``_FrameCarry``
        (``sequence=``; never with ``init_latents`` or member parallelism)."""
        _bs = batch_size if batch_size > 0 else find_batch_size(
            ensemble_size=ensemble_size, input_res=max(rgb_norm.shape[1:]), dtype=self.dtype)
        E = ensemble_size
        members = list(range(E))
        step_noises_all = None
        if self._sharded():
            # every rank draws the full [E,4,h,w] noise (same generator state) and keeps its slice, so results do not depend on
            # the number of GPUs: they are what ONE process draws when its batch holds all E members (batch_size >= E, the
            # default on this hardware).  With a smaller batch_size the reference draws batch by batch (:281-289), and so
            # does the single-process path below - the reference's own results depend on the batch size in that case
            if init_latents is None:
                hh, ww = self._latent_hw(rgb_norm.shape[-2:])
                init_latents = self._randn((E, self._target_latent_channels, hh, ww), generator)
            # the LCM scheduler consumes the generator once per non-final step (:466-468): those draws are made for
            # all E members on every rank too, in the order a single process holding the E members in one batch makes
            # them (initial latents, then one [E,...] draw per step), and sliced by member
            n_noise = self._step_noise_count(denoising_steps)
            if n_noise:
                step_noises_all = [self._randn(init_latents.shape, generator) for _ in range(n_noise)]
            members = mdist.shard_members(E, mdist.world_size(self._member_group),
                                          mdist.rank(self._member_group))
        preds = []
        for i in range(0, len(members), _bs):
            idx = members[i:i + _bs]
            lat = None if init_latents is None else init_latents[idx]
            rgb = rgb_norm.expand(len(idx), -1, -1, -1)
            nzs = None if step_noises_all is None else [nz[idx] for nz in step_noises_all]
            rows = None if carry is None else (carry, slice(idx[0], idx[-1] + 1), i + _bs >= len(members))
            preds.append(self.single_infer(rgb, denoising_steps, generator, False, lat, step_noises=nzs, carry=rows))
        local = torch.cat(preds, dim=0) if preds else None
        if self._sharded():
            C = self._pred_channels
            # decoded maps are latent size x 2^(levels-1), which is smaller than the image when its size is not a
            # multiple of 8 (KITTI 1242x375 -> 768x231 -> latent 96x28 -> decoded 768x224); ranks without members
            # need the shape too, so it is computed, not taken from `local`
            f = getattr(self.vae, "scale_factor", None) or 2 ** (len(self.vae.config.block_out_channels) - 1)
            hh, ww = (f * d for d in self._latent_hw(rgb_norm.shape[-2:]))
            # maps in flight: the gather is a collective on ONE process group - every rank issues the gathers of maps 0, 1, 2 ...
            # in that order, one at a time, whichever lane (thread, stream) predicted them (map_images hands each call its turn)
            turn = self._gather_turn
            if turn is not None:
                turn[0].wait(turn[1])
            local = mdist.gather_members(local, E, (C, hh, ww), self.device, self._member_group, self._member_root,
                                         force=self._member_force)
            if turn is not None:
                turn[0].done(turn[1])   # only a gather that succeeded hands the turn on; a failed one aborts the turnstile (run_lanes)
        return local

    def _predict_group(self, rgb_norms, ensemble_size, denoising_steps, batch_size, generators):
        """The E members of each of k images of one processed size -> [k E,C,h,w], image-major.  Image i's initial latents and
        LCM step noises come from ``generators[i]`` in the order and shapes of its lone call (``_predict_members``: per batch of
        the lone batch size, the initial latents, then one draw per noised step); the members then run as programs of whole
        images (k E members, or as many images as ``batch_size`` holds), or - when one image's members exceed ``batch_size`` -
        image by image in batches of ``batch_size``."""
        E, k = ensemble_size, len(rgb_norms)
        res = max(rgb_norms[0].shape[1:])
        hh, ww = self._latent_hw(rgb_norms[0].shape[-2:])
        C = self._target_latent_channels
        n_noise = self._step_noise_count(denoising_steps)
        lone_bs = batch_size if batch_size > 0 else find_batch_size(ensemble_size=E, input_res=res, dtype=self.dtype)
        lats, noises = [], [[] for _ in range(n_noise)]
        for g in generators:
            for i in range(0, E, lone_bs):
                m = min(lone_bs, E - i)
                lats.append(self._randn((m, C, hh, ww), g))
                for s in range(n_noise):
                    noises[s].append(self._randn((m, C, hh, ww), g))
        init = torch.cat(lats, dim=0)
        noises = [torch.cat(z, dim=0) for z in noises]
        rgb = torch.cat([r.to(self.device) for r in rgb_norms], dim=0)   # [k,3,h,w]
        _bs = batch_size if batch_size > 0 else find_batch_size(ensemble_size=k * E, input_res=res, dtype=self.dtype)
        if _bs >= E:
            runs = [(j, min(k, j + _bs // E), 0, E) for j in range(0, k, _bs // E)]   # (first image, end image, members)
        else:
            runs = [(j, j + 1, i, min(E, i + _bs)) for j in range(k) for i in range(0, E, _bs)]
        preds = []
        for j0, j1, m0, m1 in runs:
            if j1 - j0 == 1:   # one image: the lone call's program
                rows = slice(j0 * E + m0, j0 * E + m1)
                preds.append(self.single_infer(rgb[j0:j1].expand(m1 - m0, -1, -1, -1), denoising_steps, None, False,
                                               init[rows], step_noises=[z[rows] for z in noises]))
            else:
                rows = slice(j0 * E, j1 * E)
                preds.append(self.single_infer(rgb[j0:j1], denoising_steps, None, False, init[rows],
                                               step_noises=[z[rows] for z in noises], rgb_members=E))
        return torch.cat(preds, dim=0) if len(preds) > 1 else preds[0]

    _call_args = ("denoising_steps", "ensemble_size", "processing_res", "match_input_res", "resample_method", "batch_size",
                  "show_progress_bar", "ensemble_kwargs", "guided_upsample")

    @torch.no_grad()
    def _call_group(self, images, generators, call_kwargs):
        """[pipe(image, generator=g, **call_kwargs) for image, g in zip(images, generators)] with the images' members in shared
        programs (``map_images(images_per_program=k)``): every image preprocessed as ``__call__`` does (one processed size),
        one ``_predict_group``, then ``__call__``'s tail per image on its own [E, ...] slice."""
        kw = dict(call_kwargs)
        unknown = set(kw) - set(self._call_args) - set(self._finish_args)
        if unknown:
            raise TypeError(f"{type(self).__name__}() got unexpected keyword arguments {sorted(unknown)}")
        denoising_steps, ensemble_size, processing_res, resample = self._call_settings(
            kw.get("denoising_steps"), kw.get("ensemble_size", 1), kw.get("processing_res"), kw.get("resample_method", "bilinear"))
        plans = [self._guided_plan(kw.get("guided_upsample"), kw.get("match_input_res", True), im) for im in images]
        prepared = [self._guided_prepared(im, processing_res, resample, plan) for im, plan in zip(images, plans)]
        sizes = {tuple(r.shape[-2:]) for r, _, _ in prepared}
        if len(sizes) != 1:
            raise ValueError(f"images of one program must have one processed size, got {sorted(sizes)}")
        preds = self._predict_group([r for r, _, _ in prepared], ensemble_size, denoising_steps, kw.get("batch_size", 0),
                                    [None] * len(images) if generators is None else list(generators))
        E = ensemble_size
        finish = {a: kw[a] for a in self._finish_args if a in kw}
        return [self._finish(preds[j * E:(j + 1) * E], input_size, ensemble_size, kw.get("match_input_res", True), resample,
                             kw.get("ensemble_kwargs"), guided=guided, **finish) for j, (_, input_size, guided) in enumerate(prepared)]

    _finish_args = ()   # the keywords of ``__call__`` that go to the kind's ``_tail``

    @torch.no_grad()
    def _call(self, input_image, denoising_steps, ensemble_size, processing_res, match_input_res, resample_method, batch_size,
              generator, ensemble_kwargs, init_latents, sequence, guided_upsample=None, align=None, **finish):
        """What every kind's ``__call__`` runs; ``finish``: its keywords of ``_finish_args``."""
        denoising_steps, ensemble_size, processing_res, resample = self._call_settings(
            denoising_steps, ensemble_size, processing_res, resample_method)
        plan = self._guided_plan(guided_upsample, match_input_res, input_image)
        carry = self._frame_carry(sequence, init_latents, input_image, processing_res, ensemble_size)
        align = self._align_plan(align, input_image, processing_res)
        rgb_norm, input_size, guided = self._guided_prepared(input_image, processing_res, resample, plan)

        target_preds = self._predict_members(rgb_norm, ensemble_size, denoising_steps, batch_size,
                                             generator, init_latents, carry)
        return self._finish(target_preds, input_size, ensemble_size, match_input_res, resample, ensemble_kwargs, guided=guided, align=align,
                            **finish)

    def _align_plan(self, align, input_image, processing_res):
        """``__call__``'s check of ``align=``, before anything is launched -> the frame's ``DepthAlignState`` | None.  ``input_image``
        None (``map_video``, before its first frame): the kind and the device alone."""
        if align is None:
            return None
        if not isinstance(align, DepthAlignState):
            raise TypeError(f"align must be a DepthAlignState (got {type(align).__name__})")
        if self._kind != "depth":
            raise ValueError(f"align fits the scale and shift of an affine-invariant depth map: the {self._kind} pipeline has no such ambiguity")
        if self._member_parallel or self._sharded():
            raise ValueError("align is not available on a member-parallel pipeline")
        if getattr(self.device, "type", None) != "cuda":
            raise ValueError("align runs on the device: it needs a CUDA pipeline")
        if self._device_out:
            raise ValueError("align cannot be combined with tiles")
        if input_image is not None:
            align._check((tuple(int(v) for v in self._decoded_size(self._processed_size(input_image, processing_res))), self.device))
        return align

    def _decoded_size(self, hw):
        """(height, width) of a prediction decoded from the latent of a picture processed at ``hw``: the latent's size times the VAE's
        factor, which is below ``hw`` where that is no multiple of the factor."""
        f = getattr(self.vae, "scale_factor", None) or 2 ** (len(self.vae.config.block_out_channels) - 1)
        return tuple(f * d for d in self._latent_hw(hw))

    def _guided_plan(self, guided_upsample, match_input_res, input_image):
        """``__call__``'s check of ``guided_upsample=``, before anything is launched -> None (the keyword is off) | (radius, sigma)."""
        plan = guided_settings(guided_upsample)
        if plan is None:
            return None
        if not match_input_res:
            raise ValueError("guided_upsample enlarges the prediction to the input size: it cannot be combined with match_input_res=False")
        if getattr(self.device, "type", None) != "cuda" or not getattr(self, "device_io_stages", False):
            raise ValueError("guided_upsample runs on the device: it needs a CUDA pipeline with device_io_stages")
        if self._member_parallel or self._sharded():
            raise ValueError("guided_upsample is not available on a member-parallel pipeline")
        if not isinstance(input_image, Image.Image) and not (
                isinstance(input_image, torch.Tensor) and input_image.dtype == torch.uint8 and input_image.dim() == 4
                and tuple(input_image.shape[:2]) == (1, 3)):
            raise ValueError("guided_upsample is guided by the input picture's bytes: the input must be a PIL image or a uint8 "
                             "[1, 3, H, W] tensor")
        return plan

    def _guided_prepared(self, input_image, processing_res, resample, plan):
        """``_preprocess`` -> (rgb_norm, input_size, ``_finish``'s ``guided``): with a plan the picture's bytes, uploaded once for the
        input stage, are kept for the finish stage."""
        if plan is None:
            return self._preprocess(input_image, processing_res, resample) + (None,)
        rgb_norm, input_size, picture, hwc = self._preprocess_device(input_image, processing_res, resample, keep_picture=True)
        return rgb_norm, input_size, plan + (picture, hwc)

    def _call_settings(self, denoising_steps, ensemble_size, processing_res, resample_method):
        """``__call__``'s defaults and argument checks -> (denoising_steps, ensemble_size, processing_res, resample mode)."""
        if denoising_steps is None:
            denoising_steps = self.default_denoising_steps
        if processing_res is None:
            processing_res = self.default_processing_resolution
        assert processing_res >= 0
        assert ensemble_size >= 1
        self._check_inference_step(denoising_steps)
        return denoising_steps, ensemble_size, processing_res, get_tv_resample_method(resample_method)

    def _latent_hw(self, hw):
        """The VAE's own rule (the KL encoder's down-samplers floor, the tiny autoencoder's ceil); a VAE object without
        ``latent_hw`` is taken for an AutoencoderKL of ``config.block_out_channels`` levels."""
        if hasattr(self.vae, "latent_hw"):
            return self.vae.latent_hw(hw)
        h, w = hw
        for _ in range(len(self.vae.config.block_out_channels) - 1):
            h, w = (h - 2) // 2 + 1, (w - 2) // 2 + 1
        return h, w

    # The uint8 ends of a CUDA pipeline run on the device (csrc/resize.hip): MG_OP_RGB_PREP in ``_preprocess``, MG_OP_NORMALS_VIS in the
    # normals pipeline's ``_tail``.  False: the host code of both (what host pipelines and float inputs run anyway) - the same bits.
    device_io_stages = True

    def _preprocess_device(self, input_image, processing_res, resample_method, keep_picture=False):
        """``_preprocess`` of a PIL image or a uint8 [1,3,H,W] tensor on the device -> (rgb_norm on the device, input_size), or None
        where the host code must run to give the same bits.  The picture goes up once as uint8 - PIL's HWC bytes as they are, no
        host transpose - and one MG_OP_RGB_PREP makes what the VAE encoder reads.  The range assert of the host code is vacuous
        here: the bytes 0 ... 255 map into [-1, 1] exactly (0 -> -1, 255 -> 1, monotonic in between), so it is not repeated.
        ``keep_picture``: -> (rgb_norm, input_size, the uploaded bytes, whether they are HWC) - the one upload serves the finish stage
        too (``guided_upsample=``)."""
        if isinstance(input_image, Image.Image):
            u8 = torch.from_numpy(np.array(input_image.convert("RGB")))   # [H,W,3]; (np.array: torch wants a writable buffer)
            hwc, hw = True, tuple(u8.shape[:2])
            input_size = torch.Size((1, 3) + hw)
        elif isinstance(input_image, torch.Tensor) and input_image.dtype == torch.uint8 and input_image.dim() == 4 and \
                tuple(input_image.shape[:2]) == (1, 3):
            u8, hwc, hw, input_size = input_image, False, tuple(input_image.shape[-2:]), input_image.shape
        else:
            return None
        # where the host code computes: on the device (torch's device kernels: x * fp32(1 / 255)) if the tensor is there or goes
        # there to be resampled, else on the host (IEEE division) - the stage rounds the same way
        resample = processing_res > 0 and max(hw) != processing_res   # (else resize_max_res's factor is exactly 1: the same size)
        on_device = u8.is_cuda or resample
        size = max_res_size(hw, processing_res) if resample else hw
        if keep_picture or (u8.is_cuda and u8.device != self.device):
            u8 = u8.to(self.device)
        rgb_norm = prepare_rgb_device(u8, size, resample_method, self.io_dtype, hwc, device=self.device, reciprocal=on_device)
        return (rgb_norm, input_size, u8, hwc) if keep_picture else (rgb_norm, input_size)

    def _preprocess(self, input_image, processing_res, resample_method):
        if getattr(self, "device_io_stages", False) and getattr(self.device, "type", None) == "cuda":
            staged = self._preprocess_device(input_image, processing_res, resample_method)
            if staged is not None:
                return staged
        if isinstance(input_image, Image.Image):
            input_image = input_image.convert("RGB")
            rgb = pil_to_tensor(input_image).unsqueeze(0)
        elif isinstance(input_image, torch.Tensor):
            rgb = input_image
        else:
            raise TypeError(f"Unknown input type: {type(input_image) = }")
        input_size = rgb.shape
        assert 4 == rgb.dim() and 3 == input_size[-3], f"Wrong input shape {input_size}, expected [1, rgb, H, W]"
        if processing_res > 0:
            if max(input_size[-2:]) != processing_res and self.device.type == "cuda":
                rgb = rgb.to(self.device)   # resample on the device (csrc/resize.hip)
            rgb = resize_max_res(rgb, max_edge_resolution=processing_res, resample_method=resample_method)
        rgb_norm = rgb / 255.0 * 2.0 - 1.0
        rgb_norm = rgb_norm.to(self.io_dtype)
        assert rgb_norm.min() >= -1.0 and rgb_norm.max() <= 1.0
        return rgb_norm, input_size


class MarigoldDepthPipeline(_MarigoldPipelineBase):
    """Affine-invariant monocular depth (reference marigold/marigold_depth_pipeline.py:78-516)."""
    _kind = "depth"
    _ckpt_hint = "prs-eth/marigold-depth-v1-1"

    def _lcm_policy(self, n_step):
        logging.warning("DeprecationWarning: LCMScheduler will not be supported in the future. "
                        "Consider using `prs-eth/marigold-depth-v1-1` for the best experience.")
        if n_step > 10:
            logging.warning(f"Setting too many denoising steps ({n_step}) may degrade the prediction; "
                            f"consider relying on the default values.")

    def _decode(self, latent):
        return self.decode_depth(latent)

    def decode_depth(self, depth_latent: torch.Tensor) -> torch.Tensor:
        """latent -> depth in [0,1], [B,1,H,W] (decode, channel mean, clip, shift fused on device;
        reference :498-516 + :473-475)."""
        return self.vae.decode(depth_latent, post=L.POST_DEPTH)

    def __call__(self, input_image: Union[Image.Image, torch.Tensor], denoising_steps: Optional[int] = None,
                 ensemble_size: int = 1, processing_res: Optional[int] = None, match_input_res: bool = True,
                 resample_method: str = "bilinear", batch_size: int = 0,
                 generator: Union[torch.Generator, None] = None, color_map: str = "Spectral",
                 show_progress_bar: bool = True, ensemble_kwargs: Dict = None,
                 init_latents: Optional[torch.Tensor] = None,
                 sequence: Optional[SequenceState] = None, guided_upsample=None,
                 align: Optional[DepthAlignState] = None) -> MarigoldDepthOutput:
        return self._call(input_image, denoising_steps, ensemble_size, processing_res, match_input_res, resample_method, batch_size,
                          generator, ensemble_kwargs, init_latents, sequence, guided_upsample, align, color_map=color_map)

    _finish_args = ("color_map",)

    def _empty_output(self) -> MarigoldDepthOutput:
        return MarigoldDepthOutput(depth_np=None, depth_colored=None, uncertainty=None)

    def _ensemble(self, target_preds, ensemble_kwargs):
        return ensemble_depth(target_preds, scale_invariant=self.scale_invariant, shift_invariant=self.shift_invariant,
                              **(ensemble_kwargs or {}))

    def _tail(self, final_pred, pred_uncert, color_map="Spectral") -> MarigoldDepthOutput:
        return _depth_tail(final_pred, pred_uncert, color_map)


def _depth_tail(final_pred, pred_uncert, color_map) -> MarigoldDepthOutput:
    """The tail of the depth pipeline's ``_finish``: the coloured picture, the arrays to the host, the clip."""
    colored_dev = None
    if color_map is not None and final_pred.is_cuda:
        # colour table look-up on the device (clip(0, 1) is part of the kernel); the host gets a uint8 HWC image
        colored_dev = colorize_depth_device(final_pred.squeeze().float(), 0.0, 1.0, cmap=color_map)
    final_pred = final_pred.squeeze().cpu().numpy()
    if pred_uncert is not None:
        pred_uncert = pred_uncert.squeeze().cpu().numpy()
    final_pred = final_pred.clip(0, 1)
    if colored_dev is not None:
        depth_colored_img = Image.fromarray(colored_dev.cpu().numpy())
    elif color_map is not None:
        colored = colorize_depth_maps(final_pred, 0, 1, cmap=color_map).squeeze()
        colored = (colored * 255).astype(np.uint8)
        depth_colored_img = Image.fromarray(chw2hwc(colored))
    else:
        depth_colored_img = None
    return MarigoldDepthOutput(depth_np=final_pred, depth_colored=depth_colored_img, uncertainty=pred_uncert)


class MarigoldNormalsPipeline(_MarigoldPipelineBase):
    """Surface normals (reference marigold/marigold_normals_pipeline.py:77-479)."""
    _kind = "normals"
    _ckpt_hint = "prs-eth/marigold-normals-v1-1"
    _pred_channels = 3

    def __init__(self, unet, vae, scheduler, text_encoder=None, tokenizer=None,
                 default_denoising_steps: Optional[int] = None,
                 default_processing_resolution: Optional[int] = None, empty_text_embed=None):
        super().__init__(unet, vae, scheduler, text_encoder, tokenizer, None, None, default_denoising_steps,
                         default_processing_resolution, empty_text_embed)
        self.config = dict(default_denoising_steps=default_denoising_steps,
                           default_processing_resolution=default_processing_resolution)

    def _lcm_policy(self, n_step):
        raise RuntimeError("This pipeline implementation does not support the LCMScheduler. Please refer to "
                           "the project README.md for instructions about using LCM.")

    def _decode(self, latent):
        return self.decode_normals(latent)

    def decode_normals(self, normals_latent: torch.Tensor) -> torch.Tensor:
        """latent -> unit normals [B,3,H,W] (decode, clip, L2 normalise fused; reference :463-479,
        :437-440)."""
        return self.vae.decode(normals_latent, post=L.POST_NORMALS)

    def __call__(self, input_image: Union[Image.Image, torch.Tensor], denoising_steps: Optional[int] = None,
                 ensemble_size: int = 1, processing_res: Optional[int] = None, match_input_res: bool = True,
                 resample_method: str = "bilinear", batch_size: int = 0,
                 generator: Union[torch.Generator, None] = None, show_progress_bar: bool = True,
                 ensemble_kwargs: Dict = None,
                 init_latents: Optional[torch.Tensor] = None,
                 sequence: Optional[SequenceState] = None, guided_upsample=None, align=None) -> MarigoldNormalsOutput:
        return self._call(input_image, denoising_steps, ensemble_size, processing_res, match_input_res, resample_method, batch_size,
                          generator, ensemble_kwargs, init_latents, sequence, guided_upsample, align)

    _clip_range = (-1, 1)

    def _empty_output(self) -> MarigoldNormalsOutput:
        return MarigoldNormalsOutput(normals_np=None, normals_img=None, uncertainty=None)

    def _ensemble(self, target_preds, ensemble_kwargs):
        return ensemble_normals(target_preds, **(ensemble_kwargs or {}))

    def _tail(self, final_pred, pred_uncert) -> MarigoldNormalsOutput:
        return _normals_tail(final_pred, pred_uncert, final_pred.is_cuda and self.device_io_stages)


def _normals_tail(final_pred, pred_uncert, device_picture) -> MarigoldNormalsOutput:
    """The tail of the normals pipeline's ``_finish``: the picture, the arrays to the host, the clip."""
    img_dev = None
    if device_picture and final_pred.squeeze().dim() == 3:
        # the picture on the device (the clip to [-1, 1] is part of the kernel); the host gets the map and a uint8 HWC image
        img_dev = normals_visualization_device(final_pred.squeeze().float())
    final_pred = final_pred.squeeze().cpu().numpy()
    if pred_uncert is not None:
        pred_uncert = pred_uncert.squeeze().cpu().numpy()
    final_pred = final_pred.clip(-1, 1)
    if img_dev is not None:
        normals_img = Image.fromarray(img_dev.cpu().numpy())
    else:
        normals_img = ((final_pred + 1) * 127.5).astype(np.uint8)
        normals_img = Image.fromarray(chw2hwc(normals_img))
    return MarigoldNormalsOutput(normals_np=final_pred, normals_img=normals_img, uncertainty=pred_uncert)


# ------------------------------------------------------------------------------------------ IID

@dataclass
class IIDEntry:
    """One decomposed component (reference marigold/marigold_iid_pipeline.py:59-77): ``array`` [3,H,W] in
    [0,1], ``image`` PIL RGB, ``uncertainty`` [3,H,W] | None.  ``device_array`` (extension): the fp32 CUDA tensor ``array`` was read
    back from, [3,H,W], when the prediction was finished on the GPU - what the device scorer takes in place of an upload."""
    name: str
    array: Optional[np.ndarray] = None
    image: Optional[Image.Image] = None
    uncertainty: Optional[np.ndarray] = None
    device_array: Optional[torch.Tensor] = None


class MarigoldIIDOutput:
    """Named container of the predicted modalities (reference :80-161)."""

    def __init__(self, target_names: List[str]):
        self.n_targets = len(target_names)
        self.target_names = target_names
        self.entries: List[IIDEntry] = [IIDEntry(name=n) for n in target_names]
        self._by_name = {e.name: e for e in self.entries}
        self._filled = set()

    def _check_unfilled(self, name: str) -> None:
        if name not in self._by_name:
            raise KeyError(f"Unknown entry name: {name}")
        if name in self._filled:
            raise RuntimeError(f"Entry {name} already filled")

    def fill_entry(self, name: str, prediction: torch.Tensor, uncertainty: Optional[torch.Tensor] = None,
                   target_properties: Optional[Dict[str, Any]] = None) -> None:
        self._check_unfilled(name)
        array = prediction.squeeze().cpu().numpy()
        vis = array
        space = target_properties[name].get("prediction_space", "srgb")
        if space == "linear":   # linear radiometric space -> display gamma, optionally normalised to its maximum
            if target_properties[name].get("up_to_scale", False):
                vis = vis / max(vis.max(), 1e-6)
            vis = vis ** (1 / 2.2)
        self._set_entry(name, array, chw2hwc((vis * 255).astype(np.uint8)),
                        None if uncertainty is None else uncertainty.squeeze().cpu().numpy())

    def _set_entry(self, name: str, array: np.ndarray, image_hwc: np.ndarray, uncertainty: Optional[np.ndarray] = None,
                   device_array: Optional[torch.Tensor] = None) -> None:
        """Store one finished component: ``image_hwc`` is the uint8 [H,W,3] picture of ``array``."""
        self._check_unfilled(name)
        entry = self._by_name[name]
        entry.array = array
        entry.image = Image.fromarray(image_hwc)
        entry.uncertainty = uncertainty
        entry.device_array = device_array
        self._filled.add(name)

    @property
    def is_complete(self) -> bool:
        return len(self._filled) == self.n_targets

    def __getitem__(self, key: str) -> IIDEntry:
        return self._by_name[key]

    def __iter__(self):
        return iter(self.entries)


class MarigoldIIDPipeline(_MarigoldPipelineBase):
    """Intrinsic image decomposition (reference marigold/marigold_iid_pipeline.py:164-585): the UNet
    predicts 4 latent channels per modality in ``target_properties["target_names"]``
    (8 + ... input channels = image latent + all modality latents), every modality is decoded by the
    VAE separately (here: as extra batch entries of ONE decode program) and mapped to [0,1]."""
    _kind = "iid"
    _ckpt_hint = "prs-eth/marigold-iid-appearance-v1-1` or `prs-eth/marigold-iid-lighting-v1-1"

    def __init__(self, unet, vae, scheduler, text_encoder=None, tokenizer=None,
                 target_properties: Optional[Dict[str, Any]] = None, default_denoising_steps: Optional[int] = None,
                 default_processing_resolution: Optional[int] = None, empty_text_embed=None):
        super().__init__(unet, vae, scheduler, text_encoder, tokenizer, None, None, default_denoising_steps,
                         default_processing_resolution, empty_text_embed)
        self.target_properties = target_properties
        self.target_names = target_properties["target_names"]
        self.n_targets = len(self.target_names)
        self._target_latent_channels = 4 * self.n_targets
        self._pred_channels = 3 * self.n_targets
        if unet.config.out_channels != self._target_latent_channels or \
                unet.config.in_channels != 4 + self._target_latent_channels:
            raise ValueError(f"UNet with {unet.config.in_channels}->{unet.config.out_channels} channels does not "
                             f"match {self.n_targets} target(s) {self.target_names}")
        self.config = dict(target_properties=target_properties, default_denoising_steps=default_denoising_steps,
                           default_processing_resolution=default_processing_resolution)

    def _lcm_policy(self, n_step):
        raise RuntimeError("This pipeline implementation does not support the LCMScheduler. Please refer to the "
                           "project README.md for instructions about using LCM.")

    def _decode(self, latent):
        return self.decode_targets(latent)

    def decode_targets(self, target_latent: torch.Tensor) -> torch.Tensor:
        """[B,4n,h,w] -> [B,3n,H,W] in [0,1]: every modality through post_quant_conv + decoder
        (reference :556-585) with the clip / shift of :523-526 fused; modalities ride in the batch."""
        B, _, h, w = target_latent.shape
        dec = self.vae.decode(target_latent.reshape(B * self.n_targets, 4, h, w), post=L.POST_UNIT)
        return dec.reshape(B, 3 * self.n_targets, dec.shape[-2], dec.shape[-1])

    def fill_outputs(self, output: MarigoldIIDOutput, final_pred: torch.Tensor,
                     pred_uncert: Optional[torch.Tensor] = None):
        """``final_pred`` [1,3n,H,W] -> the entries of ``output``.  A CUDA prediction is finished on the device: one launch pair for
        the pictures of all targets (MG_OP_IID_VIS), then one read-back each for the arrays, the uncertainties and the pictures;
        a host tensor goes through ``fill_entry`` (numpy)."""
        if final_pred.is_cuda:
            props, n = self.target_properties, self.n_targets
            linear = [props[t].get("prediction_space", "srgb") == "linear" for t in self.target_names]
            up_to_scale = [bool(props[t].get("up_to_scale", False)) for t in self.target_names]
            dev = final_pred.contiguous().reshape(n, 3, final_pred.shape[-2], final_pred.shape[-1])
            images = iid_visualization_device(dev, linear, up_to_scale)
            arrays = dev.cpu().numpy()
            uncerts = None if pred_uncert is None else pred_uncert.reshape(n, 3, *pred_uncert.shape[-2:]).cpu().numpy()
            images = images.cpu().numpy()
            for i, name in enumerate(self.target_names):   # (squeeze: what fill_entry does to its slice)
                output._set_entry(name, arrays[i].squeeze(), images[i], None if uncerts is None else uncerts[i].squeeze(), dev[i])
            return
        for i, name in enumerate(self.target_names):
            output.fill_entry(name=name, prediction=final_pred[:, 3 * i:3 * i + 3],
                              uncertainty=None if pred_uncert is None else pred_uncert[:, 3 * i:3 * i + 3],
                              target_properties=self.target_properties)

    def __call__(self, input_image: Union[Image.Image, torch.Tensor], denoising_steps: Optional[int] = None,
                 ensemble_size: int = 1, processing_res: Optional[int] = None, match_input_res: bool = True,
                 resample_method: str = "bilinear", batch_size: int = 0,
                 generator: Union[torch.Generator, None] = None, show_progress_bar: bool = True,
                 ensemble_kwargs: Dict = None, init_latents: Optional[torch.Tensor] = None,
                 sequence: Optional[SequenceState] = None, guided_upsample=None, align=None) -> MarigoldIIDOutput:
        return self._call(input_image, denoising_steps, ensemble_size, processing_res, match_input_res, resample_method, batch_size,
                          generator, ensemble_kwargs, init_latents, sequence, guided_upsample, align)

    def _empty_output(self) -> MarigoldIIDOutput:
        return MarigoldIIDOutput(target_names=self.target_names)

    def _ensemble(self, target_preds, ensemble_kwargs):
        return ensemble_iid(target_preds, **(ensemble_kwargs or {}))

    def _tail(self, final_pred, pred_uncert) -> MarigoldIIDOutput:
        assert final_pred.dim() == 4 and final_pred.shape[1] == 3 * self.n_targets
        output = self._empty_output()
        self.fill_outputs(output, final_pred, pred_uncert)
        assert output.is_complete
        return output
