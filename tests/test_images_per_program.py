"""Host checks of ``map_images(images_per_program=k)``: the grouping of consecutive images by processed size (stand-in
pipelines, no engine), the refusals, the denoising programs with several images' latents (``rgb_members``) against the
kernels' contract at full size, and today's programs pinned op for op."""
import hashlib
import struct
from types import SimpleNamespace

import pytest
import torch

from marigold_amd.pipeline import MarigoldDepthPipeline


class _StandIn(MarigoldDepthPipeline):
    """Records what reaches the engine: lone calls and groups; outputs are (image tag, generator tag)."""

    def __init__(self, processing_res=0):
        self.unet = SimpleNamespace(device=torch.device("cpu"))
        self.default_processing_resolution = processing_res
        self.empty_text_embed = None
        self._member_group = None
        self._member_parallel = False
        self._member_root = None
        self._member_force = False
        self._lanes = []
        self.calls = []

    def __call__(self, image, generator=None, **kw):
        self.calls.append(("lone", [image.tag]))
        return (image.tag, generator)

    def _call_group(self, images, generators, call_kwargs):
        self.calls.append(("group", [im.tag for im in images]))
        return [(im.tag, None if generators is None else g) for im, g in zip(images, generators or [None] * len(images))]


def _img(tag, h, w):
    t = torch.zeros(1, 3, h, w, dtype=torch.uint8)
    t.tag = tag
    return t


def test_grouping_order_size_flush_and_last_partial_group():
    pipe = _StandIn()
    sizes = [(8, 16)] * 5 + [(16, 8)] * 2 + [(8, 16)] * 3
    imgs = [_img(i, *s) for i, s in enumerate(sizes)]
    gens = [f"g{i}" for i in range(len(imgs))]
    outs = list(pipe.map_images(imgs, generators=gens, images_per_program=3, ensemble_size=2))
    assert outs == [(i, f"g{i}") for i in range(len(imgs))]   # input order, each image with its own generator
    assert pipe.calls == [("group", [0, 1, 2]), ("group", [3, 4]), ("group", [5, 6]), ("group", [7, 8, 9])]
    pipe.calls = []
    outs = list(pipe.map_images(iter(imgs[:8]), images_per_program=4))   # any iterable; a lone image of a size runs alone
    assert [o[0] for o in outs] == list(range(8))
    assert pipe.calls == [("group", [0, 1, 2, 3]), ("lone", [4]), ("group", [5, 6]), ("lone", [7])]
    pipe.calls = []
    list(pipe.map_images(imgs[:3], images_per_program=1))                 # default form: one call per image
    assert pipe.calls == [("lone", [0]), ("lone", [1]), ("lone", [2])]


def test_grouping_uses_the_processed_size():
    """With processing_res > 0 images of different input sizes but one processed size share a program."""
    pipe = _StandIn(processing_res=64)
    imgs = [_img(0, 32, 64), _img(1, 64, 128), _img(2, 64, 64), _img(3, 128, 128)]
    list(pipe.map_images(imgs, images_per_program=4))
    assert pipe.calls == [("group", [0, 1]), ("group", [2, 3])]
    pipe.calls = []
    list(pipe.map_images(imgs, images_per_program=4, processing_res=0))
    assert pipe.calls == [("lone", [0]), ("lone", [1]), ("lone", [2]), ("lone", [3])]


def test_images_per_program_refusals():
    pipe = _StandIn()
    imgs = [_img(i, 8, 16) for i in range(4)]
    with pytest.raises(ValueError, match="images_per_program"):
        list(pipe.map_images(imgs, images_per_program=0))
    with pytest.raises(ValueError, match="init_latents"):
        list(pipe.map_images(imgs, images_per_program=2, init_latents=torch.zeros(1, 4, 1, 2)))
    with pytest.raises(ValueError, match="generator"):
        list(pipe.map_images(imgs, images_per_program=2, generator=torch.Generator()))
    pipe._sharded = lambda: True
    with pytest.raises(ValueError, match="member-parallel"):
        list(pipe.map_images(imgs, images_per_program=2))
    with pytest.raises(TypeError):
        list(_StandIn().map_images([imgs[0], "not an image"], images_per_program=2))


def test_lanes_count_programs():
    """The default lane count is that of the members one program holds."""
    pipe = _StandIn()
    assert pipe.maps_in_flight_for(4 * 2) == pipe.small_ensemble_maps_in_flight
    assert pipe.maps_in_flight_for(5 * 2) == pipe.default_maps_in_flight


def test_cli_and_harness_flag():
    from marigold_amd import cli
    from marigold_amd.evaluation import harness
    base = ["--input_rgb_dir", "in", "--output_dir", "out"]
    assert cli.build_parser("depth").parse_args(base).images_per_program == 1
    assert cli.build_parser("iid").parse_args(base + ["--images_per_program", "4"]).images_per_program == 4
    req = ["--dataset_config", "c", "--base_data_dir", "d", "--output_dir", "o", "--denoise_steps", "1",
           "--processing_res", "0", "--ensemble_size", "1"]
    assert harness.infer_parser("normals").parse_args(req).images_per_program == 1
    assert harness.infer_parser("depth").parse_args(req + ["--images_per_program", "8"]).images_per_program == 8


# ---- programs ------------------------------------------------------------------------------------------------------

def _dry_unet(cfg):
    from marigold_amd.arch import unet_param_shapes
    from marigold_amd.modules import UNet2DConditionModelHIP
    unet = UNet2DConditionModelHIP({k: torch.zeros(s) for k, s in unet_param_shapes(cfg).items()}, cfg).dry()
    unet.set_context(torch.zeros(1, 2, cfg.cross_attention_dim))
    return unet


def test_several_images_programs_validate_at_full_size():
    """denoise_program(B = k E, rgb_members = E) at 768^2 (96 x 96 latent) passes the kernels' contract (mg_program_validate);
    conv_in's staging reads image b // E; bad divisors are refused by the host and by the validator."""
    from marigold_amd import _lib as L, ops as O
    from marigold_amd.arch import UNetConfig
    from marigold_amd.schedulers import DDIMScheduler
    unet = _dry_unet(UNetConfig())
    for k, E in ((4, 1), (2, 5)):
        prog = unet.denoise_program(k * E, 96, 96, DDIMScheduler(), 2, rgb_members=E)
        prog.seq.validate()
        assert tuple(prog.rgb_latent.shape) == (k, 4, 96, 96) and tuple(prog.x.shape) == (k * E, 4, 96, 96)
        i2c = [op for op in prog.seq.ops if op.kind == L.OP_IM2COL_SMALL]
        assert len(i2c) == 2 and all(r.src0_broadcast == 0 and r.members_per_src0 == E and r.src0 == prog.rgb_latent.data_ptr() for r in map(O.Raw, i2c))
    # the legacy programs' keys are untouched; a divisor form is a program of its own
    assert unet.denoise_program(4, 96, 96, DDIMScheduler(), 2, rgb_members=1) is not unet.denoise_program(4, 96, 96, DDIMScheduler(), 2,
                                                                                                        rgb_broadcast=False)
    with pytest.raises(ValueError, match="rgb_members"):
        unet.denoise_program(4, 96, 96, DDIMScheduler(), 2, rgb_members=3)
    buf = torch.zeros(1 << 16, dtype=torch.float32)
    for kw, what in ((dict(members_per_src0=3), "not a multiple"), (dict(members_per_src0=2, bcast0=True), "both set")):
        bad = O.OpSeq("bad")
        bad.add(O.im2col_small(buf, buf, buf, B=4, H=4, W=4, C0=4, C1=4, Kp=128, **kw), what)
        with pytest.raises(L.MarigoldHipError, match=what):
            bad.validate()
    ok = O.OpSeq("ok")
    ok.add(O.im2col_small(buf, buf, buf, B=6, H=4, W=4, C0=4, C1=4, Kp=128, members_per_src0=3), "divisor")
    ok.validate()


def _digest(ops):
    """sha256 of every op word; device addresses replaced by their order of first appearance (they differ per run)."""
    from marigold_amd import _lib as L
    h = hashlib.sha256()
    ids = {}

    def pid(v):
        return ids.setdefault(v, len(ids) + 1) if v else 0
    for op in ops:
        i = list(op.i)
        if op.kind == L.OP_IGEMM and (i[29] or i[30]):   # the row-block tickets' address as two int32 halves
            i[29:31] = [pid((i[29] & 0xffffffff) | ((i[30] & 0xffffffff) << 32)), 0]
        h.update(struct.pack("<i", op.kind) + struct.pack("<40i", *i) + bytes(op.f) + bytes(op.l))
        h.update(struct.pack("<16q", *[pid(v) for v in op.p]))
    return h.hexdigest()


# digests of the programs the engine emitted before images_per_program existed
_PINNED = {
    ("tiny", True): "5153301258281755d059480e1b004f0ce7b8d28dff59c304b4ac0cbb9b7b83ec",
    ("tiny", False): "088136f42e21fa3599892aabfb53665789944ecd905ba8a15ee7f20eca258293",
    ("full", True): "a992d2bae53931e7beb445f212fed55816a6f5a0dba0d5d4bc158d3f44ee05c5",
    ("full", False): "60c50c83d432f1042e18368a973aad0f9485a08be06cd03f9e1e9d34438ad597",
    ("full1", True): "2e6626fa675b2a22bc62f92354732def1531dfe580e6cd0db268325b421f1ff9",
}


def test_todays_programs_are_unchanged():
    """Every op of the rgb_broadcast=True / False programs (tiny B = 3; full size B = 10 and B = 1, 2 DDIM steps) is
    byte-identical to what the engine emitted before the divisor form existed."""
    from marigold_amd.arch import TINY_UNET, UNetConfig
    from marigold_amd.schedulers import DDIMScheduler
    for name, cfg, B, hw, T in (("tiny", TINY_UNET, 3, (8, 16), 2), ("full", UNetConfig(), 10, (96, 96), 2),
                                ("full1", UNetConfig(), 1, (96, 96), 1)):
        unet = _dry_unet(cfg)
        for bc in ((True,) if B == 1 else (True, False)):
            prog = unet.denoise_program(B, *hw, DDIMScheduler(), T, rgb_broadcast=bc)
            assert _digest(prog.seq.ops) == _PINNED[(name, bc)], (name, bc)
