"""The tile gather ``mg_tile_crop`` (csrc/tiles.hip; ``tiles.crop``) on a real MI355X against the torch slicing it stands for, on both
operand libraries, in both layouts ([H, W, 3] and [3, H, W]), with canaries in front of and behind ``dst``.

The bound is equality: the kernel moves bytes.  Shapes: the smallest call (one 8 x 8 tile on an 8 x 8 canvas: fewer words than a
workgroup has lanes); tiles of 16 with an overlap of 8 = T / 2 on 24 x 40 (2 x 4 tiles); tiles of 64 with an overlap of 16 on 120 x 120,
where three tiles cover one coordinate along either axis (starts 0, 24, 56); tiles of 64 x 128 on 128 x 256 (the geometry of
tests/test_gpu_tiles.py: several workgroups per tile).  On each: the whole grid, a middle group that straddles a grid row,
and the last tile alone.  Every case runs with ``src`` and ``dst`` on a 16-byte boundary (the 8-byte vector path) and one byte behind
one (either pointer, or both: the byte path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LIBS = pytest.mark.parametrize("f16", [False, True], ids=["bf16-lib", "f16-lib"])
LAYOUTS = pytest.mark.parametrize("hwc", [True, False], ids=["hwc", "chw"])
# (canvas, tile size, overlap | None for the lone 8 x 8 tile, which no plan makes: an overlap of 8 is more than half of it)
PLANS = (((8, 8), (8, 8), None), ((24, 40), (16, 16), (8, 8)), ((120, 120), (64, 64), (16, 16)), ((128, 256), (64, 128), (16, 32)))
PAD, CANARY = 32, 0xA5


@pytest.fixture(scope="module")
def libs():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return {False: L.init(0), True: L.init(0, True)}


def _offset_buffer(nbytes, offset, fill=None):
    """-> (the whole buffer, its view of ``nbytes`` bytes that starts ``offset`` bytes behind a 16-byte boundary, PAD bytes into it)"""
    buf = torch.full((PAD + 16 + nbytes + PAD,), CANARY if fill is None else fill, dtype=torch.uint8, device="cuda")
    start = PAD + (-(buf.data_ptr() + PAD) % 16) + offset
    view = buf[start:start + nbytes]
    assert view.data_ptr() % 16 == offset
    return buf, view, start


def _groups(n, nx):
    """(first, count): everything; a middle group across the end of a grid row; the last tile alone"""
    out = [(0, n), (n - 1, 1)]
    if n > nx > 1:
        out.append((nx - 1, min(3, n - nx + 1)))
    return out


@LIBS
@LAYOUTS
def test_crop_is_the_torch_slicing(libs, f16, hwc):
    from marigold_amd import tiles as T
    lib = libs[f16]
    straddled = covered3 = False
    for k, (canvas, tile, overlap) in enumerate(PLANS):
        plan = T.TilePlan((0,), (0,), (8, 8), ((0, 0),)) if overlap is None else T.plan(canvas, tile, overlap)
        (H, W), (th, tw), n, nx = canvas, plan.tile_hw, len(plan.origins), len(plan.xstarts)
        covered3 |= any(sum(x <= c < x + tw for x in plan.xstarts) == 3 for c in range(W))
        g = torch.Generator().manual_seed(700 + k)
        host = torch.randint(0, 256, (H, W, 3) if hwc else (3, H, W), generator=g, dtype=torch.uint8)
        for src_off, dst_off in ((0, 0), (1, 1), (0, 1), (1, 0)):
            _, src, _ = _offset_buffer(host.numel(), src_off, fill=0)
            src.copy_(host.reshape(-1).cuda())
            picture = src.view(host.shape)
            for first, count in _groups(n, nx):
                straddled |= first % nx + count > nx and count < n
                want = torch.stack([host[y:y + th, x:x + tw] if hwc else host[:, y:y + th, x:x + tw] for y, x in plan.origins[first:first + count]])
                buf, dst, start = _offset_buffer(count * 3 * th * tw, dst_off)
                got = T.crop(picture, plan, first, count, out=dst, lib=lib)
                torch.cuda.synchronize()
                where = f"canvas {canvas} tiles {th}x{tw} [{first}, {first}+{count}) src+{src_off} dst+{dst_off}"
                assert got.shape == want.shape and got.data_ptr() == dst.data_ptr(), where
                assert np.array_equal(got.cpu().numpy(), want.numpy()), where
                whole = buf.cpu().numpy()
                assert (whole[:start] == CANARY).all() and (whole[start + dst.numel():] == CANARY).all(), where   # nothing beside dst is written
                assert np.array_equal(picture.cpu().numpy(), host.numpy()), where                                    # the picture is read only
    assert straddled and covered3


@LIBS
def test_crop_allocates_and_takes_a_batched_picture(libs, f16):
    """Without ``out``: a fresh tensor; [1, 3, H, W], what the pipelines hold, is the planes layout; the default is every tile."""
    from marigold_amd import tiles as T
    plan = T.plan((128, 256), (64, 128), (16, 32))
    host = torch.randint(0, 256, (1, 3, 128, 256), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    got = T.crop(host.cuda(), plan, lib=libs[f16])
    torch.cuda.synchronize()
    want = torch.stack([host[0, :, y:y + 64, x:x + 128] for y, x in plan.origins])
    assert got.shape == (9, 3, 64, 128) and np.array_equal(got.cpu().numpy(), want.numpy())
    with pytest.raises(Exception, match=r"mg_tile_crop: tiles \[8, 8 \+ 2\) of a grid of 3 x 3"):
        T.crop(host.cuda(), plan, 8, 2, lib=libs[f16])
    with pytest.raises(ValueError, match="out must be a contiguous uint8 tensor of 24576 elements"):
        T.crop(host.cuda(), plan, 0, 1, out=torch.empty(5, dtype=torch.uint8, device="cuda"), lib=libs[f16])
