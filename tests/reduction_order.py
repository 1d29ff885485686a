"""The order of the fp64 sums of the fit and score kernels (csrc/reduce.h), emulated in numpy float64: every product and every sum is
one numpy operation, so it rounds once, and the sums are taken in the device's order -

* a thread's own terms in the order its kernel adds them (``accumulate``),
* the 64 lanes of a wave in the xor butterfly: six steps ``v = v + v[lane ^ m]``, m = 32 ... 1 (``butterfly``),
* the waves of a block in wave order (``waves_sum``),
* the rows of the partial table in row order (``rows_sum``) or lane-strided, lane l taking rows l, l + 64, ... (``lane_rows_sum``),

followed by the 2 x 2 solve with the guards of each caller.  The three emulations below (``align_fit``, ``tile_fit``, ``eval_depth_ls``)
give the BITS the kernels give; tests/test_gpu_reduction_order.py asserts that on the device and tests/test_reduction_order_host.py
that they agree with the order-free restatements (tests/align_reference.py, the tile and score references) within 1e-11.  The cases
both files run are built here, once."""
import functools

import numpy as np

CHUNK = 4096                   # ALIGN_CHUNK, MG_TILE_FIT_CHUNK: pixels per workgroup of the two fits
THREADS = 256                  # ALIGN_THREADS, FIT_THREADS, EV_THREADS
EV_BLOCKS = 512                # rows of a score's partial table (csrc/iid_images.h)
_XOR = [np.arange(64) ^ m for m in (32, 16, 8, 4, 2, 1)]


# ---- the steps of csrc/reduce.h ------------------------------------------------------------------------------------------------------

def butterfly(v):
    """wave_sum_xor: v [64, ...], one entry per lane -> the same shape, every lane holding the sum"""
    for partner in _XOR:
        v = v + v[partner]
    return v


def waves_sum(w):
    """waves_sum_store: w [..., waves, N] -> [..., N], waves 0, 1, 2, ... in that order"""
    s = w[..., 0, :]
    for i in range(1, w.shape[-2]):
        s = s + w[..., i, :]
    return s


def block_sum(acc):
    """block_sum_store: acc [..., threads, N], the threads' own sums -> [..., N], the block's row of the partial table"""
    waves = acc.reshape(acc.shape[:-2] + (acc.shape[-2] // 64, 64, acc.shape[-1]))
    return waves_sum(butterfly(np.moveaxis(waves, -2, 0))[0])


def rows_sum(table):
    """column_sum / rows_sum: table [rows, N] -> [N], b ascending from 0.0"""
    s = np.zeros(table.shape[1:])
    for row in table:
        s = s + row
    return s


def lane_rows_sum(table):
    """lane_rows_sum: table [rows, N] -> [N]; lane l adds rows l, l + 64, ... from 0.0, then the butterfly"""
    a = np.zeros((64,) + table.shape[1:])
    for r0 in range(0, len(table), 64):
        rows = table[r0:r0 + 64]
        a[:len(rows)] = a[:len(rows)] + rows
    return butterfly(a)[0]


def accumulate(terms, valid):
    """terms [steps, ..., N], valid [steps, ...] -> [..., N]: from 0.0, step by step, a term joins where it is valid"""
    acc = np.zeros(terms.shape[1:])
    for term, ok in zip(terms, valid):
        acc = np.where(ok[..., None], acc + np.where(ok[..., None], term, 0.0), acc)
    return acc


def scale_shift_solve(n, Sx, Sy, Sxx, Sxy):
    """scale_shift_solve -> (det, s, t), unguarded"""
    with np.errstate(all="ignore"):
        det = n * Sxx - Sx * Sx
        s = (n * Sxy - Sx * Sy) / det
        t = (Sy - s * Sx) / n
    return det, s, t


def _padded(a, size, fill):
    out = np.full(size, fill, a.dtype)
    out[:a.size] = a.reshape(-1)
    return out


# ---- mg_depth_align_fit with iters = 0: the unweighted sums and the solve (csrc/align.hip) ------------------------------------------

def align_fit(d, ref, mask=None, fit_shift=True):
    """-> (s, t, flag).  Chunk c, thread t takes pixels c 4096 + t + 256 j, j = 0 ... 15 in that order."""
    d32, g32 = np.asarray(d, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    n = d32.size
    chunks = -(-n // CHUNK)
    inside = _padded(np.ones(n, bool) if mask is None else np.asarray(mask).reshape(-1) != 0, chunks * CHUNK, False)
    d32, g32 = _padded(d32, chunks * CHUNK, np.nan), _padded(g32, chunks * CHUNK, np.nan)
    valid = inside & np.isfinite(d32) & np.isfinite(g32)
    x, g = np.where(valid, d32, 0).astype(np.float64), np.where(valid, g32, 0).astype(np.float64)
    w = np.ones_like(x)
    wd = w * x
    terms = np.stack([np.ones_like(x), w, wd, w * g, wd * x, wd * g], axis=-1)
    steps = CHUNK // THREADS
    terms = terms.reshape(chunks, steps, THREADS, 6).transpose(1, 0, 2, 3)
    valid = valid.reshape(chunks, steps, THREADS).transpose(1, 0, 2)
    count, N, Sd, Sg, Sdd, Sdg = lane_rows_sum(block_sum(accumulate(terms, valid)))
    s, t, bad = np.float64(1.0), np.float64(0.0), 1
    with np.errstate(all="ignore"):
        if count >= 2.0:
            if fit_shift:
                det, fs, ft = scale_shift_solve(N, Sd, Sg, Sdd, Sdg)
                if det > 1e-12 * N * N:
                    s, t, bad = fs, ft, 0
            elif Sdd > 1e-12 * N:
                s, bad = Sdg / Sdd, 0
    if bad or not s > 0.0 or not np.isfinite(s) or not np.isfinite(t):
        s, t, bad = np.float64(1.0), np.float64(0.0), 1
    return float(s), float(t), bad


ALIGN_SIZES = (1, 65, 4097, 12293, 270341)   # 270 341: 66 chunks and a ragged one - the solve's lanes 0 and 1 take a second row


@functools.lru_cache(maxsize=None)
def align_cases():
    """[(d, ref, mask | None, fit_shift)]: the scenes of tests/test_gpu_align.py at ALIGN_SIZES, with and without the mask, with and
    without the planted NaN and +-inf, with and without the shift"""
    from tests.test_gpu_align import _scene
    cases = []
    for n in ALIGN_SIZES:
        for masked in (False, True):
            for planted in (False, True):
                if planted and n < 63:
                    continue
                d, ref, mask = _scene(n, masked, planted)
                cases += [(d, ref, mask, fit_shift) for fit_shift in (1, 0)]
    return cases


# ---- mg_tile_fit (csrc/tiles.hip) -------------------------------------------------------------------------------------------------------

def _bilinear_src(n_out, n_in):
    """bilinear_src of csrc/tiles.hip along one axis -> (i0, i1, l1) for every destination index"""
    scale = np.float64(n_in) / np.float64(n_out)
    src = scale * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5
    src = np.where(src < 0.0, 0.0, src)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.where(i0 < n_in - 1, i0 + 1, i0)
    return i0, i1, np.clip(src - i0.astype(np.float64), 0.0, 1.0)


def guide_on_canvas(guide, canvas):
    """The guide sampled at every canvas pixel in fp64 as tile_fit_partial_kernel samples it, product by product: torch's bilinear rule
    with align_corners = False.  The tile reference (tests/test_gpu_tiles.py) takes the same samples from ``F.interpolate`` in double,
    whose last bits differ from these (it rounds differently: the host test bounds the difference); bits need the kernel's own
    roundings, so they are restated here."""
    g = np.asarray(guide, np.float32).astype(np.float64)
    r0, r1, ly = _bilinear_src(canvas[0], g.shape[0])
    c0, c1, lx = _bilinear_src(canvas[1], g.shape[1])
    top = (1.0 - lx) * g[r0][:, c0] + lx * g[r0][:, c1]
    bot = (1.0 - lx) * g[r1][:, c0] + lx * g[r1][:, c1]
    return (1.0 - ly)[:, None] * top + ly[:, None] * bot


def tile_fit(tiles, ys, xs, full):
    """tiles [n, th, tw] fp32 (tile i at (ys[i // nx], xs[i % nx])), full = guide_on_canvas -> (coef [n, 2], flags [n]).  Chunk c,
    thread t takes the float4s c 1024 + 256 j + t, j = 0 ... 3, and the four pixels of each in turn."""
    tiles = np.asarray(tiles, np.float32)
    n, th, tw = tiles.shape
    chunks = -(-th * tw // CHUNK)
    coef, flags = np.zeros((n, 2)), np.zeros(n, np.int32)
    for i, (y0, x0) in enumerate((y, x) for y in ys for x in xs):
        d32 = _padded(tiles[i], chunks * CHUNK, np.nan)                       # beyond the tile a NaN, which no sum takes
        G = _padded(np.ascontiguousarray(full[y0:y0 + th, x0:x0 + tw]), chunks * CHUNK, 0.0)
        valid = np.isfinite(d32) & np.isfinite(G)
        d, G = np.where(valid, d32, 0).astype(np.float64), np.where(valid, G, 0.0)
        terms = np.stack([np.ones_like(d), d, G, d * d, d * G], axis=-1)
        # pixel = c 4096 + j 1024 + t 4 + k -> steps (j, k)
        terms = terms.reshape(chunks, 4, THREADS, 4, 5).transpose(1, 3, 0, 2, 4).reshape(16, chunks, THREADS, 5)
        valid = valid.reshape(chunks, 4, THREADS, 4).transpose(1, 3, 0, 2).reshape(16, chunks, THREADS)
        N, Sd, Sg, Sdd, Sdg = lane_rows_sum(block_sum(accumulate(terms, valid)))
        s, t, flag = 0.0, (Sg / N if N > 0.0 else 0.0), 1
        det, fs, ft = scale_shift_solve(N, Sd, Sg, Sdd, Sdg)
        if N >= 2.0 and det > 1e-12 * N * N and fs > 0.0:
            s, t, flag = fs, ft, 0
        coef[i], flags[i] = (s, t), flag
    return coef, flags


TILE_SHAPES = ((8, 8), (64, 72), (520, 520))   # one part-filled chunk; two chunks; 67 chunks: the solve's lanes 0 - 2 take a second row


@functools.lru_cache(maxsize=None)
def tile_cases():
    """[(tiles [2, th, tw], ys, xs, canvas, guide)]: two tiles side by side, eight pixels apart, on a canvas that a smaller guide is
    sampled onto; the second tile has holes (NaN, +-inf)"""
    import torch
    cases = []
    for k, (th, tw) in enumerate(TILE_SHAPES):
        g = torch.Generator().manual_seed(900 + k)
        ys, xs, canvas = [8], [0, 8], (th + 16, tw + 8)
        guide = torch.rand((5, 7) if th < 100 else (61, 93), generator=g).numpy()
        full = torch.from_numpy(guide_on_canvas(guide, canvas))
        tiles = []
        for i, x0 in enumerate(xs):
            s, t = 0.3 + 2.7 * float(torch.rand((), generator=g)), float(torch.rand((), generator=g)) * 2 - 1
            d = ((full[8:8 + th, x0:x0 + tw] - t) / s + 0.05 * torch.randn(th, tw, generator=g, dtype=torch.float64)).float().contiguous()
            if i == 1:
                flat = d.view(-1)
                for j, v in enumerate((float("nan"), float("inf"), float("-inf"), float("nan"))):
                    flat[(j * 13 + 5) % flat.numel()] = v
            tiles.append(d)
        cases.append((torch.stack(tiles).numpy(), ys, xs, canvas, guide))
    return cases


# ---- MG_OP_EVAL_DEPTH_LS: the five raw sums (csrc/evalscore.hip) ---------------------------------------------------------------------------

def eval_depth_ls(pred, gt, mask, max_res=None, disparity=False):
    """-> [n, Sx, Sy, Sxx, Sxy].  Block b, thread t takes the fit's pixels b 256 + t, then every (blocks 256)-th after it."""
    from marigold_amd import ops
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    H, W = pred.shape
    ow, inv = ops.eval_fit_width(H, W, max_res)
    total = H * (ow or W)
    src = np.arange(total)
    if ow:   # fit_pixel: the width alone is sub-sampled, the source column in fp32
        row, col = src // ow, src % ow
        sc = np.minimum(np.floor(col.astype(np.float32) * np.float32(inv)), np.float32(W - 1)).astype(np.int64)
        src = row * W + sc
    nblk = max(1, min(-(-total // THREADS), EV_BLOCKS))
    p, g = pred.reshape(-1)[src], gt.reshape(-1)[src]
    valid = np.asarray(mask).reshape(-1)[src] != 0
    y = g
    if disparity:
        with np.errstate(all="ignore"):
            valid &= (g > 0) & (p > 0)
            y = np.float32(1.0) / g
    x, yd = np.where(valid, p, 0).astype(np.float64), np.where(valid, y, 0).astype(np.float64)
    terms = np.stack([np.ones_like(x), x, yd, x * x, x * yd], axis=-1)
    stride = nblk * THREADS
    steps = -(-total // stride)
    terms = np.concatenate([terms, np.zeros((steps * stride - total, 5))]).reshape(steps, nblk, THREADS, 5)
    valid = _padded(valid, steps * stride, False).reshape(steps, nblk, THREADS)
    return rows_sum(block_sum(accumulate(terms, valid)))


@functools.lru_cache(maxsize=None)
def eval_cases():
    """[(pred, gt, mask, max_res, disparity)]: 3 x 5 (a part of one block), 37 x 53, 256 x 512 (exactly 512 full blocks), 384 x 384 (the
    grid-stride loop takes a second pixel); 37 x 53 sub-sampled to a width of 20; 384 x 384 as disparity, with holes in both maps"""
    r = np.random.default_rng(4242)
    cases = []
    for (h, w), max_res, disparity in (((3, 5), None, False), ((37, 53), None, False), ((256, 512), None, False), ((384, 384), None, False),
                                       ((37, 53), 20, False), ((384, 384), None, True)):
        gt = r.uniform(0.5, 9.5, (h, w)).astype(np.float32)
        pred = ((gt.max() - gt) / (gt.max() - gt.min()) * 0.9 + 0.05 + r.normal(0, 0.02, gt.shape)).astype(np.float32)
        mask = (r.uniform(size=gt.shape) > 0.25).astype(np.uint8)
        if disparity:
            gt[r.uniform(size=gt.shape) < 0.05] = 0.0
            pred[r.uniform(size=gt.shape) < 0.05] = -0.01
        cases.append((pred, gt, mask, max_res, disparity))
    return cases
