"""Model images: the pipeline's native programs for ONE problem shape, compiled ahead of time into a single file that
``libmarigold_hip.so`` loads and runs WITHOUT Python (``mg_model_load`` / ``mg_model_vae_encode`` / ``mg_model_denoise`` /
``mg_model_vae_decode`` in include/marigold_hip.h) - the module-level C entry points SURVEY.md section 8(b) proposes for the
seams ``single_infer`` calls (marigold_depth_pipeline.py:396-477: ``encode_rgb`` :491-495, the T-step ``unet`` +
``scheduler.step`` loop :455-468, ``decode_depth`` :498-516).

The Python engine stays the program BUILDER (graph emission in engine.py, weight packing in weights.py run once, here, at
export time); what a host in any language needs at run time is the flat op lists, the kernel-ready weights and a memory plan -
exactly what this file holds:

    header | buffer table | program table (+ named input / output slots) | relocation table | op arrays | weight bytes

Every device pointer inside an ``mg_op`` is recorded as (buffer, byte offset) - the loader allocates the buffers, uploads the
weights, zeroes what must start zeroed and patches the pointers.  ``export_model_image`` works on a host without a GPU (the
programs are built against host buffers exactly as ``mg_program_validate`` does), so the CPU test-suite round-trips an image
through the C loader.
"""
import ctypes
import struct

import torch

from . import _lib as L
from . import ops as O
from .modules import AutoencoderKLHIP, UNet2DConditionModelHIP

MAGIC = b"MGIMG1\0\0"
VERSION = 1
KIND_SCRATCH, KIND_ZERO, KIND_DATA = 0, 1, 2
SLOT_LN_COUNTERS = 100   # relocation slot of MG_OP_IGEMM's ticket address pair (ops.igemm_tickets); slots 0..15 = p[k]
_PRED = {"depth": (L.POST_DEPTH, 1), "normals": (L.POST_NORMALS, 3), "iid": (L.POST_UNIT, 3)}


def _tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, (tuple, list)):
        for o in obj:
            yield from _tensors(o)
    elif isinstance(obj, dict):
        for o in obj.values():
            yield from _tensors(o)


class _Buffers:
    """Interval map of every tensor the programs can point into."""

    def __init__(self):
        self.items = []   # [start, end, kind, tensor]

    def add(self, t, kind):
        n = t.numel() * t.element_size()
        if n == 0:
            return
        assert t.is_contiguous(), "model image: non-contiguous buffer"
        self.items.append([t.data_ptr(), t.data_ptr() + n, kind, t])

    def finalize(self):
        # merge overlapping / duplicate intervals (views of one storage); data beats zero beats scratch
        self.items.sort(key=lambda it: (it[0], -it[1]))
        merged = []
        for it in self.items:
            if merged and it[0] < merged[-1][1]:
                m = merged[-1]
                assert it[1] <= m[1], "model image: partially overlapping buffers"
                m[2] = max(m[2], it[2])
                continue
            merged.append(list(it))
        self.items = merged
        self.starts = [it[0] for it in merged]

    def find(self, ptr):
        import bisect
        k = bisect.bisect_right(self.starts, ptr) - 1
        if k < 0 or ptr >= self.items[k][1]:
            return None
        return k, ptr - self.items[k][0]


def _pad(f, align=64):
    pos = f.tell()
    f.write(b"\0" * ((-pos) % align))
    return f.tell()


def export_model_image(pipe, path, *, ensemble_size, height, width, denoising_steps=None, images_per_program=1):
    """Write the model image of ``pipe`` for images of ``height`` x ``width`` (the size fed to the VAE: after the pipeline's
    ``processing_res`` resize), ``ensemble_size`` members per picture and ``denoising_steps`` scheduler steps.  Works with the
    modules on the GPU (``pipe.to("cuda")``) or, without one, in the host-only mode.  Returns a dict describing the image.

    ``images_per_program`` = K > 1: the image runs K pictures per call (``mg_model_predict_many``) through the programs
    ``map_images(images_per_program=K)`` runs for a full group - one encode of K pictures, one denoising program of K x
    ``ensemble_size`` members, one decode; the header's ``cfg[13]`` is K.  K = 1 writes the one-picture image, ``cfg[13]`` = 0."""
    K = int(images_per_program)
    if K < 1:
        raise ValueError(f"export_model_image: images_per_program must be >= 1 (got {images_per_program})")
    if K > 1 and pipe._kind == "iid":
        raise ValueError("export_model_image: intrinsic-image models are exported for one picture per call (images_per_program=1): "
                         "mg_model_predict_iid takes one picture")
    unet, vae = pipe.unet, pipe.vae
    assert isinstance(unet, UNet2DConditionModelHIP) and isinstance(vae, AutoencoderKLHIP)
    if unet.ws is None:
        unet.dry()
        vae.dry()
    kind = pipe._kind
    post, cpred = _PRED[kind]
    B, T = int(ensemble_size), int(denoising_steps or pipe.default_denoising_steps)
    if pipe.empty_text_embed is None:
        pipe.encode_empty_text()
    if getattr(unet, "f16", False) or getattr(vae, "f16", False):
        raise ValueError("export_model_image: model images carry bf16 operands (the C host loads libmarigold_hip.so); "
                         "build the pipeline with compute_dtype=torch.bfloat16")
    unet.set_context(pipe.empty_text_embed)
    enc_seq, enc_in, enc_out = vae._program("encode", K, height, width)
    h, w = enc_out.shape[-2:]
    if K == 1:
        den = unet.denoise_program(B, h, w, pipe.scheduler, T, rgb_broadcast=True)
    else:   # the programs of a full group (pipeline._predict_group -> single_infer(..., rgb_members=B))
        den = unet.denoise_program(K * B, h, w, pipe.scheduler, T, rgb_members=B)
    n_mod = getattr(pipe, "n_targets", 1)
    dec_seq, dec_in, dec_out = vae._program("decode", K * B * n_mod, h, w, post)

    bufs = _Buffers()
    for mod in (unet, vae):
        for v in mod.ws.cache.values():
            for t in _tensors(v):
                bufs.add(t, KIND_DATA)
        for t in mod.pool.all:
            bufs.add(t, KIND_SCRATCH)
    progs = [("vae.encode", enc_seq, {"rgb": enc_in, "latent": enc_out}),
             ("denoise", den.seq, dict({"rgb_latent": den.rgb_latent, "x": den.x}, **{f"noise{k}": nz for k, nz in enumerate(den.noises)})),
             ("vae.decode", dec_seq, {"latent": dec_in, "pred": dec_out})]
    for _, seq, io in progs:
        for t in seq.keep:
            # zero-initialised state the kernels rely on (V^T pad columns, tickets, flash workspace): tagged by the builder
            # (Builder.zeros_persistent -> OpSeq.zero_state); everything else held by the program is a constant or an input /
            # output slot
            bufs.add(t, KIND_ZERO if t.data_ptr() in seq.zero_state else KIND_DATA)
    bufs.finalize()
    # the workspace pools also hold buffers of programs built earlier in this process for OTHER shapes: only what these three
    # programs point into travels
    used = set()
    for _, seq, io in progs:
        for op in seq.ops:
            for s_ in range(16):
                if op.p[s_]:
                    hit = bufs.find(op.p[s_])
                    if hit is not None:
                        used.add(hit[0])
            if op.kind == L.OP_IGEMM and O.igemm_tickets(op):
                hit = bufs.find(O.igemm_tickets(op))
                if hit is not None:
                    used.add(hit[0])
        for t in io.values():
            hit = bufs.find(t.data_ptr())
            if hit is not None:
                used.add(hit[0])
    bufs.items = [it for k, it in enumerate(bufs.items) if it[2] != KIND_SCRATCH or k in used]
    bufs.starts = [it[0] for it in bufs.items]

    sz_op = ctypes.sizeof(L.MgOp)
    with open(path, "wb") as f:
        ptab, relocs_all, ops_all = [], [], []
        for name, seq, io in progs:
            relocs, raw = [], bytearray()
            for k, op in enumerate(seq.ops):
                c = L.MgOp()
                ctypes.memmove(ctypes.addressof(c), ctypes.addressof(op), sz_op)
                for s in range(16):
                    ptr = c.p[s]
                    if ptr:
                        hit = bufs.find(ptr)
                        if hit is None:
                            raise RuntimeError(f"model image: op {k} ({seq.labels[k]}) of {name} points outside every known buffer (p[{s}])")
                        relocs.append((k, s, hit[0], hit[1]))
                        c.p[s] = None
                if c.kind == L.OP_IGEMM and O.igemm_tickets(c):
                    hit = bufs.find(O.igemm_tickets(c))
                    if hit is None:
                        raise RuntimeError(f"model image: the row-statistics tickets of op {k} of {name} are not in a known buffer")
                    relocs.append((k, SLOT_LN_COUNTERS, hit[0], hit[1]))
                    O.set_igemm_tickets(c, None)
                raw += bytes(c)
            slots = []
            for nm, t in io.items():
                hit = bufs.find(t.data_ptr())
                slots.append((nm, hit[0], hit[1], t.numel() * t.element_size()))
            ptab.append((name, len(seq.ops), slots))
            relocs_all.append(relocs)
            ops_all.append(bytes(raw))
        # ---- layout: header, buffer table, program table, then 64-byte aligned blobs
        n_buf, n_prog = len(bufs.items), len(progs)
        HDR, BUF, PROG, SLOT, REL = "<8sIIII16I", "<QQII", "<32sIIQQI", "<24sIIQQ", "<IIIIQ"
        MAXSLOT = 16
        prog_sz = struct.calcsize(PROG) + 4 + MAXSLOT * struct.calcsize(SLOT)
        table_end = struct.calcsize(HDR) + n_buf * struct.calcsize(BUF) + n_prog * prog_sz
        f.write(b"\0" * table_end)
        buf_off = []
        for (start, end, k, t) in bufs.items:
            if k == KIND_DATA:
                off = _pad(f)
                f.write(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() if t.numel() * t.element_size() == end - start
                        else bytes((ctypes.c_char * (end - start)).from_address(start)))
                buf_off.append(off)
            else:
                buf_off.append(0)
        ops_off, rel_off = [], []
        for raw, relocs in zip(ops_all, relocs_all):
            ops_off.append(_pad(f))
            f.write(raw)
            rel_off.append(_pad(f))
            for (k, s, b, o) in relocs:
                f.write(struct.pack(REL, k, s, b, 0, o))
        total = f.tell()
        f.seek(0)
        cfg = [B, height, width, h, w, T, cpred * n_mod, post, len(den.noises), sz_op, n_mod, dec_out.shape[-2], dec_out.shape[-1],
               K if K > 1 else 0] + [0] * 2
        f.write(struct.pack(HDR, MAGIC, VERSION, L.ABI_VERSION, n_buf, n_prog, *cfg))
        for (start, end, k, _t), off in zip(bufs.items, buf_off):
            f.write(struct.pack(BUF, end - start, off, k, 0))
        for (name, n_ops, slots), oo, ro, relocs in zip(ptab, ops_off, rel_off, relocs_all):
            assert len(slots) <= MAXSLOT, "model image: too many program slots"
            f.write(struct.pack(PROG, name.encode(), n_ops, len(relocs), oo, ro, len(slots)))
            f.write(b"\0" * 4)
            for (nm, b, o, n) in slots:
                f.write(struct.pack(SLOT, nm.encode(), b, 0, o, n))
            f.write(b"\0" * ((MAXSLOT - len(slots)) * struct.calcsize(SLOT)))
        assert f.tell() == table_end
    nbytes = {k: sum(it[1] - it[0] for it in bufs.items if it[2] == k) for k in (KIND_SCRATCH, KIND_ZERO, KIND_DATA)}
    return dict(path=path, file_bytes=total, buffers=n_buf, scratch_bytes=nbytes[KIND_SCRATCH], zero_bytes=nbytes[KIND_ZERO],
                data_bytes=nbytes[KIND_DATA], ops={n: c for (n, c, _s) in ptab}, latent_hw=(int(h), int(w)), B=B, steps=T,
                pred_channels=cpred * n_mod, step_noises=len(den.noises), images_per_program=K)


def export_color_table(cmap, path):
    """Write the 768 bytes (256 x RGB, uint8) of the matplotlib colour map ``cmap`` as the depth pipelines index it - the table
    ``util.image_util.colorize_depth_device`` builds - to ``path``: what a host without matplotlib uploads as
    ``mg_output_opts.lut256x3`` (examples/host_picture.cpp).  Returns the table (uint8 [256, 3])."""
    from .util.image_util import colormap_lut_u8
    table = colormap_lut_u8(cmap)
    assert table.shape == (256, 3) and table.dtype.itemsize == 1
    with open(path, "wb") as f:
        f.write(table.tobytes())
    return table


class ModelImage:
    """ctypes handle on a loaded model image - what a non-Python host does, spelled in Python for the tests and as a second,
    graph-free way to run a fixed-shape deployment: ``encode`` / ``denoise`` / ``decode`` take and return torch CUDA tensors
    but only their raw pointers cross into the library."""

    def __init__(self, path, device=0):
        lib = L.load()
        self._lib = lib
        self.handle = lib.mg_model_load(path.encode(), int(device))
        if not self.handle:
            L.check(1, "mg_model_load")
        cfg = (ctypes.c_int * 16)()
        L.check(lib.mg_model_info(self.handle, cfg), "mg_model_info")
        (self.B, self.H, self.W, self.h, self.w, self.steps, self.pred_channels, self.post, self.n_noise) = list(cfg)[:9]
        self.Hout, self.Wout = cfg[11], cfg[12]
        self.K = cfg[13] or 1   # pictures per call; B: the members of each
        self.device = device

    def validate(self):
        L.check(self._lib.mg_model_validate(self.handle), "mg_model_validate")

    def encode(self, rgb):
        out = torch.empty(self.K, 4, self.h, self.w, device=rgb.device, dtype=torch.float32)
        rgb = rgb.to(torch.float32).contiguous()
        assert tuple(rgb.shape) == (self.K, 3, self.H, self.W)
        L.check(self._lib.mg_model_vae_encode(self.handle, rgb.data_ptr(), out.data_ptr(), O.current_stream_handle()), "mg_model_vae_encode")
        return out

    def denoise(self, rgb_latent, x, step_noises=None):
        """``rgb_latent`` [K, 4, h, w]; ``x`` [K B, C, h, w], image-major; ``step_noises``: ``n_noise`` tensors shaped like ``x``."""
        x = x.to(torch.float32).contiguous().clone()
        assert rgb_latent.shape[0] == self.K and x.shape[0] == self.K * self.B
        nz = None
        if self.n_noise:
            nz = torch.stack(list(step_noises)).to(torch.float32).contiguous()
            assert nz.shape[0] == self.n_noise and nz.shape[1:] == x.shape
        L.check(self._lib.mg_model_denoise(self.handle, rgb_latent.contiguous().data_ptr(), x.data_ptr(),
                                           None if nz is None else nz.data_ptr(), O.current_stream_handle()), "mg_model_denoise")
        return x

    def decode(self, latent):
        out = torch.empty(self.K * self.B, self.pred_channels, self.Hout, self.Wout, device=latent.device, dtype=torch.float32)
        L.check(self._lib.mg_model_vae_decode(self.handle, latent.to(torch.float32).contiguous().data_ptr(), out.data_ptr(),
                                              O.current_stream_handle()), "mg_model_vae_decode")
        return out

    def predict_iid(self, u8, seed, *, opts=None, pictures=False, mode=0, reciprocal=None):
        """``mg_model_predict_iid`` on the uint8 CUDA picture ``u8`` [Hin, Win, 3]: -> (pred fp32 [3 n, out_h, out_w], unc fp32
        [3 n, Hout, Wout] | None for a single member, pictures uint8 [n, out_h, out_w, 3] | None unless ``pictures``).  ``opts``: an
        ``_lib.MgIidOpts`` (None = the defaults); ``mode`` / ``reciprocal``: the input resampling as in ``mg_rgb_prepare`` (by default
        the reciprocal normalisation when the picture is resampled, as the pipelines' input stage)."""
        assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[-1] == 3, "predict_iid: a uint8 CUDA [H, W, 3] picture"
        u8 = u8.contiguous()
        Hin, Win = u8.shape[:2]
        if reciprocal is None:
            reciprocal = (Hin, Win) != (self.H, self.W)
        oh, ow = ((opts.out_h or self.Hout), (opts.out_w or self.Wout)) if opts is not None else (self.Hout, self.Wout)
        n = self.pred_channels // 3
        pred = torch.empty(self.pred_channels, oh, ow, device=u8.device, dtype=torch.float32)
        unc = torch.empty(self.pred_channels, self.Hout, self.Wout, device=u8.device, dtype=torch.float32) if self.B > 1 else None
        pics = torch.empty(n, oh, ow, 3, device=u8.device, dtype=torch.uint8) if pictures else None
        L.check(self._lib.mg_model_predict_iid(self.handle, u8.data_ptr(), 1, Hin, Win, int(mode), int(bool(reciprocal)), int(seed) & ((1 << 64) - 1),
                                               None if opts is None else ctypes.byref(opts), pred.data_ptr(),
                                               None if unc is None else unc.data_ptr(), None if pics is None else pics.data_ptr(),
                                               O.current_stream_handle()), "mg_model_predict_iid", self._lib)
        return pred, unc, pics

    def predict_out(self, u8, seed, *, out_size=None, out_mode=0, lut=None, u16=False, picture=False, opts=None, mode=0, reciprocal=None):
        """``mg_model_predict_out`` on the uint8 CUDA picture ``u8`` [Hin, Win, 3]: the pipelines' output with ``match_input_res`` ->
        (pred fp32 [C, out_h, out_w] clipped, unc fp32 [Hout, Wout] | None for a single member, u16 uint16 [out_h, out_w] | None unless
        ``u16``, picture uint8 [out_h, out_w, 3] | None unless ``picture``, info = the four numbers of ``mg_ensemble_depth``).
        ``out_size``: (out_h, out_w), None = the model's output size; ``out_mode``: a key of ``ops.RESIZE_MODES`` or its number;
        ``lut``: the colour table, uint8 CUDA [256, 3] (a depth model's picture needs it); ``opts``: an ``_lib.MgPredictOpts``;
        ``mode`` / ``reciprocal``: the input resampling as in ``predict_iid``."""
        assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[-1] == 3, "predict_out: a uint8 CUDA [H, W, 3] picture"
        u8 = u8.contiguous()
        Hin, Win = u8.shape[:2]
        if reciprocal is None:
            reciprocal = (Hin, Win) != (self.H, self.W)
        oh, ow = (self.Hout, self.Wout) if out_size is None else (int(out_size[0]), int(out_size[1]))
        if lut is not None:
            assert lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 768, "predict_out: the colour table is uint8 CUDA [256, 3]"
            lut = lut.contiguous()
        out_opts = L.MgOutputOpts(0 if out_size is None else oh, 0 if out_size is None else ow, int(O.RESIZE_MODES.get(out_mode, out_mode)),
                                  None if lut is None else lut.data_ptr())
        dev = u8.device
        pred = torch.empty(self.pred_channels, oh, ow, device=dev, dtype=torch.float32)
        unc = torch.empty(self.Hout, self.Wout, device=dev, dtype=torch.float32) if self.B > 1 else None
        d16 = torch.empty(oh, ow, device=dev, dtype=torch.uint16) if u16 else None
        pic = torch.empty(oh, ow, 3, device=dev, dtype=torch.uint8) if picture else None
        info = (ctypes.c_double * 4)()
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        L.check(self._lib.mg_model_predict_out(self.handle, u8.data_ptr(), 1, Hin, Win, int(O.RESIZE_MODES.get(mode, mode)), int(bool(reciprocal)),
                                               int(seed) & ((1 << 64) - 1), None if opts is None else ctypes.byref(opts), ctypes.byref(out_opts),
                                               pred.data_ptr(), ptr(unc), ptr(d16), ptr(pic), info, O.current_stream_handle()),
                "mg_model_predict_out", self._lib)
        return pred, unc, d16, pic, list(info)

    def predict_many(self, u8s, seeds, *, out_size=None, out_mode=0, lut=None, u16=False, picture=False, opts=None, mode=0, reciprocal=None):
        """``mg_model_predict_many`` on n <= K uint8 CUDA pictures ``u8s`` (each [Hin, Win, 3], one size) with one seed each: what
        ``predict_out`` returns, stacked image-major -> (pred fp32 [n, C, out_h, out_w] clipped, unc fp32 [n, Hout, Wout] | None for a
        single member, u16 uint16 [n, out_h, out_w] | None unless ``u16``, picture uint8 [n, out_h, out_w, 3] | None unless
        ``picture``, info = n lists of the four numbers of ``mg_ensemble_depth``).  The other arguments are ``predict_out``'s and
        apply to every picture."""
        u8s, seeds = list(u8s), list(seeds)
        n = len(u8s)
        assert n >= 1 and len(seeds) == n, "predict_many: one seed per picture"
        for u8 in u8s:
            assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[-1] == 3, "predict_many: uint8 CUDA [H, W, 3] pictures"
            assert u8.shape == u8s[0].shape, "predict_many: the pictures of one call have one size"
        u8s = [u8.contiguous() for u8 in u8s]
        Hin, Win = u8s[0].shape[:2]
        if reciprocal is None:
            reciprocal = (Hin, Win) != (self.H, self.W)
        oh, ow = (self.Hout, self.Wout) if out_size is None else (int(out_size[0]), int(out_size[1]))
        if lut is not None:
            assert lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 768, "predict_many: the colour table is uint8 CUDA [256, 3]"
            lut = lut.contiguous()
        out_opts = L.MgOutputOpts(0 if out_size is None else oh, 0 if out_size is None else ow, int(O.RESIZE_MODES.get(out_mode, out_mode)),
                                  None if lut is None else lut.data_ptr())
        dev = u8s[0].device
        pred = torch.empty(n, self.pred_channels, oh, ow, device=dev, dtype=torch.float32)
        unc = torch.empty(n, self.Hout, self.Wout, device=dev, dtype=torch.float32) if self.B > 1 else None
        d16 = torch.empty(n, oh, ow, device=dev, dtype=torch.uint16) if u16 else None
        pic = torch.empty(n, oh, ow, 3, device=dev, dtype=torch.uint8) if picture else None
        info = (ctypes.c_double * (4 * n))()
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        L.check(self._lib.mg_model_predict_many(self.handle, n, (ctypes.c_void_p * n)(*[u8.data_ptr() for u8 in u8s]), 1, Hin, Win,
                                                int(O.RESIZE_MODES.get(mode, mode)), int(bool(reciprocal)),
                                                (ctypes.c_uint64 * n)(*[int(s) & ((1 << 64) - 1) for s in seeds]),
                                                None if opts is None else ctypes.byref(opts), ctypes.byref(out_opts),
                                                pred.data_ptr(), ptr(unc), ptr(d16), ptr(pic), info, O.current_stream_handle()),
                "mg_model_predict_many", self._lib)
        return pred, unc, d16, pic, [list(info[4 * i:4 * i + 4]) for i in range(n)]

    def close(self):
        if self.handle:
            self._lib.mg_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
