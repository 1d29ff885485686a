"""Model images: the pipeline's native programs for one problem shape - or, with ``configs=[...]``, for several - compiled ahead of
time into a single file that
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

An image of several configurations (version 2) has the same parts with one more table in front:

    header | configurations, scratch region | configuration table (16 words + three programs each) | buffer table | blobs

The modules' packed weights (``mod.ws.cache``) are written once, as buffers every configuration refers to; the loader keeps them in
an allocation that ``mg_model_replica`` handles share.  A call with the keywords of one configuration writes the version-1 file it
always wrote.

An image with the tiny autoencoder (``tiny_vae=True``, version 3) is a version-2 file, for one configuration or several, with two
differences: the ``vae.encode`` and ``vae.decode`` entries of a configuration hold no ops, only their named slots and a workspace slot
(scratch: the loader runs ``mg_tiny_vae_encode`` / ``mg_tiny_vae_decode`` on them), and behind the buffer table lies one table more, the
members of ``struct mg_tiny_vae`` as (shared buffer, byte offset):

    header | configurations, scratch region | configuration table | buffer table | tiny VAE members | blobs
"""
import ctypes
import struct

import torch

from . import _lib as L
from . import ops as O
from .modules import AutoencoderKLHIP, AutoencoderTinyHIP, UNet2DConditionModelHIP

MAGIC = b"MGIMG1\0\0"
VERSION = 1
VERSION_CONFIGS = 2   # several configurations in one image (export_model_image(configs=[...]))
VERSION_TINY = 3      # the tiny autoencoder instead of the AutoencoderKL (export_model_image(tiny_vae=True)): the version-2 layout, the
                      # two VAE entries of a configuration without ops, one table more (the members of struct mg_tiny_vae)
TINY_MEMBER, TINY_ABSENT = "<IIQ", 0xFFFFFFFF   # a member of mg_tiny_vae: buffer (TINY_ABSENT: a NULL member), pad, byte offset
KIND_SCRATCH, KIND_ZERO, KIND_DATA, KIND_SHARED = 0, 1, 2, 3   # SHARED: the weight cache of a version-2 image, stored once
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


_CFG_KEYS = ("ensemble_size", "height", "width", "denoising_steps", "images_per_program")
HDR, BUF, PROG, SLOT, REL = "<8sIIII16I", "<QQII", "<32sIIQQI", "<24sIIQQ", "<IIIIQ"
V2, MAXSLOT = "<IIQ", 16   # version 2, after the header: configurations, pad, bytes of the scratch region


def _r256(n):
    return (n + 255) // 256 * 256


class _Region:
    """``nbytes`` of scratch that exist in an image's memory plan only - the slots and workspaces of the tiny autoencoder's calls: an
    address range no tensor has, with what ``_Buffers`` and ``_relocate`` ask of a tensor."""
    _next = 1 << 60

    def __init__(self, nbytes):
        self.nbytes, self.ptr = int(nbytes), _Region._next
        _Region._next += _r256(self.nbytes) + 256

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def is_contiguous(self):
        return True


class _NoOps:
    """What stands where a VAE program stands in a tiny image: no ops, the named slots only."""
    ops, keep, labels, zero_state = (), (), (), frozenset()


def _build_tiny_vae(pipe, K, B, n_mod, height, width, post, cpred):
    """The two VAE entries of a tiny configuration: the slots ``mg_tiny_vae_encode`` (K pictures) and ``mg_tiny_vae_decode`` (all
    K B n_mod members in one call) read and write, and their workspaces -> (encode entry, decode entry, (h, w))."""
    h, w = pipe.vae.latent_hw((height, width))
    lib = L.load()
    need = [lib.mg_tiny_vae_workspace_bytes(0, K, height, width), lib.mg_tiny_vae_workspace_bytes(1, K * B * n_mod, h, w)]
    if min(need) < 0:
        L.check(1, "mg_tiny_vae_workspace_bytes", lib)
    enc = ("vae.encode", _NoOps, {"rgb": _Region(K * 3 * height * width * 4), "latent": _Region(K * 4 * h * w * 4), "ws": _Region(need[0])})
    dec = ("vae.decode", _NoOps, {"latent": _Region(K * B * n_mod * 4 * h * w * 4), "pred": _Region(K * B * n_mod * cpred * 64 * h * w * 4),
                                  "ws": _Region(need[1])})
    return enc, dec, (h, w)


def _build(pipe, ensemble_size, height, width, denoising_steps=None, images_per_program=1):
    """The three programs of one configuration, built (or found) in the modules of ``pipe``, and its 16 words (``_lib.CFG``)."""
    K = int(images_per_program)
    if K < 1:
        raise ValueError(f"export_model_image: images_per_program must be >= 1 (got {images_per_program})")
    if K > 1 and pipe._kind == "iid":
        raise ValueError("export_model_image: intrinsic-image models are exported for one picture per call (images_per_program=1): "
                         "mg_model_predict_iid takes one picture")
    unet, vae = pipe.unet, pipe.vae
    tiny = isinstance(vae, AutoencoderTinyHIP)   # (no op program: nothing of it to build, host-only or not)
    assert isinstance(unet, UNet2DConditionModelHIP) and (tiny or isinstance(vae, AutoencoderKLHIP))
    if unet.ws is None:
        unet.dry()
        if not tiny:
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
    n_mod = getattr(pipe, "n_targets", 1)
    if tiny:
        enc, dec, (h, w) = _build_tiny_vae(pipe, K, B, n_mod, int(height), int(width), post, cpred)
        out_hw = (8 * h, 8 * w)
    else:
        enc_seq, enc_in, enc_out = vae._program("encode", K, height, width)
        h, w = enc_out.shape[-2:]
    if K == 1:
        den = unet.denoise_program(B, h, w, pipe.scheduler, T, rgb_broadcast=True)
    else:   # the programs of a full group (pipeline._predict_group -> single_infer(..., rgb_members=B))
        den = unet.denoise_program(K * B, h, w, pipe.scheduler, T, rgb_members=B)
    if not tiny:
        dec_seq, dec_in, dec_out = vae._program("decode", K * B * n_mod, h, w, post)
        enc, dec = ("vae.encode", enc_seq, {"rgb": enc_in, "latent": enc_out}), ("vae.decode", dec_seq, {"latent": dec_in, "pred": dec_out})
        out_hw = dec_out.shape[-2:]
    progs = [enc,
             ("denoise", den.seq, dict({"rgb_latent": den.rgb_latent, "x": den.x}, **{f"noise{k}": nz for k, nz in enumerate(den.noises)})),
             dec]
    words = dict(members=B, height=height, width=width, latent_h=h, latent_w=w, steps=T, channels=cpred * n_mod, post=post,
                 step_noises=len(den.noises), op_bytes=ctypes.sizeof(L.MgOp), modalities=n_mod, out_h=out_hw[0], out_w=out_hw[1],
                 pictures=K if K > 1 else 0, vae=L.VAE_TINY if tiny else L.VAE_KL)
    assert set(words) == set(L.CFG), "model image: every configuration word is named once"
    return progs, [int(words[name]) for name in L.CFG] + [0] * (L.CFG_WORDS - len(L.CFG))


def _plan(pipe, progs, cache_kind=KIND_DATA):
    """Every buffer the programs point into: the modules' weight cache (kind ``cache_kind``), the scratch of the workspace pools that
    these programs use, and what the programs hold themselves (zeroed state, constants, input / output slots)."""
    bufs = _Buffers()
    for mod in (pipe.unet, pipe.vae):
        if isinstance(mod, AutoencoderTinyHIP):   # its weights as mg_tiny_vae lays them out, packed on the host; no pool of its own
            for t in mod.host_pack()[1]:
                bufs.add(t, cache_kind)
            continue
        for v in mod.ws.cache.values():
            for t in _tensors(v):
                bufs.add(t, cache_kind)
        for t in mod.pool.all:
            bufs.add(t, KIND_SCRATCH)
    for _, seq, io in progs:
        for t in io.values():
            if isinstance(t, _Region):
                bufs.add(t, KIND_SCRATCH)
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
    return bufs


def _relocate(progs, bufs, index=None):
    """The programs' op arrays with every device pointer taken out and recorded as (op, slot, buffer, byte offset); ``index``: the
    buffer numbers to write (the image's table), by position in ``bufs`` (None: the position itself)."""
    sz_op = ctypes.sizeof(L.MgOp)
    num = (lambda b: b) if index is None else (lambda b: index[b])
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
                    relocs.append((k, s, num(hit[0]), hit[1]))
                    c.p[s] = None
            if c.kind == L.OP_IGEMM and O.igemm_tickets(c):
                hit = bufs.find(O.igemm_tickets(c))
                if hit is None:
                    raise RuntimeError(f"model image: the row-statistics tickets of op {k} of {name} are not in a known buffer")
                relocs.append((k, SLOT_LN_COUNTERS, num(hit[0]), hit[1]))
                O.set_igemm_tickets(c, None)
            raw += bytes(c)
        slots = []
        for nm, t in io.items():
            hit = bufs.find(t.data_ptr())
            slots.append((nm, num(hit[0]), hit[1], t.numel() * t.element_size()))
        ptab.append((name, len(seq.ops), slots))
        relocs_all.append(relocs)
        ops_all.append(bytes(raw))
    return ptab, relocs_all, ops_all


def _write_data(f, item):
    start, end, _k, t = item
    off = _pad(f)
    f.write(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() if t.numel() * t.element_size() == end - start
            else bytes((ctypes.c_char * (end - start)).from_address(start)))
    return off


def _write_blobs(f, ops_all, relocs_all):
    ops_off, rel_off = [], []
    for raw, relocs in zip(ops_all, relocs_all):
        ops_off.append(_pad(f))
        f.write(raw)
        rel_off.append(_pad(f))
        for (k, s, b, o) in relocs:
            f.write(struct.pack(REL, k, s, b, 0, o))
    return ops_off, rel_off


def _write_programs(f, ptab, ops_off, rel_off, relocs_all):
    for (name, n_ops, slots), oo, ro, relocs in zip(ptab, ops_off, rel_off, relocs_all):
        assert len(slots) <= MAXSLOT, "model image: too many program slots"
        f.write(struct.pack(PROG, name.encode(), n_ops, len(relocs), oo, ro, len(slots)))
        f.write(b"\0" * 4)
        for (nm, b, o, n) in slots:
            f.write(struct.pack(SLOT, nm.encode(), b, 0, o, n))
        f.write(b"\0" * ((MAXSLOT - len(slots)) * struct.calcsize(SLOT)))


def _describe(path, total, bufs, ptab, cfg):
    """What ``export_model_image`` returns for one configuration.  ``arena``: the device bytes the loader places (every buffer
    rounded up to 256): the weight cache, the configuration's own constants and zeroed state, its scratch."""
    items, c = bufs.items, dict(zip(L.CFG, cfg))
    nbytes = {k: sum(it[1] - it[0] for it in items if it[2] == k) for k in (KIND_SCRATCH, KIND_ZERO, KIND_DATA, KIND_SHARED)}
    arena = {k: sum(_r256(it[1] - it[0]) for it in items if it[2] in ks)
             for k, ks in (("shared", (KIND_SHARED,)), ("private", (KIND_ZERO, KIND_DATA)), ("scratch", (KIND_SCRATCH,)))}
    return dict(path=path, file_bytes=total, buffers=len(items), scratch_bytes=nbytes[KIND_SCRATCH], zero_bytes=nbytes[KIND_ZERO],
                data_bytes=nbytes[KIND_DATA] + nbytes[KIND_SHARED], ops={n: k for (n, k, _s) in ptab}, latent_hw=(c["latent_h"], c["latent_w"]),
                B=c["members"], steps=c["steps"], pred_channels=c["channels"], step_noises=c["step_noises"],
                images_per_program=c["pictures"] or 1, cfg16=list(cfg), arena=arena)


def export_model_image(pipe, path, *, configs=None, ensemble_size=None, height=None, width=None, denoising_steps=None, images_per_program=1,
                       tiny_vae=False):
    """Write the model image of ``pipe`` for images of ``height`` x ``width`` (the size fed to the VAE: after the pipeline's
    ``processing_res`` resize), ``ensemble_size`` members per picture and ``denoising_steps`` scheduler steps.  Works with the
    modules on the GPU (``pipe.to("cuda")``) or, without one, in the host-only mode.  Returns a dict describing the image.

    ``images_per_program`` = K > 1: the image runs K pictures per call (``mg_model_predict_many``) through the programs
    ``map_images(images_per_program=K)`` runs for a full group - one encode of K pictures, one denoising program of K x
    ``ensemble_size`` members, one decode; the header's word ``pictures`` (``_lib.CFG``) is K.  K = 1 writes the one-picture image, ``pictures`` = 0.

    ``configs`` = a list of dicts of the keywords above (instead of them): ONE image for several configurations - a version-2 file
    with a configuration table and one buffer table, the modules' packed weights stored once (kind ``KIND_SHARED``) and each
    configuration's own constants, zeroed state and scratch tagged with its index.  ``mg_model_select`` picks the configuration a
    loaded image runs.  The dict returned then holds ``configs`` (one dict as above per entry), ``shared_bytes`` and
    ``scratch_bytes`` (the scratch region: the largest configuration's, not the sum).

    ``tiny_vae=True``: the pipeline's VAE is an ``AutoencoderTinyHIP`` (``pipe.set_vae(load_tiny_vae(...))``) and the image runs it:
    ``mg_tiny_vae_encode`` / ``mg_tiny_vae_decode`` where an AutoencoderKL image runs its encode and decode programs, all members of a
    call in one decode.  Such an image is a NEW FILE VERSION (3, for one configuration or several, in the layout of version 2 with the
    members of ``struct mg_tiny_vae`` as one more table; the word ``vae`` = ``VAE_TINY``, the latent size by the tiny encoder's ceiling
    rule): no library built before the version existed can read it, which is why it is written on request only.  Without the
    keyword a pipeline with a tiny VAE is refused as before, and an AutoencoderKL pipeline writes the version-1 / version-2 bytes it
    always wrote.  One image has one VAE; the dict returned for one configuration is that of a version-1 export plus ``shared_bytes``
    (``arena``: "shared" lies in the allocation replicas share, "private" + "scratch" are ``mg_model_device_bytes``)."""
    if tiny_vae and not isinstance(pipe.vae, AutoencoderTinyHIP):
        raise ValueError(f"export_model_image: tiny_vae=True takes a pipeline whose VAE is an AutoencoderTinyHIP; this pipeline's is a "
                         f"{type(pipe.vae).__name__}" + (" (an AutoencoderKLHIP is exported with tiny_vae=False, the default)"
                                                         if isinstance(pipe.vae, AutoencoderKLHIP) else ""))
    if not tiny_vae and not isinstance(pipe.vae, AutoencoderKLHIP):
        raise ValueError(f"export_model_image: model images carry an AutoencoderKL as op programs; this pipeline's VAE is a "
                         f"{type(pipe.vae).__name__} (set_vae the checkpoint's AutoencoderKL back to export" +
                         (", or pass tiny_vae=True for a version-3 image that runs the tiny autoencoder)"
                          if isinstance(pipe.vae, AutoencoderTinyHIP) else ")"))
    if configs is not None:
        if any(v is not None for v in (ensemble_size, height, width, denoising_steps)) or images_per_program != 1:
            raise ValueError("export_model_image: pass either configs=[...] or the keywords of one configuration, not both")
        return _export_configs(pipe, path, list(configs), tiny_vae)
    if ensemble_size is None or height is None or width is None:
        raise TypeError("export_model_image: ensemble_size, height and width are required (or configs=[...])")
    if tiny_vae:   # one configuration in the layout of several: the description of that one
        whole = _export_configs(pipe, path, [dict(ensemble_size=ensemble_size, height=height, width=width, denoising_steps=denoising_steps,
                                                  images_per_program=images_per_program)], True)
        return dict(whole["configs"][0], buffers=whole["buffers"], shared_bytes=whole["shared_bytes"])
    progs, cfg = _build(pipe, ensemble_size, height, width, denoising_steps, images_per_program)
    bufs = _plan(pipe, progs)
    with open(path, "wb") as f:
        ptab, relocs_all, ops_all = _relocate(progs, bufs)
        # ---- layout: header, buffer table, program table, then 64-byte aligned blobs
        n_buf, n_prog = len(bufs.items), len(progs)
        prog_sz = struct.calcsize(PROG) + 4 + MAXSLOT * struct.calcsize(SLOT)
        table_end = struct.calcsize(HDR) + n_buf * struct.calcsize(BUF) + n_prog * prog_sz
        f.write(b"\0" * table_end)
        buf_off = [_write_data(f, it) if it[2] == KIND_DATA else 0 for it in bufs.items]
        ops_off, rel_off = _write_blobs(f, ops_all, relocs_all)
        total = f.tell()
        f.seek(0)
        f.write(struct.pack(HDR, MAGIC, VERSION, L.ABI_VERSION, n_buf, n_prog, *cfg))
        for (start, end, k, _t), off in zip(bufs.items, buf_off):
            f.write(struct.pack(BUF, end - start, off, k, 0))
        _write_programs(f, ptab, ops_off, rel_off, relocs_all)
        assert f.tell() == table_end
    # (the same plan with the weight cache told apart from the constants: what a version-2 image would share)
    return _describe(path, total, _plan(pipe, progs, KIND_SHARED), ptab, cfg)


def _export_configs(pipe, path, configs, tiny=False):
    if not configs:
        raise ValueError("export_model_image: configs is empty")
    seen, built = set(), []
    for n, c in enumerate(configs):
        c = dict(c)
        p = c.pop("pipe", pipe)   # (an entry may name its own pipeline object over the same modules)
        unknown = sorted(set(c) - set(_CFG_KEYS))
        if unknown or not all(k in c for k in _CFG_KEYS[:3]):
            raise ValueError(f"export_model_image: configuration {n} takes the keywords {', '.join(_CFG_KEYS)} (the first three are required); "
                             f"got {sorted(c)}")
        if p._kind != pipe._kind:
            raise ValueError(f"export_model_image: the configurations of one image are of one pipeline kind: configuration {n} is "
                             f"'{p._kind}', the image '{pipe._kind}'")
        if p.unet is not pipe.unet or p.vae is not pipe.vae:
            raise ValueError(f"export_model_image: configuration {n} belongs to other modules: one image shares one set of weights")
        key = (int(c["ensemble_size"]), int(c["height"]), int(c["width"]), int(c.get("denoising_steps") or p.default_denoising_steps),
               int(c.get("images_per_program", 1)))
        if key in seen:
            raise ValueError(f"export_model_image: configuration {n} (ensemble_size, height, width, denoising_steps, images_per_program = {key}) "
                             "is listed twice")
        seen.add(key)
        built.append(_build(p, **c))
    # every configuration is built: the weight cache now holds what all of them need
    plans = [_plan(pipe, progs, KIND_SHARED) for progs, _cfg in built]
    shared = {}   # (start, end) -> number in the image's buffer table; the shared buffers come first
    for bufs in plans:
        for it in bufs.items:
            if it[2] == KIND_SHARED:
                shared.setdefault((it[0], it[1]), (len(shared), it))
    table = [(it[1] - it[0], KIND_SHARED, 0, it) for _n, it in sorted(shared.values(), key=lambda v: v[0])]
    per_cfg, scratch_region = [], 0
    for ci, (bufs, (progs, cfg)) in enumerate(zip(plans, built)):
        index, scratch = [], 0
        for it in bufs.items:
            if it[2] == KIND_SHARED:
                index.append(shared[it[0], it[1]][0])
                continue
            index.append(len(table))
            table.append((it[1] - it[0], it[2], ci, scratch if it[2] == KIND_SCRATCH else it))
            if it[2] == KIND_SCRATCH:   # its place in the scratch region every configuration overlays
                scratch += _r256(it[1] - it[0])
        scratch_region = max(scratch_region, scratch)
        per_cfg.append(_relocate(progs, bufs, index))
    members = b""
    if tiny:   # the members of struct mg_tiny_vae in the struct's order, each (shared buffer, byte offset); a NULL member: absent
        net = pipe.vae.host_pack()[0]
        for ptr in (ctypes.c_uint64 * (ctypes.sizeof(net) // 8)).from_buffer_copy(bytes(net)):
            hit = plans[0].find(ptr) if ptr else None
            assert hit is not None or not ptr, "model image: a member of the tiny VAE lies outside its packed tensors"
            it = plans[0].items[hit[0]] if ptr else None
            members += struct.pack(TINY_MEMBER, shared[it[0], it[1]][0], 0, hit[1]) if ptr else struct.pack(TINY_MEMBER, TINY_ABSENT, 0, 0)
    prog_sz = struct.calcsize(PROG) + 4 + MAXSLOT * struct.calcsize(SLOT)
    with open(path, "wb") as f:
        # ---- layout: header, version-2 words, configuration table (16 words + three programs each), buffer table, blobs
        # (version 3: the table of the tiny VAE's members behind the buffer table)
        table_end = struct.calcsize(HDR) + struct.calcsize(V2) + len(built) * (64 + 3 * prog_sz) + len(table) * struct.calcsize(BUF) + len(members)
        f.write(b"\0" * table_end)
        rows = []
        for (nbytes, kind, ci, what) in table:
            rows.append((nbytes, what if kind == KIND_SCRATCH else _write_data(f, what) if kind in (KIND_DATA, KIND_SHARED) else 0, kind, ci))
        offs = [_write_blobs(f, ops_all, relocs_all) for (_ptab, relocs_all, ops_all) in per_cfg]
        total = f.tell()
        f.seek(0)
        f.write(struct.pack(HDR, MAGIC, VERSION_TINY if tiny else VERSION_CONFIGS, L.ABI_VERSION, len(table), 3 * len(built), *built[0][1]))
        f.write(struct.pack(V2, len(built), 0, scratch_region))
        for (_progs, cfg), (ptab, relocs_all, _ops), (ops_off, rel_off) in zip(built, per_cfg, offs):
            f.write(struct.pack("<16I", *cfg))
            _write_programs(f, ptab, ops_off, rel_off, relocs_all)
        for row in rows:
            f.write(struct.pack(BUF, *row))
        f.write(members)
        assert f.tell() == table_end
    described = [_describe(path, total, bufs, ptab, cfg) for bufs, (_p, cfg), (ptab, _r, _o) in zip(plans, built, per_cfg)]
    return dict(path=path, file_bytes=total, buffers=len(table), configs=described,
                shared_bytes=sum(_r256(n) for (n, k, _c, _w) in table if k == KIND_SHARED), scratch_bytes=scratch_region,
                private_bytes=sum(d["arena"]["private"] for d in described) + scratch_region)


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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _u64(seed):
    return int(seed) & ((1 << 64) - 1)


class ModelImage:
    """ctypes handle on a loaded model image - what a non-Python host does, spelled in Python for the tests and as a second,
    graph-free way to run a fixed-shape deployment: ``encode`` / ``denoise`` / ``decode`` take and return torch CUDA tensors
    but only their raw pointers cross into the library."""

    def __init__(self, path, device=0, *, _handle=None):
        lib = L.load()
        self._lib = lib
        self.handle = _handle if _handle is not None else lib.mg_model_load(path.encode(), int(device))
        if not self.handle:
            L.check(1, "mg_model_load")
        self.path, self.device = path, device
        self.configs = []   # the 16 cfg words of every configuration the image holds (a version-1 image: one)
        cfg = (ctypes.c_int * L.CFG_WORDS)()
        for i in range(lib.mg_model_num_configs(self.handle)):
            L.check(lib.mg_model_config_info(self.handle, i, cfg), "mg_model_config_info")
            self.configs.append(list(cfg))
        self._selected()

    def config(self, index):
        """Configuration ``index`` by name: {name of ``_lib.CFG``: word}, as the image has them (``pictures``: 0 = one per call)."""
        return dict(zip(L.CFG, self.configs[int(index)]))

    def _selected(self):
        """The attributes of the selected configuration (``mg_model_info``)."""
        cfg = (ctypes.c_int * L.CFG_WORDS)()
        L.check(self._lib.mg_model_info(self.handle, cfg), "mg_model_info")
        c = dict(zip(L.CFG, cfg))
        self.B, self.H, self.W, self.h, self.w, self.steps = (c[k] for k in ("members", "height", "width", "latent_h", "latent_w", "steps"))
        self.pred_channels, self.post, self.n_noise, self.Hout, self.Wout = (c[k] for k in ("channels", "post", "step_noises", "out_h", "out_w"))
        self.K = c["pictures"] or 1   # pictures per call; B: the members of each

    def find(self, height=-1, width=-1, ensemble_size=-1, denoising_steps=-1, images_per_program=-1):
        """``mg_model_find_config``: the index of the first configuration that matches (-1 = any value); raises if none does."""
        i = self._lib.mg_model_find_config(self.handle, int(height), int(width), int(ensemble_size), int(denoising_steps), int(images_per_program))
        if i < 0:
            L.check(1, "mg_model_find_config", self._lib)
        return i

    def select(self, index):
        """``mg_model_select``: every call below acts on configuration ``index`` from now on.  Returns ``self``."""
        L.check(self._lib.mg_model_select(self.handle, int(index)), "mg_model_select", self._lib)
        self.selected = int(index)
        self._selected()
        return self

    selected = 0

    def replica(self):
        """``mg_model_replica``: a second handle over the same device-resident weights, with its own arena, programs and
        temporaries - to be driven from another thread on another stream."""
        h = self._lib.mg_model_replica(self.handle)
        if not h:
            L.check(1, "mg_model_replica", self._lib)
        r = ModelImage(self.path, self.device, _handle=h)
        r.selected = self.selected
        return r

    @property
    def shared_bytes(self):
        return self._lib.mg_model_shared_bytes(self.handle)

    @property
    def device_bytes(self):
        return self._lib.mg_model_device_bytes(self.handle)

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

    # ---- what the one-call predictions share: their checks of the pictures, their output options, their output tensors
    @staticmethod
    def _pictures(who, u8s, reciprocal, size):
        """The uint8 CUDA pictures of a call, one [Hin, Win, 3] or a list of one size, checked in ``who``'s name -> (contiguous, Hin, Win,
        reciprocal: by default the reciprocal normalisation when the input is resampled - its size is not ``size``; None: never)."""
        many = isinstance(u8s, list)
        for u8 in u8s if many else [u8s]:
            assert u8.is_cuda and u8.dtype == torch.uint8 and u8.dim() == 3 and u8.shape[-1] == 3, \
                f"{who}: uint8 CUDA [H, W, 3] pictures" if many else f"{who}: a uint8 CUDA [H, W, 3] picture"
            assert not many or u8.shape == u8s[0].shape, f"{who}: the pictures of one call have one size"
        Hin, Win = (u8s[0] if many else u8s).shape[:2]
        if reciprocal is None:
            reciprocal = size is not None and (Hin, Win) != tuple(size)
        return ([u8.contiguous() for u8 in u8s] if many else u8s.contiguous()), Hin, Win, int(bool(reciprocal))

    @staticmethod
    def _out_opts(who, out_size, out_mode, lut):
        """``_lib.MgOutputOpts`` of (out_size | None, out_mode, lut | None) -> (the struct, the table it points to: keep it until the call)."""
        if lut is not None:
            assert lut.is_cuda and lut.dtype == torch.uint8 and lut.numel() == 768, f"{who}: the colour table is uint8 CUDA [256, 3]"
            lut = lut.contiguous()
        oh, ow = (0, 0) if out_size is None else (int(out_size[0]), int(out_size[1]))
        return L.MgOutputOpts(oh, ow, int(O.RESIZE_MODES.get(out_mode, out_mode)), _ptr(lut)), lut

    @staticmethod
    def _outputs(dev, lead, C, out_hw, unc_shape, u16=False, picture=False):
        """The tensors a call writes, each behind the leading shape ``lead`` -> (pred fp32 [C, oh, ow], unc fp32 ``unc_shape`` | None for
        None, u16 uint16 [oh, ow] | None, picture uint8 [oh, ow, 3] | None)."""
        new = lambda dtype, *shape: torch.empty(*lead, *shape, device=dev, dtype=dtype)   # noqa: E731
        return (new(torch.float32, C, *out_hw), None if unc_shape is None else new(torch.float32, *unc_shape),
                new(torch.uint16, *out_hw) if u16 else None, new(torch.uint8, *out_hw, 3) if picture else None)

    def predict_iid(self, u8, seed, *, opts=None, pictures=False, mode=0, reciprocal=None):
        """``mg_model_predict_iid`` on the uint8 CUDA picture ``u8`` [Hin, Win, 3]: -> (pred fp32 [3 n, out_h, out_w], unc fp32
        [3 n, Hout, Wout] | None for a single member, pictures uint8 [n, out_h, out_w, 3] | None unless ``pictures``).  ``opts``: an
        ``_lib.MgIidOpts`` (None = the defaults); ``mode`` / ``reciprocal``: the input resampling as in ``mg_rgb_prepare`` (by default
        the reciprocal normalisation when the picture is resampled, as the pipelines' input stage)."""
        u8, Hin, Win, reciprocal = self._pictures("predict_iid", u8, reciprocal, (self.H, self.W))
        oh, ow = ((opts.out_h or self.Hout), (opts.out_w or self.Wout)) if opts is not None else (self.Hout, self.Wout)
        C = self.pred_channels
        pred, unc, _, _ = self._outputs(u8.device, (), C, (oh, ow), (C, self.Hout, self.Wout) if self.B > 1 else None)
        pics = torch.empty(C // 3, oh, ow, 3, device=u8.device, dtype=torch.uint8) if pictures else None
        L.check(self._lib.mg_model_predict_iid(self.handle, u8.data_ptr(), 1, Hin, Win, int(mode), reciprocal, _u64(seed),
                                               None if opts is None else ctypes.byref(opts), pred.data_ptr(), _ptr(unc), _ptr(pics),
                                               O.current_stream_handle()), "mg_model_predict_iid", self._lib)
        return pred, unc, pics

    def predict_next(self, u8, seed, strength=0.1, **kw):
        """``mg_model_predict_next``: ``predict_out`` (its arguments, its results) for the next frame of a sequence - the frame starts
        from ``(1 - strength) noise + strength latent``, the denoised latent of the frame this handle predicted before; the first
        frame after the load, ``replica()``, ``select()`` or ``seq_reset()`` carries nothing and is ``predict_out`` bit for bit."""
        return self.predict_out(u8, seed, _next=float(strength), **kw)

    def seq_reset(self):
        """``mg_model_seq_reset``: forget the carried latent; the next ``predict_next`` starts a new sequence."""
        L.check(self._lib.mg_model_seq_reset(self.handle), "mg_model_seq_reset", self._lib)

    def predict_out(self, u8, seed, *, out_size=None, out_mode=0, lut=None, u16=False, picture=False, opts=None, mode=0, reciprocal=None,
                    _next=None):
        """``mg_model_predict_out`` on the uint8 CUDA picture ``u8`` [Hin, Win, 3]: the pipelines' output with ``match_input_res`` ->
        (pred fp32 [C, out_h, out_w] clipped, unc fp32 [Hout, Wout] | None for a single member, u16 uint16 [out_h, out_w] | None unless
        ``u16``, picture uint8 [out_h, out_w, 3] | None unless ``picture``, info = the four numbers of ``mg_ensemble_depth``).
        ``out_size``: (out_h, out_w), None = the model's output size; ``out_mode``: a key of ``ops.RESIZE_MODES`` or its number;
        ``lut``: the colour table, uint8 CUDA [256, 3] (a depth model's picture needs it); ``opts``: an ``_lib.MgPredictOpts``;
        ``mode`` / ``reciprocal``: the input resampling as in ``predict_iid``."""
        u8, Hin, Win, reciprocal = self._pictures("predict_out", u8, reciprocal, (self.H, self.W))
        out_opts, lut = self._out_opts("predict_out", out_size, out_mode, lut)
        out_hw = (self.Hout, self.Wout) if out_size is None else (out_opts.out_h, out_opts.out_w)
        pred, unc, d16, pic = self._outputs(u8.device, (), self.pred_channels, out_hw, (self.Hout, self.Wout) if self.B > 1 else None, u16, picture)
        info = (ctypes.c_double * 4)()
        # (_next: the strength - the call is mg_model_predict_next, the same arguments and the strength behind them)
        name = "mg_model_predict_out" if _next is None else "mg_model_predict_next"
        L.check(getattr(self._lib, name)(self.handle, u8.data_ptr(), 1, Hin, Win, int(O.RESIZE_MODES.get(mode, mode)), reciprocal, _u64(seed),
                                         None if opts is None else ctypes.byref(opts), ctypes.byref(out_opts), pred.data_ptr(), _ptr(unc),
                                         _ptr(d16), _ptr(pic), info, O.current_stream_handle(), *(() if _next is None else (_next,))),
                name, self._lib)
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
        u8s, Hin, Win, reciprocal = self._pictures("predict_many", u8s, reciprocal, (self.H, self.W))
        out_opts, lut = self._out_opts("predict_many", out_size, out_mode, lut)
        out_hw = (self.Hout, self.Wout) if out_size is None else (out_opts.out_h, out_opts.out_w)
        pred, unc, d16, pic = self._outputs(u8s[0].device, (n,), self.pred_channels, out_hw, (self.Hout, self.Wout) if self.B > 1 else None,
                                            u16, picture)
        info = (ctypes.c_double * (4 * n))()
        L.check(self._lib.mg_model_predict_many(self.handle, n, (ctypes.c_void_p * n)(*[u8.data_ptr() for u8 in u8s]), 1, Hin, Win,
                                                int(O.RESIZE_MODES.get(mode, mode)), reciprocal, (ctypes.c_uint64 * n)(*[_u64(s) for s in seeds]),
                                                None if opts is None else ctypes.byref(opts), ctypes.byref(out_opts),
                                                pred.data_ptr(), _ptr(unc), _ptr(d16), _ptr(pic), info, O.current_stream_handle()),
                "mg_model_predict_many", self._lib)
        return pred, unc, d16, pic, [list(info[4 * i:4 * i + 4]) for i in range(n)]

    def predict_tiled(self, u8, seed, guide_config, tile_config, overlap, *, out_size=None, out_mode=0, lut=None, u16=False, picture=False,
                      opts=None, mode=0, reciprocal=None, uncertainty=True, flags=True, tail_config=None):
        """``mg_model_predict_tiled`` on the LARGE uint8 CUDA picture ``u8`` [Hin, Win, 3] (both multiples of 8): ``pipe.predict_tiled``
        with ``match_input_res`` -> (pred fp32 [C, out_h, out_w] clipped, unc fp32 [Hin, Win] | None for a single member or unless
        ``uncertainty``, u16 uint16 [out_h, out_w] | None unless ``u16``, picture uint8 [out_h, out_w, 3] | None unless ``picture``,
        info = the guide's four numbers of ``mg_ensemble_depth``, flags int32 CUDA [n tiles] | None for normals or unless ``flags``:
        ``mg_tile_fit``'s flag per tile - ``int(flags.sum())`` is ``degenerate_tiles``).  ``guide_config`` / ``tile_config``: indices of
        ``find`` (the guide's is ignored for normals); ``tail_config``: None, or the configuration of n mod K tiles per call that runs the
        short last group as ``map_images`` does (without it the group is padded: the same up to the arithmetic of the batch); ``overlap``: an int or (y, x); ``out_size``: None = the picture's size;
        ``mode`` / ``reciprocal``: the resampling of the GUIDE's input as in ``predict_out`` (by default the reciprocal normalisation
        when the guide is resampled).  The handle stays on the configuration it was on."""
        tile_config, guide_config = int(tile_config), int(guide_config)
        if not 0 <= tile_config < len(self.configs):
            raise ValueError(f"predict_tiled: tile configuration {tile_config} of {len(self.configs)}")
        tc = self.config(tile_config)
        B, C, depth = tc["members"], tc["channels"], tc["channels"] == 1
        gc = self.config(guide_config) if depth and 0 <= guide_config < len(self.configs) else None
        u8, Hin, Win, reciprocal = self._pictures("predict_tiled", u8, reciprocal, None if gc is None else (gc["height"], gc["width"]))
        oy, ox = (int(overlap[0]), int(overlap[1])) if isinstance(overlap, (tuple, list)) else (int(overlap), int(overlap))
        out_opts, lut = self._out_opts("predict_tiled", out_size, out_mode, lut)
        tiled = L.MgTiledOpts(guide_config, tile_config, oy, ox, -1 if tail_config is None else int(tail_config))
        # (a size the call refuses is refused by the call: the tensors it would have written are empty)
        out_hw = (Hin, Win) if out_size is None else (max(out_opts.out_h, 0), max(out_opts.out_w, 0))
        pred, unc, d16, pic = self._outputs(u8.device, (), C, out_hw, (Hin, Win) if B > 1 and uncertainty else None, u16, picture)
        flg = torch.zeros(L.TILE_MAX_PER_AXIS ** 2, device=u8.device, dtype=torch.int32) if depth and flags else None
        info = (ctypes.c_double * 4)()
        L.check(self._lib.mg_model_predict_tiled(self.handle, u8.data_ptr(), 1, Hin, Win, int(O.RESIZE_MODES.get(mode, mode)), reciprocal,
                                                 _u64(seed), ctypes.byref(tiled), None if opts is None else ctypes.byref(opts),
                                                 ctypes.byref(out_opts), pred.data_ptr(), _ptr(unc), _ptr(d16), _ptr(pic), info, _ptr(flg),
                                                 O.current_stream_handle()), "mg_model_predict_tiled", self._lib)
        if flg is not None:   # the plan the call made: its number of tiles
            from . import tiles as tiling
            flg = flg[:len(tiling.plan((Hin, Win), (tc["height"], tc["width"]), (oy, ox)).origins)]
        return pred, unc, d16, pic, list(info), flg

    def close(self):
        if self.handle:
            self._lib.mg_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
