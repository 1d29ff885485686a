"""Canonical text and digest of the programs the engine builds, without a GPU.  A plain helper module for
tests/test_program_digest_host.py (not collected), with a ``__main__`` that writes the fixture or dumps the full text.

Every configuration of ``CONFIGS`` is built in ``dry()`` mode from an all-zero state dict, each from a fresh buffer pool (a pool
that served an earlier program would hand out its buffers in another order).  One line per op:

    label|kind|i=<40 integers>|f=<8 floats as their bits>|p=<16 pointers>|l=<4 integers>

A pointer is written as the buffer it points into - the module's pooled buffers, the program's held tensors and the weight
store's - numbered by order of first appearance in that program, plus its byte offset; ``-`` is null.  The one integer field
that carries an address, the ticket pair of MG_OP_IGEMM (``tickets_lo`` / ``tickets_hi``; no other integer name of ``L.FIELDS``
holds one), is written the same way.  So the text states every launch, every field and the buffer aliasing of a program, and is
the same in every process.

    python -m tests.program_digest --write            regenerate tests/golden/program_digest.json (records git's HEAD)
    python -m tests.program_digest --dump DIR         one text file per configuration, to ``diff -r`` two trees
"""
import bisect
import dataclasses
import hashlib
import json
import os
import struct
import sys
from collections import Counter

import torch

from marigold_amd import _lib as L, ops as O
from marigold_amd.arch import TINY_UNET, TINY_VAE, UNetConfig, VAEConfig, unet_param_shapes, vae_param_shapes
from marigold_amd.modules import AutoencoderKLHIP, UNet2DConditionModelHIP
from marigold_amd.schedulers import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "program_digest.json")
SIZES = (1, 2, 3, 5, 6, 8, 10)
IID_UNET = UNetConfig(in_channels=12, out_channels=8)
TINY_IID_UNET = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8)


def _switches():
    """The module that holds the engine's switches (FOLD_SHORTCUT)."""
    from marigold_amd import routes
    return routes


def _configs():
    """[(name, model key, dtype, fold, build(module) -> OpSeq)] in a fixed order."""
    def unet(B, h, w, steps=1, **kw):
        return lambda m: m.denoise_program(B, h, w, DDIMScheduler(), steps, **kw).seq

    def vae(kind, B, h, w, post=0):
        return lambda m: m._program(kind, B, h, w, post)[0]

    bf, hf = torch.bfloat16, torch.float16
    c = []
    c += [(f"unet/96x96/E={n}", "unet", bf, True, unet(n, 96, 96)) for n in SIZES]
    c += [(f"unet/76x100/E={n}", "unet", bf, True, unet(n, 76, 100)) for n in (1, 10)]
    c += [("unet/96x96/B=4,rgb_members=2", "unet", bf, True, unet(4, 96, 96, rgb_members=2))]
    c += [("unet12/96x96/E=2", "unet12", bf, True, unet(2, 96, 96))]
    c += [("vae.encode/768x768", "vae", bf, True, vae("encode", 1, 768, 768)),
          ("vae.encode/608x800", "vae", bf, True, vae("encode", 1, 608, 800))]
    c += [(f"vae.decode/96x96/E={n}", "vae", bf, True, vae("decode", n, 96, 96, L.POST_DEPTH)) for n in SIZES]
    c += [(f"vae.decode/76x100/E={n}", "vae", bf, True, vae("decode", n, 76, 100, L.POST_DEPTH)) for n in (1, 10)]
    c += [(f"fp16/unet/96x96/E={n}", "unet", hf, True, unet(n, 96, 96)) for n in (1, 10)]
    c += [(f"fp16/vae.decode/96x96/E={n}", "vae", hf, True, vae("decode", n, 96, 96, L.POST_DEPTH)) for n in (1, 10)]
    # the tiny architecture as the GPU tests run it (test_gpu_pipeline.py, test_gpu_fp16.py, test_gpu_images_per_program.py)
    c += [(f"tiny/unet/8x16/B={n},T=2", "tiny_unet", bf, True, unet(n, 8, 16, 2)) for n in (1, 2, 3)]
    c += [("tiny/unet/8x16/B=4,rgb_members=2", "tiny_unet", bf, True, unet(4, 8, 16, 2, rgb_members=2)),
          ("tiny/unet12/8x16/B=2,T=2", "tiny_unet12", bf, True, unet(2, 8, 16, 2)),
          ("tiny/vae.encode/64x128", "tiny_vae", bf, True, vae("encode", 1, 64, 128)),
          ("tiny/vae.decode/8x16/B=1", "tiny_vae", bf, True, vae("decode", 1, 8, 16, L.POST_DEPTH)),
          ("tiny/vae.decode/8x16/B=3,normals", "tiny_vae", bf, True, vae("decode", 3, 8, 16, L.POST_NORMALS)),
          ("fp16/tiny/unet/8x16/B=2,T=2", "tiny_unet", hf, True, unet(2, 8, 16, 2)),
          ("fp16/tiny/vae.decode/8x16/B=1", "tiny_vae", hf, True, vae("decode", 1, 8, 16, L.POST_NONE))]
    c += [("unfolded/unet/96x96/E=10", "unet", bf, False, unet(10, 96, 96)),
          ("unfolded/vae.decode/96x96/E=10", "vae", bf, False, vae("decode", 10, 96, 96, L.POST_DEPTH))]
    return c


CONFIGS = [name for name, *_ in _configs()]
_MODELS = dict(unet=(UNet2DConditionModelHIP, UNetConfig()), unet12=(UNet2DConditionModelHIP, IID_UNET),
               vae=(AutoencoderKLHIP, VAEConfig()), tiny_unet=(UNet2DConditionModelHIP, TINY_UNET),
               tiny_unet12=(UNet2DConditionModelHIP, TINY_IID_UNET), tiny_vae=(AutoencoderKLHIP, TINY_VAE))
_modules = {}


def _module(key, dtype):
    """The dry module of a model (its packed weights are kept between configurations) with a fresh pool and no programs."""
    if (key, dtype) not in _modules:
        cls, cfg = _MODELS[key]
        shapes = unet_param_shapes(cfg) if cls is UNet2DConditionModelHIP else vae_param_shapes(cfg)
        m = cls({k: torch.zeros(s) for k, s in shapes.items()}, cfg, compute_dtype=dtype).dry()
        if cls is UNet2DConditionModelHIP:
            m.set_context(torch.zeros(1, 2, cfg.cross_attention_dim))
        _modules[(key, dtype)] = m
    m = _modules[(key, dtype)]
    m.pool, m._programs = type(m.pool)(m.device), {}
    return m


def _tensors(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from _tensors(y)


def canonical(seq, module):
    """The program as text, one line per op (see the module's docstring)."""
    spans = {}
    for t in [*module.pool.all, *_tensors(seq.keep), *_tensors(list(module.ws.cache.values()))]:
        s = t.untyped_storage()
        if s.nbytes():
            spans[s.data_ptr()] = max(spans.get(s.data_ptr(), 0), s.nbytes())
    bases = sorted(spans)
    names = {}

    def ptr(p):
        if not p:
            return "-"
        k = bisect.bisect_right(bases, p) - 1
        base = bases[k] if k >= 0 and p < bases[k] + spans[bases[k]] else p   # (a pointer into no known buffer: its own name)
        name = names.setdefault(base, f"b{len(names)}")
        return name if p == base else f"{name}+{p - base}"

    lines = []
    for op, label in zip(seq.ops, seq.labels):
        ints = [str(v) for v in op.i]
        if op.kind == L.OP_IGEMM:
            names_i = L.FIELDS[L.OP_IGEMM][1]["i"]
            ints[names_i.index("tickets_lo")] = ptr(O.igemm_tickets(op))
            ints[names_i.index("tickets_hi")] = "^"
        floats = [struct.pack("<f", v).hex() for v in op.f]
        lines.append(f"{label}|{L.OP_NAMES.get(op.kind, op.kind)}|i={','.join(ints)}|f={','.join(floats)}|"
                     f"p={','.join(ptr(p) for p in op.p)}|l={','.join(str(v) for v in op.l)}")
    return "\n".join(lines) + "\n"


def texts(only=None):
    """Yield (configuration, canonical text, [op kind names]) for every configuration (or those named in ``only``)."""
    sw = _switches()
    fold0 = sw.FOLD_SHORTCUT
    try:
        for name, key, dtype, fold, build in _configs():
            if only is not None and name not in only:
                continue
            sw.FOLD_SHORTCUT = fold
            m = _module(key, dtype)
            seq = build(m)
            yield name, canonical(seq, m), [L.OP_NAMES.get(op.kind, str(op.kind)) for op in seq.ops]
    finally:
        sw.FOLD_SHORTCUT = fold0


BLOCK = 16   # ops per checkpoint of the running hash: what lets a mismatch be narrowed down without the other tree's text


def entry(text, kinds):
    """What the fixture holds of a program: the SHA-256 of its text, the op count, the count per kind and, to find where two
    programs part, four hex digits of the running hash after every ``BLOCK`` lines."""
    h, marks = hashlib.sha256(), []
    for k, line in enumerate(text.splitlines(keepends=True)):
        h.update(line.encode())
        if (k + 1) % BLOCK == 0:
            marks.append(h.hexdigest()[:4])
    assert h.hexdigest() == hashlib.sha256(text.encode()).hexdigest()
    return dict(sha256=h.hexdigest(), ops=len(kinds), kinds=dict(sorted(Counter(kinds).items())), marks="".join(marks))


def first_difference(text, want):
    """-> (index of the first op of the first ``BLOCK`` lines whose running hash leaves the fixture entry ``want``, those lines)."""
    got = entry(text, text.splitlines())["marks"]
    k = next((j for j in range(0, min(len(got), len(want["marks"])), 4) if got[j:j + 4] != want["marks"][j:j + 4]),
             min(len(got), len(want["marks"]))) // 4 * BLOCK
    return k, text.splitlines()[k:k + BLOCK]


def main(argv):
    if len(argv) == 2 and argv[0] == "--dump":
        os.makedirs(argv[1], exist_ok=True)
        for name, text, _ in texts():
            with open(os.path.join(argv[1], name.replace("/", "__") + ".txt"), "w") as f:
                f.write(text)
        return 0
    if argv == ["--write"]:
        import subprocess
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=os.path.dirname(FIXTURE), capture_output=True, text=True).stdout.strip()
        doc = dict(generated_at_commit=commit or "unknown", programs={name: entry(text, kinds) for name, text, kinds in texts()})
        with open(FIXTURE, "w") as f:
            rows = ",\n".join(f'  {json.dumps(k)}: {json.dumps(v, sort_keys=True, separators=(",", ":"))}' for k, v in sorted(doc["programs"].items()))
            f.write(f'{{\n "generated_at_commit": {json.dumps(doc["generated_at_commit"])},\n "programs": {{\n{rows}\n }}\n}}\n')   # (a program per line)
        print(f"{FIXTURE}: {len(doc['programs'])} programs, {sum(p['ops'] for p in doc['programs'].values())} ops")
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
