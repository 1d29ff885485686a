"""The configurations of the scratch-independence tests (tests/scratch_state.py) and the three production programs built at one of
them: shared by the GPU tests (tests/test_gpu_fullsize.py for the full architecture, tests/test_gpu_scratch_independence.py for
the tiny one) and the host test that dry-builds the same programs (tests/test_scratch_state_host.py).

A configuration is (E, h, w): E ensemble members at an h x w latent; the encoder runs on one 8h x 8w image whatever E is.
The full-architecture shapes are the benchmark's own: the row-resident GEMM's 8- and 12-wave forms and a few more launch forms
exist only for E >= 3 at 96 x 96 (routes.rowgemm_ok and the tuning table are keyed on these shapes), so no smaller shape stands
in for them - tests/test_scratch_state_host.py holds the union of launch forms against BASELINE's configurations.
"""
import time

import torch

from marigold_amd import _lib as L
from marigold_amd import engine as E_
from tests import scratch_state as SS

PROGRAMS = ("encode", "denoise", "decode")
# product recycling (a replica's own pool): the benchmark's sizes, the C1-style 72 x 96, an odd size (every tile ragged, ldvt padding
# live) and ten members at 48 x 48.  E = 2 and E = 5 at 96 x 96 are here because the launch forms demand them: the decoder's plain
# patch convolutions (no fused norm) occur only at E = 2, the 8-wave row-resident GEMMs and the 5-member patch / split-K forms only
# at E = 5 (ten forms in all that E = 1, 3, 10 do not reach)
FULL_RECYCLED = ((1, 96, 96), (3, 96, 96), (10, 96, 96), (2, 72, 96), (1, 33, 41), (10, 48, 48), (2, 96, 96), (5, 96, 96))
BENCHMARK_SHAPES = ((96, 96), (72, 96))   # the latent sizes of BASELINE's configurations
FULL_F16 = ((1, 96, 96), (1, 33, 41))
# no recycling (Pool.put a no-op): every buffer a first use.  Never E = 10: its decoder pool would be tens of GB and test nothing new.
FULL_FRESH = ((1, 96, 96), (1, 33, 41))
TINY_FRESH = ((3, 8, 16), (1, 5, 7))
BASELINE = ((1, 96, 96), (2, 96, 96), (3, 96, 96), (5, 96, 96), (10, 96, 96), (2, 72, 96))


def cases(configs):
    """[(program, E, h, w)]: every program of every configuration; the encoder (B = 1) once per image size."""
    out, seen = [], set()
    for (E, h, w) in configs:
        for prog in PROGRAMS:
            key = (prog, 1, h, w) if prog == "encode" else (prog, E, h, w)
            if key not in seen:
                seen.add(key)
                out.append(key)
    return out


def case_id(case):
    prog, E, h, w = case
    return f"{prog}-E{E}-{h}x{w}"


def own_pool(module, recycle=True):
    """The module again over the same weight store with a pool and programs of its own (what ``replica()`` makes on a GPU; a dry
    module has no replica()).  ``recycle=False``: ``Pool.put`` does nothing on this pool, so every buffer is a first use."""
    if module.device.type == "cuda":
        r = module.replica()
    else:
        r = object.__new__(type(module))
        r.__dict__.update(module.__dict__)
        r.pool = E_.Pool(module.device)
        r._programs = {}
    assert r.ws is module.ws and r.pool is not module.pool and not r.pool.all and not r._programs
    if not recycle:
        r.pool.put = lambda t: None
    return r


def build(unet, vae, case, recycle=True, seed=0):
    """-> (seq, the module whose pool the program draws from, scratch_state.IO) of one case, on the modules' device, in a fresh pool."""
    from marigold_amd.schedulers import DDIMScheduler
    prog, E, h, w = case
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    if prog == "denoise":
        m = own_pool(unet, recycle)
        p = m.denoise_program(E, h, w, DDIMScheduler(), n_steps=1)
        assert not p.noises
        io = SS.IO([(p.rgb_latent, rnd(1, 4, h, w).to(m.device)), (p.x, rnd(E, 4, h, w).to(m.device))], [p.x])
        return p.seq, m, io
    m = own_pool(vae, recycle)
    if prog == "encode":
        f = 2 ** (len(m.config.block_out_channels) - 1)
        seq, inp, out = m._program("encode", 1, f * h, f * w)
        assert tuple(out.shape[-2:]) == (h, w)
        value = torch.rand(1, 3, f * h, f * w, generator=g) * 2 - 1
    else:
        seq, inp, out = m._program("decode", E, h, w, L.POST_DEPTH)
        value = rnd(E, m.config.latent_channels, h, w)
    return seq, m, SS.IO([(inp, value.to(m.device))], [out])


def run_case(unet, vae, case, recycle=True):
    """Build one case on replicas of the given GPU modules and hold it to the three properties; prints the bytes and the wall time."""
    t0 = time.perf_counter()
    seq, m, io = build(unet, vae, case, recycle)
    t1 = time.perf_counter()
    rep = SS.check_program(seq, m, io)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"[scratch] {case_id(case)} {'recycled' if recycle else 'no recycling'} {'fp16' if seq.f16 else 'bf16'}: "
          f"pool.bytes {m.pool.bytes} ({m.pool.bytes / 2 ** 30:.2f} GiB), build {t1 - t0:.2f} s, five runs + checks {t2 - t1:.2f} s")
    return rep
