"""tests/scratch_state.py without a GPU: the pointer partition of the production programs at the configurations the GPU tests run
(dry builds on CPU buffers), the launch forms those configurations reach against BASELINE's, and the fill / localiser machinery on
CPU tensors with a runner that interprets MG_OP_COPY / MG_OP_MEMSET."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from marigold_amd import _lib as L, engine as E, ops as O
from tests import scratch_cases as SC, scratch_state as SS


def _zero_modules(ucfg, vcfg, dtype=torch.bfloat16):
    from marigold_amd.arch import unet_param_shapes, vae_param_shapes
    from marigold_amd.modules import AutoencoderKLHIP, UNet2DConditionModelHIP
    usd = {k: torch.zeros(s) for k, s in unet_param_shapes(ucfg).items()}
    vsd = {k: torch.zeros(s) for k, s in vae_param_shapes(vcfg).items()}
    unet = UNet2DConditionModelHIP(usd, ucfg, compute_dtype=dtype).dry()
    unet.set_context(torch.zeros(1, 2, ucfg.cross_attention_dim))
    return unet, AutoencoderKLHIP(vsd, vcfg, compute_dtype=dtype).dry()


@pytest.fixture(scope="module")
def full_dry():
    from marigold_amd.arch import UNetConfig, VAEConfig
    return {dt: _zero_modules(UNetConfig(), VAEConfig(), dt) for dt in (torch.bfloat16, torch.float16)}


@pytest.fixture(scope="module")
def full_forms(full_dry):
    """{case: its launch forms} of every full-architecture bf16 case of the GPU tests and of BASELINE; each build is classified on the way."""
    unet, vae = full_dry[torch.bfloat16]
    out = {}
    for case in SC.cases(tuple(SC.FULL_RECYCLED) + tuple(SC.BASELINE)):
        seq, m, io = SC.build(unet, vae, case)
        _partition(seq, m, io)
        out[case] = {SS.launch_form(op) for op in seq.ops}
    return out


def _partition(seq, m, io):
    cls = SS.classify(seq, m, io)
    assert len(cls.op_ptrs) == len(seq.ops) and all(ptrs for ptrs in cls.op_ptrs)
    named = {c for ptrs in cls.op_ptrs for _, c, _ in ptrs}
    assert named == {SS.SCRATCH, SS.ZERO, SS.CONST, SS.IO_SLOT}, (seq.name, named)
    assert seq.zero_state and {t.data_ptr() for t in cls.zero} == seq.zero_state
    assert sum(t.numel() for t in cls.scratch) == m.pool.bytes
    assert all(t.is_contiguous() for t in cls.cache + cls.mutable())   # poison / checksums take whole buffers as bytes
    assert len(cls.tables) == (3 if seq.name.startswith("denoise") else 0)   # time_embedding.linear_1 / linear_2 / the stacked projections
    return cls


def test_every_pointer_of_the_gpu_tests_programs_classifies(full_dry, full_forms):
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    assert set(SC.cases(SC.FULL_RECYCLED)) <= set(full_forms)   # (the bf16 recycled cases: classified by the fixture)
    n = 0
    for dt, configs, recycle in ((torch.float16, SC.FULL_F16, True), (torch.bfloat16, SC.FULL_FRESH, False)):
        for case in SC.cases(configs):
            seq, m, io = SC.build(*full_dry[dt], case, recycle)
            _partition(seq, m, io)
            assert seq.f16 == (dt == torch.float16)
            n += 1
    tiny = _zero_modules(TINY_UNET, TINY_VAE)
    for case in SC.cases(SC.TINY_FRESH):
        seq, m, io = SC.build(*tiny, case, recycle=False)
        cls = _partition(seq, m, io)
        assert not any(m.pool.free_lists.values()) and len(cls.scratch) == len(m.pool.all)   # nothing was ever handed back
        n += 1
    assert n == 6 + 6 + 6


def test_no_recycling_makes_every_buffer_a_first_use(full_dry):
    unet, vae = full_dry[torch.bfloat16]
    case = ("denoise", 1, 33, 41)
    a, b = SC.build(unet, vae, case)[1], SC.build(unet, vae, case, recycle=False)[1]
    assert b.pool.bytes > 2 * a.pool.bytes and not any(b.pool.free_lists.values()) and any(a.pool.free_lists.values())
    assert unet.pool.bytes == 0   # the fixture's own pool is never drawn from


def test_a_stray_pointer_names_its_op(full_dry):
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    unet, vae = _zero_modules(TINY_UNET, TINY_VAE)
    seq, m, io = SC.build(unet, vae, ("decode", 1, 5, 7))
    k = next(i for i, op in enumerate(seq.ops) if op.kind == L.OP_GN_APPLY)
    stray = torch.empty(64, dtype=torch.uint8)   # a buffer the program does not own
    good = O.Raw(seq.ops[k]).ss
    O.Raw(seq.ops[k]).ss = stray.data_ptr()
    with pytest.raises(SS.ContractError, match=f"op '{seq.labels[k]}'.*pointer ss .*resolves nowhere"):
        SS.classify(seq, m, io)
    O.Raw(seq.ops[k]).ss = good
    SS.classify(seq, m, io)
    m.ws.cache[("alias",)] = m.pool.all[0]   # a scratch buffer that is also a "weight": two classes
    with pytest.raises(SS.ContractError, match="resolves into 2 classes"):
        SS.classify(seq, m, io)
    del m.ws.cache[("alias",)]
    seq.zero_state = seq.zero_state | {stray.data_ptr()}
    with pytest.raises(SS.ContractError, match="zero-state pointers the program does not hold"):
        SS.classify(seq, m, io)


def test_launch_forms_of_the_gpu_configurations_cover_baselines(full_forms):
    union = lambda cs: set().union(*(full_forms[c] for c in cs))
    base = union(SC.cases(SC.BASELINE))
    gpu = union(SC.cases(SC.FULL_RECYCLED))
    on_benchmark_shapes = union(c for c in SC.cases(SC.FULL_RECYCLED) if c[2:] in SC.BENCHMARK_SHAPES)
    print(f"launch forms: BASELINE's configurations {len(base)}, the GPU tests' {len(gpu)} ({len(gpu - base)} more from the off-benchmark shapes)")
    missing = sorted(base - gpu)
    assert not missing, "launch forms of BASELINE's configurations that no GPU scratch test runs:\n" + "\n".join(map(str, missing))
    assert on_benchmark_shapes == base   # at the benchmark's shapes the two unions are the same set
    # what the odd and the small shape add are other paths of the same kernels, not other kernels
    assert {f[0] for f in gpu - base} <= {f[0] for f in base}
    # the forms that need E >= 3 at 96 x 96 are why those shapes are run: the 8- and 12-wave row-resident GEMMs are among them
    small = union(c for c in SC.cases(SC.FULL_RECYCLED) if c[1] < 3 or c[2:] != (96, 96))
    waves = {dict(f[2]).get("waves") for f in base - small if f[0] == "rowgemm"}
    assert {8, 12} <= waves, waves


# ---------------------------------------------------------------------------------------------------- fills and the localiser (CPU)

class _CpuSeq:
    """An op list with OpSeq's run / run_range over MG_OP_COPY and MG_OP_MEMSET descriptors on CPU tensors."""

    def __init__(self, name="fake"):
        self.name, self.ops, self.labels, self.keep, self.zero_state, self.f16 = name, [], [], [], set(), False

    def add(self, op, label):
        self.ops.append(op)
        self.labels.append(label)

    def run_range(self, first, count):
        for op in self.ops[first:first + count]:
            r = O.Raw(op)
            if op.kind == L.OP_COPY:
                ctypes.memmove(r.dst, r.src, r.bytes)
            else:
                assert op.kind == L.OP_MEMSET
                ctypes.memset(r.dst, r.value, r.bytes)

    def run(self):
        self.run_range(0, len(self.ops))


def _fake(planted):
    """in -> a (first half only) -> b -> out; ``planted``: the last op copies all of b, whose second half nobody wrote."""
    pool = E.Pool(torch.device("cpu"))
    seq = _CpuSeq()
    inp, out = torch.zeros(64), torch.zeros(64)
    w = torch.arange(64, dtype=torch.float32)
    zs = torch.zeros(256, dtype=torch.uint8)
    seq.keep += [inp, out, zs]
    seq.zero_state = {zs.data_ptr()}
    a, b = pool.get(256), pool.get(256)
    seq.add(O.copy(inp, a, 128), "in->a")
    seq.add(O.copy(w.data_ptr() + 128, a.data_ptr() + 128, 128), "w->a")
    seq.add(O.copy(a, b, 128), "a->b (half)")
    seq.add(O.memset(zs, 16, 0), "tickets")
    seq.add(O.copy(b, out, 256 if planted else 128), "b->out")
    seq.add(O.copy(a.data_ptr() + 128, out.data_ptr() + 128, 128), "a->out (tail)")
    if planted:
        seq.ops.pop(), seq.labels.pop()
    module = SimpleNamespace(pool=pool, ws=SimpleNamespace(cache={("w",): w}))
    io = SS.IO([(inp, torch.arange(64, dtype=torch.float32) * 0.5)], [out])
    return seq, module, io


def test_fills_reach_every_byte_and_are_reproducible():
    ts = [torch.empty(1000, dtype=torch.uint8), torch.empty(7, 3), torch.empty(5, dtype=torch.bfloat16)]
    for pattern in (0x00, 0xFF, 0x7F):
        assert SS.poison(ts, pattern) == 1000 + 84 + 10
        assert all(bool((t.reshape(-1).view(torch.uint8) == pattern).all()) for t in ts)
    SS.poison(ts, 0xFF)
    assert torch.isnan(ts[1]).all() and torch.isnan(ts[2]).all()
    SS.poison(ts, 0x7F)
    assert torch.isfinite(ts[1]).all() and float(ts[1].min()) > 3e38 and float(ts[2].float().min()) > 3e38
    SS.poison(ts, "random", seed=3)
    first = [t.clone() for t in ts]
    assert len(torch.unique(ts[0])) > 200
    SS.poison(ts, 0)
    SS.poison(ts, "random", seed=3)
    assert all(torch.equal(a.view(torch.uint8) if a.dtype == torch.uint8 else a.reshape(-1).view(torch.uint8),
                           b.reshape(-1).view(torch.uint8)) for a, b in zip(first, ts))
    # checksums: a changed byte and two swapped words both show
    t = torch.arange(64, dtype=torch.int32)
    c0 = SS.checksums([t])
    t[3], t[9] = 9, 3
    c1 = SS.checksums([t])
    assert c0[0][0] == c1[0][0] and c0[0][1] != c1[0][1]
    u = torch.zeros(7, dtype=torch.uint8)
    c2 = SS.checksums([u])
    u[6] = 1
    assert SS.checksums([u]) != c2


def test_a_clean_sequence_passes_and_localises_nothing():
    seq, module, io = _fake(planted=False)
    rep = SS.check_program(seq, module, io, say=lambda s: None)
    assert rep["filled_bytes"] == 512 == module.pool.bytes
    assert SS.first_dependent_op(seq, SS.classify(seq, module, io)) is None


def test_a_planted_read_of_unwritten_scratch_is_found_by_index():
    seq, module, io = _fake(planted=True)
    cls = SS.classify(seq, module, io)
    a, _ = SS.run_with_fill(seq, cls, 0x00)
    b, _ = SS.run_with_fill(seq, cls, 0xFF)
    assert not torch.equal(a[0], b[0]) and torch.equal(a[0][:32], b[0][:32])
    assert SS.first_dependent_op(seq, cls) == 4
    with pytest.raises(SS.ContractError, match=r"first dependent op 4: 'b->out'"):
        SS.check_program(seq, module, io, say=lambda s: None)


def test_a_store_into_a_weight_or_an_input_is_reported():
    seq, module, io = _fake(planted=False)
    seq.add(O.memset(module.ws.cache[("w",)].data_ptr() + 4, 1, 0x55), "stray store")
    with pytest.raises(SS.ContractError, match="constant tensor"):
        SS.check_program(seq, module, io, say=lambda s: None)
    seq, module, io = _fake(planted=False)
    seq.add(O.memset(seq.keep[2], 1, 5), "ticket left set")   # zero state that a run leaves changed ... and changes again
    SS.check_program(seq, module, io, say=lambda s: None)      # (set to the same value by every run: a fixed point)
    seq, module, io = _fake(planted=False)
    zs = seq.keep[2]   # state that a run does not hand back as it found it: every run moves it on
    seq.add(O.copy(zs.data_ptr() + 32, zs.data_ptr() + 48, 16), "tickets move on")
    seq.add(O.copy(seq.keep[1].data_ptr() + 4, zs.data_ptr() + 32, 16), "output into the tickets")
    with pytest.raises(SS.ContractError, match="zero state changed"):
        SS.check_program(seq, module, io, say=lambda s: None)
