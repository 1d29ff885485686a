"""The native noise generator (MG_OP_RANDN) and the one-call C prediction, the parts that need no GPU: the numpy restatement that
judges the kernel against Random123's known answers; the slots the builder fills (the names against the header: tests/test_host.py); its
contract through both libraries' dry run; the new C entry points in the header, the binding and both libraries; the stream
bookkeeping of ``NativeNoise``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from marigold_amd import _lib as L, ops, opstats
from tests import philox_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "marigold_hip.h")).read()


# ---- the restatement ---------------------------------------------------------------------------------------------------------


def test_restatement_reproduces_the_known_answers():
    """Random123's known-answer vector for an all-zero counter and key, and its two other philox4x32-10 vectors."""
    got = P.philox4x32_10(np.zeros(4, dtype=np.uint32), np.zeros(2, dtype=np.uint32))
    assert [f"{int(v):08x}" for v in got] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    P.check_known_answers()
    assert (P.M0, P.M1, P.W0, P.W1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)


def test_restatement_indexing():
    """Element offset + i is word (offset + i) % 4 of block (offset + i) / 4, whatever the draw; the 64-bit block, stream and seed
    each reach their own counter / key word."""
    seed, stream = 0xFEDCBA9876543210, (1 << 32) + 5
    whole = P.words(seed, stream, 0, 64)
    for offset, n in ((0, 1), (1, 3), (2, 4), (3, 5), (7, 50), (5, 59)):
        assert np.array_equal(P.words(seed, stream, offset, n), whole[offset:offset + n])
    blocks = P.block_words(seed, stream, 3, 2)
    assert np.array_equal(blocks.reshape(-1), whole[12:20])
    at = (1 << 34) - 2   # blocks 2^32 - 1 and 2^32: the high counter word comes into play
    w = P.words(seed, stream, at, 8)
    assert np.array_equal(w[:2], P.block_words(seed, stream, (1 << 32) - 1, 1)[0, 2:])
    assert np.array_equal(w[2:6], P.philox4x32_10(np.array([0, 1, 5, 1]), np.array([0x76543210, 0xFEDCBA98])))
    assert not np.array_equal(w[2:6], P.block_words(seed, stream, 0, 1)[0])   # a truncated counter would give block 0
    assert not np.array_equal(P.words(seed, 5, 0, 4), P.words(seed, stream, 0, 4))
    assert not np.array_equal(P.words(seed & 0xFFFFFFFF, stream, 0, 4), P.words(seed, stream, 0, 4))
    z = P.normals(seed, stream, 0, 1 << 12)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(46 * np.log(2)) and np.array_equal(P.normals(seed, stream, 5, 9), z[5:14])


# ---- the op ------------------------------------------------------------------------------------------------------------------


def test_builder_fills_the_documented_slots():
    op = ops.randn(101, n=1000, seed=0xFEDCBA9876543210, stream=(1 << 63) + 2, offset=7, out16=True)
    assert op.kind == L.OP_RANDN
    assert list(op.i) == [0, 1] + [0] * 38 and [x or 0 for x in op.p] == [101] + [0] * 15 and list(op.f) == [0.0] * 8
    assert [v & ((1 << 64) - 1) for v in op.l] == [1000, 7, 0xFEDCBA9876543210, (1 << 63) + 2]
    raw = ops.Raw(op)
    assert (raw.mode, raw.out16, raw.dst, raw.n, raw.offset) == (0, 1, 101, 1000, 7)
    assert list(ops.randn(1, n=4, seed=3, words=True).i[:2]) == [1, 0]
    with pytest.raises(ValueError, match="outside 64 bits"):
        ops.randn(1, n=4, seed=1 << 64)
    with pytest.raises(ValueError, match="outside 64 bits"):
        ops.randn(1, n=4, seed=0, stream=-1)
    assert opstats.op_cost(ops.randn(1, n=10 * 4 * 96 * 96, seed=0)) == ("noise", 0, 10 * 4 * 96 * 96 * 4)
    assert opstats.op_cost(ops.randn(1, n=64, seed=0, out16=True)) == ("noise", 0, 128)


def test_op_contract_dry_run_in_both_libraries():
    a = 0x10000   # a fake, aligned device address
    for f16 in (False, True):
        seq = ops.OpSeq("randn", f16=f16)
        seq.add(ops.randn(a, n=10 * 4 * 96 * 96, seed=1))
        seq.add(ops.randn(a + 4, n=5, seed=1, offset=3))                       # unaligned for the vector store: element by element
        seq.add(ops.randn(a + 2, n=1023, seed=(1 << 64) - 1, stream=(1 << 64) - 1, out16=True))
        seq.add(ops.randn(a, n=8, seed=1, offset=(1 << 34) - 2, words=True))
        seq.add(ops.randn(a, n=1, seed=0, offset=(1 << 62) - 1))
        seq.validate()
        for op, msg in ((ops.randn(None, n=4, seed=0), "null"),
                        (ops.randn(a, n=0, seed=0), "bad range"),
                        (ops.randn(a, n=4, seed=0, offset=-1), "bad range"),
                        (ops.randn(a, n=2, seed=0, offset=(1 << 62) - 1), "bad range"),
                        (ops.randn(a + 2, n=4, seed=0), "aligned"),
                        (ops.randn(a + 1, n=4, seed=0, out16=True), "aligned"),
                        (ops.randn(a, n=4, seed=0, words=True, out16=True), "32 bits"),
                        (ops.build_op(L.OP_RANDN, mode=2, dst=a, n=4), "mode")):
            s = ops.OpSeq("bad", f16=f16)
            s.add(op)
            with pytest.raises(L.MarigoldHipError, match=msg):
                s.validate()


# ---- the C entry points ------------------------------------------------------------------------------------------------------


def test_c_entry_points_in_header_binding_and_libraries():
    header = _header()
    assert re.search(r"\bint mg_randn\(uint64_t seed, uint64_t stream_id, int64_t offset, int64_t n, void\* dst, int out16, void\* stream\);", header)
    assert re.search(r"\bint mg_model_predict\(mg_model\* m, const uint8_t\* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,\s+"
                     r"const mg_predict_opts\* opts_or_null, float\* pred_out, float\* unc_out_or_null, double\* info4_or_null, void\* stream\);", header)
    for name, nargs in (("mg_randn", 7), ("mg_resize", 11), ("mg_colorize", 7), ("mg_iid_visualize", 9), ("mg_model_predict", 13)):
        assert re.search(rf"\bint {name}\(", header) and name in L.EXPORTS
        for f16 in (False, True):
            assert len(getattr(L.load(f16), name).argtypes) == nargs
    # mg_predict_opts: the struct of the header, field for field, and the reference's defaults (marigold/util/ensemble.py:39-49, :199-203)
    body = re.search(r"typedef struct mg_predict_opts \{(.*?)\} mg_predict_opts;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"\b(int|double)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [({ctypes.c_int: "int", ctypes.c_double: "double"}[t], n) for n, t in L.MgPredictOpts._fields_]
    defaults = re.search(r"#define MG_PREDICT_OPTS_DEFAULT \{([^}]*)\}", header).group(1)
    o = L.MgPredictOpts()
    assert [float(v) for v in defaults.split(",")] == [float(getattr(o, n)) for n, _ in L.MgPredictOpts._fields_]
    assert (o.scale_invariant, o.shift_invariant, o.reduction, o.max_iter, o.max_res, o.normals_reduction, o.regularizer_strength, o.tol) == \
        (1, 1, 0, 50, 1024, 0, 0.02, 1e-6)


def test_calls_check_their_arguments_without_a_device():
    lib = L.load()
    assert lib.mg_randn(1, 0, 0, 4, None, 0, None) != 0 and b"null" in lib.mg_last_error()
    assert lib.mg_randn(1, 0, -1, 4, 0x10000, 0, None) != 0 and b"bad range" in lib.mg_last_error()
    assert lib.mg_model_predict(None, None, 1, 8, 8, 0, 0, 1, None, None, None, None, None) != 0 and b"mg_model_predict" in lib.mg_last_error()
    assert lib.mg_resize(None, None, None, 1, 8, 8, 4, 4, 0, 0, None) != 0 and b"resize: null pointer" in lib.mg_last_error()
    assert lib.mg_colorize(None, None, None, 4, 0.0, 1.0, None) != 0 and b"colorize" in lib.mg_last_error()
    assert lib.mg_iid_visualize(None, None, None, 1, 8, 8, 0, 0, None) != 0 and b"null" in lib.mg_last_error()


# ---- NativeNoise -------------------------------------------------------------------------------------------------------------


def test_native_noise_stream_bookkeeping(monkeypatch):
    import marigold_amd as M
    from marigold_amd import noise
    from marigold_amd.pipeline import _MarigoldPipelineBase
    assert M.NativeNoise is noise.NativeNoise and M.native_randn is noise.native_randn
    draws = []

    def fake(shape, seed, stream=0, offset=0, dtype=torch.float32, device=None):
        draws.append((tuple(shape), seed, stream, offset, dtype))
        return torch.zeros(tuple(shape), dtype=dtype)
    monkeypatch.setattr(noise, "native_randn", fake)
    g = M.NativeNoise(7)
    assert (g.seed, g.next_stream) == (7, 0)
    from types import SimpleNamespace
    stand_in = SimpleNamespace(device=torch.device("cpu"), io_dtype=torch.float32, noise_dtype=torch.bfloat16)   # noise_dtype: ignored
    for k in range(3):   # every _randn call takes the next stream, from element 0
        out = _MarigoldPipelineBase._randn(stand_in, (2, 4, 8, 16), g)
        assert out.dtype == torch.float32 and tuple(out.shape) == (2, 4, 8, 16)
        assert draws[-1] == ((2, 4, 8, 16), 7, k, 0, torch.float32) and g.next_stream == k + 1
    stand_in.io_dtype = torch.bfloat16   # rounded to io_dtype in the store
    assert _MarigoldPipelineBase._randn(stand_in, (1, 4), g).dtype == torch.bfloat16 and draws[-1][2:] == (3, 0, torch.bfloat16)
    assert g.manual_seed(9) is g and (g.seed, g.next_stream) == (9, 0)
    _MarigoldPipelineBase._randn(stand_in, (1, 4), g)
    assert draws[-1][1:3] == (9, 0) and g.next_stream == 1
    assert M.NativeNoise(-1).seed == (1 << 64) - 1 and M.NativeNoise((1 << 64) + 3).seed == 3   # seeds are 64 bits
    assert "seed=9" in repr(g) and "next_stream=1" in repr(g)
    # a torch.Generator and None draw exactly as before
    stand_in.io_dtype, stand_in.noise_dtype = torch.float32, torch.float32
    a = _MarigoldPipelineBase._randn(stand_in, (3, 5), torch.Generator().manual_seed(4))
    assert torch.equal(a, torch.randn(3, 5, generator=torch.Generator().manual_seed(4))) and len(draws) == 5
    torch.manual_seed(12)
    b = _MarigoldPipelineBase._randn(stand_in, (3, 5), None)
    torch.manual_seed(12)
    assert torch.equal(b, torch.randn(3, 5))


def test_native_randn_refuses_what_it_cannot_draw():
    from marigold_amd import native_randn
    with pytest.raises(ValueError, match="CUDA device"):
        native_randn((4,), 1, device="cpu")
    with pytest.raises(ValueError, match="fp32, bf16 or fp16"):
        native_randn((4,), 1, dtype=torch.float64)
