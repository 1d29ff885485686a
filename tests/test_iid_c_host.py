"""The intrinsic-image ensemble op (MG_OP_ENS_IID) and the one-call C prediction for intrinsic-image models (mg_model_predict_iid),
the parts that need no GPU: the builder fills the op's slots (the names against the header: tests/test_host.py); the header, the binding and the built
libraries agree on both entry points and on the options struct; the calls check their arguments; the op's contract runs dry in both libraries; the example host
program compiles against the header."""
import ctypes
import os
import re
import subprocess

import pytest

from marigold_amd import _lib as L, ops, opstats

from tests import c_hosts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "marigold_hip.h")).read()


def test_builder_fills_the_documented_slots():
    op = ops.ens_iid(101, 102, 103, E=10, n=3 * 768 * 768, reduction=1)
    assert op.kind == L.OP_ENS_IID
    assert list(op.i) == [10, 1] + [0] * 38 and [x or 0 for x in op.p] == [101, 102, 103] + [0] * 13
    assert list(op.l) == [3 * 768 * 768, 0, 0, 0] and list(op.f) == [0.0] * 8
    raw = ops.Raw(op)
    assert (raw.e, raw.reduction, raw.preds, raw.pred, raw.unc, raw.n) == (10, 1, 101, 102, 103, 3 * 768 * 768)
    assert ops.Raw(ops.ens_iid(1, 2, None, E=2, n=4)).unc == 0 and ops.ens_iid(1, 2, None, E=2, n=4).i[1] == 0
    # every member read once, the prediction and (when asked for) the uncertainty written once
    assert opstats.op_cost(op) == ("ensemble", 0, 12 * 3 * 768 * 768 * 4)
    assert opstats.op_cost(ops.ens_iid(1, 2, None, E=3, n=100)) == ("ensemble", 0, 4 * 100 * 4)


def test_op_contract_dry_run_in_both_libraries():
    a = 0x10000   # a fake, aligned device address
    for f16 in (False, True):
        seq = ops.OpSeq("ens_iid", f16=f16)
        for E in (1, 2, 4, 5, 10, 11, 17, 32, 33, 128, 129, 1000):   # every kernel the launcher chooses between
            seq.add(ops.ens_iid(a, a + (1 << 20), a + (2 << 20), E=E, n=6 * 8 * 16, reduction=E & 1))
        seq.add(ops.ens_iid(a + 4, a + (1 << 20), None, E=3, n=6 * 8 * 16))    # unaligned for the 16-byte accesses: one element per lane
        seq.add(ops.ens_iid(a, a + (1 << 20), None, E=3, n=210))               # n % 4 != 0: likewise
        seq.validate()
        for op, msg in ((ops.ens_iid(None, a, None, E=2, n=4), "null"),
                        (ops.ens_iid(a, None, None, E=2, n=4), "null"),
                        (ops.ens_iid(a, a, None, E=0, n=4), "E 0 must be >= 1"),
                        (ops.ens_iid(a, a, None, E=2, n=0), "bad element count"),
                        (ops.ens_iid(a, a, None, E=2, n=4, reduction=2), "Unrecognized reduction method: 2"),
                        (ops.ens_iid(a + 2, a, None, E=2, n=4), "4-byte aligned"),
                        (ops.ens_iid(a, a, a + 1, E=2, n=4), "4-byte aligned")):
            s = ops.OpSeq("bad", f16=f16)
            s.add(op)
            with pytest.raises(L.MarigoldHipError, match=msg):
                s.validate()


def test_c_entry_points_in_header_binding_and_libraries():
    header = _header()
    assert re.search(r"\bint mg_ensemble_iid\(const float\* preds, int E, int64_t n, int reduction, float\* pred_out, float\* unc_out_or_null, "
                     r"void\* stream\);", header)
    assert re.search(r"\bint mg_model_predict_iid\(mg_model\* m, const uint8_t\* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,\s+"
                     r"const mg_iid_opts\* opts_or_null, float\* pred_out, float\* unc_out_or_null, uint8_t\* pictures_out_or_null,\s+void\* stream\);", header)
    for name, nargs in (("mg_ensemble_iid", 7), ("mg_model_predict_iid", 13)):
        assert name in L.EXPORTS
        for f16 in (False, True):
            assert len(getattr(L.load(f16), name).argtypes) == nargs
    # mg_iid_opts: the struct of the header, field for field, and its defaults
    body = re.search(r"typedef struct mg_iid_opts \{(.*?)\} mg_iid_opts;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip() for names in re.findall(r"\bint\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [n for n, _ in L.MgIidOpts._fields_] == ["reduction", "linear_bits", "up_to_scale_bits", "out_h", "out_w", "out_mode"]
    assert all(t is ctypes.c_int for _, t in L.MgIidOpts._fields_)
    defaults = re.search(r"#define MG_IID_OPTS_DEFAULT \{([^}]*)\}", header).group(1)
    o = L.MgIidOpts()
    assert [int(v) for v in defaults.split(",")] == [getattr(o, n) for n, _ in L.MgIidOpts._fields_] == [0] * 6
    # the sentence above mg_model_predict stays true, and points to the new entry
    doc = header[header.index("The whole prediction of one picture as ONE call"):header.index("typedef struct mg_predict_opts")]
    assert "An intrinsic-image model is refused" in doc and "mg_model_predict_iid" in doc


def test_calls_check_their_arguments_without_a_device():
    for f16 in (False, True):
        lib = L.load(f16)
        assert lib.mg_ensemble_iid(None, 2, 4, 0, None, None, None) != 0 and b"mg_ensemble_iid" in lib.mg_last_error()
        assert lib.mg_ensemble_iid(0x10000, 2, 4, 0, None, None, None) != 0 and b"mg_ensemble_iid" in lib.mg_last_error()
        assert lib.mg_model_predict_iid(None, None, 1, 8, 8, 0, 0, 1, None, None, None, None, None) != 0
        assert b"mg_model_predict_iid" in lib.mg_last_error()
        assert lib.mg_model_predict(None, None, 1, 8, 8, 0, 0, 1, None, None, None, None, None) != 0
        assert b"mg_model_predict:" in lib.mg_last_error()   # the older entry still speaks for itself


def test_options_struct_size_and_the_example_compile(tmp_path):
    """``sizeof(mg_iid_opts)`` as a C++ compiler sees it equals the ctypes mirror's; examples/host_iid.cpp (which static_asserts the same
    size) compiles with hipcc against the header."""
    src = tmp_path / "size.cpp"
    src.write_text('#include <stdio.h>\n#include "marigold_hip.h"\nint main() { printf("%zu %zu", sizeof(mg_iid_opts), sizeof(mg_op)); return 0; }\n')
    exe = c_hosts.compile_only(src, tmp_path / "size")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [ctypes.sizeof(L.MgIidOpts), ctypes.sizeof(L.MgOp)] == [24, 360]
    example = os.path.join(ROOT, "examples", "host_iid.cpp")
    assert "static_assert(sizeof(mg_iid_opts)" in open(example).read()
    c_hosts.compile_only(example, tmp_path / "host_iid.o")
