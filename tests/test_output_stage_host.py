"""The depth / normals output stage and ``mg_model_predict_out``, the parts that need no GPU: the new symbols in the header, the binding
and both libraries; the argument checks that come before any device work; the wire format of MG_OP_COLORIZE's two appended fields
(tests/test_gpu_out_stage_kernels.py and tests/test_gpu_predict_out_c_host.py run them on the device).

MG_OP_NORMALS_VIS gains no field: tests/test_host.py pins its table to (h, w | pred, out), so the clipped normals map is an
argument of the call ``mg_normals_finish`` and not of the op - asserted below on purpose."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from marigold_amd import _lib as L, ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "marigold_hip.h")) as f:
        return f.read()


def test_new_symbols_in_header_binding_and_libraries():
    header = _header()
    assert re.search(r"\bint mg_depth_visualize\(const float\* depth, const uint8_t\* lut256x3_or_null, int64_t n, float\* clipped_out_or_null,\s+"
                     r"uint16_t\* u16_out_or_null, uint8_t\* picture_out_or_null, void\* stream\);", header)
    assert re.search(r"\bint mg_normals_finish\(const float\* pred, int H, int W, float\* clipped_out_or_null, uint8_t\* picture_out_or_null, "
                     r"void\* stream\);", header)
    assert re.search(r"\bint mg_model_predict_out\(mg_model\* m, const uint8_t\* rgb, int hwc, int Hin, int Win, int mode, int reciprocal, uint64_t seed,\s+"
                     r"const mg_predict_opts\* opts_or_null, const mg_output_opts\* out_opts_or_null, float\* pred_out,\s+"
                     r"float\* unc_out_or_null, uint16_t\* u16_out_or_null, uint8_t\* picture_out_or_null, double\* info4_or_null,\s+"
                     r"void\* stream\);", header)
    for name, nargs in (("mg_depth_visualize", 7), ("mg_normals_finish", 6), ("mg_model_predict_out", 16)):
        assert name in L.EXPORTS
        for f16 in (False, True):
            assert len(getattr(L.load(f16), name).argtypes) == nargs
    # the entry points this one stands beside keep their declarations
    assert re.search(r"\bint mg_normals_visualize\(const float\* pred, int H, int W, uint8_t\* out_hwc, void\* stream\);", header)
    assert re.search(r"\bint mg_colorize\(const float\* depth, const uint8_t\* lut256x3, uint8_t\* out_hwc, int64_t n, float min_depth, "
                     r"float max_depth, void\* stream\);", header)
    # mg_output_opts: the struct of the header, field for field, and all-zero defaults
    body = re.search(r"typedef struct mg_output_opts \{(.*?)\} mg_output_opts;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip().lstrip("*").strip() for _t, names in re.findall(r"\b(int|const uint8_t\*)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [n for n, _ in L.MgOutputOpts._fields_] == ["out_h", "out_w", "out_mode", "lut256x3"]
    assert [t for _, t in L.MgOutputOpts._fields_] == [ctypes.c_int] * 3 + [ctypes.c_void_p]
    assert re.search(r"#define MG_OUTPUT_OPTS_DEFAULT \{0, 0, 0, 0\}", header)
    o = L.MgOutputOpts()
    assert (o.out_h, o.out_w, o.out_mode, o.lut256x3) == (0, 0, 0, None)
    assert ctypes.sizeof(L.MgOutputOpts) == 24 and L.MgOutputOpts.lut256x3.offset == 16   # three ints, padding, a pointer


def test_calls_refuse_bad_arguments_without_a_device(tmp_path):
    lib = L.load()
    a = 0x10000   # a made-up aligned address: every call below must fail before it would be read

    def refused(rc, *words):
        msg = lib.mg_last_error().decode()
        assert rc != 0 and all(w in msg for w in words), msg

    # the two stage functions
    refused(lib.mg_depth_visualize(None, None, 4, a, None, None, None), "colorize", "null")
    refused(lib.mg_depth_visualize(a, None, 4, None, None, None, None), "colorize", "null")      # no output at all
    refused(lib.mg_depth_visualize(a, None, 4, None, None, a, None), "colorize", "null")         # a picture without a table
    refused(lib.mg_depth_visualize(a, None, 0, a, None, None, None), "colorize", "empty")
    refused(lib.mg_depth_visualize(a, None, 4, a + 2, None, None, None), "colorize", "aligned")
    refused(lib.mg_normals_finish(None, 8, 8, a, a, None), "normals_vis", "null")
    refused(lib.mg_normals_finish(a, 8, 8, None, None, None), "normals_vis", "null")            # no output at all
    refused(lib.mg_normals_finish(a, 0, 8, a, a, None), "normals_vis", "bad size")
    refused(lib.mg_normals_visualize(a, 8, 8, None, None), "normals_vis", "null")
    # the one-call prediction: null arguments
    refused(lib.mg_model_predict_out(None, a, 1, 8, 8, 0, 0, 1, None, None, a, None, None, None, None, None), "mg_model_predict_out", "null")
    # ... and a host-only model
    import marigold_amd as M
    from marigold_amd import image
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    pipe = M.build_synthetic_pipeline("depth", TINY_UNET, TINY_VAE, default_processing_resolution=0, default_denoising_steps=2)
    path = str(tmp_path / "tiny.mgimg")
    image.export_model_image(pipe, path, ensemble_size=1, height=64, width=128)
    m = image.ModelImage(path, device=-1)
    try:
        refused(lib.mg_model_predict_out(m.handle, None, 1, 64, 128, 0, 0, 1, None, None, a, None, None, None, None, None), "mg_model_predict_out", "null")
        refused(lib.mg_model_predict_out(m.handle, a, 1, 64, 128, 0, 0, 1, None, None, None, None, None, None, None, None), "mg_model_predict_out", "null")
        refused(lib.mg_model_predict_out(m.handle, a, 1, 64, 128, 0, 0, 1, None, None, a, None, None, None, None, None), "mg_model_predict_out", "host-only")
    finally:
        m.close()


def test_the_ops_validate_without_a_device():
    """MG_OP_COLORIZE's contract as ``mg_program_validate`` sees it: the new outputs with a range other than (0, 1) and an op with no
    output at all are refused; each output alone, all together and the in-place form are launchable."""
    a, b, c, d = 0x10000, 0x20000, 0x30000, 0x40000

    def validate(op):
        s = O.OpSeq("stage")
        s.add(op)
        s.validate()

    for kw in (dict(out=c), dict(out=None, clipped=a), dict(out=None, u16=d, lut=None), dict(out=c, clipped=a, u16=d),
               dict(out=None, clipped=a, lut=None), dict(out=c, lo=0.5, hi=2.0)):
        kw = dict(dict(lut=b, out=None), **kw)
        validate(O.colorize(a, kw.pop("lut"), kw.pop("out"), n=37 * 53, **kw))
    for kw, words in ((dict(out=c, clipped=a, lo=0.0, hi=2.0), "range"), (dict(out=c, u16=d, lo=-1.0, hi=1.0), "range"),
                      (dict(out=None), "null"), (dict(out=c, lut=None), "null"), (dict(out=c, u16=d + 1), "aligned")):
        kw = dict(dict(lut=b), **kw)
        with pytest.raises(L.MarigoldHipError, match=words):
            validate(O.colorize(a, kw.pop("lut"), kw.pop("out"), n=64, **kw))
    validate(O.normals_vis(a, c, H=8, W=8))
    with pytest.raises(L.MarigoldHipError, match="null"):
        validate(O.normals_vis(a, None, H=8, W=8))


def test_wire_format_of_the_new_fields():
    """Builders called as before give the bytes already in tests/golden/op_wire.json; the new arguments land in p[3] and p[4] and read
    back by name; MG_OP_NORMALS_VIS's table is untouched."""
    with open(os.path.join(ROOT, "tests", "golden", "op_wire.json")) as f:
        want = json.load(f)
    P = lambda k: 0x1000 * k   # noqa: E731  (tests/op_wire.py's pointers)
    assert bytes(O.colorize(P(1), P(2), P(3), n=2, lo=1.5, hi=2.5)).hex() == want["colorize/all"]
    assert bytes(O.colorize(P(1), P(2), P(3), n=2)).hex() == want["colorize/min"]
    assert bytes(O.colorize(P(1), P(2), P(3), n=2, clipped=None, u16=None)).hex() == want["colorize/min"]
    assert bytes(O.normals_vis(P(1), P(2), H=2, W=3)).hex() == want["normals_vis"]
    header = _header()
    assert L.FIELDS[L.OP_COLORIZE][1] == dict(f=("min_depth", "max_depth"), p=("depth", "lut", "out", "clipped", "u16"), l=("n",))
    for name, slot in (("DEPTH", 0), ("LUT", 1), ("OUT", 2), ("CLIPPED", 3), ("U16", 4)):   # appended: the old positions stay
        assert re.search(rf"\bMG_COLORIZE_P_{name} = {slot}\b", header)
    op = O.colorize(101, 102, 103, n=7, clipped=104, u16=105)
    assert [x or 0 for x in op.p] == [101, 102, 103, 104, 105] + [0] * 11 and list(op.l) == [7, 0, 0, 0]
    assert list(op.f) == [0.0, 1.0] + [0.0] * 6 and not any(op.i)
    raw = O.Raw(op)
    assert (raw.depth, raw.lut, raw.out, raw.clipped, raw.u16, raw.n, raw.min_depth, raw.max_depth) == (101, 102, 103, 104, 105, 7, 0.0, 1.0)
    op = O.colorize(101, None, None, n=7, u16=105)
    assert [x or 0 for x in op.p] == [101, 0, 0, 0, 105] + [0] * 11
    assert L.FIELDS[L.OP_NORMALS_VIS][1] == dict(i=("h", "w"), p=("pred", "out"))
    assert not re.search(r"\bMG_NORMALS_VIS_P_CLIPPED\b", header)


def test_export_color_table(tmp_path):
    """The 768 bytes a C host uploads are the table ``colorize_depth_device`` builds from matplotlib."""
    from marigold_amd import image
    from marigold_amd.util.image_util import colormap_lut_u8
    path = str(tmp_path / "spectral.lut")
    table = image.export_color_table("Spectral", path)
    raw = open(path, "rb").read()
    assert len(raw) == 768 and np.array_equal(np.frombuffer(raw, dtype=np.uint8).reshape(256, 3), colormap_lut_u8("Spectral"))
    assert np.array_equal(table, colormap_lut_u8("Spectral"))
