"""Several pictures per call from C (``mg_model_predict_many``), the part that needs no GPU: the prototype in the header and in the
ctypes layer, the exporter's ``images_per_program`` (K = 1 writes the file it always wrote; K > 1 writes the programs of a full
``map_images(images_per_program=K)`` group and ``cfg[13]`` = K), the loader's slot chain for K pictures in the host-only mode, and
the refusals that come before any device is touched.  tests/test_gpu_predict_many_c_host.py runs the call on the device."""
import ctypes
import os
import re
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPE = """int mg_model_predict_many(mg_model* m, int n, const uint8_t* const* rgb, int hwc, int Hin, int Win, int mode, int reciprocal,
                          const uint64_t* seeds, const mg_predict_opts* opts_or_null, const mg_output_opts* out_opts_or_null,
                          float* pred_out, float* unc_out_or_null, uint16_t* u16_out_or_null, uint8_t* picture_out_or_null,
                          double* info4_or_null, void* stream);"""
# what the header tells the caller of the one-picture entry points about an image of several pictures per call
COMPANION = ("On an image of K > 1 pictures per call mg_model_predict, mg_model_predict_out and mg_model_predict_iid refuse and name "
             "mg_model_predict_many.")


def _header():
    return open(os.path.join(ROOT, "include", "marigold_hip.h")).read()


def _tiny(kind="depth"):
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0)


def test_header_declares_the_prototype():
    words = lambda t: " ".join(t.split())   # noqa: E731
    hdr = words(_header())
    assert words(PROTOTYPE) in hdr
    assert re.search(r"#define MG_ABI_VERSION 4\b", _header())
    assert words(COMPANION) in re.sub(r"\s*\*\s+", " ", hdr)   # (a comment's line breaks carry " * ")
    assert "cfg16[13] = K" in _header()


def test_ctypes_signature():
    from marigold_amd import _lib as L
    lib = L.load()
    assert L.ABI_VERSION == 4 and lib.mg_abi_version() == 4
    assert "mg_model_predict_many" in L.EXPORTS
    args = lib.mg_model_predict_many.argtypes
    assert len(args) == 17
    assert args[1] is ctypes.c_int and args[2] is ctypes.POINTER(ctypes.c_void_p) and args[8] is ctypes.POINTER(ctypes.c_uint64)
    assert args[9] is ctypes.POINTER(L.MgPredictOpts) and args[10] is ctypes.POINTER(L.MgOutputOpts)


def test_one_picture_per_program_is_the_file_written_before(tmp_path):
    from marigold_amd import image
    pipe = _tiny()
    a, b = str(tmp_path / "a.mgimg"), str(tmp_path / "b.mgimg")
    ia = image.export_model_image(pipe, a, ensemble_size=2, height=64, width=128)
    ib = image.export_model_image(pipe, b, ensemble_size=2, height=64, width=128, images_per_program=1)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    assert ia["images_per_program"] == ib["images_per_program"] == 1
    cfg = struct.unpack_from("<16I", raw, 24)
    assert cfg[0] == 2 and cfg[13:] == (0, 0, 0)
    m = image.ModelImage(a, device=-1)
    try:
        info = (ctypes.c_int * 16)()
        assert m._lib.mg_model_info(m.handle, info) == 0
        assert info[13] == 0 and m.K == 1 and m.B == 2
    finally:
        m.close()


def test_three_pictures_of_two_members_load_and_validate(tmp_path):
    """K = 3, E = 2 in the host-only mode: the header, the slot sizes the loader chains, every op's contract, and the refusal of the
    new entry point on a model without a device."""
    from marigold_amd import image, _lib as L
    path = str(tmp_path / "k3.mgimg")
    got = image.export_model_image(_tiny(), path, ensemble_size=2, height=64, width=128, images_per_program=3)
    assert got["images_per_program"] == 3 and got["B"] == 2 and got["latent_hw"] == (8, 16)
    m = image.ModelImage(path, device=-1)
    try:
        info = (ctypes.c_int * 16)()
        assert m._lib.mg_model_info(m.handle, info) == 0
        assert info[0] == 2 and info[13] == 3 and (m.B, m.K, m.H, m.W, m.Hout, m.Wout) == (2, 3, 64, 128, 64, 128)
        m.validate()
        lib = L.load()
        rc = lib.mg_model_predict_many(m.handle, 1, None, 1, 64, 128, 0, 0, None, None, None, None, None, None, None, None, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_many:") and "host-only" in msg, msg
    finally:
        m.close()
    # the slot table of the file: [K,3,H,W] -> [K,4,h,w] | [K,4,h,w], [K E,4,h,w] | [K E,4,h,w] -> [K E,1,Ho,Wo], fp32
    raw = open(path, "rb").read()
    n_buf, n_prog = struct.unpack_from("<II", raw, 16)
    assert n_prog == 3
    slots = {}
    prog_sz = struct.calcsize("<32sIIQQI") + 4 + 16 * struct.calcsize("<24sIIQQ")
    for k in range(3):
        at = struct.calcsize("<8sIIII16I") + n_buf * struct.calcsize("<QQII") + k * prog_sz
        name, _, _, _, _, n_slots = struct.unpack_from("<32sIIQQI", raw, at)
        at += struct.calcsize("<32sIIQQI") + 4
        for s in range(n_slots):
            nm, _, _, _, nbytes = struct.unpack_from("<24sIIQQ", raw, at + s * struct.calcsize("<24sIIQQ"))
            slots[name.rstrip(b"\0").decode(), nm.rstrip(b"\0").decode()] = nbytes
    K, E, H, W, h, w = 3, 2, 64, 128, 8, 16
    assert slots == {("vae.encode", "rgb"): K * 3 * H * W * 4, ("vae.encode", "latent"): K * 4 * h * w * 4,
                     ("denoise", "rgb_latent"): K * 4 * h * w * 4, ("denoise", "x"): K * E * 4 * h * w * 4,
                     ("vae.decode", "latent"): K * E * 4 * h * w * 4, ("vae.decode", "pred"): K * E * 1 * H * W * 4}
    # a header that claims another K no longer chains: refused at load
    bad = str(tmp_path / "bad.mgimg")
    hdr = bytearray(raw[:88])
    struct.pack_into("<I", hdr, 24 + 4 * 13, 2)
    open(bad, "wb").write(bytes(hdr) + raw[88:])
    with pytest.raises(L.MarigoldHipError, match="do not chain"):
        image.ModelImage(bad, device=-1)


def test_exporter_refusals(tmp_path):
    from marigold_amd import image
    with pytest.raises(ValueError, match="images_per_program must be >= 1"):
        image.export_model_image(_tiny(), str(tmp_path / "k0.mgimg"), ensemble_size=1, height=64, width=128, images_per_program=0)
    with pytest.raises(ValueError, match="one picture per call"):
        image.export_model_image(_tiny("iid"), str(tmp_path / "iid.mgimg"), ensemble_size=1, height=64, width=128, images_per_program=2)
    assert not os.path.exists(str(tmp_path / "k0.mgimg")) and not os.path.exists(str(tmp_path / "iid.mgimg"))
