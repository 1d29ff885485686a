"""Model images with the tiny autoencoder (``export_model_image(tiny_vae=True)``, a version-3 file), the part that needs no GPU: the
export on a host without one, the file's header and tables, the loader's accounting (the tiny network once in the shared weights, its
workspaces in the scratch region every configuration overlays), ``mg_model_validate`` on the tiny calls' arguments, the exporter's
refusals, the refusal of corrupt version-3 files - all in the host-only mode (``mg_model_load(path, -1)``) - and that an AutoencoderKL
pipeline writes the versions it always wrote.  tests/test_gpu_tiny_image.py runs such images on the device."""
import ctypes
import dataclasses
import os
import struct

import pytest
import torch

HDR, V2, BUF, SLOT, MEMBER = "<8sIIII16I", "<IIQ", "<QQII", "<24sIIQQ", "<IIQ"
PROG_HEAD = struct.calcsize("<32sIIQQI") + 4
PROG_SZ = PROG_HEAD + 16 * struct.calcsize(SLOT)
CFG_SZ = 64 + 3 * PROG_SZ
CFG_AT = struct.calcsize(HDR) + struct.calcsize(V2)
MEMBERS, HALF, ABSENT = 140, 70, 0xFFFFFFFF
SMALL, WIDE = dict(ensemble_size=2, height=30, width=44, denoising_steps=2), dict(ensemble_size=1, height=64, width=128, denoising_steps=2)


def _pipe(kind="depth", tiny=True, dtype=None):
    import marigold_amd as M
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.modules import AutoencoderTinyHIP
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    pipe = M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0, compute_dtype=dtype)
    if tiny:
        pipe.set_vae(AutoencoderTinyHIP(syn.synthetic_tiny_vae_state_dict(), **({} if dtype is None else dict(compute_dtype=dtype))))
    return pipe


@pytest.fixture(scope="module")
def lib():
    from marigold_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """One depth pipeline with the tiny VAE -> (pipe, {name: description}): 30 x 44 with two members, 64 x 128, three pictures per
    call, and one image of the two sizes."""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("tiny_image")
    pipe = _pipe()
    # (the image of both sizes before their single images: the UNet's weight cache then holds what every one of the three needs)
    out = {"k3": image.export_model_image(pipe, str(d / "k3.mgimg"), tiny_vae=True, images_per_program=3, **WIDE),
           "multi": image.export_model_image(pipe, str(d / "multi.mgimg"), tiny_vae=True, configs=[WIDE, SMALL]),
           "small": image.export_model_image(pipe, str(d / "small.mgimg"), tiny_vae=True, **SMALL),
           "wide": image.export_model_image(pipe, str(d / "wide.mgimg"), tiny_vae=True, **WIDE)}
    return pipe, out


def _cfg(lib, handle):
    cfg = (ctypes.c_int * 16)()
    assert lib.mg_model_info(handle, cfg) == 0
    return list(cfg)


def _tables(raw):
    """(number of configurations, offset of the buffer table, its rows, offset of the tiny table, its rows)"""
    n_buf = struct.unpack_from("<I", raw, 16)[0]
    n_cfg = struct.unpack_from(V2, raw, struct.calcsize(HDR))[0]
    buf_at = CFG_AT + n_cfg * CFG_SZ
    rows = [struct.unpack_from(BUF, raw, buf_at + 24 * k) for k in range(n_buf)]
    tiny_at = buf_at + 24 * n_buf
    return n_cfg, buf_at, rows, tiny_at, [struct.unpack_from(MEMBER, raw, tiny_at + 16 * k) for k in range(MEMBERS)]


def test_header_tables_and_accounting_of_a_tiny_image(lib, exported):
    from marigold_amd import image
    _pipe_, out = exported
    assert (image.VERSION, image.VERSION_CONFIGS, image.VERSION_TINY) == (1, 2, 3)
    tiny_bytes = None
    for name, K, (E, H, W, h, w) in (("small", 1, (2, 30, 44, 4, 6)), ("wide", 1, (1, 64, 128, 8, 16)), ("k3", 3, (1, 64, 128, 8, 16))):
        d = out[name]
        raw = open(d["path"], "rb").read()
        magic, version, abi, n_buf, n_prog, *cfg = struct.unpack_from(HDR, raw, 0)
        assert magic == b"MGIMG1\0\0" and version == 3 and abi == 4 and n_prog == 3 and n_buf == d["buffers"] and len(raw) == d["file_bytes"]
        # cfg: the ceiling rule (30 x 44 -> 4 x 6 -> 32 x 48), the VAE named in cfg[14]
        assert cfg == d["cfg16"] and cfg[:5] == [E, H, W, h, w] and cfg[11:13] == [8 * h, 8 * w] and cfg[13] == (K if K > 1 else 0) and cfg[14:] == [1, 0]
        assert d["latent_hw"] == (h, w) and d["ops"]["vae.encode"] == 0 == d["ops"]["vae.decode"] and d["ops"]["denoise"] > 0
        n_cfg, _buf_at, rows, _tiny_at, members = _tables(raw)
        assert n_cfg == 1 and {r[2] for r in rows} == {0, 1, 2, 3}
        # the tiny network: 134 members, each at the start of a shared buffer of its own; six biases absent
        absent = [k for k, m in enumerate(members) if m[0] == ABSENT]
        assert absent == [35 + 3, 35 + 13, 35 + 23, HALF + 35 + 9, HALF + 35 + 19, HALF + 35 + 29]
        present = [m for m in members if m[0] != ABSENT]
        assert len({m[0] for m in present}) == 134 and all(rows[m[0]][2] == 3 and m[2] == 0 for m in present)
        assert rows[members[0][0]][0] == 27 * 64 * 4 and rows[members[HALF][0]][0] == 36 * 64 * 4 and rows[members[2][0]][0] == 9 * 64 * 64 * 2
        net = sum((rows[m[0]][0] + 255) // 256 * 256 for m in present)
        assert tiny_bytes in (None, net)
        tiny_bytes = net
        # the slots of the two entries and their workspaces: scratch
        for k, names in ((0, [b"rgb", b"latent", b"ws"]), (2, [b"latent", b"pred", b"ws"])):
            at = CFG_AT + 64 + k * PROG_SZ
            _nm, n_ops, n_rel, _oo, _ro, n_slots = struct.unpack_from("<32sIIQQI", raw, at)
            slots = [struct.unpack_from(SLOT, raw, at + PROG_HEAD + 48 * i) for i in range(n_slots)]
            assert (n_ops, n_rel) == (0, 0) and [s[0].rstrip(b"\0") for s in slots] == names and all(rows[s[1]][2] == 0 for s in slots)
            B = K if k == 0 else K * E
            assert slots[2][4] == lib.mg_tiny_vae_workspace_bytes(*((0, B, H, W) if k == 0 else (1, B, h, w)))
            # (three buffers of the call's largest level, one 128-byte line per pixel, each rounded up to 256 bytes)
            assert slots[2][4] == 3 * ((B * (H * W if k == 0 else 64 * h * w) * 128 + 255) // 256 * 256)
        m = image.ModelImage(d["path"], device=-1)
        try:
            assert _cfg(lib, m.handle) == cfg == m.configs[0] and (m.B, m.H, m.W, m.h, m.w, m.Hout, m.Wout, m.K) == (E, H, W, h, w, 8 * h, 8 * w, K)
            m.validate()
            # the arena the description gives is what the loader places: the weights shared, the rest the handle's own
            assert m.device_bytes == d["arena"]["private"] + d["arena"]["scratch"] == lib.mg_model_device_bytes(m.handle)
            assert m.shared_bytes == d["arena"]["shared"] == d["shared_bytes"] == lib.mg_model_shared_bytes(m.handle)
            r = m.replica()
            try:
                r.validate()
                assert r.shared_bytes == m.shared_bytes and r.device_bytes == m.device_bytes
            finally:
                r.close()
        finally:
            m.close()
    # the tiny weights are counted once, whatever the configuration - and once in an image of two
    assert out["small"]["shared_bytes"] == out["wide"]["shared_bytes"] >= out["k3"]["shared_bytes"] > tiny_bytes > 0
    multi = out["multi"]
    raw = open(multi["path"], "rb").read()
    assert struct.unpack_from("<8sI", raw, 0) == (b"MGIMG1\0\0", 3) and _tables(raw)[0] == 2
    m = image.ModelImage(multi["path"], device=-1)
    try:
        assert len(m.configs) == 2 and [c[14] for c in m.configs] == [1, 1] and m.configs[0][:5] == [1, 64, 128, 8, 16] and m.configs[1][:5] == [2, 30, 44, 4, 6]
        assert m.shared_bytes == multi["shared_bytes"] == out["wide"]["shared_bytes"]
        scratch = [out["wide"]["arena"]["scratch"], out["small"]["arena"]["scratch"]]
        assert multi["scratch_bytes"] == max(scratch) < sum(scratch)
        assert m.device_bytes == multi["private_bytes"] == out["wide"]["arena"]["private"] + out["small"]["arena"]["private"] + max(scratch)
        for i in (0, 1, 0):
            m.select(i).validate()
        assert m.find(height=30, width=44) == 1 and (m.select(1).h, m.w, m.Hout, m.Wout) == (4, 6, 32, 48)
    finally:
        m.close()


@pytest.mark.parametrize("kind", ["normals", "iid"])
def test_normals_and_intrinsic_images_export_without_a_gpu(lib, tmp_path, kind):
    from marigold_amd import image
    pipe = _pipe(kind)
    d = image.export_model_image(pipe, str(tmp_path / "m.mgimg"), tiny_vae=True, ensemble_size=2, height=30, width=44)
    n = 2 if kind == "iid" else 1
    assert d["cfg16"][3:5] == [4, 6] and d["cfg16"][6] == 3 * n and d["cfg16"][10] == n and d["cfg16"][11:15] == [32, 48, 0, 1]
    raw = open(d["path"], "rb").read()
    at = CFG_AT + 64 + 2 * PROG_SZ + PROG_HEAD
    lat, pred, ws = (struct.unpack_from(SLOT, raw, at + 48 * i) for i in range(3))
    # every member of every target in ONE decode call
    assert lat[4] == 2 * n * 4 * 4 * 6 * 4 and pred[4] == 2 * n * 3 * 32 * 48 * 4 and ws[4] == lib.mg_tiny_vae_workspace_bytes(1, 2 * n, 4, 6)
    m = image.ModelImage(d["path"], device=-1)
    try:
        m.validate()
        assert m.pred_channels == 3 * n and m.device_bytes == d["arena"]["private"] + d["arena"]["scratch"]
    finally:
        m.close()


def test_kl_images_are_what_they_were(lib, tmp_path):
    """An AutoencoderKL pipeline writes version 1 (or 2 with ``configs``), ``cfg[14]`` 0, nothing behind the buffer table but blobs."""
    from marigold_amd import image
    pipe = _pipe(tiny=False)
    one = image.export_model_image(pipe, str(tmp_path / "one.mgimg"), **WIDE)
    two = image.export_model_image(pipe, str(tmp_path / "two.mgimg"), configs=[WIDE, SMALL])
    for d, version in ((one, 1), (two, 2)):
        raw = open(d["path"], "rb").read()
        assert struct.unpack_from("<8sI", raw, 0) == (b"MGIMG1\0\0", version)
        m = image.ModelImage(d["path"], device=-1)
        try:
            assert all(c[14] == 0 and c[15] == 0 for c in m.configs) and len(m.configs) == version
            for i in range(version):
                m.select(i).validate()
            assert (m.h, m.w) == ((8, 16) if version == 1 else (3, 5))   # the AutoencoderKL floors: 30 x 44 -> 3 x 5
        finally:
            m.close()
    # the version-2 tables end where the first stored buffer begins (64-byte aligned): no table was added
    raw = open(two["path"], "rb").read()
    n_buf = struct.unpack_from("<I", raw, 16)[0]
    rows = [struct.unpack_from(BUF, raw, CFG_AT + 2 * CFG_SZ + 24 * k) for k in range(n_buf)]
    end = CFG_AT + 2 * CFG_SZ + 24 * n_buf
    assert min(r[1] for r in rows if r[2] in (2, 3)) == (end + 63) // 64 * 64
    # a KL image that claims the tiny VAE in cfg[14] is refused
    b = bytearray(open(one["path"], "rb").read())
    struct.pack_into("<I", b, 24 + 4 * 14, 1)
    open(tmp_path / "bad.mgimg", "wb").write(bytes(b))
    assert not lib.mg_model_load(str(tmp_path / "bad.mgimg").encode(), -1) and "cfg[14]" in lib.mg_last_error().decode()


def test_exporter_refusals(tmp_path):
    from marigold_amd import image
    path = str(tmp_path / "no.mgimg")
    tiny, kl = _pipe(), _pipe(tiny=False)
    for kw in (WIDE, dict(configs=[WIDE, SMALL])):   # without the keyword: the refusal of before, now with a hint
        with pytest.raises(ValueError, match="model images carry an AutoencoderKL.*AutoencoderTinyHIP.*tiny_vae=True"):
            image.export_model_image(tiny, path, **kw)
        with pytest.raises(ValueError, match="tiny_vae=True.*AutoencoderTinyHIP.*AutoencoderKLHIP"):
            image.export_model_image(kl, path, tiny_vae=True, **kw)
    with pytest.raises(ValueError, match="compute_dtype=torch.bfloat16"):
        image.export_model_image(_pipe(dtype=torch.float16), path, tiny_vae=True, **WIDE)
    with pytest.raises(ValueError, match="one picture per call"):
        image.export_model_image(_pipe("iid"), path, tiny_vae=True, images_per_program=2, **WIDE)
    with pytest.raises(ValueError, match="either configs"):
        image.export_model_image(tiny, path, tiny_vae=True, configs=[WIDE], ensemble_size=1)
    assert not os.path.exists(path)


def test_host_pack_is_the_device_layout():
    """``host_pack`` packs what ``.to(device)`` packs (one ``_pack``), once: the struct's 134 addresses lie in its tensors."""
    from marigold_amd import _lib as L
    vae = _pipe().vae
    net, keep = vae.host_pack()
    assert vae.host_pack()[0] is net and len(keep) == 134 and all(t.device.type == "cpu" and t.is_contiguous() for t in keep)
    ptrs = list((ctypes.c_uint64 * MEMBERS).from_buffer_copy(bytes(net)))
    assert sorted(p for p in ptrs if p) == sorted(t.data_ptr() for t in keep) and ptrs.count(0) == 6
    assert ctypes.sizeof(L.MgTinyVae) == 8 * MEMBERS and vae.ws is None   # the module is still off the device
    with pytest.raises(RuntimeError, match="no op program"):
        vae.dry()


def corrupt_tiny_images(raw, lib):
    """{name: (bytes, words of the refusal)} - the version-3 image ``raw`` broken in the ways the loader must refuse."""
    n_cfg, buf_at, rows, tiny_at, members = _tables(raw)
    out = {"truncated-in-the-tiny-table": (raw[:tiny_at + 16 * 50 + 3], "")}

    def patched(fmt, at, *values):
        b = bytearray(raw)
        struct.pack_into(fmt, b, at, *values)
        return bytes(b)

    nbytes = rows[members[2][0]][0]
    out["member-past-its-buffer"] = (patched("<Q", tiny_at + 16 * 2 + 8, nbytes), "spans")
    out["member-half-past-its-buffer"] = (patched("<Q", tiny_at + 16 * 2 + 8, 16), "spans")
    out["member-not-aligned"] = (patched("<Q", tiny_at + 16 * 1 + 8, 8), "16-byte aligned")
    out["member-in-a-private-buffer"] = (patched("<I", tiny_at, next(i for i, r in enumerate(rows) if r[2] == 2)), "not a shared one")
    out["member-out-of-range"] = (patched("<I", tiny_at, len(rows)), "not a shared one")
    out["bias-where-none-belongs"] = (patched(MEMBER, tiny_at + 16 * (35 + 3), *members[35 + 2]), "has no bias")
    out["bias-missing"] = (patched(MEMBER, tiny_at + 16 * (35 + 4), ABSENT, 0, 0), "absent")
    for k, name in ((0, "encode"), (2, "decode")):
        at = CFG_AT + 64 + k * PROG_SZ + PROG_HEAD + 48 * 2
        ws = struct.unpack_from(SLOT, raw, at)
        assert ws[0].rstrip(b"\0") == b"ws"
        out[f"{name}-workspace-one-byte-short"] = (patched("<Q", at + 40, ws[4] - 1), "workspaces")
    out["unknown-vae"] = (patched("<I", CFG_AT + 4 * 14, 2), "cfg[14]")
    out["kl-in-a-tiny-image"] = (patched("<I", CFG_AT + 4 * 14, 0), "cfg[14]")
    out["latent-floored"] = (patched("<I", CFG_AT + 4 * 3, 3), "do not chain")
    out["decoded-size"] = (patched("<I", CFG_AT + 4 * 11, 30), "do not chain")
    out["ops-in-a-vae-entry"] = (patched("<I", CFG_AT + 64 + 32, 1), "corrupt program table")
    out["unknown-version"] = (patched("<I", 8, 4), "unknown version")
    return out


def test_corrupt_tiny_images_are_refused(lib, exported, tmp_path):
    from marigold_amd import image, _lib as L
    _pipe_, out = exported
    raw = open(out["small"]["path"], "rb").read()
    broken = corrupt_tiny_images(raw, lib)
    assert len(broken) == 16
    for name, (data, words) in broken.items():
        path = str(tmp_path / (name + ".mgimg"))
        open(path, "wb").write(data)
        assert not lib.mg_model_load(path.encode(), -1), name
        msg = lib.mg_last_error().decode()
        assert msg.startswith("mg_model_load:") and words in msg, (name, msg)
    with pytest.raises(L.MarigoldHipError, match="mg_model_load"):
        image.ModelImage(str(tmp_path / "unknown-vae.mgimg"), device=-1)
    # the image itself loads
    assert open(out["small"]["path"], "rb").read() == raw
    image.ModelImage(out["small"]["path"], device=-1).close()
