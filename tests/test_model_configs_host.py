"""One model image for several configurations (``export_model_image(configs=[...])``, a version-2 file) and replicas of a loaded
image (``mg_model_replica``), the part that needs no GPU: the file's layout, the loader's accounting (weights shared, one scratch
region overlaid by every configuration), lookup and selection, ``mg_processed_size`` against ``resize_max_res``'s arithmetic, the
refusal of corrupt version-2 files and the exporter's refusals - all in the host-only mode (``mg_model_load(path, -1)``).
tests/test_gpu_model_configs.py runs the configurations and the replicas on the device."""
import ctypes
import os
import struct

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (E, H, W, T, K)
CONFIGS = [dict(ensemble_size=1, height=64, width=128, denoising_steps=2, images_per_program=1),
           dict(ensemble_size=2, height=64, width=128, denoising_steps=2, images_per_program=1),
           dict(ensemble_size=1, height=128, width=64, denoising_steps=2, images_per_program=1),
           dict(ensemble_size=1, height=64, width=128, denoising_steps=2, images_per_program=2)]
HDR, V2, BUF, REL = "<8sIIII16I", "<IIQ", "<QQII", "<IIIIQ"
PROG_SZ = struct.calcsize("<32sIIQQI") + 4 + 16 * struct.calcsize("<24sIIQQ")
CFG_SZ = 64 + 3 * PROG_SZ


def _tiny(kind="depth"):
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    return M.build_synthetic_pipeline(kind, TINY_UNET, TINY_VAE, default_denoising_steps=2, default_processing_resolution=0)


@pytest.fixture(scope="module")
def lib():
    from marigold_amd import _lib as L
    return L.load()


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """The four-configuration image, then each configuration's own single image (-> multi, [single...]); the multi export comes
    first, so that the modules' weight cache holds what every configuration needs when the singles are written."""
    from marigold_amd import image
    d = tmp_path_factory.mktemp("configs")
    pipe = _tiny()
    multi = image.export_model_image(pipe, str(d / "multi.mgimg"), configs=CONFIGS)
    singles = [image.export_model_image(pipe, str(d / f"single{i}.mgimg"), **c) for i, c in enumerate(CONFIGS)]
    return multi, singles


def _cfg(lib, handle, index=None):
    cfg = (ctypes.c_int * 16)()
    assert (lib.mg_model_info(handle, cfg) if index is None else lib.mg_model_config_info(handle, index, cfg)) == 0
    return list(cfg)


def test_layout_of_a_multi_configuration_image(lib, exported):
    from marigold_amd import image
    multi, singles = exported
    raw = open(multi["path"], "rb").read()
    magic, version, _abi, n_buf, n_prog = struct.unpack_from("<8sIIII", raw, 0)
    assert magic == b"MGIMG1\0\0" and version == 2 and n_prog == 12 and n_buf == multi["buffers"]
    n_cfg, _pad, scratch_region = struct.unpack_from(V2, raw, struct.calcsize(HDR))
    assert n_cfg == 4 and scratch_region == multi["scratch_bytes"]
    m = image.ModelImage(multi["path"], device=-1)
    try:
        assert lib.mg_model_num_configs(m.handle) == 4 and len(m.configs) == 4
        for i, one in enumerate(singles):
            s = image.ModelImage(one["path"], device=-1)
            try:
                want = _cfg(lib, s.handle)
                assert lib.mg_model_num_configs(s.handle) == 1 and lib.mg_model_shared_bytes(s.handle) == 0
                # a version-1 image keeps everything in the handle's own arena
                assert lib.mg_model_device_bytes(s.handle) == sum(one["arena"].values())
            finally:
                s.close()
            assert _cfg(lib, m.handle, i) == want == one["cfg16"] == multi["configs"][i]["cfg16"] == m.configs[i]
            assert want[0] == CONFIGS[i]["ensemble_size"] and want[1:3] == [CONFIGS[i]["height"], CONFIGS[i]["width"]]
            assert want[13] == (0 if CONFIGS[i]["images_per_program"] == 1 else CONFIGS[i]["images_per_program"])
            assert lib.mg_model_select(m.handle, i) == 0 and _cfg(lib, m.handle) == want
            assert lib.mg_model_validate(m.handle) == 0, lib.mg_last_error().decode()
            for key in ("ops", "scratch_bytes", "zero_bytes", "data_bytes", "latent_hw", "B", "steps", "images_per_program", "arena"):
                assert multi["configs"][i][key] == one[key], key
        # the weights once: what ONE single export carries of the modules' weight cache
        shared = singles[0]["arena"]["shared"]
        assert shared > 0 and all(one["arena"]["shared"] == shared for one in singles)
        assert lib.mg_model_shared_bytes(m.handle) == multi["shared_bytes"] == shared == m.shared_bytes
        # the private arena: every configuration's constants and zeroed state, and ONE scratch region - the largest, not the sum
        scratch = [one["arena"]["scratch"] for one in singles]
        assert all(one["scratch_bytes"] > 0 and one["arena"]["scratch"] >= one["scratch_bytes"] for one in singles)
        assert scratch_region == max(scratch) < sum(scratch)
        private = sum(one["arena"]["private"] for one in singles)
        assert lib.mg_model_device_bytes(m.handle) == private + max(scratch) == multi["private_bytes"] == m.device_bytes
    finally:
        m.close()
    assert multi["file_bytes"] == len(raw) < sum(one["file_bytes"] for one in singles)
    # every scratch buffer lies inside the region, at its own offset, and names its configuration
    at = struct.calcsize(HDR) + struct.calcsize(V2) + 4 * CFG_SZ
    rows = [struct.unpack_from(BUF, raw, at + 24 * k) for k in range(n_buf)]
    assert {r[2] for r in rows} == {0, 1, 2, 3} and {r[3] for r in rows if r[2] != 3} == {0, 1, 2, 3}
    assert all(r[1] % 256 == 0 and r[1] + r[0] <= scratch_region for r in rows if r[2] == 0)


def test_configurations_read_by_name(exported):
    """``ModelImage.config(i)`` is ``ModelImage.configs[i]`` under the names of ``_lib.CFG``; the word ``pictures`` is written 0 for one
    picture per call and K otherwise."""
    from marigold_amd import image, _lib as L
    multi, singles = exported
    for path in [multi["path"]] + [one["path"] for one in singles]:
        m = image.ModelImage(path, device=-1)
        try:
            for i, words in enumerate(m.configs):
                named = m.config(i)
                assert list(named) == list(L.CFG) and len(words) == L.CFG_WORDS == 16 and words[len(L.CFG):] == [0]
                for n in L.CFG:
                    assert named[n] == words[L.CFG.index(n)], (path, i, n)
        finally:
            m.close()
    m = image.ModelImage(multi["path"], device=-1)
    try:
        for i, c in enumerate(CONFIGS):
            K, named = c["images_per_program"], m.config(i)
            assert named["pictures"] == (0 if K == 1 else K) and m.select(i).K == K
            assert (named["members"], named["height"], named["width"], named["steps"]) == (c["ensemble_size"], c["height"], c["width"], 2)
            assert (named["latent_h"], named["latent_w"], named["out_h"], named["out_w"]) == (c["height"] // 8, c["width"] // 8, c["height"], c["width"])
            assert (named["channels"], named["post"], named["step_noises"], named["modalities"], named["vae"]) == (1, L.POST_DEPTH, 0, 1, L.VAE_KL)
            assert named["op_bytes"] == ctypes.sizeof(L.MgOp) == 360
    finally:
        m.close()


def test_version_1_is_unchanged(lib, exported):
    from marigold_amd import image
    _multi, singles = exported
    raw = open(singles[1]["path"], "rb").read()
    assert struct.unpack_from("<8sI", raw, 0) == (b"MGIMG1\0\0", 1) and struct.unpack_from("<I", raw, 20)[0] == 3
    # the version-1 layout: header | buffer table | three programs
    n_buf = struct.unpack_from("<I", raw, 16)[0]
    at = struct.calcsize(HDR) + 24 * n_buf
    assert [raw[at + k * PROG_SZ:at + k * PROG_SZ + 32].rstrip(b"\0") for k in range(3)] == [b"vae.encode", b"denoise", b"vae.decode"]
    assert {struct.unpack_from(BUF, raw, struct.calcsize(HDR) + 24 * k)[2:] for k in range(n_buf)} == {(0, 0), (1, 0), (2, 0)}
    m = image.ModelImage(singles[1]["path"], device=-1)
    try:
        assert lib.mg_model_num_configs(m.handle) == 1
        assert _cfg(lib, m.handle) == _cfg(lib, m.handle, 0) == list(struct.unpack_from("<16I", raw, 24))
        assert (m.B, m.H, m.W, m.h, m.w, m.steps, m.K) == (2, 64, 128, 8, 16, 2, 1)
        m.validate()
    finally:
        m.close()


def test_lookup_selection_and_refusals(lib, exported):
    from marigold_amd import image, _lib as L
    multi, _singles = exported
    m = image.ModelImage(multi["path"], device=-1)
    try:
        find = lambda *a: lib.mg_model_find_config(m.handle, *a)   # noqa: E731  (H, W, E, steps, K)
        assert find(64, 128, 1, 2, 1) == 0 and find(64, 128, 2, 2, 1) == 1 and find(128, 64, 1, 2, 1) == 2 and find(64, 128, 1, 2, 2) == 3
        assert find(-1, -1, -1, -1, -1) == 0 and find(-1, -1, 2, -1, -1) == 1 and find(128, -1, -1, -1, -1) == 2 and find(-1, -1, -1, -1, 2) == 3
        assert find(64, 128, -1, -1, -1) == 0 and find(-1, 64, -1, 2, -1) == 2
        assert m.find(height=128, width=64) == 2 and m.find(ensemble_size=2) == 1
        assert find(96, 128, -1, -1, -1) == -1
        msg = lib.mg_last_error().decode()
        assert msg.startswith("mg_model_find_config:") and "64 x 128" in msg and "128 x 64" in msg and "96 x 128" in msg, msg
        assert find(64, 128, 3, -1, -1) == -1 and find(64, 128, 1, 3, -1) == -1
        with pytest.raises(L.MarigoldHipError, match="mg_model_find_config"):
            m.find(height=32)
        # selection: configuration 0 after the load; out of range is refused and changes nothing
        assert _cfg(lib, m.handle) == m.configs[0]
        assert m.select(2) is m and (m.H, m.W, m.B, m.K) == (128, 64, 1, 1) and _cfg(lib, m.handle) == m.configs[2]
        for bad in (-1, 4, 1 << 20):
            assert lib.mg_model_select(m.handle, bad) != 0
            assert lib.mg_last_error().decode().startswith("mg_model_select:")
            assert _cfg(lib, m.handle) == m.configs[2]
        assert lib.mg_model_config_info(m.handle, 4, (ctypes.c_int * 16)()) != 0
        # the refusals act on the selected configuration, in the words they always had
        m.select(3)
        assert m.K == 2
        rc = lib.mg_model_predict_out(m.handle, None, 1, 64, 128, 0, 0, 1, None, None, None, None, None, None, None, None)
        assert rc != 0 and "null argument" in lib.mg_last_error().decode()
        rc = lib.mg_model_predict_many(m.handle, 3, None, 1, 64, 128, 0, 0, None, None, None, None, None, None, None, None, None)
        assert rc != 0 and "host-only" in lib.mg_last_error().decode()
    finally:
        m.close()


def test_exporter_refusals(tmp_path):
    import dataclasses
    import marigold_amd as M
    from marigold_amd import image
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    pipe = _tiny()
    path = str(tmp_path / "no.mgimg")
    with pytest.raises(ValueError, match="listed twice"):
        image.export_model_image(pipe, path, configs=[CONFIGS[0], CONFIGS[1], dict(CONFIGS[0])])
    with pytest.raises(ValueError, match="listed twice"):   # the default steps are the steps
        image.export_model_image(pipe, path, configs=[CONFIGS[0], dict(ensemble_size=1, height=64, width=128)])
    with pytest.raises(ValueError, match="either configs"):
        image.export_model_image(pipe, path, configs=CONFIGS[:2], ensemble_size=1, height=64, width=128)
    with pytest.raises(ValueError, match="either configs"):
        image.export_model_image(pipe, path, configs=CONFIGS[:2], images_per_program=2)
    with pytest.raises(ValueError, match="one pipeline kind"):
        image.export_model_image(pipe, path, configs=[CONFIGS[0], dict(CONFIGS[1], pipe=_tiny("normals"))])
    with pytest.raises(ValueError, match="images_per_program must be >= 1"):
        image.export_model_image(pipe, path, configs=[CONFIGS[0], dict(CONFIGS[1], images_per_program=0)])
    with pytest.raises(ValueError, match="configs is empty"):
        image.export_model_image(pipe, path, configs=[])
    with pytest.raises(ValueError, match="takes the keywords"):
        image.export_model_image(pipe, path, configs=[dict(CONFIGS[0], size=3)])
    iid = M.build_synthetic_pipeline("iid", dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8), TINY_VAE,
                                     default_denoising_steps=2, default_processing_resolution=0)
    with pytest.raises(ValueError, match="one picture per call"):
        image.export_model_image(iid, path, configs=[CONFIGS[0], CONFIGS[3]])
    assert not os.path.exists(path)


def test_processed_size_is_resize_max_res(lib):
    import torch
    from marigold_amd.util.image_util import max_res_size, resize_max_res
    H, W = ctypes.c_int(), ctypes.c_int()

    def got(hin, win, res):
        assert lib.mg_processed_size(hin, win, res, ctypes.byref(H), ctypes.byref(W)) == 0
        return H.value, W.value

    for res in (0, 32, 48):
        for hin in range(1, 65):
            for win in range(1, 65):
                assert got(hin, win, res) == (max_res_size((hin, win), res) if res else (hin, win)), (hin, win, res)
    for size, want in (((375, 1242), (231, 768)), ((480, 640), (576, 768)), ((4032, 6048), (512, 768))):
        assert got(*size, 768) == max_res_size(size, 768) == want
    # max_res_size is the size resize_max_res resizes to
    for size, res in (((375, 1242), 768), ((48, 64), 32), ((7, 64), 48), ((96, 192), 128)):
        assert tuple(resize_max_res(torch.zeros(1, 3, *size), res).shape[-2:]) == got(*size, res)
    assert got(96, 192, 128) == (64, 128)
    for bad in ((0, 4, 8), (4, -1, 8), (4, 4, -8)):
        assert lib.mg_processed_size(*bad, ctypes.byref(H), ctypes.byref(W)) != 0
        assert lib.mg_last_error().decode().startswith("mg_processed_size:")


def corrupt_images(raw):
    """{name: bytes} - the version-2 image ``raw`` broken in the three ways the loader must refuse (also what
    tools/model_image_check.cpp is fed under a sanitizer)."""
    n_buf = struct.unpack_from("<I", raw, 16)[0]
    n_cfg, _pad, region = struct.unpack_from(V2, raw, struct.calcsize(HDR))
    cfg_at = struct.calcsize(HDR) + struct.calcsize(V2)
    buf_at = cfg_at + n_cfg * CFG_SZ
    rows = [struct.unpack_from(BUF, raw, buf_at + 24 * k) for k in range(n_buf)]
    out = {"truncated-configs": raw[:cfg_at + CFG_SZ + 100]}
    # the last scratch buffer of configuration 1 moved to the end of the region: its offset plus its size lies beyond it
    k = max(i for i, r in enumerate(rows) if r[2] == 0 and r[3] == 1)
    b = bytearray(raw)
    struct.pack_into("<Q", b, buf_at + 24 * k + 8, region)
    out["scratch-beyond-region"] = bytes(b)
    # the first relocation of configuration 0's denoise program aimed at a constant of configuration 1
    other = next(i for i, r in enumerate(rows) if r[2] == 2 and r[3] == 1)
    _name, _n_ops, n_rel, _ops_off, rel_off, _n_slots = struct.unpack_from("<32sIIQQI", raw, cfg_at + 64 + PROG_SZ)
    assert n_rel > 0
    b = bytearray(raw)
    op, slot, _buf, _p, _off = struct.unpack_from(REL, raw, rel_off)
    struct.pack_into(REL, b, rel_off, op, slot, other, 0, 0)
    out["relocation-into-another-configuration"] = bytes(b)
    return out


def test_corrupt_version_2_images_are_refused(lib, exported, tmp_path):
    from marigold_amd import image, _lib as L
    multi, _singles = exported
    raw = open(multi["path"], "rb").read()
    words = {"truncated-configs": "short read (configuration table)", "scratch-beyond-region": "scratch region",
             "relocation-into-another-configuration": "of configuration 1"}
    broken = corrupt_images(raw)
    assert set(broken) == set(words)
    for name, data in broken.items():
        path = str(tmp_path / (name + ".mgimg"))
        open(path, "wb").write(data)
        assert not lib.mg_model_load(path.encode(), -1)
        msg = lib.mg_last_error().decode()
        assert msg.startswith("mg_model_load:") and words[name] in msg, (name, msg)
        with pytest.raises(L.MarigoldHipError, match="mg_model_load"):
            image.ModelImage(path, device=-1)
    # more of the same: a configuration count the file cannot hold, a slot in another configuration's buffer, an unknown kind
    cfg_at = struct.calcsize(HDR) + struct.calcsize(V2)
    buf_at = cfg_at + 4 * CFG_SZ
    rows = [struct.unpack_from(BUF, raw, buf_at + 24 * k) for k in range(multi["buffers"])]
    more = {}
    b = bytearray(raw)
    struct.pack_into("<I", b, struct.calcsize(HDR), 5)
    more["count"] = b
    b = bytearray(raw)
    struct.pack_into("<I", b, cfg_at + 64 + struct.calcsize("<32sIIQQI") + 4 + 24, next(i for i, r in enumerate(rows) if r[2] == 2 and r[3] == 2))
    more["slot"] = b
    b = bytearray(raw)
    struct.pack_into("<I", b, buf_at + 16, 4)
    more["kind"] = b
    b = bytearray(raw)
    struct.pack_into("<I", b, buf_at + 24 * next(i for i, r in enumerate(rows) if r[2] == 1) + 20, 4)
    more["owner"] = b
    for name, data in more.items():
        path = str(tmp_path / (name + ".mgimg"))
        open(path, "wb").write(bytes(data))
        assert not lib.mg_model_load(path.encode(), -1), name
        assert lib.mg_last_error().decode().startswith("mg_model_load:"), (name, lib.mg_last_error().decode())


def test_replica_accounting(lib, exported):
    from marigold_amd import image
    multi, singles = exported
    m = image.ModelImage(multi["path"], device=-1)
    m.select(1)
    r = m.replica()
    try:
        assert r.handle != m.handle and r.configs == m.configs
        assert r.shared_bytes == m.shared_bytes == multi["shared_bytes"] and r.device_bytes == m.device_bytes == multi["private_bytes"]
        assert _cfg(lib, r.handle) == m.configs[1] and (r.B, r.selected) == (2, 1)   # it starts where the parent stands
        r.select(3)
        assert _cfg(lib, m.handle) == m.configs[1]   # a handle's selection is its own
        m.close()                                    # the parent first: the replica goes on
        assert r.shared_bytes == multi["shared_bytes"] and lib.mg_model_num_configs(r.handle) == 4
        for i in range(4):
            r.select(i)
            r.validate()
            assert _cfg(lib, r.handle) == r.configs[i]
        assert r.find(height=128) == 2
        rr = r.replica()   # a replica of a replica, destroyed before it
        rr.validate()
        rr.close()
        r.validate()
    finally:
        m.close()
        r.close()
    # a version-1 image replicates too: nothing shared, everything its own
    s = image.ModelImage(singles[0]["path"], device=-1)
    t = s.replica()
    try:
        assert t.shared_bytes == 0 and t.device_bytes == s.device_bytes == sum(singles[0]["arena"].values())
        s.close()
        t.validate()
    finally:
        s.close()
        t.close()
    assert not lib.mg_model_replica(None) and lib.mg_last_error().decode().startswith("mg_model_replica:")


def test_header_and_bindings_declare_the_entry_points(lib):
    import re
    from marigold_amd import _lib as L
    hdr = " ".join(open(os.path.join(ROOT, "include", "marigold_hip.h")).read().split())
    for proto in ("int mg_model_num_configs(const mg_model* m);", "int mg_model_config_info(const mg_model* m, int index, int* cfg16);",
                  "int mg_model_find_config(const mg_model* m, int H, int W, int E, int steps, int K);", "int mg_model_select(mg_model* m, int index);",
                  "int mg_processed_size(int Hin, int Win, int processing_res, int* H, int* W);",
                  "long long mg_model_shared_bytes(const mg_model* m);", "mg_model* mg_model_replica(const mg_model* m);"):
        assert proto in hdr, proto
        assert re.match(r"[\w ]+?\*? ?(mg_\w+)\(", proto).group(1) in L.EXPORTS
    assert re.search(r"#define MG_ABI_VERSION 4\b", hdr) and L.ABI_VERSION == 4 and lib.mg_abi_version() == 4
