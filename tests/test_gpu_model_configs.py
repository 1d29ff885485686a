"""One model image of several configurations, and replicas of a loaded image, on a real MI355X: every result of a configuration
selected in a multi-configuration image equals (``np.array_equal``) what a single-configuration image of the same configuration
returns - today's code path, which tests/test_gpu_predict_out_c_host.py, test_gpu_predict_many_c_host.py and
test_gpu_predict_iid_c_host.py tie to the Python pipelines.  The programs and their launches are the same, so are the bits.

The models are the tiny synthetic ones of tests/test_gpu_predict_out_c_host.py, two steps.  The configurations run in the order
A, B, C, A, D on one handle: the second A catches a zeroed-state buffer another configuration wrote to, or a scratch overlay that
reaches into private data.  Replicas run from two host threads on two streams, switching configuration between pictures."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from tests import c_hosts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = dict(ensemble_size=1, height=64, width=128, denoising_steps=2, images_per_program=1)
B = dict(ensemble_size=2, height=64, width=128, denoising_steps=2, images_per_program=1)
C = dict(ensemble_size=1, height=128, width=64, denoising_steps=2, images_per_program=1)
D = dict(ensemble_size=1, height=64, width=128, denoising_steps=2, images_per_program=2)
DEPTH = {"A": A, "B": B, "C": C, "D": D}
SEEDS = {"A": (1 << 63) + 11, "B": 12, "C": (1 << 40) + 13, "D": 14}
JOIN_S = 120


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from marigold_amd import _lib as L
    return L.init(0)


@functools.lru_cache(maxsize=None)
def _tiny_pipe(kind, lcm=False):
    """``_tiny_pipe`` of tests/test_gpu_native_noise.py."""
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.schedulers import LCMScheduler
    ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8) if kind == "iid" else TINY_UNET
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=LCMScheduler() if lcm else None, default_denoising_steps=2,
                                      default_processing_resolution=0).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _u8(h, w, seed=5):
    from marigold_amd import synthetic as syn
    return syn.synthetic_image(h, w, seed=seed)[0].permute(1, 2, 0).contiguous().numpy()


@pytest.fixture(scope="module")
def table():
    from marigold_amd.util.image_util import colormap_lut_u8
    return colormap_lut_u8("Spectral")


def _np(ts):
    torch.cuda.current_stream().synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in ts)


def _run(mi, cfg, seed, lut, kind="depth"):
    """One prediction of the selected configuration ``cfg`` with everything the entry point can return, as numpy arrays: one picture
    of the configuration's own size and one seed (K = 2: ``predict_many`` of that picture and of a second, with the next seed)."""
    size = (cfg["height"], cfg["width"])
    u8 = torch.from_numpy(_u8(*size)).cuda()
    if kind == "iid":
        return _np(mi.predict_iid(u8, seed, pictures=True))
    kw = dict(lut=lut if kind == "depth" else None, u16=kind == "depth", picture=True)
    if cfg["images_per_program"] > 1:
        got = mi.predict_many([u8, torch.from_numpy(_u8(*size, seed=6)).cuda()], [seed, seed + 1], **kw)
    else:
        got = mi.predict_out(u8, seed, **kw)
    return _np(got[:4]) + (np.array(got[4]),)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w)
    assert np.isfinite(want[0]).all() and want[0].max() > want[0].min()


def _export(tmp, kind, lcm, configs, seeds):
    """The multi-configuration image of ``configs`` and, from each configuration's own single image, the result to expect
    (computed once, never modified) -> (path of the multi image, [expected...], lut)."""
    from marigold_amd import image
    from marigold_amd.util.image_util import colormap_lut_u8
    pipe = _tiny_pipe(kind, lcm)
    lut = torch.from_numpy(colormap_lut_u8("Spectral")).cuda()
    multi = str(tmp / "multi.mgimg")
    info = image.export_model_image(pipe, multi, configs=configs)
    assert len(info["configs"]) == len(configs)
    want = []
    for i, (cfg, seed) in enumerate(zip(configs, seeds)):
        path = str(tmp / f"single{i}.mgimg")
        image.export_model_image(pipe, path, **cfg)
        mi = image.ModelImage(path)
        try:
            want.append(_run(mi, cfg, seed, lut, kind))
        finally:
            mi.close()
        os.remove(path)
    return multi, want, lut


@pytest.fixture(scope="module")
def depth(lib, tmp_path_factory):
    multi, want, lut = _export(tmp_path_factory.mktemp("configs_depth"), "depth", False, list(DEPTH.values()), list(SEEDS.values()))
    return multi, dict(zip(DEPTH, want)), lut


def test_depth_configurations_in_the_order_a_b_c_a_d(lib, depth):
    from marigold_amd import image
    multi, want, lut = depth
    mi = image.ModelImage(multi)
    try:
        assert len(mi.configs) == 4 and mi.shared_bytes > 0
        first = {}
        for name in "ABCAD":
            cfg = DEPTH[name]
            i = mi.find(cfg["height"], cfg["width"], cfg["ensemble_size"], cfg["denoising_steps"], cfg["images_per_program"])
            assert i == list(DEPTH).index(name)
            mi.select(i)
            got = _run(mi, cfg, SEEDS[name], lut)
            _same(got, want[name])
            if name in first:   # the second A
                _same(got, first[name])
            first[name] = got
        # B has an uncertainty and an alignment report, the single-member configurations have neither
        assert want["B"][1] is not None and want["B"][4][1] >= 1 and want["A"][1] is None and want["D"][0].shape[0] == 2
        # the refusals act on the selected configuration, in their words: D takes its pictures through mg_model_predict_many only
        rc = lib.mg_model_predict_out(mi.handle, lut.data_ptr(), 1, 64, 128, 0, 0, 1, None, None, lut.data_ptr(), None, None, None, None, None)
        msg = lib.mg_last_error().decode()
        assert rc != 0 and msg.startswith("mg_model_predict_out:") and "use mg_model_predict_many" in msg, msg
        # the staged entry points follow the selection too: C's encoder takes C's picture
        mi.select(2)
        rgb = torch.rand(1, 3, 128, 64, device="cuda") * 2 - 1
        lat = mi.encode(rgb)
        torch.cuda.synchronize()
        one = image.ModelImage(multi).select(2)
        try:
            assert lat.shape == (1, 4, 16, 8) and torch.equal(lat, one.encode(rgb))
        finally:
            one.close()
    finally:
        mi.close()


def test_normals_two_configurations(lib, tmp_path):
    from marigold_amd import image
    cfgs = [dict(A), dict(C, ensemble_size=3)]
    multi, want, lut = _export(tmp_path, "normals", False, cfgs, [21, 22])
    mi = image.ModelImage(multi)
    try:
        for i in (0, 1, 0):
            _same(_run(mi.select(i), cfgs[i], 21 + i, lut, "normals"), want[i])
        assert want[0][0].shape == (3, 64, 128) and want[1][1] is not None and want[1][2] is None
    finally:
        mi.close()


def test_iid_one_and_two_members(lib, tmp_path):
    from marigold_amd import image
    cfgs = [dict(A), dict(B)]
    multi, want, lut = _export(tmp_path, "iid", False, cfgs, [31, 32])
    mi = image.ModelImage(multi)
    try:
        for i in (0, 1, 0):
            _same(_run(mi.select(i), cfgs[i], 31 + i, lut, "iid"), want[i])
        assert want[0][1] is None and want[1][1] is not None and want[0][2] is not None
    finally:
        mi.close()


def test_lcm_step_noise_slots_differ_per_configuration(lib, tmp_path):
    """An LCM image draws step noise into slots of its denoising program: one slot of [2,4,8,16] at T = 2 in the first configuration,
    two of [1,4,16,8] at T = 3 in the second."""
    from marigold_amd import image
    cfgs = [dict(B), dict(C, denoising_steps=3)]
    multi, want, lut = _export(tmp_path, "depth", True, cfgs, [41, 42])
    mi = image.ModelImage(multi)
    try:
        assert [c[8] for c in mi.configs] == [1, 2] and [c[5] for c in mi.configs] == [2, 3]
        for i in (0, 1, 0, 1):
            _same(_run(mi.select(i), cfgs[i], 41 + i, lut), want[i])
            assert mi.n_noise == i + 1
    finally:
        mi.close()


def test_replicas_on_two_streams_from_two_threads(lib, depth):
    from marigold_amd import image
    multi, want, lut = depth
    parent = image.ModelImage(multi)
    replica = parent.replica()
    private = parent.device_bytes
    assert replica.shared_bytes == parent.shared_bytes > 0 and replica.device_bytes == private
    orders = {"parent": "ABC", "replica": "CAB"}
    handles = {"parent": parent, "replica": replica}
    streams = {k: torch.cuda.Stream() for k in handles}
    got, errors = {k: [] for k in handles}, []
    barrier = threading.Barrier(2)

    def lane(who):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[who]):
                barrier.wait(JOIN_S)
                for name in orders[who]:
                    handles[who].select(list(DEPTH).index(name))
                    got[who].append(_run(handles[who], DEPTH[name], SEEDS[name], lut))
        except BaseException as e:   # noqa: BLE001
            errors.append((who, e))
            barrier.abort()

    try:
        threads = [threading.Thread(target=lane, args=(who,), daemon=True) for who in handles]
        for t in threads:
            t.start()
        for t in threads:
            t.join(JOIN_S)
            assert not t.is_alive(), "a lane did not finish"
        assert not errors, errors
        for who in handles:
            assert len(got[who]) == 3
            for name, g in zip(orders[who], got[who]):
                _same(g, want[name])
        # the parent goes first: the replica keeps the weights
        parent.close()
        replica.select(1)
        _same(_run(replica, B, SEEDS["B"], lut), want["B"])
        assert replica.shared_bytes > 0 and replica.device_bytes >= private
    finally:
        parent.close()
        replica.close()
    torch.cuda.synchronize()


# ---- the C host ----------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def host_sizes(tmp_path_factory):
    """examples/host_sizes.cpp, built as the ``host_picture`` fixture of tests/test_gpu_predict_out_c_host.py builds its example."""
    return c_hosts.build_example("host_sizes", tmp_path_factory.mktemp("host_sizes"))


def _pnm(path, magic, h, w, maxval, dtype, channels):
    raw = open(path, "rb").read()
    head = b"%s\n%d %d\n%d\n" % (magic, w, h, maxval)
    assert raw.startswith(head) and len(raw) == len(head) + np.dtype(dtype).itemsize * channels * h * w
    return np.frombuffer(raw[len(head):], dtype=dtype).reshape((h, w, channels) if channels > 1 else (h, w))


def test_c_host_sizes(lib, depth, host_sizes, tmp_path):
    """examples/host_sizes.cpp in a fresh process: three pictures whose processed sizes are 64 x 128, 128 x 64 and 64 x 128 (the
    third: 96 x 192 at processing resolution 128) through one image, every file against the pipeline's own output."""
    import marigold_amd as M
    from marigold_amd import image
    multi, _want, _lut = depth
    pipe = _tiny_pipe("depth")
    pictures = [((64, 128), 0, 51), ((128, 64), 0, 52), ((96, 192), 128, (1 << 63) + 53)]
    lut_path, prefix = str(tmp_path / "spectral.lut"), str(tmp_path / "out")
    image.export_color_table("Spectral", lut_path)
    args = [host_sizes, multi, "1", prefix, lut_path, "--"]
    for i, (size, res, seed) in enumerate(pictures):
        raw = str(tmp_path / f"image{i}.u8")
        _u8(*size, seed=7 + i).tofile(raw)
        args += [raw, str(size[0]), str(size[1]), str(res), str(seed)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    print("[host_sizes] " + (r.stdout + r.stderr).strip().replace("\n", " | "))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    for i, (size, res, seed) in enumerate(pictures):
        ref = pipe(Image.fromarray(_u8(*size, seed=7 + i)), denoising_steps=2, ensemble_size=1, processing_res=res, match_input_res=True,
                   resample_method="bilinear", generator=M.NativeNoise(seed), show_progress_bar=False)
        pre = f"{prefix}.{i}"
        pred = np.fromfile(pre + ".f32", dtype=np.float32).reshape(size)
        assert np.isfinite(ref.depth_np).all() and ref.depth_np.shape == size and np.array_equal(pred, ref.depth_np)
        u16 = _pnm(pre + ".pgm", b"P5", size[0], size[1], 65535, ">u2", 1).astype(np.uint16)
        assert np.array_equal(u16, (ref.depth_np * 65535.0).astype(np.uint16)) and u16.max() > u16.min()
        assert np.array_equal(_pnm(pre + ".ppm", b"P6", size[0], size[1], 255, np.uint8, 3), np.asarray(ref.depth_colored))
        assert not os.path.exists(pre + ".unc.f32")
    assert "configuration 0" in r.stdout and "configuration 2" in r.stdout
    # a picture the image has no configuration for is refused by name, with the sizes it holds
    r = subprocess.run(args[:6] + [args[6], "96", "128", "0", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "mg_model_find_config" in r.stderr and "64 x 128" in r.stderr, (r.stdout + r.stderr)[-2000:]
