"""``map_images(images_per_program=k)`` on a real MI355X: the divisor form of MG_OP_IM2COL_SMALL against a torch gather,
each image's noise against its lone call, companion independence, outputs against the lone calls (tiny model: depth,
normals, IID; mixed sizes), the full-size latents against the lone engine call, and the CLI end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from marigold_amd import _lib
    _lib.init(0)
    return torch.device("cuda:0")


def _gens(seeds):
    return [torch.Generator(device="cuda:0").manual_seed(s) for s in seeds]


def _tiny(kind="depth", scheduler=None):
    import dataclasses
    import marigold_amd as M
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    ucfg = TINY_UNET
    if kind == "iid":   # 2 modalities: 12 -> 8 latent channels
        ucfg = dataclasses.replace(TINY_UNET, in_channels=12, out_channels=8)
    return M.build_synthetic_pipeline(kind, ucfg, TINY_VAE, scheduler=scheduler, default_denoising_steps=2,
                                      default_processing_resolution=0).to("cuda:0")


@pytest.mark.parametrize("B,H,W,C0,C1,Kp", [(6, 7, 13, 4, 4, 128), (6, 5, 9, 4, 8, 128), (4, 11, 3, 4, 12, 192)])
def test_im2col_small_members_per_src0_exact(dev, B, H, W, C0, C1, Kp):
    """Row b of the staging reads image b // E of an [B / E, C0, H, W] latent: bit-exact against a torch gather for
    E in {1, 3, B} (odd sizes)."""
    from marigold_amd import _lib, ops
    g = torch.Generator().manual_seed(B * 100 + H)
    for E in sorted({1, 3 if B % 3 == 0 else 2, B}):
        src0 = torch.randn(B // E, C0, H, W, generator=g)
        src1 = torch.randn(B, C1, H, W, generator=g)
        x = torch.cat([src0[torch.arange(B) // E], src1], dim=1)                    # the gather the kernel must not make
        cin = C0 + C1
        u = F.unfold(x, 3, padding=1).reshape(B, cin, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * cin)
        want = torch.zeros(B * H * W, Kp, dtype=torch.bfloat16)
        want[:, :9 * cin] = u.to(torch.bfloat16)
        col = torch.full((B * H * W, Kp), float("nan"), device=dev, dtype=torch.bfloat16)
        ops.launch(ops.im2col_small(src0.to(dev), src1.to(dev), col, B=B, H=H, W=W, C0=C0, C1=C1, Kp=Kp, members_per_src0=E),
                   lib=_lib.load())
        torch.cuda.synchronize()
        assert torch.equal(col.cpu(), want), f"E={E}"


@pytest.mark.parametrize("E,k,batch_size", [(1, 3, 0), (3, 2, 2), (2, 3, 4)])
def test_noise_is_each_images_lone_noise(dev, E, k, batch_size):
    """LCM (4 steps: initial latents + 3 step noises): the rows of image i in the shared programs are bitwise the draws of its
    lone call, including when batch_size splits the members (lone: per batch; shared: whole images or per image)."""
    from marigold_amd import synthetic as syn
    from marigold_amd.schedulers import LCMScheduler
    pipe = _tiny("depth", LCMScheduler())
    imgs = [syn.synthetic_image(32, 64, seed=s) for s in range(k)]
    kw = dict(denoising_steps=4, ensemble_size=E, processing_res=0, batch_size=batch_size, color_map=None,
              show_progress_bar=False)
    n_noise = 3
    lone_init, lone_nz = [], [[] for _ in range(n_noise)]
    draws = []
    base_randn = pipe._randn
    pipe._randn = lambda shape, g: draws.append(base_randn(shape, g)) or draws[-1]
    for im, g in zip(imgs, _gens(range(50, 50 + k))):
        draws.clear()
        pipe(im, generator=g, **kw)
        lone_init += draws[0::1 + n_noise]
        for s in range(n_noise):
            lone_nz[s] += draws[1 + s::1 + n_noise]
    pipe._randn = base_randn
    seen = []
    base_infer = pipe.single_infer
    pipe.single_infer = lambda rgb, T, g, pbar, lat, step_noises=None, **x: (
        seen.append((lat.clone(), [z.clone() for z in step_noises])) or base_infer(rgb, T, g, pbar, lat, step_noises=step_noises, **x))
    outs = list(pipe.map_images(imgs, generators=_gens(range(50, 50 + k)), images_per_program=k, in_flight=1, **kw))
    del pipe.single_infer
    assert len(outs) == k and len(seen) >= 1
    assert torch.equal(torch.cat([s[0] for s in seen]), torch.cat(lone_init))
    for s in range(n_noise):
        assert torch.equal(torch.cat([x[1][s] for x in seen]), torch.cat(lone_nz[s])), f"step noise {s}"


def test_companion_independence(dev):
    """Image A's map is bit-identical whether its program is shared with image B or with image C (same k, E): the UNet, the
    VAE and the ensembling have no reduction across images."""
    from marigold_amd import synthetic as syn
    pipe = _tiny("depth")
    A, B, C = (syn.synthetic_image(64, 128, seed=s) for s in (1, 2, 3))
    for E in (1, 2):
        kw = dict(denoising_steps=2, ensemble_size=E, processing_res=0, color_map=None, show_progress_bar=False)
        with_b = list(pipe.map_images([A, B], generators=_gens([7, 8]), images_per_program=2, in_flight=1, **kw))
        with_c = list(pipe.map_images([A, C], generators=_gens([7, 9]), images_per_program=2, in_flight=1, **kw))
        assert np.array_equal(with_b[0].depth_np, with_c[0].depth_np), f"E={E}"
        assert not np.array_equal(with_b[1].depth_np, with_c[1].depth_np)


def _depth_err(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt((d ** 2).mean())), float(np.abs(d).max())


# Tolerances against the lone calls (tiny model): the shared programs run the same kernels on a larger batch; members are
# independent, so differences are those of the launch forms a batch size picks (test_gpu_fullsize.py::test_768_properties
# holds a member inside a batch to rmse 5e-3 of the member alone; the same bound here).
RMSE_BOUND = 5e-3


@pytest.mark.parametrize("E", [1, 3])
def test_depth_against_lone_calls(dev, E):
    from marigold_amd import synthetic as syn
    pipe = _tiny("depth")
    imgs = [syn.synthetic_image(64, 128, seed=10 + s) for s in range(4)]
    kw = dict(denoising_steps=2, ensemble_size=E, processing_res=0, color_map="Spectral", show_progress_bar=False,
              ensemble_kwargs=dict(output_uncertainty=True) if E > 1 else None)
    alone = [pipe(im, generator=g, **kw) for im, g in zip(imgs, _gens(range(20, 24)))]
    for n in (1, 2):
        got = list(pipe.map_images(imgs, generators=_gens(range(20, 24)), images_per_program=4, in_flight=n, **kw))
        assert len(got) == 4
        for i, (a, b) in enumerate(zip(alone, got)):
            rmse, mx = _depth_err(a.depth_np, b.depth_np)
            print(f"[images_per_program] depth E={E} k=4 in_flight={n} image {i}: rmse {rmse:.2e} max {mx:.2e}")
            assert b.depth_np.shape == a.depth_np.shape and b.depth_colored.size == a.depth_colored.size
            assert rmse < RMSE_BOUND
            assert (a.uncertainty is None) == (b.uncertainty is None)


def test_normals_and_iid_against_lone_calls(dev):
    from marigold_amd import synthetic as syn
    imgs = [syn.synthetic_image(64, 128, seed=30 + s) for s in range(3)]
    pipe = _tiny("normals")
    kw = dict(denoising_steps=2, ensemble_size=3, processing_res=0, show_progress_bar=False)
    alone = [pipe(im, generator=g, **kw).normals_np for im, g in zip(imgs, _gens(range(3)))]
    got = [o.normals_np for o in pipe.map_images(imgs, generators=_gens(range(3)), images_per_program=3, **kw)]
    for i, (a, b) in enumerate(zip(alone, got)):
        ang = np.degrees(np.arccos(np.clip((a.astype(np.float64) * b).sum(0), -1, 1)))
        print(f"[images_per_program] normals E=3 k=3 image {i}: mean angle {ang.mean():.3f} deg, p99 {np.percentile(ang, 99):.3f}")
        assert ang.mean() < 1.0
    pipe = _tiny("iid")
    kw = dict(denoising_steps=2, ensemble_size=2, processing_res=0, show_progress_bar=False)
    alone = [pipe(im, generator=g, **kw) for im, g in zip(imgs, _gens(range(3)))]
    got = list(pipe.map_images(imgs, generators=_gens(range(3)), images_per_program=2, **kw))
    for i, (a, b) in enumerate(zip(alone, got)):
        assert b.is_complete
        for name in pipe.target_names:
            err = np.abs(a[name].array.astype(np.float64) - b[name].array)
            print(f"[images_per_program] IID E=2 k=2 image {i} {name}: mean {err.mean():.2e} max {err.max():.2e}")
            assert a[name].array.shape == b[name].array.shape and err.mean() < 6e-3


def test_two_sizes_keep_their_order(dev):
    from marigold_amd import synthetic as syn
    pipe = _tiny("depth")
    sizes = [(64, 128), (64, 128), (48, 96), (48, 96), (64, 128)]
    imgs = [syn.synthetic_image(h, w, seed=40 + s) for s, (h, w) in enumerate(sizes)]
    kw = dict(denoising_steps=2, ensemble_size=1, processing_res=0, color_map=None, show_progress_bar=False)
    alone = [pipe(im, generator=g, **kw).depth_np for im, g in zip(imgs, _gens(range(5)))]
    got = [o.depth_np for o in pipe.map_images(imgs, generators=_gens(range(5)), images_per_program=3, in_flight=2, **kw)]
    assert [g.shape for g in got] == [tuple(s) for s in sizes]
    for a, b in zip(alone, got):
        assert _depth_err(a, b)[0] < RMSE_BOUND


def test_full_size_latents_against_lone_engine_calls(dev):
    """768^2, k = 4 synthetic images, E = 1, 10 DDIM steps on the full SD-v2 UNet: each image's final latent from the shared
    programs (one encode of B = 4, one denoising program of 4 members with rgb_members = 1) against its lone engine call
    (encode B = 1, the broadcast program of one member), held to the bound test_gpu_fullsize.py holds the engine to against
    the fp32 oracle (LAT_REL_BOUND = 2e-2, relative rmse).  Measured on an MI355X: 3.49e-3 - 3.53e-3 for the four images (the
    batch of four takes other launch forms than one member alone; the tiny model's E = 1 maps come out bit-identical)."""
    from marigold_amd import synthetic as syn
    import marigold_amd as M
    pipe = M.build_synthetic_pipeline("depth").to("cuda:0")
    unet, vae = pipe.unet, pipe.vae
    unet.set_context(pipe.empty_text_embed)
    rgb = torch.cat([syn.synthetic_image(768, 768, seed=60 + s).float() / 255.0 * 2.0 - 1.0 for s in range(4)]).to(dev)
    lat0 = syn.synthetic_latents(4, 96, 96, seed=7).to(dev)
    prog = unet.denoise_program(4, 96, 96, pipe.scheduler, 10, rgb_members=1)
    prog.rgb_latent.copy_(vae.encode_rgb_latent(rgb))
    prog.x.copy_(lat0)
    prog.run()
    shared = prog.x.clone()
    for i in range(4):
        one = unet.denoise_program(1, 96, 96, pipe.scheduler, 10, rgb_broadcast=True)
        one.rgb_latent.copy_(vae.encode_rgb_latent(rgb[i:i + 1]))
        one.x.copy_(lat0[i:i + 1])
        one.run()
        ref = one.x.double()
        rel = float(((shared[i:i + 1].double() - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())
        print(f"[images_per_program] full size k=4 E=1 T=10 image {i}: final latent rmse/rms vs lone {rel:.3e}")
        assert rel < 2e-2


def test_cli_images_per_program(dev, tmp_path):
    """script/depth/run.py --images_per_program 4 on a synthetic checkpoint folder writes the files --images_per_program 1
    writes, with the same shapes and values within RMSE_BOUND."""
    from PIL import Image
    from marigold_amd import checkpoint as ck, cli, synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.schedulers import DDIMScheduler
    ckpt = str(tmp_path / "ckpt")
    ck.save_synthetic_checkpoint(ckpt, "MarigoldDepthPipeline", syn.synthetic_unet_state_dict(TINY_UNET),
                                 syn.synthetic_vae_state_dict(TINY_VAE), TINY_UNET, TINY_VAE, DDIMScheduler(),
                                 syn.synthetic_text_embedding(TINY_UNET.cross_attention_dim), scale_invariant=True,
                                 shift_invariant=True, default_denoising_steps=2, default_processing_resolution=0)
    src = tmp_path / "in"
    src.mkdir()
    for s, (h, w) in enumerate([(64, 128)] * 3 + [(48, 96)] + [(64, 128)] * 2):
        Image.fromarray(np.ascontiguousarray(syn.synthetic_image(h, w, seed=s)[0].permute(1, 2, 0).numpy())).save(src / f"im{s}.png")
    args = ["--checkpoint", ckpt, "--input_rgb_dir", str(src), "--processing_res", "0", "--seed", "5"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "script", "depth", "run.py")] + args +
                       ["--output_dir", str(tmp_path / "k4"), "--images_per_program", "4"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert cli.main("depth", args + ["--output_dir", str(tmp_path / "k1")]) == 0
    for sub in ("depth_npy", "depth_bw", "depth_colored"):
        names = sorted(os.listdir(tmp_path / "k1" / sub))
        assert len(names) == 6 and names == sorted(os.listdir(tmp_path / "k4" / sub)), sub
    for name in sorted(os.listdir(tmp_path / "k1" / "depth_npy")):
        a, b = np.load(tmp_path / "k1" / "depth_npy" / name), np.load(tmp_path / "k4" / "depth_npy" / name)
        assert a.shape == b.shape and _depth_err(a, b)[0] < RMSE_BOUND, name
