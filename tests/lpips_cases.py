"""What the LPIPS tests share (tests/test_lpips_host.py, tests/test_gpu_lpips.py): seeded synthetic weights under the key names of
torchvision's AlexNet and of the lpips package's lin layers, writers for the two files, image pairs, the host chain of
``compute_iid_metric`` up to the images LPIPS sees, and the fp64 reference (``metrics.lpips(..., dtype=torch.float64)``), computed
once per case and shared.

Two weight sets.  "live": He-scaled convolutions, biases N(0, 0.1), lin weights >= 0.  "dead": the same with biases N(-0.6, 0.1),
which switches whole positions off (every channel 0 after the ReLU) - the case the channel norm's eps exists for."""
import functools

import numpy as np
import torch

from marigold_amd.evaluation import LpipsNet, metrics as M

BACKBONE_LAYERS = (0, 3, 6, 8, 10)
BIAS_MEAN = {"live": 0.0, "dead": -0.6}
SIZES = ((31, 31), (31, 64), (35, 47), (64, 80), (97, 131), (231, 300))
UP_TO_SCALE = ("shading", "residual")


def state_dicts(kind, seed=0):
    """(backbone, lin) state dicts with the files' key names; the backbone carries ``classifier.*`` entries like the real file."""
    g = torch.Generator().manual_seed(seed)
    backbone, lin = {}, {}
    for l, (cin, cout, k, _, _) in enumerate(M.LPIPS_CONVS):
        std = (2.0 / (cin * k * k)) ** 0.5
        backbone[f"features.{BACKBONE_LAYERS[l]}.weight"] = torch.randn(cout, cin, k, k, generator=g) * std
        backbone[f"features.{BACKBONE_LAYERS[l]}.bias"] = BIAS_MEAN[kind] + 0.1 * torch.randn(cout, generator=g)
        lin[f"lin{l}.model.1.weight"] = torch.rand(1, cout, 1, 1, generator=g) * (2.0 / cout)
    backbone["classifier.1.weight"] = torch.randn(8, 16, generator=g)
    backbone["classifier.1.bias"] = torch.randn(8, generator=g)
    return backbone, lin


@functools.lru_cache(maxsize=None)
def net(kind):
    return LpipsNet.from_state_dicts(*state_dicts(kind))


def write_files(folder, kind="live"):
    """The two weight files as ``torch.save`` writes state dicts -> (backbone path, lin path)."""
    backbone, lin = state_dicts(kind)
    paths = str(folder / f"alexnet_{kind}.pth"), str(folder / f"lin_alex_{kind}.pth")
    torch.save(backbone, paths[0])
    torch.save(lin, paths[1])
    return paths


def pair(h, w, seed=0, masked=False):
    """g ~ U[0,1], p = clip(g + 0.1 n, 0, 1) as fp32 [3,h,w]; with ``masked`` a [3,h,w] bool mask that drops ~15 % of the pixels."""
    r = np.random.default_rng(1000 * h + w + seed)
    g = r.uniform(0, 1, (3, h, w)).astype(np.float32)
    p = np.clip(g + 0.1 * r.normal(size=g.shape), 0, 1).astype(np.float32)
    mask = np.broadcast_to(r.uniform(size=(1, h, w)) > 0.15, g.shape).copy() if masked else None
    return p, g, mask


GAMMA = {0: None, 1: 2.2, 3: (2.2, 1.0 / 2.2)}   # MG_IID_GAMMA_* -> score_iid's argument


def gamma_np(x, mode):
    """The conversions of script/iid/eval.py on fp32 arrays, as harness._score_iid applies them."""
    if mode & 1:
        x = x ** 2.2
    if mode & 2:
        x = x ** (1.0 / 2.2)
    return x.astype(np.float32)


def scored_images(pred, gt, target, mask):
    """The two [1,3,H,W] fp32 images LPIPS sees for this target: ``compute_iid_metric``'s chain (alignment scale and brightness map
    for an up-to-scale target, invalid elements -> 0), restated."""
    p, g = pred.astype(np.float32), gt.astype(np.float32)
    if target in UP_TO_SCALE:
        p = np.float32(M.compute_alignment_scale(p, g, mask)) * p
        p, g = M.quantile_map(p, g, mask)
    p = p[None] if p.ndim == 3 else p
    g = g[None] if g.ndim == 3 else g
    if mask is not None:
        p, g = np.where(mask[None], p, 0).astype(np.float32), np.where(mask[None], g, 0).astype(np.float32)
    return p, g


# per size: a plain and an up-to-scale target, each with and without a mask, and every gamma mode on both kinds of target
VARIANTS = (("albedo", False, 0), ("albedo", True, 1), ("shading", False, 3), ("shading", True, 0), ("albedo", True, 3),
            ("shading", False, 1))


def cases():
    """Every (size, target, masked, gamma mode) of the device test."""
    return [(hw,) + v for hw in SIZES for v in VARIANTS]


def case_inputs(hw, target, masked, gamma_mode):
    """(pred, gt, mask) as the caller hands them to the scorer (gamma not yet applied) for one case."""
    return pair(hw[0], hw[1], masked=masked)


@functools.lru_cache(maxsize=None)
def host_terms(kind, hw, target, masked, gamma_mode, f64):
    """The host function's five terms for one case (fp64: the reference; fp32: what D is measured on), computed once."""
    p, g, mask = case_inputs(hw, target, masked, gamma_mode)
    ps, gs = scored_images(gamma_np(p, gamma_mode), gamma_np(g, gamma_mode), target, mask)
    return tuple(M.lpips_terms(ps, gs, net(kind), torch.float64 if f64 else torch.float32))


def total(terms):
    return (((terms[0] + terms[1]) + terms[2]) + terms[3]) + terms[4]


TERM_FLOOR = 0.01


def rel_dev(got, want):
    """Largest deviation over the total and the five terms, each relative to max(|reference|, TERM_FLOOR * |reference total|): a tap
    that carries at least 1 % of the case's score is held relatively (every tap of the "live" set does, the tests assert it); a
    smaller one - a map of positions that are nearly switched off, where f / sqrt(eps + |f|^2) turns the rounding of a cancelled
    sum into a large relative error of next to nothing - is held against 1 % of the score, so that it cannot set the scale for the
    others.  A term that is exactly 0 in the reference (every position dead) must be exactly 0."""
    floor = TERM_FLOOR * abs(total(want))
    worst = 0.0
    for a, b in zip([total(got)] + list(got), [total(want)] + list(want)):
        worst = max(worst, abs(a - b) / max(abs(b), floor) if b != 0 else (0.0 if a == 0 else float("inf")))
    return worst


def enlarge_iid_sample(folder, hw=(36, 44)):
    """Rewrite the rasters of ``write_synthetic_datasets``' Hypersim IID sample (24 x 32, below LPIPS's 31 x 31) at ``hw``: the same
    files, names and distributions."""
    import os
    from PIL import Image
    r = np.random.default_rng(7)
    h, w = hw
    alb = r.uniform(0, 1, (h, w, 3)).astype(np.float32)
    alb[:3, :4] = 0
    arrays = {"albedo": alb, "shading": r.gamma(2.0, 0.5, (h, w, 3)).astype(np.float32),
              "residual": r.gamma(1.0, 0.2, (h, w, 3)).astype(np.float32)}
    folder = str(folder)
    for name, a in arrays.items():
        path = os.path.join(folder, "ai", f"{name}_cam_00_fr0000.npy")
        assert os.path.exists(path)
        np.save(path, a)
    Image.fromarray(r.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(folder, "ai", "rgb_cam_00_fr0000.png"))


def dead_positions(kind, case):
    """Per image of one case, (all-zero positions, positions) of the last tap - in fp64, on the images LPIPS sees."""
    hw, target, masked, gamma_mode = case
    p, g, mask = case_inputs(*case)
    out = []
    for x in scored_images(gamma_np(p, gamma_mode), gamma_np(g, gamma_mode), target, mask):
        f5 = M.lpips_features(x, net(kind), torch.float64)[4]
        out.append((int((f5.abs().sum(dim=1) == 0).sum()), f5.shape[-2] * f5.shape[-1]))
    return out


def noisy_predictions(sample, targets):
    """Stand-in predictions for a dataset sample: the ground truth scaled (0.9 for albedo, 0.5 for the up-to-scale targets) plus
    noise, kept >= 0 (and <= 1 for albedo, which is scored as it stands)."""
    r = np.random.default_rng(11)
    out = {}
    for t in targets:
        x = np.nan_to_num(sample[t]) * (0.9 if t == "albedo" else 0.5) + 0.05 * r.normal(size=sample[t].shape)
        out[t] = np.clip(x, 0, 1 if t == "albedo" else None).astype(np.float32)
    return out
