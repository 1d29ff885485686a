#!/usr/bin/env python
"""Pin the repository's restatement of the tiny autoencoder against diffusers' own ``AutoencoderTiny``, where diffusers imports.

Nothing is downloaded: the module is built from the config the engine accepts (config_check.TAESD_VAE_CONFIG) and loaded, strictly,
with the seeded weights of synthetic.synthetic_tiny_vae_state_dict.  Written to tests/golden/tiny_vae_diffusers.npz (a few kB; the
weights themselves are regenerated from the seed, the file keeps each tensor's sum to notice a generator that drifted): diffusers'
state-dict names and shapes, one small image and one small latent, and diffusers' ``encode(x).latents`` and ``decode(z).sample``
for them (fp32).
tests/test_tiny_vae_host.py::test_reference_pinned_against_diffusers holds tests/tiny_vae_reference.py - and through it the shape
table of arch.py - to the file; until the file exists that test skips with "unpinned against diffusers".

    python tools/pin_tiny_vae_against_diffusers.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    try:
        from diffusers import AutoencoderTiny
    except ImportError as e:
        print(f"diffusers does not import here ({e}); nothing written")
        return 1
    from marigold_amd.config_check import TAESD_VAE_CONFIG
    from marigold_amd.synthetic import synthetic_tiny_vae_state_dict
    seed = 20240
    cfg = {k: v for k, v in TAESD_VAE_CONFIG.items() if not k.startswith("_") and v is not None}
    model = AutoencoderTiny(**cfg).eval()
    weights = synthetic_tiny_vae_state_dict(seed=seed)
    model.load_state_dict(weights, strict=True)   # diffusers' own check of the 134 names and shapes
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        rgb = torch.rand(2, 3, 21, 34, generator=g) * 2 - 1
        latent = torch.randn(2, 4, 3, 5, generator=g)
        encoded = model.encode(rgb).latents
        decoded = model.decode(latent).sample
    sd = model.state_dict()
    names = sorted(sd)
    shapes = np.full((len(names), 4), -1, dtype=np.int64)
    for i, n in enumerate(names):
        shapes[i, :sd[n].dim()] = tuple(sd[n].shape)
    out = os.path.join(ROOT, "tests", "golden", "tiny_vae_diffusers.npz")
    np.savez_compressed(out, names=np.array(names), shapes=shapes, seed=np.int64(seed), sums=np.array([float(weights[n].double().sum()) for n in names]),
                        rgb=rgb.numpy(), latent=latent.numpy(), encoded=encoded.numpy(), decoded=decoded.numpy())
    print(f"wrote {out}: {len(names)} tensors, {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
