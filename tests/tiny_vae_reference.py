"""The tiny autoencoder (diffusers' AutoencoderTiny, TAESD layout) restated in fp64 torch on the CPU, from the layer list of
DESIGN.md "Tiny VAE" and nothing of the engine: a plain helper module for tests/test_gpu_tiny_vae.py, tests/test_tiny_vae_host.py
and tools/tiny_vae_bench.py.

``round_to`` (None, torch.bfloat16, torch.float16): the CPU emulation of the engine - the weights and every activation the engine
STORES between two launches are rounded to that type (the output of the first convolution, of every 64 -> 64 convolution after its
bias / residual / ReLU, never the mapped input or the last convolution's fp32 output); sums stay fp64.  None: the fp64 network.
"""
import torch

F = torch.nn.functional

POST_NONE, POST_DEPTH, POST_NORMALS, POST_UNIT = 0, 1, 2, 3

# diffusers' nn.Sequential indices, written out (the engine derives its own from arch.tiny_vae_layers; the host test compares them)
ENCODER = [(0, "conv_in"), (1, "block"), (2, "down"), (3, "block"), (4, "block"), (5, "block"), (6, "down"), (7, "block"),
           (8, "block"), (9, "block"), (10, "down"), (11, "block"), (12, "block"), (13, "block"), (14, "conv_out")]
DECODER = [(0, "conv_in"), (1, "relu"), (2, "block"), (3, "block"), (4, "block"), (5, "up"), (6, "conv"), (7, "block"), (8, "block"),
           (9, "block"), (10, "up"), (11, "conv"), (12, "block"), (13, "block"), (14, "block"), (15, "up"), (16, "conv"),
           (17, "block"), (18, "conv_out")]


def param_shapes():
    """The 134 tensors: name -> shape."""
    d = {}
    for half, layers, cin, cout in (("encoder", ENCODER, 3, 4), ("decoder", DECODER, 4, 3)):
        for i, kind in layers:
            n = f"{half}.layers.{i}"
            if kind == "conv_in":
                d[f"{n}.weight"], d[f"{n}.bias"] = (64, cin, 3, 3), (64,)
            elif kind == "conv_out":
                d[f"{n}.weight"], d[f"{n}.bias"] = (cout, 64, 3, 3), (cout,)
            elif kind == "block":
                for j in (0, 2, 4):
                    d[f"{n}.conv.{j}.weight"], d[f"{n}.conv.{j}.bias"] = (64, 64, 3, 3), (64,)
            elif kind in ("down", "conv"):
                d[f"{n}.weight"] = (64, 64, 3, 3)
    return d


def rounder(round_to):
    if round_to is None:
        return lambda t: t
    return lambda t: t.to(torch.float32).to(round_to).to(torch.float64)


def _run(sd, half, layers, x, rnd):
    w = {k: (rnd(v.double()) if k.endswith(".weight") else v.double()) for k, v in sd.items() if k.startswith(half + ".")}
    pending = None   # the first convolution's output is stored after the ReLU that follows it in the decoder
    for i, kind in layers:
        n = f"{half}.layers.{i}"
        if kind == "conv_in":
            x = F.conv2d(x, w[f"{n}.weight"], w[f"{n}.bias"], padding=1)
            pending = True
            if half == "encoder":
                x, pending = rnd(x), None
        elif kind == "relu":
            x = rnd(torch.relu(x))
            pending = None
        elif kind == "block":
            y = x
            for j in (0, 2):
                y = rnd(torch.relu(F.conv2d(y, w[f"{n}.conv.{j}.weight"], w[f"{n}.conv.{j}.bias"], padding=1)))
            x = rnd(torch.relu(F.conv2d(y, w[f"{n}.conv.4.weight"], w[f"{n}.conv.4.bias"], padding=1) + x))
        elif kind == "down":
            x = rnd(F.conv2d(x, w[f"{n}.weight"], None, stride=2, padding=1))
        elif kind == "up":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        elif kind == "conv":
            x = rnd(F.conv2d(x, w[f"{n}.weight"], None, padding=1))
        elif kind == "conv_out":
            x = F.conv2d(x, w[f"{n}.weight"], w[f"{n}.bias"], padding=1)
    assert pending is None
    return x


def encode(sd, rgb, round_to=None):
    """rgb [B,3,H,W] in [-1, 1] -> the scaled latent [B,4,h,w], fp64."""
    return _run(sd, "encoder", ENCODER, (rgb.double() + 1.0) / 2.0, rounder(round_to))


def tail(v, post):
    """The pipelines' pointwise tails on the [-1, 1]-space image v [B,3,H,W] (fp64), as MG_OP_POST_NCHW defines them."""
    if post == POST_DEPTH:
        return (v.mean(dim=1, keepdim=True).clip(-1.0, 1.0) + 1.0) / 2.0
    if post == POST_NORMALS:
        c = v.clip(-1.0, 1.0)
        return c / torch.linalg.vector_norm(c, dim=1, keepdim=True).clamp(min=1e-6)
    if post == POST_UNIT:
        return (v.clip(-1.0, 1.0) + 1.0) / 2.0
    return v


def decode_preclip(sd, z, round_to=None):
    """latent [B,4,h,w] -> the decoded image in [-1, 1] space before any tail, [B,3,8h,8w] fp64."""
    x = 3.0 * torch.tanh(z.double() / 3.0)
    return _run(sd, "decoder", DECODER, x, rounder(round_to)) * 2.0 - 1.0


def decode(sd, z, post=POST_NONE, round_to=None):
    return tail(decode_preclip(sd, z, round_to), post)


def conv_layer(x, w, bias=None, residual=None, stride=1, up2=False, relu=False):
    """One 64 -> 64 layer on fp64 NCHW operands (already rounded by the caller), unrounded: nearest x2 of the input, 3x3 / pad 1,
    + bias, + residual, ReLU.  -> (result, magnitude) where magnitude = conv(|x|, |w|) + |bias| + |residual|, the sum the test's
    accumulation-error bound is taken of."""
    if up2:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    y = F.conv2d(x, w, None, stride=stride, padding=1)
    mag = F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=1)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
        mag = mag + bias.abs().view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual
        mag = mag + residual.abs()
    if relu:
        y = torch.relu(y)
    return y, mag
