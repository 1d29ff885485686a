"""Native Gaussian noise: MG_OP_RANDN (csrc/randn.hip) behind the pipelines' ``generator=`` argument.

``torch.Generator`` streams exist only where torch does.  The library's own generator is stateless - Philox4x32-10 + Box-Muller,
every value a function of (seed, stream, element index) alone - so a C host (``mg_model_predict``) and the Python pipelines draw
the same latents from the same seed.  The stream is unrelated to torch's: a map made with ``NativeNoise(seed)`` differs from the
``torch.Generator().manual_seed(seed)`` map by design.
"""
import torch

from . import _lib as L, ops as O

_MASK64 = (1 << 64) - 1


def native_randn(shape, seed, stream=0, offset=0, dtype=torch.float32, device=None):
    """Elements [offset, offset + numel) of stream ``stream`` of ``seed`` as a CUDA tensor of ``shape``: fp32, or bf16 / fp16 - the
    fp32 value rounded to nearest even in the store, through the library of that operand type.  A slice of a larger draw is that
    draw's slice, bit for bit."""
    if dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise ValueError(f"native_randn: dtype {dtype} is not fp32, bf16 or fp16")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError(f"native_randn: the generator is a HIP kernel, a CUDA device is required (got {device})")
    out = torch.empty(tuple(int(d) for d in shape), dtype=dtype, device=device)
    if out.numel():
        with torch.cuda.device(out.device):
            O.launch(O.randn(out, n=out.numel(), seed=int(seed) & _MASK64, stream=int(stream) & _MASK64, offset=int(offset),
                             out16=dtype != torch.float32), lib=L.load(dtype == torch.float16))
    return out


class NativeNoise:
    """What a pipeline takes as ``generator=`` in place of a ``torch.Generator``: the seed and the id of the next stream.  Every draw
    a pipeline makes takes one stream, from element 0 - the initial latents of a call stream 0, the LCM scheduler's step noises
    streams 1, 2, ... - in fp32, rounded to the pipeline's ``io_dtype`` in the store (``noise_dtype`` does not apply).
    ``mg_model_predict`` draws the same streams from the same seed."""

    def __init__(self, seed=0):
        self.manual_seed(seed)

    def manual_seed(self, seed):
        """Reset: the new seed, and stream 0 next.  Returns self, like ``torch.Generator.manual_seed``."""
        self.seed = int(seed) & _MASK64
        self.next_stream = 0
        return self

    def take_stream(self):
        """The id of the next stream; the one after it is next."""
        k = self.next_stream
        self.next_stream = k + 1
        return k

    def randn(self, shape, dtype=torch.float32, device=None):
        return native_randn(shape, self.seed, stream=self.take_stream(), dtype=dtype, device=device)

    def __repr__(self):
        return f"NativeNoise(seed={self.seed}, next_stream={self.next_stream})"
