"""When a resampled image of csrc/resize.hip counts as torch's: one rule for every test that holds the kernels against the host branch
of ``marigold_amd.util.image_util.resize`` (torch on the CPU; uint8 computed in fp32, bicubic clamped, ``round()``).

* fp32 data in [-1, 1]: ``max|got - ref| < 2e-5`` (the bound of ``test_resize_vs_torch_cpu``).
* nearest-exact: ``torch.equal``.
* uint8 data: no byte differs by more than 1; the unrounded fp32 reference value of every differing byte lies within
  ``255 * 2e-5 = 5.1e-3`` of a half-integer (the fp32 bound on the byte range: only a value that close to a tie may round the other
  way); differing bytes stay under 2e-3 of all outputs, counted over a whole test by a ``Tally`` (a 3-element output cannot carry a
  share).

An output buffer filled by ``prefill`` before the launch cannot pass in an element the kernel did not write: NaN for fp32, the
reference byte with its top bit flipped (128 away) for uint8.
"""
import torch
import torch.nn.functional as F

FP32_BOUND = 2e-5
HALF_BOUND = 255 * 2e-5
SHARE_CAP = 2e-3


def host_resize(x, size, mode):
    """The reference: the host branch of ``resize`` on the CPU tensor ``x`` (a copy when the size already matches)."""
    from marigold_amd.util.image_util import InterpolationMode, resize
    assert not x.is_cuda
    return resize(x, size, InterpolationMode(mode))


def unrounded(x_u8, size, mode):
    """The fp32 value the host branch rounds to a byte: ``F.interpolate`` on the float copy, bicubic clamped."""
    y = F.interpolate(x_u8.to(torch.float32), size=tuple(size), mode=mode, align_corners=False, antialias=True)
    return y.clamp(0, 255) if mode == "bicubic" else y


def prefill(ref):
    """What the output buffer holds before the launch (on the host; same shape and type as ``ref``)."""
    if ref.dtype == torch.uint8:
        return ref ^ 0x80
    return torch.full_like(ref, float("nan"))


class Tally:
    """Worst figures and the share of differing bytes over one test."""

    def __init__(self, name):
        self.name, self.worst, self.flips, self.outputs, self.half = name, 0.0, 0, 0, 0.0

    def line(self):
        return (f"[resample] {self.name}: worst fp32 difference {self.worst:.2e}, differing bytes {self.flips} of {self.outputs}, "
                f"worst distance of one from a half {self.half:.2e}")

    def close(self):
        print(self.line())
        if self.outputs:
            assert self.flips < SHARE_CAP * self.outputs, self.line()


def accept(got, ref, x, size, mode, tally, tag=""):
    """``got`` (on the host) against ``ref = host_resize(x, size, mode)``."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == x.dtype, tag
    if mode == "nearest-exact":
        assert torch.equal(got, ref), (tag, int((got != ref).sum()))
        return
    if x.dtype != torch.uint8:
        d = float((got - ref).abs().max())
        tally.worst = max(tally.worst, d) if d == d else d
        assert d < FP32_BOUND, (tag, d)      # (a NaN fails it)
        return
    d = (got.int() - ref.int()).abs()
    differ = d > 0
    tally.outputs += d.numel()
    if not bool(differ.any()):
        return
    assert int(d.max()) <= 1, (tag, int(d.max()), int((d > 1).sum()))
    u = unrounded(x, size, mode)[differ].double()
    half = float(((u - torch.floor(u)) - 0.5).abs().max())
    tally.flips += int(differ.sum())
    tally.half = max(tally.half, half)
    assert half <= HALF_BOUND, (tag, half)
