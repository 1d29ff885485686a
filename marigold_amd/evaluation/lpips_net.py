"""The weights of the LPIPS network (AlexNet's five convolutions and the five 1 x 1 "lin" layers), read from the two files a user
of torchvision / lpips / torchmetrics already has.  Nothing is downloaded and nothing is searched for: the paths are given, like the
checkpoint folder.  ``LpipsNet`` keeps the torch-layout host tensors for ``metrics.lpips`` and, after ``.to(device)``, fp32 device
copies packed once in the layout csrc/lpips.hip reads (``mg_lpips_net`` in include/marigold_hip.h)."""
import torch

from .metrics import LPIPS_CONVS

BACKBONE_LAYERS = (0, 3, 6, 8, 10)   # torchvision.models.alexnet: features.<i> of the five convolutions


def _backbone_key(layer, what):
    return f"features.{BACKBONE_LAYERS[layer]}.{what}"


def _lin_key(layer):
    return f"lin{layer}.model.1.weight"


def _take(sd, key, shape, source):
    if key not in sd:
        raise ValueError(f"LpipsNet: key '{key}' is missing from the {source}")
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"LpipsNet: key '{key}' of the {source} has shape {got}, expected {tuple(shape)}")
    return t.detach().to(dtype=torch.float32, device="cpu").contiguous()


class LpipsNet:
    """``conv_w[l]`` [Cout,Cin,k,k], ``conv_b[l]`` [Cout], ``lin_w[l]`` [1,Cout,1,1]: fp32 host tensors, l = 0..4."""

    def __init__(self, conv_w, conv_b, lin_w):
        self.conv_w, self.conv_b, self.lin_w = list(conv_w), list(conv_b), list(lin_w)
        self.device = None
        self._packed = None    # the device tensors, kept alive
        self._struct = None    # _lib.MgLpipsNet over them
        self._as_f64 = None

    @classmethod
    def from_state_dicts(cls, backbone, lin):
        """``backbone``: a torchvision AlexNet state dict (``features.{0,3,6,8,10}.{weight,bias}``; ``classifier.*`` and anything else
        is ignored); ``lin``: the lin layers' state dict (``lin{0..4}.model.1.weight``).  A missing key or a wrong shape is a
        ``ValueError`` that names the key."""
        conv_w, conv_b, lin_w = [], [], []
        for l, (cin, cout, k, _, _) in enumerate(LPIPS_CONVS):
            conv_w.append(_take(backbone, _backbone_key(l, "weight"), (cout, cin, k, k), "backbone state dict"))
            conv_b.append(_take(backbone, _backbone_key(l, "bias"), (cout,), "backbone state dict"))
            lin_w.append(_take(lin, _lin_key(l), (1, cout, 1, 1), "lin state dict"))
        return cls(conv_w, conv_b, lin_w)

    @classmethod
    def from_files(cls, backbone_path, lin_path):
        return cls.from_state_dicts(torch.load(backbone_path, map_location="cpu", weights_only=True),
                                    torch.load(lin_path, map_location="cpu", weights_only=True))

    def host(self, dtype=torch.float32):
        """(conv_w, conv_b, lin_w) as ``dtype`` host tensors in torch's layout."""
        if dtype == torch.float32:
            return self.conv_w, self.conv_b, self.lin_w
        if self._as_f64 is None or self._as_f64[0] != dtype:
            self._as_f64 = (dtype, tuple([t.to(dtype) for t in ts] for ts in (self.conv_w, self.conv_b, self.lin_w)))
        return self._as_f64[1]

    def to(self, device):
        """Upload fp32 copies in the kernels' layout (once per device): conv_w[l] as [k*k*Cin, Cout] with row (ky*k + kx)*Cin + ci.
        One device at a time, for the single-GPU, single-stream callers of this package: the copies are made on the stream that is
        current at the first use, and moving to another device replaces them - do that only when no launch on the earlier device
        is still queued."""
        from .. import _lib as L
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("LpipsNet.to: the device path needs a GPU (the host function takes the object as it is)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device == device:
            return self
        cw = [w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous().to(device) for w in self.conv_w]
        cb = [b.to(device) for b in self.conv_b]
        lw = [w.reshape(-1).contiguous().to(device) for w in self.lin_w]
        s = L.MgLpipsNet()
        for l in range(5):
            s.conv_w[l], s.conv_b[l], s.lin_w[l] = cw[l].data_ptr(), cb[l].data_ptr(), lw[l].data_ptr()
        self._packed, self._struct, self.device = (cw, cb, lw), s, device
        return self
