"""The device scorer of intrinsic images, the parts that need no GPU: the C ABI (header, binding, both libraries), the new op
kinds, their contracts through the library's dry run, and the refusal to run without a GPU."""
import os
import re

import numpy as np
import pytest

from marigold_amd import _lib as L, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "marigold_hip.h")).read()


def test_abi_symbol_in_header_binding_and_libraries():
    assert re.search(r"\bint mg_eval_iid\(", _header())
    assert "mg_eval_iid" in L.EXPORTS
    for f16 in (False, True):
        assert hasattr(L.load(f16), "mg_eval_iid"), f16
    assert L.load().mg_eval_iid.argtypes is not None and len(L.load().mg_eval_iid.argtypes) == 11


def test_op_kinds_and_enums_match_the_header():
    header = _header()
    kinds = dict(re.findall(r"(MG_OP_IIDSCORE_\w+) = (\d+)", header))
    assert kinds == {"MG_OP_IIDSCORE_PREP": str(L.OP_IIDSCORE_PREP), "MG_OP_IIDSCORE_PSNR": str(L.OP_IIDSCORE_PSNR),
                     "MG_OP_IIDSCORE_SSIM": str(L.OP_IIDSCORE_SSIM)}
    every = [int(n) for n in re.findall(r"^\s*MG_OP_\w+ = (\d+)", header, flags=re.M)]
    assert len(every) == len(set(every))   # additive: on unused numbers
    for k in kinds:
        assert L.OP_NAMES[int(kinds[k])] == k[len("MG_OP_"):].lower()
    gam = dict(re.findall(r"(MG_IID_GAMMA_\w+) = (\d+)", header))
    assert [int(gam[k]) for k in ("MG_IID_GAMMA_NONE", "MG_IID_GAMMA_2_2", "MG_IID_GAMMA_INV_2_2", "MG_IID_GAMMA_BOTH")] == \
        [L.IID_GAMMA[None], L.IID_GAMMA[2.2], L.IID_GAMMA[1.0 / 2.2], L.IID_GAMMA[(2.2, 1.0 / 2.2)]]
    met = dict(re.findall(r"(MG_IID_(?:PSNR|SSIM)) = (\d+)", header))
    assert {k[len("MG_IID_"):].lower(): int(v) for k, v in met.items()} == L.IID_METRICS


def test_gamma_modes_are_matched_with_a_tolerance():
    assert [L.iid_gamma_mode(g) for g in (None, 2.2, np.float32(2.2), 1 / 2.2, 0.4545, np.float64(0.45454545), [2.2], (2.2, 0.4545))] == \
        [0, 1, 1, 2, 2, 2, 1, 3]
    for bad in (2.0, 1.0, 0.5, (1 / 2.2, 2.2), (2.2, 2.2), ()):
        with pytest.raises(ValueError, match="gamma"):
            L.iid_gamma_mode(bad)


def test_op_contracts_dry_run():
    """mg_program_validate runs each launcher's checks without touching a device."""
    a = 0x10000   # fake, aligned device addresses
    seq = ops.OpSeq("iid")
    seq.add(ops.iidscore_prep(a, a, a, a, a, H=120, W=200, gamma=2.2))
    seq.add(ops.iidscore_prep(a, a, None, a, a, H=1, W=7))             # no window: any size
    seq.add(ops.iidscore_psnr(a, a, a, a, a, H=120, W=200, gamma=1.0 / 2.2, up_to_scale=True))
    seq.add(ops.iidscore_psnr(a, a, None, a, a, H=3, W=3, write_psnr=False))
    seq.add(ops.iidscore_ssim(a, a, None, a, a, H=11, W=11, gamma=(2.2, 1.0 / 2.2)))
    seq.add(ops.iidscore_ssim(a, a, a, a, a, H=768, W=768, up_to_scale=True))
    seq.validate()
    odd_gamma = ops.iidscore_psnr(a, a, a, a, a, H=16, W=16)
    ops.Raw(odd_gamma).gamma = 4
    for op, msg in ((ops.iidscore_ssim(a, a, a, a, a, H=10, W=64), "H, W >= 11 required"),
                    (ops.iidscore_ssim(a, a, a, a, a, H=64, W=10), "H, W >= 11 required"),
                    (ops.iidscore_prep(a, None, a, a, a, H=16, W=16), "null"),
                    (ops.iidscore_psnr(a, a, a, None, a, H=16, W=16), "null"),
                    (ops.iidscore_ssim(a, a, a, a, None, H=16, W=16), "null"),
                    (ops.iidscore_psnr(a, a, a, a + 4, a, H=16, W=16), "8-byte aligned"),
                    (ops.iidscore_prep(a + 2, a, a, a, a, H=16, W=16), "4-byte aligned"),
                    (ops.iidscore_psnr(a, a, a, a, a, H=0, W=16), "bad size"),
                    (ops.iidscore_ssim(a, a, a, a, a, H=40000, W=40000), "bad size"),
                    (odd_gamma, "gamma mode")):
        s = ops.OpSeq("bad")
        s.add(op)
        with pytest.raises(L.MarigoldHipError, match=msg):
            s.validate()
    lib = L.load()
    for args, msg in (((a, a, None, 10, 64, 0, 0, 3, a, a, None), b"H, W >= 11 required"),
                      ((a, None, None, 16, 16, 0, 0, 3, a, a, None), b"null"),
                      ((a, a, None, 16, 16, 0, 0, 4, a, a, None), b"metrics mask"),
                      ((a, a, None, 16, 16, 0, 0, 3, a + 4, a, None), b"aligned")):
        assert lib.mg_eval_iid(*args) != 0
        assert msg in lib.mg_last_error(), (args, lib.mg_last_error())


def test_no_gpu_no_score(monkeypatch):
    import torch
    from marigold_amd import evaluation as EV
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = np.zeros((3, 16, 16), np.float32)
    with pytest.raises(RuntimeError, match="no MI355X visible"):
        EV.score_iid(x, x, "albedo")
    with pytest.raises(RuntimeError, match="no MI355X visible"):
        EV.score_iid_sample({"albedo": x}, {"albedo": x}, ["albedo"], metrics=("psnr",), use_mask=False, linear_targets=(),
                            dataset_name="x")
    # nothing to score needs no device: the row of a sample whose every target is missing
    assert EV.score_iid_sample({}, {}, ["albedo", "shading"], metrics=("psnr", "ssim"), use_mask=True, linear_targets=(),
                               dataset_name="x") == [None] * 4
