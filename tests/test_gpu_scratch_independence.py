"""No output depends on what a scratch buffer held before the run (tests/scratch_state.py), on a real MI355X: the tiny architecture's
three production programs without pool recycling, the harness itself on a planted read of unwritten scratch, and the scratch users
outside the programs that Python holds a handle to (the device scorer's workspaces, the depth aligner's buffers).  The
full-architecture cases live in tests/test_gpu_fullsize.py, next to the fixture that owns the full-size weights."""
import re
import time

import numpy as np
import pytest
import torch

from tests import scratch_cases as SC, scratch_state as SS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import TINY_UNET, TINY_VAE
    from marigold_amd.modules import AutoencoderKLHIP, UNet2DConditionModelHIP
    unet = UNet2DConditionModelHIP(syn.synthetic_unet_state_dict(TINY_UNET), TINY_UNET).to("cuda:0")
    unet.set_context(syn.synthetic_text_embedding(TINY_UNET.cross_attention_dim))
    return unet, AutoencoderKLHIP(syn.synthetic_vae_state_dict(TINY_VAE), TINY_VAE).to("cuda:0")


@pytest.mark.parametrize("case", SC.cases(SC.TINY_FRESH), ids=SC.case_id)
def test_tiny_programs_without_recycling(tiny, case):
    rep = SC.run_case(*tiny, case, recycle=False)
    assert rep["filled_bytes"] == rep["pool_bytes"] > 0


def _planted(dev, n=1000):
    """copy(x -> a); sched_step(out = x + b) with b a pool buffer nobody wrote: valid memory, undefined contents."""
    from marigold_amd import engine as E, ops as O
    from types import SimpleNamespace
    pool = E.Pool(dev)
    seq = O.OpSeq("planted read of unwritten scratch")
    x, out = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    seq.hold(x, out)
    a, b = pool.get(4 * n), pool.get(4 * n)
    seq.add(O.copy(x, a, 4 * n), "x->a")
    seq.add(O.sched_step(a, b, None, out, n=n, cx=1.0, cm=1.0), "sched_step(a, unwritten b)")
    module = SimpleNamespace(pool=pool, ws=SimpleNamespace(cache={}))
    return seq, module, SS.IO([(x, torch.linspace(-1, 1, n, device=dev))], [out]), b


def test_the_harness_reports_a_planted_read_of_unwritten_scratch():
    dev = torch.device("cuda", 0)
    from marigold_amd import _lib as L
    L.init(0)
    seq, module, io, b = _planted(dev)
    cls = SS.classify(seq, module, io)
    o0, n0 = SS.run_with_fill(seq, cls, 0x00)
    off, _ = SS.run_with_fill(seq, cls, 0xFF)
    assert n0 == module.pool.bytes == 2 * 4096
    assert torch.equal(o0[0], io.inputs[0][1]) and torch.isnan(off[0]).all() and not torch.equal(o0[0], off[0])
    assert SS.first_dependent_op(seq, cls) == 1
    with pytest.raises(SS.ContractError, match=r"first dependent op 1: 'sched_step\(a, unwritten b\)'"):
        SS.check_program(seq, module, io)
    # the same program with b written first is clean
    from marigold_amd import ops as O
    seq.ops.insert(1, O.memset(b, b.numel(), 0))
    seq.labels.insert(1, "b = 0")
    seq._prog = None
    SS.check_program(seq, module, io)
    assert SS.first_dependent_op(seq, SS.classify(seq, module, io)) is None


def test_the_localiser_on_a_production_program(tiny):
    """A clean denoising program shows no dependent op; the decoder with one GroupNorm pass pointed at a scale / shift buffer nobody
    wrote (a pool buffer of the same size: valid memory) fails, and the message names the pass' consumer: under 0x00 the pass writes x * 0 + 0 = all-zero bytes, under 0xFF NaN with an
    all-ones payload (bf16 0xFFFF) - each run's own fill, which the localiser cannot tell from unwritten - so the first op with a
    visibly dependent result is the convolution that reads it, one op later.  (The localiser also asks more than
    the contract does: the clean decoder's attention scores GEMM reads the K slack rows engine.vae_attention leaves unwritten and
    stores fill-dependent score columns that the softmax never reads - a later op than the planted one.)"""
    from marigold_amd import _lib as L, ops as O
    seq, m, io = SC.build(*tiny, ("denoise", 1, 5, 7), recycle=False)
    assert SS.first_dependent_op(seq, SS.classify(seq, m, io)) is None
    SS.check_program(seq, m, io, say=lambda s: None)   # (the localiser hands the zero state back: the program still passes)
    seq, m, io = SC.build(*tiny, ("decode", 1, 5, 7), recycle=False)
    k = next(i for i, op in enumerate(seq.ops) if op.kind == L.OP_GN_APPLY)
    r = O.Raw(seq.ops[k])
    r.ss = m.pool.get(r.b * 2 * r.c * 4)
    seq._prog = None
    with pytest.raises(SS.ContractError, match=rf"non-finite output with scratch fill 0xff; first dependent op {k + 1}: '{re.escape(seq.labels[k + 1])}' \(igemm\)"):
        SS.check_program(seq, m, io, say=lambda s: None)


# ------------------------------------------------------------------------------------------ scratch users outside the programs

def _bits(res):
    """A result dict / sequence as bytes: NaN compares by its bits."""
    vals = [res[k] for k in sorted(res)] if isinstance(res, dict) else list(res)
    return np.asarray(vals, dtype=np.float64).tobytes()


def _eval_workspaces():
    from marigold_amd.evaluation import device as DV
    return list(DV._workspaces.values()) + list(DV._act_workspaces.values())


def _scores():
    """{name: () -> result} of one small input per device scorer."""
    from marigold_amd import evaluation as EV
    from tests import lpips_cases as C
    rng = np.random.default_rng(5)
    H, W = 37, 53
    gt = rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    pred = (0.3 * gt + 0.7 + rng.normal(0, 0.05, (H, W))).astype(np.float32)
    mask = rng.uniform(size=(H, W)) > 0.2
    ng = rng.normal(size=(3, H, W)).astype(np.float32)
    ng /= np.linalg.norm(ng, axis=0, keepdims=True)
    npred = ng + rng.normal(0, 0.2, (3, H, W)).astype(np.float32)
    p, g, m = C.pair(35, 47, masked=True)
    net = C.net("live")
    return {
        "depth least squares": lambda: EV.score_depth(pred, gt, mask, alignment="least_square", min_depth=0.1, max_depth=10.0),
        "depth least squares, disparity, sub-sampled fit": lambda: EV.score_depth(pred, gt, mask, alignment="least_square_disparity", alignment_max_res=32),
        "normals": lambda: EV.score_normals(npred, ng, rounded=False),
        "iid psnr / ssim, up to scale": lambda: EV.score_iid(p, g, "shading", m),
        "iid psnr / ssim, plain, gamma": lambda: EV.score_iid(p, g, "albedo", None, gamma=2.2),
        "iid lpips": lambda: EV.score_iid(p, g, "shading", m, metrics=("psnr", "ssim", "lpips"), lpips=net),
    }


def test_device_scores_do_not_depend_on_their_workspaces():
    t0 = time.perf_counter()
    scores = _scores()
    first = {name: fn() for name, fn in scores.items()}
    ws = _eval_workspaces()
    from marigold_amd.evaluation import device as DV
    assert DV._workspaces and DV._act_workspaces, "the scorers' cached workspaces are what this test fills"
    for name, res in first.items():
        vals = [v for k, v in res.items() if not (k == "quantile" and "plain" in name)]   # (a plain target has no brightness quantile: NaN)
        assert np.isfinite(np.asarray(vals, dtype=np.float64)).all(), (name, res)
    for pattern in SS.PATTERNS:
        for name, fn in scores.items():
            n = SS.poison(ws, pattern)
            again = fn()
            assert _bits(again) == _bits(first[name]), (name, pattern, first[name], again)
    assert {t.data_ptr() for t in _eval_workspaces()} == {t.data_ptr() for t in ws}   # the same buffers throughout
    print(f"[scratch] device scorers: {len(scores)} scores x {len(SS.PATTERNS)} fills, {n} workspace bytes filled before every score, "
          f"{time.perf_counter() - t0:.2f} s")


def test_depth_alignment_does_not_depend_on_its_scratch():
    from marigold_amd import ensemble as ens
    t0 = time.perf_counter()
    E, H, W = 4, 32, 40
    g = torch.Generator().manual_seed(11)
    base = torch.rand(1, 1, H, W, generator=g)
    d = (base * torch.tensor([1.0, 2.5, 0.4, 1.7]).view(E, 1, 1, 1) + torch.tensor([0.0, 0.3, -0.1, 1.0]).view(E, 1, 1, 1)
         + 0.05 * torch.randn(E, 1, H, W, generator=g)).cuda()

    def bufs(al):
        b = al.backend
        return [b.scratch, b.mm, b.st]

    # the aligner's own handles: fill, minimise, compare
    al = ens.DepthAligner(d, True, True, "median", 0.02)
    p0 = al.init_param()
    ref = None
    for pattern in SS.PATTERNS:
        n = SS.poison(bufs(al), pattern)
        c, grad = al.cost_and_grad(p0)
        SS.poison(bufs(al), pattern)
        p, cost, nit = al.minimize_native(p0, 1e-6, 50)
        got = _bits([c, cost, nit]) + _bits(grad) + _bits(p)
        assert np.isfinite(p).all() and np.isfinite(cost)
        ref = ref or got
        assert got == ref, pattern
    # two ensemble_depth calls with the first call's buffers filled in between (the allocator hands the freed blocks to the second)
    out0, unc0, info0 = ens.ensemble_depth(d, output_uncertainty=True, return_info=True)
    assert torch.isfinite(out0).all() and torch.isfinite(unc0).all()
    info = info0
    for pattern in SS.PATTERNS:
        SS.poison(bufs(info["aligner"]), pattern)
        torch.cuda.synchronize()
        info = None
        out, unc, info = ens.ensemble_depth(d, output_uncertainty=True, return_info=True)
        assert torch.equal(out, out0) and torch.equal(unc, unc0), pattern
        assert _bits(info["param"]) == _bits(info0["param"]) and _bits([info["cost"], info["n_eval"]]) == _bits([info0["cost"], info0["n_eval"]])
    print(f"[scratch] depth aligner E={E} {H}x{W}: {n} bytes (scratch + pinned statistics) filled per call, {time.perf_counter() - t0:.2f} s")
