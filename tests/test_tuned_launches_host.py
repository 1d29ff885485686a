"""tests/tuned_forms.py against the tuning table and the production programs, without a GPU: every entry belongs to exactly one
class, a class rebuilt at an entry's own M has that entry's key, and the fields the key does not carry are what the full-size
UNet / VAE programs really launch."""
import re

import pytest
import torch

from marigold_amd import _lib as L, ops as O, tuning
from tests import tuned_forms as TF

# integer fields that follow from B, H, W or the stride of the shape (ldt = tokens rounded up to 64; the address of the program's
# tickets - compared as set / not set)
SHAPE_FIELDS = {"b", "h", "w", "ho", "wo", "ldt", "tickets_lo", "tickets_hi"}


def test_every_entry_belongs_to_exactly_one_class():
    db = tuning.load()
    cls = TF.classes()
    owner = {}
    for c in cls:
        assert c.entries and len(c.entries) == len(c.labels)
        for key in c.entries:
            assert key not in owner, key
            owner[key] = c
            assert (c.rest, c.tile, c.splits) == TF.class_of(key)
    assert set(owner) == set(db)
    assert len({c.id for c in cls}) == len(cls), "class ids collide"
    # the GPU test's parameter list is classes() itself
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_tuned_launches.py")).read()
    assign = [n for n in ast.parse(src).body if isinstance(n, ast.Assign) and n.targets[0].id == "CLASSES"]
    assert len(assign) == 1 and ast.unparse(assign[0].value) == "TF.classes()"
    assert '@pytest.mark.parametrize("cls", CLASSES,' in src


def test_rebuilt_op_has_the_entry_key():
    db = tuning.load()
    for c in TF.classes():
        small = TF.build(c, None, None, dummy=True).op
        assert (O.Raw(small).variant, O.Raw(small).splits) == (c.tile, c.splits)
        ks = tuning.key_of(small).split(",")
        for key in c.entries:
            op = TF.build(c, int(key.split(",")[0]), None, dummy=True).op
            assert tuning.key_of(op) == key, (c.id, key, tuning.key_of(op))
            assert ks[1:] == key.split(",")[1:], (c.id, key, ",".join(ks))
            r = O.Raw(op)
            r.variant = r.splits = 0
            assert tuning.apply(op) is op and (r.variant, r.splits) == (db[key][0], db[key][1])


def test_reduced_launches_pass_their_kernels_contracts():
    """Every class at its reduced shape goes through the launcher's shape / alignment checks (mg_program_validate: no device)."""
    from marigold_amd import ops as O
    seq = O.OpSeq("tuned classes")
    for c in TF.classes():
        seq.add(TF.build(c, None, None, dummy=True).op, c.id)
    seq.validate()


def _production_ops():
    """[(op, label)] of the IGEMM launches of the UNet and VAE programs at 768^2, for every ensemble size the table names, with
    conv_shortcut folded into conv2 (the product) and as its own launch (what the table's stand-alone shortcut entries were swept on)."""
    from marigold_amd import routes as R
    from marigold_amd.arch import UNetConfig, VAEConfig, unet_param_shapes, vae_param_shapes
    from marigold_amd.modules import AutoencoderKLHIP, UNet2DConditionModelHIP
    from marigold_amd.schedulers import DDIMScheduler
    sizes = sorted({1, 2, 3, 5, 10} | {int(re.match(r"E=(\d+) ", lab).group(1)) for c in TF.classes() for lab in c.labels})
    ucfg, vcfg = UNetConfig(), VAEConfig()
    usd = {k: torch.zeros(s) for k, s in unet_param_shapes(ucfg).items()}
    vsd = {k: torch.zeros(s) for k, s in vae_param_shapes(vcfg).items()}
    found = []
    fold0 = R.FOLD_SHORTCUT
    try:
        for fold in (True, False):
            R.FOLD_SHORTCUT = fold
            unet = UNet2DConditionModelHIP(usd, ucfg).dry()
            unet.set_context(torch.zeros(1, 2, 1024))
            vae = AutoencoderKLHIP(vsd, vcfg).dry()
            seqs = [vae._program("encode", 1, 768, 768)[0]]
            for n in sizes:
                seqs += [unet.denoise_program(n, 96, 96, DDIMScheduler(), 1).seq, vae._program("decode", n, 96, 96, 1)[0]]
            for seq in seqs:
                found += [(op, lab, fold) for op, lab in zip(seq.ops, seq.labels) if op.kind == L.OP_IGEMM]
    finally:
        R.FOLD_SHORTCUT = fold0
    return found


def test_classes_agree_with_the_production_programs():
    db = tuning.load()
    by_key = {TF.class_of(k): c for c in TF.classes() for k in c.entries}
    rebuilt = {}
    reached, reached_folded, wrong = set(), set(), []
    for op, lab, fold in _production_ops():
        key = tuning.key_of(op)
        if key not in db or (O.Raw(op).variant, O.Raw(op).splits) != (db[key][0], db[key][1]):
            continue
        reached.add(key)
        if fold:
            reached_folded.add(key)
        c = by_key[TF.class_of(key)]
        if c.id not in rebuilt:
            rebuilt[c.id] = TF.build(c, None, None, dummy=True).op
        mine = rebuilt[c.id]
        rp, rm, names = O.Raw(op), O.Raw(mine), L.FIELDS[L.OP_IGEMM][1]["i"]
        di = [(n, getattr(rp, n), getattr(rm, n)) for n in names if n not in SHAPE_FIELDS and getattr(rp, n) != getattr(rm, n)]
        di += [(k, op.i[k], mine.i[k]) for k in range(len(names), len(op.i)) if op.i[k] != mine.i[k]]   # (the unnamed tail stays zero)
        di += [("tickets", "set", "not set")] if bool(O.igemm_tickets(op)) != bool(O.igemm_tickets(mine)) else []
        dp = [(k, bool(op.p[k]), bool(mine.p[k])) for k in range(len(op.p)) if bool(op.p[k]) != bool(mine.p[k])]
        df = [(k, op.f[k], mine.f[k]) for k in range(3) if op.f[k] != mine.f[k]]
        if di or dp or df:
            wrong.append(f"{lab} [{c.id}]: i {di} p {dp} f {df} (field, production, rebuilt)")
    assert not wrong, "\n".join(sorted(set(wrong)))
    unreached = [f"{k} ({db[k][4]})" for k in db if k not in reached]
    assert not unreached, "table entries no production program launches:\n" + "\n".join(unreached)
    # the entries the product itself (shortcuts folded) no longer reaches are the stand-alone conv_shortcut launches of the UNet
    # levels whose conv2 runs on the implicit GEMM - nothing else (docs/history/tuned_launch_parity.md lists them)
    stale = [k for k in db if k not in reached_folded]
    assert all(db[k][4].endswith(".conv_shortcut") and "vae." not in db[k][4] for k in stale), [f"{k} ({db[k][4]})" for k in stale]
