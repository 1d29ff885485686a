"""Op-by-op shadow run of a production program on a real MI355X: every launch of the AutoencoderKL encoder program at 768^2
(seeded synthetic weights, a synthetic image) replayed alone (``seq.run_range(i, 1)``), its inputs cloned on the device before
it runs, its outputs checked against the float64 reference of tests/op_reference.py.  One parity line per op; the first op
out of bounds stops the program there and names its index and label.  ``MARIGOLD_SHADOW_TABLE=<path>`` also writes the table
(the per-layer location of the encoder's error; profiles/shadow_vae_encode_768.tsv)."""
import os

import pytest
import torch

from tests import op_reference as R

pytestmark = pytest.mark.gpu


def _shadow(seq, resolve, title, f16=False):
    table = []
    for idx, (op, lab) in enumerate(zip(seq.ops, seq.labels)):
        spec = R.decode(op, resolve, lab, f16)
        inputs = R.load_inputs(spec, resolve)
        seq.run_range(idx, 1)
        torch.cuda.synchronize()
        for nm, kind, mx, rm in R.check_op(spec, inputs, R.read_outputs(spec, resolve), f16):
            shape = "x".join(str(s) for s in spec.writes[nm].shape)
            line = f"{idx}\t{lab}\t{spec.name}\t{nm}\t{shape}\t{mx:.3e}\t{rm:.3e}"
            print(f"[shadow] {title} " + line.replace("\t", "  "))
            table.append(line)
            ok = mx <= R.MAX_REL_BOUND and rm <= R.RMS_BOUND[kind]
            assert ok, (f"{title}: op {idx} '{lab}' ({spec.name}, {nm}): max|err|/max|ref| {mx:.3e} (bound {R.MAX_REL_BOUND}), "
                        f"rmse/rms {rm:.3e} (bound {R.RMS_BOUND[kind]:.1e}) - program stopped here")
    return table


def test_vae_encode_768_shadow():
    from marigold_amd import synthetic as syn
    from marigold_amd.arch import VAEConfig
    from marigold_amd.modules import AutoencoderKLHIP
    cfg = VAEConfig()
    vae = AutoencoderKLHIP(syn.synthetic_vae_state_dict(cfg), cfg).to("cuda:0")
    seq, inp, _ = vae._program("encode", 1, 768, 768)
    inp.copy_((syn.synthetic_image(768, 768, seed=0).float() / 255.0 * 2.0 - 1.0).reshape(inp.shape))
    resolve = R.make_resolver([seq.keep, vae.ws.cache, vae.pool.all])
    table = _shadow(seq, resolve, "vae.encode 768^2")
    assert len({ln.split("\t")[0] for ln in table}) == len(seq.ops)
    path = os.environ.get("MARIGOLD_SHADOW_TABLE")
    if path:
        with open(path, "w") as fh:
            fh.write("op\tlabel\tkind\toutput\tshape\tmax_err/max_ref\trmse/rms\n" + "\n".join(table) + "\n")
