"""The bits of csrc/ensemble.hip's selection kernels: one SHA-256 per output buffer, over its raw bytes.  A plain helper module for
tests/test_gpu_ensemble_bits.py (not collected), with a ``__main__`` that writes the fixture tests/golden/ensemble_bits.json on a GPU.

The other tests hold parts of this arithmetic to a tolerance only (the fp32 mean / std of every kernel form) or compare two routes
through the same file with each other (MG_OP_ENS_IID above 32 members); the fixture holds every output bit of every kernel form, so
that a change of the file that is meant to move none can be seen to move none.

``cases()`` lists the launches:
  * MG_OP_ENS_DEPTH_MEDIAN: E in 1 ... 32 (the register forms: bounds 4, 8, 10, 16, 32), 33 and 128 (LDS), 129 (bitwise) x HW in
    1023 (one pixel per thread, a part-filled last workgroup), 1280 (four per thread) x median / mean x no ``st`` / scales / affine x
    (map + uncertainty) / neither (the optimiser's form); digests of the map, the uncertainty and the 2 + 2 E min / max table.
    One more with the members one float off a 16-byte boundary at HW = 1280 (one pixel per thread on a map of several workgroups).
  * MG_OP_ENS_IID: the same E, n in 1023, 1280, both reductions, with and without the uncertainty.
  * non-finite: E in 10, 40, 129, both ops: a NaN in one member at an interior element, +inf in another member at another.
Inputs come from ``numpy.random.default_rng`` (no dependence on the torch build): members are multiples of 1/64 in [0.5, 1.5) and
about a third of them copy another member (ties, zero deviations, plateaus of the extrema); scales in [0.5, 2), shifts in [-0.5, 0.5).

    python -m tests.ensemble_bits --write [PATH]     regenerate tests/golden/ensemble_bits.json (or PATH); needs the GPU
"""
import functools
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ensemble_bits.json")

SIZES = [1, 4, 5, 8, 10, 11, 16, 17, 32, 33, 128, 129]
LENGTHS = [1023, 1280]
NONFINITE_SIZES = [10, 40, 129]
SCRATCH_BYTES = 12288   # marigold_amd/ensemble.py: 512 blocks x (2 floats + 2 int64)


def cases():
    """[(label, op name, E, n, reduction, st form | None, outputs, nonfinite, misalign)]."""
    c = []
    for E in SIZES:
        for n in LENGTHS:
            for red in ("median", "mean"):
                for st in ("none", "scale", "affine"):
                    for outs in (True, False):
                        c.append((f"depth/E{E}/n{n}/{red}/{st}/{'maps' if outs else 'table'}", "depth", E, n, red, st, outs, False, 0))
                for outs in (True, False):
                    c.append((f"iid/E{E}/n{n}/{red}/{'unc' if outs else 'pred'}", "iid", E, n, red, None, outs, False, 0))
    c.append(("depth/E10/n1280/median/affine/maps/misaligned", "depth", 10, 1280, "median", "affine", True, False, 1))
    for E in NONFINITE_SIZES:
        for n in LENGTHS:
            for red in ("median", "mean"):
                c.append((f"depth/E{E}/n{n}/{red}/affine/maps/nonfinite", "depth", E, n, red, "affine", True, True, 0))
                c.append((f"iid/E{E}/n{n}/{red}/unc/nonfinite", "iid", E, n, red, None, True, True, 0))
    assert len({x[0] for x in c}) == len(c)
    return c


@functools.lru_cache(maxsize=None)
def inputs(E, n, nonfinite):
    """(members [E, n], st [2 E]) as fp32 numpy arrays (read-only)."""
    rng = np.random.default_rng(100000 * E + 10 * n + int(nonfinite))
    x = (rng.integers(32, 96, size=(E, n)) / 64.0).astype(np.float32)
    for e in range(E):
        src = int(rng.integers(0, E))
        if rng.random() < 1.0 / 3.0:
            x[e] = x[src]
    st = np.concatenate([rng.uniform(0.5, 2.0, E), rng.uniform(-0.5, 0.5, E)]).astype(np.float32)
    if nonfinite:
        x[E // 2, n // 3] = np.nan
        x[E - 1, (2 * n) // 3] = np.inf
    x.setflags(write=False)
    st.setflags(write=False)
    return x, st


def _sha(t):
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def run(lib, case):
    """One launch -> {buffer name: sha256 of its bytes}."""
    import torch
    from marigold_amd import ops as O
    _, op, E, n, red, st_form, outs, nonfinite, misalign = case
    x, st = inputs(E, n, nonfinite)
    hold = torch.empty(E * n + misalign, dtype=torch.float32, device="cuda")
    assert hold.data_ptr() % 16 == 0
    d = hold[misalign:].view(E, n)
    d.copy_(torch.tensor(x))
    reduction = 0 if red == "median" else 1
    got = {}
    if op == "depth":
        med = torch.empty(n, dtype=torch.float32, device="cuda") if outs else None
        mad = torch.empty(n, dtype=torch.float32, device="cuda") if outs else None
        mm = torch.zeros(2 + 2 * E, dtype=torch.float32, device="cuda")
        scratch = torch.zeros(SCRATCH_BYTES, dtype=torch.uint8, device="cuda")
        st_dev = None if st_form == "none" else torch.tensor(st).cuda()
        O.launch(O.ens_depth_median(d, st_dev, med, mad, mm, scratch, E=E, HW=n, reduction=reduction, has_shift=st_form == "affine"), lib=lib)
        if outs:
            got["map"], got["unc"] = _sha(med), _sha(mad)
        got["minmax"] = _sha(mm)
    else:
        pred = torch.empty(n, dtype=torch.float32, device="cuda")
        unc = torch.empty(n, dtype=torch.float32, device="cuda") if outs else None
        O.launch(O.ens_iid(d, pred, unc, E=E, n=n, reduction=reduction), lib=lib)
        got["map"] = _sha(pred)
        if outs:
            got["unc"] = _sha(unc)
    return got


def digests(lib):
    """{label: {buffer name: sha256}} of every case."""
    return {case[0]: run(lib, case) for case in cases()}


def main(argv):
    if argv[:1] == ["--write"] and len(argv) <= 2:
        from marigold_amd import _lib as L
        got = digests(L.init(0))
        path = argv[1] if len(argv) == 2 else FIXTURE
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in got.items()) + "\n}\n")   # (a case per line)
        print(f"{path}: {len(got)} cases, {sum(len(v) for v in got.values())} digests")
        return 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
