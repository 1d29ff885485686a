"""The contract behind every production program: an op may read only bytes that an earlier op of the same program wrote, a weight,
an input, or zero state.  The pooled buffers are ``torch.empty`` bytes recycled along the program order (engine.Pool), so an op
that reads a pad column, a slack row or a ragged tile it never wrote computes with whatever the last owner left there.

A plain helper module for the tests (no GPU code of its own; everything runs on CPU tensors too):

  ``classify(seq, module, io)``   every tensor the program can reach in one of four classes - scratch (``module.pool.all``), zero
                                  state (held tensors named by ``seq.zero_state``), constants (``module.ws.cache`` and the other held
                                  tensors), I/O slots - and every non-null pointer of every op (the ticket address of an
                                  MG_OP_IGEMM included) resolved into exactly one of them, or an error that names the op's label.
  ``poison(tensors, pattern)``    whole buffers filled byte-wise: a byte value, or ``"random"`` (seeded).
  ``run_with_fill(...)``          scratch and the output slots filled, the inputs copied in, one run, clones of the outputs.
  ``checksums(tensors)``          per tensor (sum, index-weighted sum) of its bytes read as int32, in int64.
  ``first_dependent_op(...)``     the failure localiser: the program replayed one op at a time from 0x00- and from 0xFF-filled
                                  scratch; the first op after which a byte differs between the two replays and is, in either, not
                                  that replay's fill (the outputs are filled with another byte than the scratch, so a plain copy of
                                  unwritten scratch into an output shows as well).
"""
import bisect
from dataclasses import dataclass, field

import torch

from marigold_amd import _lib as L, ops as O

SCRATCH, ZERO, CONST, IO_SLOT = "scratch", "zero state", "constants", "I/O"
# 0xFF: NaN as bf16, fp16 and fp32, -1 as an integer; 0x7F: a finite 3.4e38 as bf16 and fp32 (additive use overflows)
PATTERNS = (0x00, 0xFF, 0x7F, "random")
FORM_FIELDS = ("epi", "taps", "stride", "form", "waves", "nsplit", "subpix", "silu", "post", "vt_perm", "split", "mode")


class ContractError(AssertionError):
    pass


@dataclass
class IO:
    """``inputs``: [(slot, value)] copied in before every run; ``outputs``: the slots a run leaves its results in (a slot may be both)."""
    inputs: list
    outputs: list

    def slots(self):
        return _unique([s for s, _ in self.inputs] + list(self.outputs))

    def pure_inputs(self):
        out = {t.data_ptr() for t in self.outputs}
        return [s for s, _ in self.inputs if s.data_ptr() not in out]


@dataclass
class Classes:
    scratch: list
    zero: list
    cache: list          # module.ws.cache: the weights
    held: list           # the other held tensors (tables the program's prologue writes, slots no op names)
    io: IO
    op_ptrs: list = field(default_factory=list)   # per op: [(slot name, class, tensor)]
    tables: list = field(default_factory=list)    # the held tensors some op names as its ``out``: torch.empty tables the prologue writes

    def mutable(self):
        return _unique(self.scratch + self.zero + self.io.slots() + self.held)


def _flat(x):
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from _flat(y)
    elif isinstance(x, dict):
        for y in x.values():
            yield from _flat(y)


def _unique(tensors):
    seen, out = set(), []
    for t in tensors:
        if t.numel() and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            out.append(t)
    return out


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


class _Spans:
    """ptr -> every (class, tensor) whose span holds it (the span logic of image.export_model_image / op_reference.make_resolver,
    with a bisect in place of the scan: a full-size program has thousands of pointers)."""

    def __init__(self, by_class):
        self.spans = sorted(((*_span(t), cls, t) for cls, ts in by_class.items() for t in ts), key=lambda s: s[:2])
        self.lo = [s[0] for s in self.spans]
        self.hi_max, m = [], 0
        for s in self.spans:
            m = max(m, s[1])
            self.hi_max.append(m)

    def hits(self, ptr):
        out = []
        k = bisect.bisect_right(self.lo, ptr) - 1
        while k >= 0 and self.hi_max[k] > ptr:
            lo, hi, cls, t = self.spans[k]
            if lo <= ptr < hi:
                out.append((cls, t))
            k -= 1
        return out


def pointer_slots(op):
    """[(slot name, address)] of the non-null pointers of ``op``; the row-block tickets of an MG_OP_IGEMM count as one."""
    names = L.FIELDS.get(op.kind, ("", {}))[1].get("p", ())
    out = [(names[k] if k < len(names) else f"p[{k}]", int(op.p[k])) for k in range(len(op.p)) if op.p[k]]
    if op.kind == L.OP_IGEMM and O.igemm_tickets(op):
        out.append(("tickets", O.igemm_tickets(op)))
    return out


def classify(seq, module, io):
    held_all = _unique(_flat(seq.keep))
    held_ptrs = {t.data_ptr() for t in held_all}
    stray = sorted(p for p in seq.zero_state if p not in held_ptrs)
    if stray:
        raise ContractError(f"{seq.name}: zero-state pointers the program does not hold: {[hex(p) for p in stray]}")
    io_ptrs = {t.data_ptr() for t in io.slots()}
    zero = [t for t in held_all if t.data_ptr() in seq.zero_state]
    cache = _unique(_flat(module.ws.cache))
    cache_ptrs = {t.data_ptr() for t in cache}
    held = [t for t in held_all if t.data_ptr() not in seq.zero_state and t.data_ptr() not in io_ptrs and t.data_ptr() not in cache_ptrs]
    cls = Classes(_unique(module.pool.all), zero, cache, held, io)
    spans = _Spans({SCRATCH: cls.scratch, ZERO: zero, CONST: cache + held, IO_SLOT: io.slots()})
    for op, label in zip(seq.ops, seq.labels):
        found = []
        for name, ptr in pointer_slots(op):
            hits = spans.hits(ptr)
            kinds = sorted({c for c, _ in hits})
            if len(kinds) != 1:
                raise ContractError(f"{seq.name}: op '{label}' ({L.OP_NAMES.get(op.kind, op.kind)}) pointer {name} = {ptr:#x} resolves "
                                    + ("nowhere" if not kinds else f"into {len(kinds)} classes: {kinds}"))
            found.append((name, kinds[0], max((t for _, t in hits), key=lambda t: t.numel() * t.element_size())))
        cls.op_ptrs.append(found)
    written = {t.data_ptr() for ptrs in cls.op_ptrs for name, _, t in ptrs if name == "out"}
    cls.tables = [t for t in held if t.data_ptr() in written]
    return cls


def launch_form(op):
    """(kind, non-null pointer slots, named form fields): what decides which kernel and which of its paths a launch takes."""
    where = L.FIELDS[op.kind][1]
    names = {n for arr in ("i", "f", "l") for n in where.get(arr, ())}
    raw = O.Raw(op)
    return (L.OP_NAMES[op.kind], tuple(name for name, _ in pointer_slots(op)),
            tuple((f, getattr(raw, f)) for f in FORM_FIELDS if f in names))


def _bytes(t):
    assert t.is_contiguous(), "a pooled / held buffer is contiguous"
    return t.reshape(-1).view(torch.uint8)


def poison(tensors, pattern, seed=0):
    """Fill every byte of every tensor; -> bytes filled."""
    n = 0
    for k, t in enumerate(_unique(tensors)):
        b = _bytes(t)
        if pattern == "random":
            g = torch.Generator(device=b.device).manual_seed(seed + k)
            for i in range(0, b.numel(), 1 << 28):
                part = b[i:i + (1 << 28)]
                part.copy_(torch.randint(0, 256, part.shape, dtype=torch.uint8, device=b.device, generator=g))
        else:
            b.fill_(int(pattern))
        n += b.numel()
    return n


def _sync(tensors):
    if any(t.is_cuda for t in tensors):
        torch.cuda.synchronize()


def run_with_fill(seq, cls, pattern, seed=0):
    """-> (clones of the output slots, scratch bytes filled)."""
    n = poison(cls.scratch, pattern, seed)
    poison(cls.io.outputs, pattern, seed + 7919)
    poison(cls.tables, pattern, seed + 104729)   # (the time-embedding tables of a denoising program: held, not pooled, written by its prologue)
    for slot, value in cls.io.inputs:
        slot.copy_(value)
    seq.run()
    _sync(cls.io.outputs)
    return [o.clone() for o in cls.io.outputs], n


def checksums(tensors):
    """[(sum, index-weighted sum)] of each tensor's bytes as int32 (a tail of 1-3 bytes as bytes), in wrapping int64."""
    out = []
    for t in tensors:
        b = _bytes(t)
        n4 = b.numel() // 4 * 4
        v = torch.cat([b[:n4].view(torch.int32).to(torch.int64), b[n4:].to(torch.int64)])
        out.append(torch.stack([v.sum(), (v * torch.arange(1, v.numel() + 1, device=v.device)).sum()]).cpu())
    return [tuple(s.tolist()) for s in out]   # (one read-back per tensor, after every sum is queued)


def first_dependent_op(seq, cls, fills=(0x00, 0xFF)):
    """Index of the first op that leaves a fill-dependent byte in a scratch buffer, an output or the zero state, or None.  Two
    replays run side by side: the live buffers hold the ``fills[0]`` replay, a shadow copy of everything mutable the ``fills[1]``
    one; an op touches only the buffers its pointers name, so only those are swapped and compared."""
    mutable = cls.mutable()
    ofills = tuple(f ^ 0x5A for f in fills)   # the outputs get another byte than the scratch: a plain copy of unwritten scratch shows
    poison(cls.scratch + cls.tables, fills[0])
    poison(cls.io.outputs, ofills[0])
    for slot, value in cls.io.inputs:
        slot.copy_(value)
    shadow = {t.data_ptr(): t.clone() for t in mutable}
    in_ptrs = {s.data_ptr() for s, _ in cls.io.inputs}
    filled = {t.data_ptr(): fills for t in cls.scratch + cls.tables}
    filled.update({t.data_ptr(): ofills for t in _unique(cls.io.outputs) if t.data_ptr() not in in_ptrs})
    for p, f in filled.items():
        poison([shadow[p]], f[1])
    zero0 = [t.clone() for t in cls.zero]

    def swap(ts):
        for t in ts:
            s = shadow[t.data_ptr()]
            tmp = t.clone()
            t.copy_(s)
            s.copy_(tmp)

    found = None
    for i in range(len(seq.ops)):
        touched = _unique([t for _, _, t in cls.op_ptrs[i] if t.data_ptr() in shadow])
        seq.run_range(i, 1)
        _sync(mutable)
        swap(touched)
        seq.run_range(i, 1)
        _sync(mutable)
        for t in touched:
            a, b = _bytes(shadow[t.data_ptr()]), _bytes(t)
            d = a != b
            if t.data_ptr() in filled:
                fa, fb = filled[t.data_ptr()]
                d &= (a != fa) | (b != fb)
            if bool(d.any()):
                found = i
        swap(touched)
        if found is not None:
            break
    for t, z in zip(cls.zero, zero0):   # a half-replayed program may hold tickets: hand the zero state back as it was
        t.copy_(z)
    return found


def check_program(seq, module, io, patterns=PATTERNS, say=print):
    """The three properties for one program; on a difference the message names the first dependent op.  -> report dict."""
    cls = classify(seq, module, io)
    assert all(int(_bytes(z).max()) == 0 for z in cls.zero), f"{seq.name}: zero state is not zero before the first run"
    consts = cls.cache + io.pure_inputs()
    for slot, value in io.inputs:
        slot.copy_(value)
    before = checksums(consts)
    ref, zero_after, nbytes = None, None, 0

    def fail(what):
        i = first_dependent_op(seq, cls)
        where = "no single op shows it" if i is None else f"first dependent op {i}: '{seq.labels[i]}' ({L.OP_NAMES.get(seq.ops[i].kind)})"
        raise ContractError(f"{seq.name}: {what}; {where}")

    for pattern in list(patterns) + [None]:   # None: again on the same inputs, scratch and zero state as the last run left them
        if pattern is None:
            for slot, value in io.inputs:
                slot.copy_(value)
            seq.run()
            _sync(io.outputs)
            outs = [o.clone() for o in io.outputs]
        else:
            outs, nbytes = run_with_fill(seq, cls, pattern)
        tag = "a second run on the same inputs" if pattern is None else f"scratch fill {hex(pattern) if isinstance(pattern, int) else pattern}"
        if not all(bool(torch.isfinite(o).all()) for o in outs):
            fail(f"non-finite output with {tag}")
        if ref is None:
            ref = outs
        elif not all(torch.equal(a, b) for a, b in zip(ref, outs)):
            fail(f"outputs differ between scratch fill {hex(patterns[0])} and {tag}")
        z = [_bytes(t).clone() for t in cls.zero]
        if zero_after is not None and not all(torch.equal(a, b) for a, b in zip(zero_after, z)):
            fail(f"zero state changed over the run with {tag}")
        zero_after = z
        after = checksums(consts)
        if after != before:
            bad = [k for k, (x, y) in enumerate(zip(after, before)) if x != y]
            fail(f"{len(bad)} constant tensor(s) / input slot(s) changed over the run with {tag} (first: #{bad[0]}, {tuple(consts[bad[0]].shape)})")
    rep = dict(program=seq.name, ops=len(seq.ops), scratch_bytes=sum(t.numel() * t.element_size() for t in cls.scratch),
               filled_bytes=nbytes, pool_bytes=module.pool.bytes, zero_state_bytes=sum(t.numel() * t.element_size() for t in cls.zero),
               constants=len(consts), table_bytes=sum(t.numel() * t.element_size() for t in cls.tables))
    assert rep["filled_bytes"] == rep["scratch_bytes"] == rep["pool_bytes"], rep
    say(f"[scratch] {seq.name}: {rep['ops']} ops, {rep['filled_bytes']} scratch bytes filled per run (pool.bytes {rep['pool_bytes']}), "
        f"{rep['table_bytes']} bytes of held tables filled too, {rep['zero_state_bytes']} zero-state bytes, {rep['constants']} constants checksummed, fills {[hex(p) if isinstance(p, int) else p for p in patterns]}")
    return rep

