"""What the instruction-stream generators (gen_k4w.py, gen_cp4w.py, gen_fa4w.py) share: a stream whose s_waitcnt counts are
derived, the slot layout around numbered MFMAs, the writer of the `#define NAME \\ ...` text and two lexical hazard checks.

hipcc pastes a generated stream in as `asm volatile` text: inside it nothing schedules, counts waits or inserts hazard wait
states - what a generator writes is what the wave executes.  Hence:

  * Stream: instructions in issue order.  An LDS operation and a VMEM operation carry a queue tag; a wait names the tag it
    needs and its count is the number of later-issued items of that queue (lgkmcnt / vmcnt retire in order), so a moved
    instruction cannot leave a count stale.  A stream starts from its ENTRY queues (what the code in front of it left in
    flight, oldest first) and ends with its EXIT queues (what it did not retire): a generator chains its blocks through them
    and asserts that the chain is closed.
  * check_hazards, run on every stream before it is written:
      - a write of M0 needs an instruction between it and the LDS-DMA (buffer_load_* ... lds) that reads it;
      - a transcendental's (v_exp_f32, v_rcp_f32) result must not be read by the next instruction (gfx940-family
        TRANS -> VALU forwarding hazard: one wait state).
    NOT checked, a rule the schedules keep by construction: a VALU result needs wait states before an MFMA reads it as an
    operand (the project has no measured number for it; gen_fa4w.py puts an MFMA and five VALU instructions in between).
  * MFMA_RESULT_TAIL behind the last MFMA of every last block.
"""
import re

ALL = "*"                            # wait tag: everything in flight on that queue
LGKMCNT_MAX, VMCNT_MAX = 15, 63      # what s_waitcnt encodes on gfx950

# The epilogue's v_accvgpr_read follow in compiler code, whose hazard recogniser does not see the MFMAs of an asm stream: an
# 8-pass MFMA's result may be read 11 wait states after its issue at the earliest (round 4, first run of gen_k4w.py's stream:
# the LAST accumulator of every wave held its value from before the final MFMA).
MFMA_RESULT_TAIL = ["s_nop 7", "s_nop 7", "s_nop 7"]


class StreamError(Exception):
    pass


class _Queue:
    def __init__(self, counter, limit, entry):
        self.counter, self.limit = counter, limit
        self.issued = list(entry)    # every item's tag in issue order, the entry state included
        self.retired = 0             # issued[:retired] have been waited for

    def wait(self, tag, if_retired):
        """-> the count that retires the youngest item tagged `tag` (and, in order, everything older), None for no wait"""
        if tag == ALL:
            idx = len(self.issued) - 1
        else:
            idx = max((i for i, x in enumerate(self.issued) if x == tag), default=-1)
            if idx < self.retired:
                if if_retired == "skip":
                    return None
                if if_retired != "emit" or idx < 0:
                    raise StreamError(f"{self.counter}: wait for {tag!r}, which is not in flight {self.issued[self.retired:]}")
        n = len(self.issued) - 1 - idx
        if n > self.limit:
            raise StreamError(f"s_waitcnt {self.counter}({n}) for {tag!r} cannot be encoded (at most {self.limit})")
        self.retired = max(self.retired, idx + 1)
        return n


class Stream:
    """The plain-append layout: every call appends at the end and resolves at once."""

    def __init__(self, lds=(), vm=()):
        self.lines = []
        self._q = {"lds": _Queue("lgkmcnt", LGKMCNT_MAX, lds), "vm": _Queue("vmcnt", VMCNT_MAX, vm)}

    @property
    def ldsq(self):
        """LDS operations in flight, oldest first: the exit queue once the stream is complete"""
        q = self._q["lds"]
        return q.issued[q.retired:]

    @property
    def vmq(self):
        q = self._q["vm"]
        return q.issued[q.retired:]

    def put(self, text, kind="op", tag=None, if_retired="raise"):
        """kind: 'op' | 'lds' | 'vm' (an operation of that queue, tagged) | 'wait_lds' | 'wait_vm' (text is None; tag or ALL).
        if_retired, for a wait whose tag an earlier wait has retired already: 'raise' | 'skip' (no instruction) | 'emit' (the
        redundant wait, with the count of what was issued since)."""
        if kind in ("lds", "vm"):
            self._q[kind].issued.append(tag)
        elif kind in ("wait_lds", "wait_vm"):
            q = self._q[kind[5:]]
            n = q.wait(tag, if_retired)
            if n is None:
                return
            text = f"s_waitcnt {q.counter}({n})"
        elif kind != "op":
            raise StreamError(f"unknown item kind {kind!r}")
        self.lines.append(text)

    def op(self, text):
        self.put(text)

    def lds(self, text, tag):
        self.put(text, "lds", tag)

    def vmem(self, text, tag):
        self.put(text, "vm", tag)

    def wait_lds(self, tag=ALL, if_retired="raise"):
        self.put(None, "wait_lds", tag, if_retired)

    def wait_vm(self, tag=ALL, if_retired="raise"):
        self.put(None, "wait_vm", tag, if_retired)


class Slots:
    """The layout around nm numbered MFMAs: slot 2 g in front of MFMA g, slot 2 g + 1 behind it, slot 2 nm the tail.  Items
    (the arguments of Stream.put) are placed in any order and resolved when the slots are played into a stream."""

    def __init__(self, nm):
        self.nm = nm
        self.slots = [[] for _ in range(2 * nm + 1)]

    def put(self, slot, text, kind="op", tag=None, if_retired="raise"):
        self.slots[slot].append((text, kind, tag, if_retired))

    def pre(self, g, *item):
        self.put(2 * g, *item)

    def post(self, g, *item):
        self.put(2 * g + 1, *item)

    def tail(self, *item):
        self.put(2 * self.nm, *item)

    def play(self, st, mfma):
        for g in range(self.nm):
            for it in self.slots[2 * g]:
                st.put(*it)
            st.op(mfma(g))
            for it in self.slots[2 * g + 1]:
                st.put(*it)
        for it in self.slots[2 * self.nm]:
            st.put(*it)
        return st


def renamed(queue, names):
    """an exit queue in the next block's terms (its "tile t + 2" is the next block's "tile t + 1")"""
    return [names.get(x, x) for x in queue]


# ---- hazard checks ---------------------------------------------------------------------------------------------------
_REG = re.compile(r"%\[\w+\]|\bv\[(\d+):(\d+)\]|\bv(\d+)\b")


def _regs(text):
    """vector registers named in an operand text: (name,) for %[x], (lo, hi) for physical registers and tuples"""
    out = []
    for m in _REG.finditer(text):
        if m.group(0).startswith("%"):
            out.append((m.group(0),))
        elif m.group(1) is not None:
            out.append((int(m.group(1)), int(m.group(2))))
        else:
            out.append((int(m.group(3)), int(m.group(3))))
    return out


def _overlap(a, b):
    if len(a) != len(b):
        return False                 # a named operand against a physical register: not knowable here
    return a == b if len(a) == 1 else a[0] <= b[1] and b[0] <= a[1]


def _split(ins):
    mnem, _, rest = ins.partition(" ")
    return mnem, [o.strip() for o in rest.split(",")]


def check_hazards(lines):
    ins = [ln for ln in lines if not ln.endswith(":")]       # labels are not instructions
    for a, b in zip(ins, ins[1:]):
        ma, oa = _split(a)
        mb, ob = _split(b)
        if oa[0] == "m0" and mb.startswith("buffer_load") and b.split()[-1] == "lds":
            raise StreamError(f"M0 written right in front of the LDS-DMA that reads it: {a!r} ; {b!r}")
        if ma in ("v_exp_f32", "v_rcp_f32"):
            srcs = ob if mb.startswith(("ds_write", "buffer_")) else ob[1:]       # (stores have no destination operand)
            if any(_overlap(d, s) for d in _regs(oa[0]) for s in _regs(",".join(srcs))):
                raise StreamError(f"transcendental result read by the next instruction: {a!r} ; {b!r}")
    return lines


# ---- writer ----------------------------------------------------------------------------------------------------------
def c_literal(ln):
    """One instruction as a C string literal; the operand-type mnemonics come from common.h (MG_MFMA32_ASM, MG_MFMA16_ASM,
    MG_CVT_PK_ASM: bf16 in the product build, fp16 in the fp16 build) as adjacent literals."""
    for mnem, macro in (("v_mfma_f32_32x32x16_bf16", "MG_MFMA32_ASM"), ("v_mfma_f32_16x16x32_bf16", "MG_MFMA16_ASM"),
                        ("v_cvt_pk_bf16_f32", "MG_CVT_PK_ASM")):
        if ln.startswith(mnem + " "):
            return macro + ' "' + ln[len(mnem):]
    return '"' + ln


def define(name, lines, eol="\\n"):
    """`#define name \\ ...` of a finished stream, one instruction per line, each ending in eol (the asm text's line end)"""
    check_hazards(lines)
    return "\n".join([f"#define {name} \\"] + [f'  {c_literal(ln)}{eol}" \\' for ln in lines] + ['  ""'])
