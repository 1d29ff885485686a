"""csrc/asmstream.py, the stream model under the instruction-stream generators: counted waits resolved from the queues, entry and
exit queues, the two lexical hazard checks and the C-literal writer.  A text checker tested on text: nothing runs on a device."""
import importlib.util
import os

import pytest

_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marigold_amd", "csrc", "asmstream.py")
_spec = importlib.util.spec_from_file_location("asmstream", _PATH)
A = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(A)


def toy(lds=(), vm=()):
    """issue order: LDS a, VMEM v1, LDS b, LDS c, VMEM v2, VMEM v3"""
    st = A.Stream(lds, vm)
    st.lds("ds_read_b128 v[0:3], v100", "a")
    st.vmem("buffer_load_dwordx4 v101, s[0:3], 0 offen lds", "v1")
    st.lds("ds_read_b128 v[4:7], v100 offset:16", "b")
    st.lds("ds_read_b128 v[8:11], v100 offset:32", "c")
    st.op("s_nop 0")
    st.vmem("buffer_load_dwordx4 v102, s[0:3], 0 offen lds", "v2")
    st.vmem("buffer_load_dwordx4 v103, s[0:3], 0 offen lds", "v3")
    return st


@pytest.mark.parametrize("tag,count,left", [("a", 2, ["b", "c"]), ("b", 1, ["c"]), ("c", 0, [])])
def test_lds_wait_counts_later_issued_items(tag, count, left):
    st = toy()
    st.wait_lds(tag)
    assert st.lines[-1] == f"s_waitcnt lgkmcnt({count})"      # by hand: the LDS items behind `tag` in a, b, c
    assert st.ldsq == left and st.vmq == ["v1", "v2", "v3"]


@pytest.mark.parametrize("tag,count,left", [("v1", 2, ["v2", "v3"]), ("v2", 1, ["v3"]), ("v3", 0, [])])
def test_vm_wait_counts_later_issued_items(tag, count, left):
    st = toy()
    st.wait_vm(tag)
    assert st.lines[-1] == f"s_waitcnt vmcnt({count})"
    assert st.vmq == left and st.ldsq == ["a", "b", "c"]


def test_entry_queues_are_older_items_and_exit_queues_what_was_not_retired():
    st = toy(lds=["e0", "e1"], vm=["p", "p", "p"])
    assert st.ldsq == ["e0", "e1", "a", "b", "c"] and st.vmq == ["p", "p", "p", "v1", "v2", "v3"]
    st.wait_lds("e0")                       # e1, a, b, c are younger
    st.wait_vm("p")                         # the youngest p: v1, v2, v3 are younger
    st.wait_lds("a")                        # unchanged by the entry state: b, c
    assert st.lines[-3:] == ["s_waitcnt lgkmcnt(4)", "s_waitcnt vmcnt(3)", "s_waitcnt lgkmcnt(2)"]
    assert st.ldsq == ["b", "c"] and st.vmq == ["v1", "v2", "v3"]
    st.wait_lds()                           # everything
    st.wait_vm()
    assert st.lines[-2:] == ["s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(0)"] and st.ldsq == [] and st.vmq == []
    assert A.renamed(["x2", "x2", "y"], {"x2": "x1"}) == ["x1", "x1", "y"]


def test_wait_for_a_tag_not_in_flight():
    for tag in ("nope", "a"):               # never issued; retired by the wait for b
        st = toy()
        st.wait_lds("b")
        n = len(st.lines)
        with pytest.raises(A.StreamError):
            st.wait_lds(tag)
        st.wait_lds(tag, "skip")
        assert len(st.lines) == n and st.ldsq == ["c"]
    st = toy()
    with pytest.raises(A.StreamError):
        st.wait_vm("a")                     # an LDS tag is not in the VMEM queue
    st.wait_vm("a", "skip")
    # 'emit': the redundant wait for a retired item is written, counting what was issued since; never-issued still raises
    st = toy()
    st.wait_lds("b")
    st.wait_lds("a", "emit")
    assert st.lines[-1] == "s_waitcnt lgkmcnt(2)" and st.ldsq == ["c"]
    with pytest.raises(A.StreamError):
        st.wait_lds("nope", "emit")


def test_counts_that_s_waitcnt_cannot_encode():
    st = A.Stream(lds=["first"] + ["x"] * 15)
    st.wait_lds("first")
    assert st.lines == ["s_waitcnt lgkmcnt(15)"]
    with pytest.raises(A.StreamError):
        A.Stream(lds=["first"] + ["x"] * 16).wait_lds("first")      # lgkmcnt(16)
    st = A.Stream(vm=["first"] + ["x"] * 63)
    st.wait_vm("first")
    assert st.lines == ["s_waitcnt vmcnt(63)"]
    with pytest.raises(A.StreamError):
        A.Stream(vm=["first"] + ["x"] * 64).wait_vm("first")        # vmcnt(64)


def test_slots_resolve_in_stream_order_not_in_placing_order():
    sl = A.Slots(3)
    sl.pre(2, None, "wait_lds", "r0")       # placed first, issued last: r1 is then the one younger read
    sl.post(0, "ds_read_b128 v[0:3], v9", "lds", "r0")
    sl.post(1, "ds_read_b128 v[4:7], v9", "lds", "r1")
    sl.pre(0, None, "wait_lds", "e")
    sl.tail("s_nop 1")
    st = sl.play(A.Stream(lds=["e", "e"]), lambda g: f"mfma{g}")
    assert st.lines == ["s_waitcnt lgkmcnt(0)", "mfma0", "ds_read_b128 v[0:3], v9", "mfma1", "ds_read_b128 v[4:7], v9",
                        "s_waitcnt lgkmcnt(1)", "mfma2", "s_nop 1"]
    assert st.ldsq == ["r1"]


DMA = "buffer_load_dwordx4 %[va0], %[sa], 0 offen lds"


def test_m0_write_needs_an_instruction_before_the_lds_dma():
    with pytest.raises(A.StreamError):
        A.check_hazards(["s_add_u32 m0, %[ma], 4096", DMA])
    with pytest.raises(A.StreamError):
        A.define("T", ["s_nop 0", "s_mov_b32 m0, s5", ".Llabel_%=:", DMA])      # a label is no instruction
    A.check_hazards(["s_add_u32 m0, %[ma], 4096", "v_mfma_f32_32x32x16_bf16 %[c], %[b], %[a], %[c]", DMA])
    A.check_hazards(["s_add_u32 m0, %[ma], 4096", "buffer_load_dwordx4 v[0:3], v4, s[0:3], 0 offen"])      # not to LDS


@pytest.mark.parametrize("trans,reader,bystander", [
    ("v_exp_f32 v5, v5", "v_add_f32 v6, v6, v5", "v_add_f32 v5, v6, v7"),                    # (writing v5 is no read)
    ("v_rcp_f32 v5, v5", "v_mul_f32 v1, v1, v5", "v_mul_f32 v1, v1, v15"),
    ("v_exp_f32 v5, v5", "ds_write_b128 %[fxa], v[4:7] offset:4096", "ds_write_b128 %[fxa], v[6:9]"),
    ("v_exp_f32 v5, v5", "v_mfma_f32_32x32x16_bf16 %[o], %[vf], v[4:7], %[o]", "v_mfma_f32_32x32x16_bf16 v[4:7], %[vf], v[8:11], %[o]"),
    ("v_exp_f32 %[x], %[x]", "v_add_f32 %[l], %[l], %[x]", "v_add_f32 %[l], %[l], %[x2]"),
    ("v_rcp_f32 %[x], %[y]", "v_mul_f32 v3, %[x], v3", "v_mul_f32 %[x], %[y], v3"),
])
def test_transcendental_result_is_not_read_by_the_next_instruction(trans, reader, bystander):
    with pytest.raises(A.StreamError):
        A.check_hazards(["s_nop 0", trans, reader])
    A.check_hazards(["s_nop 0", trans, bystander, reader])
    A.check_hazards([trans, bystander])


def test_c_literal_and_define():
    assert A.c_literal("v_mfma_f32_32x32x16_bf16 %[c], %[b], %[a], %[c]") == 'MG_MFMA32_ASM " %[c], %[b], %[a], %[c]'
    assert A.c_literal("v_mfma_f32_16x16x32_bf16 v[0:3], %[k], %[q], v[0:3]") == 'MG_MFMA16_ASM " v[0:3], %[k], %[q], v[0:3]'
    assert A.c_literal("v_cvt_pk_bf16_f32 v1, v2, v3") == 'MG_CVT_PK_ASM " v1, v2, v3'
    for ln in ("v_cvt_pk_bf16_f32x v1, v2, v3", "v_mfma_f32_32x32x8_bf16 a, b, c, d", "s_barrier", "ds_read_b128 %[a00], %[la0] offset:4096"):
        assert A.c_literal(ln) == '"' + ln
    assert A.define("N", ["s_barrier", "v_cvt_pk_bf16_f32 v1, v2, v3"]) == \
        '#define N \\\n  "s_barrier\\n" \\\n  MG_CVT_PK_ASM " v1, v2, v3\\n" \\\n  ""'
    assert A.define("N", ["s_barrier"], eol="\\n\\t") == '#define N \\\n  "s_barrier\\n\\t" \\\n  ""'
    assert A.MFMA_RESULT_TAIL == ["s_nop 7"] * 3
