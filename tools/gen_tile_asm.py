#!/usr/bin/env python3
"""Generates the software-pipelined k loops of an evaluator tile task (dfdx.rs:69-84, one 16-column tile of one layer for a batch of
<= 16 rows), each as ONE inline-asm block, into two files:

  azdopt_amd/csrc/tile_task_asm.inc          the product's: the evaluator groups' two loops (pool_step.inc: pool_eval_group), rows' quads
                                             from device memory, weight quads from LDS
  tools/probes/tile_task_asm_probe.inc       the measurement probe's (tools/probes/group_exchange.hip): the classic form's fp32 loop
                                             and its chained variant, weight quads from device memory, rows' quads from LDS

  gen_tile_asm.py [OUT_DIR]                  with OUT_DIR both files are written there, under their base names (tests/test_generated_sources.py)

Why asm: the loop wants the quads of the NEXT group of 8 k-steps requested before the MFMAs of the current group, and
"the current group has landed" is then `s_waitcnt vmcnt(8)`.  hipcc's own wait insertion cannot be talked into that for a loop
with a runtime trip count: at every merge of control flow it drains to vmcnt(0) and it throttles requests into registers it
believes in flight (tools/probes/group_exchange.hip: k_classic2, the ISA in profiles/r05_tile_pipeline.txt), and requests issued
by inline asm into compiler-allocated registers get spilled before they land.  Inside one asm block with registers of its own
(clobbers) nothing of that can happen.  The MFMA sequence per output element is exactly mlp_tile_task's (async_step.inc): k-steps
in ascending order, per step the quads' x, y, z, w -- results are bit-identical.

Register plan (VGPR): a0 v[56:59], a1 v[60:63] (the quads read from LDS, one step ahead), ring A v[64:95], ring B v[96:127] (8 steps
x 4 dwords each).  The probe's loops request with the SGPR-base form: the tile's wave-uniform address (and that + 4 KB: the
immediate offset reaches 4095) in SGPR pairs, the lane's offset in one VGPR that moves on by a group per group; their inputs are
the wave-uniform address of k-step 0 of the tile's fragment-major weights, the lane's byte offset inside a k-step, the LDS byte
address of its row quad at k-step 0 (64 B per step) and the number of k-steps.  A ragged last group still issues 8 requests, its
MFMAs stop at the last step.
(The bf16 forms of the probe's loops, and the classic evaluator's use of them, lost and are gone: profiles/HISTORY.md.)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_PRODUCT = os.path.join(HERE, "..", "azdopt_amd", "csrc", "tile_task_asm.inc")
OUT_PROBE = os.path.join(HERE, "probes", "tile_task_asm_probe.inc")
A0, RA, RB = 56, 64, 96


def v(lo, n=1):
    return "v%d" % lo if n == 1 else "v[%d:%d]" % (lo, lo + n - 1)


def loads_from(ring, b0, b1, lo):
    """8 requests: the tile's uniform base in an SGPR pair (b0 for steps 0-3 of the group, b1 for 4-7: the immediate offset reaches
    4095), the lane's offset (16 B per lane, 1 KB per k-step) in one VGPR"""
    return ["global_load_dwordx4 %s, %s, %s offset:%d" % (v(ring + 4 * j, 4), lo, b0 if j < 4 else b1, 1024 * (j & 3)) for j in range(8)]


def loads(ring):
    return loads_from(ring, "%[b0]", "%[b1]", "%[lo]")


def consume(ring):
    """8 k-steps out of `ring`; step j is skipped -- with everything behind it -- once done + j >= steps"""
    A1 = A0 + 4
    out = ["ds_read_b128 %s, %%[ap]" % v(A0, 4), "ds_read_b128 %s, %%[ap] offset:64" % v(A1, 4)]
    for j in range(8):
        a = A0 if (j & 1) == 0 else A1
        if j:
            out += ["s_add_i32 %[t0], %[done], " + str(j), "s_cmp_ge_i32 %[t0], %[steps]", "s_cbranch_scc1 9f"]
        out.append("s_waitcnt lgkmcnt(1)" if j < 7 else "s_waitcnt lgkmcnt(0)")
        for i in range(4):
            out.append("v_mfma_f32_16x16x4_f32 %%[acc], %s, %s, %%[acc]" % (v(a + i), v(ring + 4 * j + i)))
        if j + 2 < 8:  # the quad two steps on, into the register quad just used
            out.append("ds_read_b128 %s, %%[ap] offset:%d" % (v(a, 4), 64 * (j + 2)))
    return out


def body(chained):
    """chained: the block may start with group 0 already requested into ring A (state 1) or ring B (state 2) by the block
    before it, and during its own last group requests group 0 of the NEXT tile task (base nb0 / nb1, 0 = none) into the ring that
    is free then, leaving through `state` which ring that was; the rings are operands pinned to their registers, so that what is
    in flight between two blocks (the epilogue, the layer barrier) is the compiler's to leave alone."""
    lines = []
    if chained:
        lines += ["s_cmp_eq_u32 %[state], 0", "s_cbranch_scc0 4f"]
        lines += loads(RA)
        lines += ["4:", "s_mov_b32 %[done], 0", "s_cmp_eq_u32 %[state], 2", "s_mov_b32 %[state], 0", "s_cbranch_scc1 5f"]
    else:
        lines += loads(RA)
        lines += ["s_mov_b32 %[done], 0"]
    lines += ["1:"]
    for ring, other in ((RA, RB), (RB, RA)):
        if ring == RB and chained:
            lines += ["5:"]
        # request the group after this one into the other ring, if there is one; then this ring has landed
        lines += ["s_add_i32 %[t0], %[done], 8", "s_cmp_lt_i32 %[t0], %[steps]", "s_cbranch_scc0 2f"]
        lines += ["v_add_u32 %[lo], 0x2000, %[lo]"]  # one group of 8 k-steps
        lines += loads(other)
        lines += ["s_waitcnt vmcnt(8)", "s_branch 3f", "2:"]
        if chained:  # the tile's last group: the next task's first group into the free ring
            lines += ["s_cmp_eq_u64 %[nb0], 0", "s_cbranch_scc1 6f"]
            lines += loads_from(other, "%[nb0]", "%[nb1]", "%[lo0]")
            lines += ["s_mov_b32 %%[state], %d" % (2 if other == RB else 1), "s_waitcnt vmcnt(8)", "s_branch 3f", "6:"]
        lines += ["s_waitcnt vmcnt(0)", "3:"]
        lines += consume(ring)
        lines += ["s_add_i32 %[done], %[done], 8", "v_add_u32 %[ap], 0x200, %[ap]", "s_cmp_ge_i32 %[done], %[steps]", "s_cbranch_scc1 9f"]
    lines += ["s_branch 1b", "9:", "s_waitcnt lgkmcnt(0)" if chained else "s_waitcnt vmcnt(0) lgkmcnt(0)"]
    return lines


def emit(name):
    text = "\\n\\t\"\n        \"".join(body(False))
    clob = ['"memory"', '"scc"'] + ['"v%d"' % r for r in list(range(A0, A0 + 8)) + list(range(RA, RA + 64))]
    return ('''// ---- generated by tools/gen_tile_asm.py: do not edit
__device__ __forceinline__ void %s(azd_tile_acc &acc, const void *tile_base, uint32_t lane_off, uint32_t ap, const int steps) {
    // tile_base: wave-uniform address of the tile's k-step 0; lane_off: this lane's byte offset inside a k-step
    const unsigned long long b0 = azd_uniform_u64((unsigned long long)(uintptr_t)tile_base), b1 = b0 + 4096;
    int done, t0;
    asm volatile(
        "%s\\n\\t"
        : [acc] "+v"(acc), [ap] "+v"(ap), [lo] "+v"(lane_off), [done] "=&s"(done), [t0] "=&s"(t0)
        : [b0] "s"(b0), [b1] "s"(b1), [steps] "s"(__builtin_amdgcn_readfirstlane(steps))
        : %s);
}
''' % (name, text, ", ".join(clob)))


def emit_chained(name):
    text = "\\n\\t\"\n        \"".join(body(True))
    ring_ops = ", ".join('"+{v[%d:%d]}"(ring.r[%d])' % (RA + 4 * k, RA + 4 * k + 3, k) for k in range(16))
    clob = ['"memory"', '"scc"'] + ['"v%d"' % r for r in range(A0, A0 + 8)]
    return ('''// ---- generated by tools/gen_tile_asm.py: do not edit
// Chained form: `state` says whether group 0 of THIS task is already on its way (1: in ring.r[0..7], 2: in ring.r[8..15]; 0: no),
// `next_base` (0: none) is the task whose group 0 this block requests during its own last group; `state` leaves as what the next
// block must be told.  Nothing of the ring may be touched between two blocks of a chain: the operands are pinned to their
// registers.
__device__ __forceinline__ void %s(azd_tile_acc &acc, azd_tile_ring32 &ring, int &state, const void *tile_base, const void *next_base, uint32_t lane_off,
                                   uint32_t ap, const int steps) {
    const unsigned long long b0 = azd_uniform_u64((unsigned long long)(uintptr_t)tile_base), b1 = b0 + 4096;
    const unsigned long long nb0 = azd_uniform_u64((unsigned long long)(uintptr_t)next_base), nb1 = nb0 + 4096;
    int done, t0, st = __builtin_amdgcn_readfirstlane(state);
    const uint32_t lo0 = lane_off;
    asm volatile(
        "%s\\n\\t"
        : [acc] "+v"(acc), [ap] "+v"(ap), [lo] "+v"(lane_off), [done] "=&s"(done), [t0] "=&s"(t0), [state] "+s"(st), %s
        : [b0] "s"(b0), [b1] "s"(b1), [nb0] "s"(nb0), [nb1] "s"(nb1), [lo0] "v"(lo0), [steps] "s"(__builtin_amdgcn_readfirstlane(steps))
        : %s);
    state = st;
}
''' % (name, text, ring_ops, ", ".join(clob)))


def body_ga(stride):
    """The group evaluator's k loop (pool_step.inc: pool_eval_group): the ROWS' quads come from device memory -- the agents' state
    vectors (64 B per k-step and row) or the exchange buffer of the layer before (fragment-major: 1 KB per k-step) -- by sc1
    buffer loads, two rings of 8 k-steps as above; the WEIGHT quads come from the member's LDS (1 KB per k-step), one step ahead."""
    lines = []

    def loads(ring):
        out = []
        for j in range(8):
            if stride == 64:
                out.append("buffer_load_dwordx4 %s, %%[vo], %%[rs], 0 offen offset:%d sc1" % (v(ring + 4 * j, 4), 64 * j))
            else:
                out.append("buffer_load_dwordx4 %s, %%[vo], %%[rs], %s offen offset:%d sc1" % (v(ring + 4 * j, 4), "0" if j < 4 else "%[k4]", 1024 * (j & 3)))
        return out

    def consume(ring):
        out = ["ds_read_b128 %s, %%[bp]" % v(A0, 4), "ds_read_b128 %s, %%[bp] offset:1024" % v(A0 + 4, 4)]
        for j in range(8):
            b = A0 if (j & 1) == 0 else A0 + 4
            if j:
                out += ["s_add_i32 %[t0], %[done], " + str(j), "s_cmp_ge_i32 %[t0], %[steps]", "s_cbranch_scc1 9f"]
            out.append("s_waitcnt lgkmcnt(1)" if j < 7 else "s_waitcnt lgkmcnt(0)")
            for i in range(4):
                out.append("v_mfma_f32_16x16x4_f32 %%[acc], %s, %s, %%[acc]" % (v(ring + 4 * j + i), v(b + i)))
            if j + 2 < 8:
                out.append("ds_read_b128 %s, %%[bp] offset:%d" % (v(b, 4), 1024 * (j + 2)))
        return out

    lines += loads(RA)
    lines += ["s_mov_b32 %[done], 0", "1:"]
    for ring, other in ((RA, RB), (RB, RA)):
        lines += ["s_add_i32 %[t0], %[done], 8", "s_cmp_lt_i32 %[t0], %[steps]", "s_cbranch_scc0 2f"]
        lines += ["v_add_u32 %%[vo], 0x%x, %%[vo]" % (8 * stride)]
        lines += loads(other)
        lines += ["s_waitcnt vmcnt(8)", "s_branch 3f", "2:", "s_waitcnt vmcnt(0)", "3:"]
        lines += consume(ring)
        lines += ["s_add_i32 %[done], %[done], 8", "v_add_u32 %[bp], 0x2000, %[bp]", "s_cmp_ge_i32 %[done], %[steps]", "s_cbranch_scc1 9f"]
    lines += ["s_branch 1b", "9:", "s_waitcnt vmcnt(0) lgkmcnt(0)"]
    return lines


def emit_ga(name, stride):
    text = "\\n\\t\"\n        \"".join(body_ga(stride))
    clob = ['"memory"', '"scc"'] + ['"v%d"' % r for r in list(range(A0, A0 + 8)) + list(range(RA, RA + 64))]
    return ('''// ---- generated by tools/gen_tile_asm.py: do not edit
// The group evaluator's k loop: rows' quads from device memory (buffer resource `rs`, this lane's byte offset of k-step 0 in `vo`,
// %d B per k-step; sc1: L1 bypassed), weight quads from LDS (`bp`: this lane's quad of k-step 0, 1 KB per k-step).  A ragged last
// group still issues 8 requests: they stay inside the buffer resource or are dropped by its range check.
__device__ __forceinline__ void %s(azd_tile_acc &acc, const azd_tile_u4 rs_in, uint32_t vo, uint32_t bp, const int steps) {
    azd_tile_u4 rs; // (made uniform for the compiler's eyes: an "s" operand)
    rs[0] = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs_in[0]);
    rs[1] = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs_in[1]);
    rs[2] = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs_in[2]);
    rs[3] = (uint32_t)__builtin_amdgcn_readfirstlane((int)rs_in[3]);
    int done, t0;
    const int k4 = __builtin_amdgcn_readfirstlane(4096);
    asm volatile(
        "%s\\n\\t"
        : [acc] "+v"(acc), [vo] "+v"(vo), [bp] "+v"(bp), [done] "=&s"(done), [t0] "=&s"(t0)
        : [rs] "s"(rs), [k4] "s"(k4), [steps] "s"(__builtin_amdgcn_readfirstlane(steps))
        : %s);
}
''' % (stride, name, text, ", ".join(clob)))


def main():
    out_product, out_probe = OUT_PRODUCT, OUT_PROBE
    if len(sys.argv) > 1:
        out_product = os.path.join(sys.argv[1], os.path.basename(OUT_PRODUCT))
        out_probe = os.path.join(sys.argv[1], os.path.basename(OUT_PROBE))
    with open(out_product, "w") as f:
        f.write("// tile_task_asm.inc -- the software-pipelined k loops of the evaluator groups' tile task (see tools/gen_tile_asm.py for the why and\n"
                "// the register plan).  azd_tile_acc = float x 4 (the 16 x 16 accumulator tile: rows 4 (lane >> 4) + i, column lane & 15).\n")
        f.write("typedef float azd_tile_acc __attribute__((ext_vector_type(4)));\n")
        f.write("typedef unsigned int azd_tile_u4 __attribute__((ext_vector_type(4)));\n")
        f.write(emit_ga("tile_k_loop_f32_ga64", 64))
        f.write(emit_ga("tile_k_loop_f32_ga1024", 1024))
    with open(out_probe, "w") as f:
        f.write("// tile_task_asm_probe.inc -- the classic tile task's software-pipelined fp32 k loops, for tools/probes/group_exchange.hip only\n"
                "// (see tools/gen_tile_asm.py).  Included after azdopt_amd/csrc/tile_task_asm.inc, whose azd_tile_acc it uses.\n")
        f.write("struct azd_tile_ring32 { azd_tile_acc r[16]; }; // two rings of 8 k-steps x 16 B per lane: v[64:127]\n")
        f.write("__device__ __forceinline__ unsigned long long azd_uniform_u64(const unsigned long long x) { // an \"s\" operand must be uniform in the compiler's eyes\n"
                "    return (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x) |\n"
                "           ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32);\n}\n")
        f.write(emit("tile_k_loop_f32"))
        f.write(emit_chained("tile_k_chain_f32"))
    print("wrote", os.path.normpath(out_product), os.path.normpath(out_probe))


if __name__ == "__main__":
    main()
