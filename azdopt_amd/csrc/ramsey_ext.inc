// ramsey_ext.inc -- the Ramsey side of the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP; pool_step.inc: k_pool_search, with
// the evaluator's batched GEMM launches outside the kernel, engine_rollout.hip: ext_pool_run): the space policies of the form and the
// refusals of its plan, between the search core and the launchers they need: a searcher-only unit of a Ramsey tier, but for the
// policies it builds and the name it exports.  Included inside namespace azd after bf16.h and space_ops.h by ramsey_ext_kernels.hip
// (32-bit wide tier), ramsey64_ext_kernels.hip (64-bit tier) and ramsey64_big_ext_kernels.hip (64-bit tier, cliques up to K8).
#define AZD_TU_ASYNC 1 // (no launch-per-phase kernel is built in these units)
#define AZD_TU_POOL_SEARCH 1
#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

typedef float azd_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_sc1_x2(float *p, azd_f32x2 v) { asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ void st_sc1_u16(uint16_t *p, uint32_t v) { asm volatile("global_store_short %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }

// BASE: RamseyWideSpace<10 / 16>, RamseyU64Space or RamseyU64BigSpace, untouched (their own write_rows_direct / write_vec are
// compiled into the existing kernels).  What the form adds is the row hand-over: the f32 row (training, observe and the tests read it) and, for a bf16
// evaluator, the same entries as bf16 (bf16.h: round to nearest even -- a clique count can pass 256, where bf16 is no longer
// exact) at pitch Arenas::S16, both as write-through stores: the gathered GEMM that reads them is another kernel on another stream.
template <class BASE>
struct RamseyExtSpace : BASE {
    using Lds = typename BASE::Lds;
    using St = typename BASE::St;
    using W = typename BASE::W;
    static constexpr bool ROWS_DIRECT = true;
    // the permitted edges as a bitmap the lanes can index: Lds::seq, which only the Layered wrapper uses (the tiers take none)
    static_assert(sizeof(Lds::seq) >= (size_t)BASE::PW * 8, "the permitted-edge bitmap must fit RamseyLdsT::seq");

    // space.rs:122-153 write_vec: [counts C x E][edge bools C x E][permitted E], eight consecutive entries per lane and step.
    // The f32 row's pitch is S, which may be odd (r3333: 5049): a piece starts 0..3 floats past a 16-byte boundary -- the same
    // for every piece of a row -- and leaves as the widest aligned stores that cover it (2 to 4 instructions in place of 8).
    // The bf16 row's pitch is a multiple of 8: a whole piece is one 16-byte store.  The last piece stops at S: the padding
    // between S and S16 was zeroed at allocation and is never written.
    __device__ static __forceinline__ void write_rows_direct(const Arenas &a, Lds &s, const uint32_t dyn, const St &st, float *row, uint16_t *row16) {
        const int E = a.E, CE = a.C * a.E, S = 2 * CE + E;
        const int32_t *counts = BASE::lds_counts(dyn);
        uint32_t *pm = reinterpret_cast<uint32_t *>(s.seq);
        if (LANE == 0) {
#pragma unroll
            for (int w = 0; w < BASE::PW; ++w) {
                pm[2 * w] = (uint32_t)st.perm[w];
                pm[2 * w + 1] = (uint32_t)(st.perm[w] >> 32);
            }
        }
        LDS_SYNC();
        const uint32_t mis = (uint32_t)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u); // floats past a 16-byte boundary (wave-uniform)
        for (int i0 = 8 * LANE; i0 < S; i0 += 8 * 64) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int i = i0 + q;
                float x = 0.f;
                if (i < CE) x = (float)counts[i];
                else if (i < 2 * CE) {
                    const int j = i - CE;
                    const int c = (j >= E ? 1 : 0) + (j >= 2 * E ? 1 : 0) + (j >= 3 * E ? 1 : 0);
                    const int e = j - c * E;
                    x = (float)((s.nbr[c][s.ev[e]] >> s.eu[e]) & (W)1);
                } else if (i < S) {
                    const int e = i - 2 * CE;
                    x = (float)((pm[e >> 5] >> (e & 31)) & 1u);
                }
                v[q] = x;
            }
            float *p = row + i0;
            const bool whole = i0 + 8 <= S;
            if (whole) {
                const azd_f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
                const azd_f32x4 m1 = {v[1], v[2], v[3], v[4]}, m2 = {v[2], v[3], v[4], v[5]}, m3 = {v[3], v[4], v[5], v[6]};
                if (mis == 0u) {
                    st_sc1_x4(p, lo);
                    st_sc1_x4(p + 4, hi);
                } else if (mis == 2u) {
                    st_sc1_x2(p, azd_f32x2{v[0], v[1]});
                    st_sc1_x4(p + 2, m2);
                    st_sc1_x2(p + 6, azd_f32x2{v[6], v[7]});
                } else if (mis == 1u) {
                    st_sc1_f32(p, v[0]);
                    st_sc1_x2(p + 1, azd_f32x2{v[1], v[2]});
                    st_sc1_x4(p + 3, m3);
                    st_sc1_f32(p + 7, v[7]);
                } else {
                    st_sc1_f32(p, v[0]);
                    st_sc1_x4(p + 1, m1);
                    st_sc1_x2(p + 5, azd_f32x2{v[5], v[6]});
                    st_sc1_f32(p + 7, v[7]);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (i0 + q < S) st_sc1_f32(p + q, v[q]);
            }
            if (row16) {
                uint32_t h[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) h[q] = bf16_bits(v[2 * q]) | (bf16_bits(v[2 * q + 1]) << 16);
                if (whole) {
                    azd_f32x4 w;
                    __builtin_memcpy(&w, h, 16);
                    st_sc1_x4(reinterpret_cast<float *>(row16 + i0), w);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (i0 + 2 * q + 1 < S) st_sc1(reinterpret_cast<uint32_t *>(row16 + i0 + 2 * q), h[q]);
                        else if (i0 + 2 * q < S) st_sc1_u16(row16 + i0 + 2 * q, h[q] & 0xFFFFu);
                    }
                }
            }
        }
        LDS_SYNC();
    }
};

#include "launchers.inc"

// ---------------------------------------------------------------- host: a unit's PoolSearchOps (space_ops.h), exported as NAME, for its
// key-width switch D over the policies above, with the refusals of the tiers' plans (launchers.inc: PoolSearch)
#define RAMSEY_EXT_POOL_SEARCH_UNIT(D, WAVES, NAME)                                                                                    \
    AZD_POOL_SEARCH_ENTRIES(D, WAVES, "external pool step: more than 65536 agents or nodes per tree",                                  \
                            "external pool step: more wavefronts per searcher workgroup than the kernel is built for",                 \
                            "external pool step: the searcher waves' blocks, scratch and clique counts do not fit the CU's 160 KB of LDS") \
    const PoolSearchOps &NAME() {                                                                                                      \
        static const PoolSearchOps ops = {AZD_POOL_SEARCH_OPS(WAVES)};                                                                 \
        return ops;                                                                                                                    \
    }
