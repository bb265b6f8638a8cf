// dense_ah_wide_kernels.hip -- the Aouchiche-Hansen cost of the dense-graph space up to 64 vertices (AZD_ENGINE_DENSE_AH_WIDE beside
// AZD_ENGINE_DENSE_AH): dense_ah_cost.inc with a row limit of 64 -- the packed triangle is 2080 doubles, 16.6 KB a wave --
// under names of its own, and tree_core.inc instantiated with DenseSpace<KW, DenseCostAhWide> for key widths 2 / 4 / 10
// (max_slots <= min(E, 640)): launch-per-phase kernels, the device root policy, the pool step's searchers and the cost probe, as
// dense_ah_kernels.hip has them for 32 rows.  That unit and dense_kernels.hip are not touched by this one; the evaluator side of the
// pool step (k_ext_*) and the recovery kernels are dense_kernels.hip's.
// A wave's block is 20 KB before its scratch, so the searchers are k_pool_search_w with as many wavefronts as a CU's LDS holds
// (dense_ah_wide_waves below), not k_pool_search's sixteen.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_ah_cost_wide on the host.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_dense.inc"

#define DENSE_AH_ROWS DENSE_AH_WIDE_MAX_N
#define DenseAhLdsR DenseAhWideLds
#define DenseAhSpaceLdsR DenseAhWideSpaceLds
#define DenseCostAhR DenseCostAhWide
#define DenseAhArgminRecR DenseAhWideArgminRec
#include "dense_ah_cost.inc"

#include "root_policy.inc"

#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

#include "launchers.inc"

#define DISPATCH_DAHWKW(A, FN, ...)                                        \
    switch ((A).KW) {                                                      \
    case 2: FN<DenseSpace<2, DenseCostAhWide>>(__VA_ARGS__); break;        \
    case 4: FN<DenseSpace<4, DenseCostAhWide>>(__VA_ARGS__); break;        \
    default: FN<DenseSpace<10, DenseCostAhWide>>(__VA_ARGS__); break;      \
    }
AZD_PHASE_ENTRIES(DISPATCH_DAHWKW)
static void no_argmin_one(const Arenas &, int, uint32_t, void *) {}
#define DENSE_AH_WIDE_NO_RESIDENT "dense-graph space: its CU-resident form is the pool searchers with the evaluator outside the kernel (engine.hip: dense_pool_run)"
static bool no_resident(const Arenas &, const FusedEval &, uint32_t *, size_t *, const char **why) {
    *why = DENSE_AH_WIDE_NO_RESIDENT;
    return false;
}
static bool no_pool(const Arenas &, const FusedEval &, PoolArgs *, uint32_t *, size_t *, const char **why) {
    *why = DENSE_AH_WIDE_NO_RESIDENT;
    return false;
}
const SpaceOps &dense_ah_wide_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr}};
    return ops;
}

// ---------------------------------------------------------------- pool step, searchers only
static_assert(sizeof(PoolIdle) <= POOL_SEARCH_STATIC_LDS, "space_ops.h: POOL_SEARCH_STATIC_LDS");
constexpr size_t DENSE_AH_WIDE_LDS = 160 * 1024;
// Wavefronts per searcher workgroup of one key width: as many blocks and scratch regions (DenseSpace::dyn_bytes, rounded up to 16)
// as a CU's 160 KB hold beside the kernel's static LDS -- six at every key width built here (a block is 20.4 .. 21.4 KB).  k_pool_search_w lays out that many
// blocks and is launch-bounded for them, so the plan below takes no more; it takes fewer under AZD_DENSE_POOL_WAVES.
template <class SP>
constexpr int dense_ah_wide_waves() {
    constexpr size_t scratch = (size_t)512 * SP::KW > CORE_DYN_BYTES ? (size_t)512 * SP::KW : CORE_DYN_BYTES;
    constexpr size_t per_wave = sizeof(typename SP::Lds) + ((scratch + 15) & ~(size_t)15);
    constexpr size_t fit = (DENSE_AH_WIDE_LDS - sizeof(PoolIdle) - 256 - 16) / per_wave;
    return fit > 16 ? 16 : fit < 1 ? 1 : (int)fit;
}
template <class SP>
static void q_pool_plan(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    constexpr int WAVES = dense_ah_wide_waves<SP>();
    const size_t stride = (SP::dyn_bytes(a) + 15) & ~(size_t)15;
    const size_t sw_bytes = (WAVES * sizeof(typename SP::Lds) + 15) & ~(size_t)15; // (k_pool_search_w's SW_BYTES: the layout of WAVES blocks)
    *dyn_stride = (uint32_t)stride;
    *dyn_bytes = sw_bytes + stride * (size_t)waves;
    *why = nullptr;
    if (waves < 1 || waves > WAVES || *dyn_bytes + sizeof(PoolIdle) + 256 > DENSE_AH_WIDE_LDS)
        *why = "pool step (Aouchiche-Hansen cost, 64 rows): a CU's 160 KB of LDS hold no more than 6 searcher waves' blocks and scratch";
}
static_assert(dense_ah_wide_waves<DenseSpace<2, DenseCostAhWide>>() == 6 && dense_ah_wide_waves<DenseSpace<4, DenseCostAhWide>>() == 6 &&
                  dense_ah_wide_waves<DenseSpace<10, DenseCostAhWide>>() == 6,
              "the wave count is spelled out in q_pool_plan's reason (and every width reaches the form's waves_min = 4)");
bool dense_ah_wide_pool_plan(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    if (a.B > 65536 || a.node_cap > 65536) {
        *why = "pool step: more than 65536 agents or nodes per tree";
        return false;
    }
    const char *bad = nullptr;
    DISPATCH_DAHWKW(a, q_pool_plan, a, waves, dyn_stride, dyn_bytes, &bad);
    if (bad) *why = bad;
    return bad == nullptr;
}
template <class SP>
static void l_pool_search(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves, uint32_t dyn_stride,
                          size_t dyn_bytes, hipStream_t st) {
    constexpr int WAVES = dense_ah_wide_waves<SP>();
    if (waves < 1 || waves > WAVES) return; // (the plan refuses it)
    if (sl.hashed) { // the test harness' evaluator (FusedEval kind 4): the searchers note the call of every row they post
        if (hipFuncSetAttribute((const void *)k_pool_search_w<SP, 1, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return;
        k_pool_search_w<SP, 1, WAVES><<<dim3(n_blocks), dim3(waves * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, dyn_stride);
    } else {
        if (hipFuncSetAttribute((const void *)k_pool_search_w<SP, 0, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return;
        k_pool_search_w<SP, 0, WAVES><<<dim3(n_blocks), dim3(waves * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, dyn_stride);
    }
    k_argmin_log1<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, sl.n_calls, sl.log_key, sl.ctl);
}
void dense_ah_wide_launch_pool_search(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves, uint32_t dyn_stride,
                                      size_t dyn_bytes, void *stream) {
    DISPATCH_DAHWKW(a, l_pool_search, a, d_args, sl, n_blocks, waves, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
template <class SP>
static void q_pool_search_resident(int *out, int waves, size_t dyn_bytes) {
    constexpr int WAVES = dense_ah_wide_waves<SP>();
    int nb = 0;
    if (waves < 1 || waves > WAVES ||
        hipFuncSetAttribute((const void *)k_pool_search_w<SP, 0, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_pool_search_w<SP, 0, WAVES>, waves * 64, dyn_bytes) != hipSuccess) {
        (void)hipGetLastError();
        nb = 0;
    }
    *out = nb;
}
int dense_ah_wide_pool_search_resident(const Arenas &a, int waves, size_t dyn_bytes) {
    int nb = 0;
    DISPATCH_DAHWKW(a, q_pool_search_resident, &nb, waves, dyn_bytes);
    return nb;
}

// one wave per graph, `reps` repetitions (timing), the result of the last one
__global__ __launch_bounds__(64) void k_probe_ah_cost_wide(const uint64_t *__restrict__ adj, const int n, const int count, const int reps,
                                                           const float slope, DenseAhCost *__restrict__ out) {
    __shared__ uint64_t s_adj[DENSE_AH_WIDE_MAX_N];
    __shared__ DenseAhWideLds w;
    const int g = blockIdx.x;
    if (g >= count) return;
    s_adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    DenseAhCost c;
    for (int r = 0; r < reps; ++r) {
        dense_ah_cost_wave(s_adj, w, n, slope, DenseNoHook{}, c);
        LDS_SYNC();
    }
    if (LANE == 0) out[g] = c;
}
void launch_probe_ah_cost_wide(const uint64_t *d_adj, int n, int count, int reps, DenseAhCost *d_out, void *stream) {
    k_probe_ah_cost_wide<<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, dense_ah_eval_slope(n), d_out);
}

} // namespace azd
