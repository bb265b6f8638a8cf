// dense_inv_wide_kernels.hip -- the weighted-invariant cost of the dense-graph space up to 64 vertices (AZD_ENGINE_DENSE_INV_WIDE beside
// AZD_ENGINE_DENSE_INV): dense_inv_cost.inc's DenseCostInvWide, the cost at a row limit of 64 -- the packed triangle is 2080 doubles,
// 16.6 KB a wave, shared by the distance and the adjacency pass -- and tree_core.inc instantiated with
// DenseSpace<KW, DenseCostInvWide> for key widths 2 / 4 / 10 (max_slots <= min(E, 640)): launch-per-phase kernels, the device root
// policy, the pool step's searchers and the cost probe, as dense_inv_kernels.hip has them for 32 rows.  That unit, the AH units and
// dense_kernels.hip are not touched by this one; the evaluator side of the pool step (k_ext_*) and the recovery kernels are
// dense_kernels.hip's.
// A wave's block is the AH-wide tier's (DenseAhSpaceLdsT<KW, 64>: 20 KB before its scratch), so the searchers are k_pool_search
// built for as many wavefronts as a CU's LDS holds (dense_inv_wide_waves below: six), not the other dense units' sixteen.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_inv_cost_wide on the host.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_dense.inc"
#include "dense_spectral.inc"
#include "dense_inv_cost.inc"

#include "root_policy.inc"

#define AZD_TU_POOL_SEARCH 1
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

#include "launchers.inc"

#define DISPATCH_DINVWKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostInvWide, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DINVWKW)
AZD_DENSE_NO_RESIDENT_ENTRIES

// ---------------------------------------------------------------- pool step, searchers only
constexpr size_t DENSE_INV_WIDE_LDS = 160 * 1024;
// Wavefronts per searcher workgroup of one key width: as many blocks and scratch regions (DenseSpace::dyn_bytes, rounded up to 16)
// as a CU's 160 KB hold beside the kernel's static LDS -- the AH-wide tier's count, because the block is that tier's.
// k_pool_search is built for that many: the plan takes no more (ext_plan's count-down from AZD_DENSE_POOL_WAVES lands there) and
// takes fewer under the knob.
template <class SP>
constexpr int dense_inv_wide_waves() {
    constexpr size_t scratch = (size_t)512 * SP::KW > CORE_DYN_BYTES ? (size_t)512 * SP::KW : CORE_DYN_BYTES;
    constexpr size_t per_wave = sizeof(typename SP::Lds) + ((scratch + 15) & ~(size_t)15);
    constexpr size_t fit = (DENSE_INV_WIDE_LDS - sizeof(PoolIdle) - 256 - 16) / per_wave;
    return fit > 16 ? 16 : fit < 1 ? 1 : (int)fit;
}
constexpr int DENSE_INV_WIDE_WAVES = 6;
static_assert(dense_inv_wide_waves<DenseSpace<2, DenseCostInvWide>>() == DENSE_INV_WIDE_WAVES &&
                  dense_inv_wide_waves<DenseSpace<4, DenseCostInvWide>>() == DENSE_INV_WIDE_WAVES &&
                  dense_inv_wide_waves<DenseSpace<10, DenseCostInvWide>>() == DENSE_INV_WIDE_WAVES,
              "the wave count is spelled out in the plan's reason (and every width reaches the form's waves_min = 4)");
#define DENSE_INV_WIDE_POOL_LDS "pool step (weighted-invariant cost, 64 rows): a CU's 160 KB of LDS hold no more than 6 searcher waves' blocks and scratch"
AZD_POOL_SEARCH_ENTRIES(DISPATCH_DINVWKW, DENSE_INV_WIDE_WAVES, "pool step: more than 65536 agents or nodes per tree", DENSE_INV_WIDE_POOL_LDS,
                        DENSE_INV_WIDE_POOL_LDS)
const SpaceOps &dense_inv_wide_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 {AZD_POOL_SEARCH_OPS(DENSE_INV_WIDE_WAVES)}};
    return ops;
}

void launch_probe_inv_cost_wide(const uint64_t *d_adj, int n, int count, int reps, const DenseInvRecipe *d_recipe, DenseInvCost *d_out, void *stream) {
    k_probe_inv_cost<DENSE_INV_WIDE_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, d_recipe, d_out);
}

} // namespace azd
