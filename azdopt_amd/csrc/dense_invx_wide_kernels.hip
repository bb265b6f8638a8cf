// dense_invx_wide_kernels.hip -- the extended invariant cost of the dense-graph space up to 64 vertices (AZD_ENGINE_DENSE_INVX_WIDE beside
// AZD_ENGINE_DENSE_INVX): dense_invx_cost.inc's DenseCostInvXWide, the cost at a row limit of 64 -- the packed triangle is 2080 doubles,
// 16.6 KB a wave, shared by the distance, adjacency, Laplacian and signless-Laplacian passes -- and tree_core.inc instantiated with
// DenseSpace<KW, DenseCostInvXWide> for key widths 2 / 4 / 10 (max_slots <= min(E, 640)): launch-per-phase kernels, the device root
// policy, the pool step's searchers and the cost probe, as dense_invx_kernels.hip has them for 32 rows.  That unit, the INV and AH
// units and dense_kernels.hip are not touched by this one; the evaluator side of the pool step (k_ext_*) and the recovery kernels are
// dense_kernels.hip's.
// A wave's block is the AH-wide tier's (DenseAhSpaceLdsT<KW, 64>: 20 KB before its scratch), so the searchers are k_pool_search
// built for as many wavefronts as a CU's LDS holds (dense_invx_wide_waves below: six), as in dense_inv_wide_kernels.hip.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_invx_cost_wide on the host.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_dense.inc"
#include "dense_spectral.inc"
#include "dense_invx_cost.inc"

#include "root_policy.inc"

#define AZD_TU_POOL_SEARCH 1
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

#include "launchers.inc"

// a wave's block is the AH-wide tier's, whatever the cost keeps in registers: the pool step's plan depends on it
static_assert(sizeof(DenseSpace<2, DenseCostInvXWide>::Lds) == sizeof(DenseAhSpaceLdsT<2, DENSE_AH_WIDE_MAX_N>) &&
                  sizeof(DenseSpace<4, DenseCostInvXWide>::Lds) == sizeof(DenseAhSpaceLdsT<4, DENSE_AH_WIDE_MAX_N>) &&
                  sizeof(DenseSpace<10, DenseCostInvXWide>::Lds) == sizeof(DenseAhSpaceLdsT<10, DENSE_AH_WIDE_MAX_N>),
              "the extended invariant cost adds nothing to a wave's LDS block: the pool step plans the AH-wide tier's waves");

#define DISPATCH_DINVXWKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostInvXWide, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DINVXWKW)
AZD_DENSE_NO_RESIDENT_ENTRIES

// ---------------------------------------------------------------- pool step, searchers only
constexpr size_t DENSE_INVX_WIDE_LDS = 160 * 1024;
// Wavefronts per searcher workgroup of one key width: as many blocks and scratch regions (DenseSpace::dyn_bytes, rounded up to 16)
// as a CU's 160 KB hold beside the kernel's static LDS -- the AH-wide and INV-wide tiers' count, because the block is theirs.
// k_pool_search is built for that many: the plan takes no more (ext_plan's count-down from AZD_DENSE_POOL_WAVES lands there) and
// takes fewer under the knob.
template <class SP>
constexpr int dense_invx_wide_waves() {
    constexpr size_t scratch = (size_t)512 * SP::KW > CORE_DYN_BYTES ? (size_t)512 * SP::KW : CORE_DYN_BYTES;
    constexpr size_t per_wave = sizeof(typename SP::Lds) + ((scratch + 15) & ~(size_t)15);
    constexpr size_t fit = (DENSE_INVX_WIDE_LDS - sizeof(PoolIdle) - 256 - 16) / per_wave;
    return fit > 16 ? 16 : fit < 1 ? 1 : (int)fit;
}
constexpr int DENSE_INVX_WIDE_WAVES = 6;
static_assert(dense_invx_wide_waves<DenseSpace<2, DenseCostInvXWide>>() == DENSE_INVX_WIDE_WAVES &&
                  dense_invx_wide_waves<DenseSpace<4, DenseCostInvXWide>>() == DENSE_INVX_WIDE_WAVES &&
                  dense_invx_wide_waves<DenseSpace<10, DenseCostInvXWide>>() == DENSE_INVX_WIDE_WAVES,
              "the wave count is spelled out in the plan's reason (and every width reaches the form's waves_min = 4)");
#define DENSE_INVX_WIDE_POOL_LDS "pool step (extended invariant cost, 64 rows): a CU's 160 KB of LDS hold no more than 6 searcher waves' blocks and scratch"
AZD_POOL_SEARCH_ENTRIES(DISPATCH_DINVXWKW, DENSE_INVX_WIDE_WAVES, "pool step: more than 65536 agents or nodes per tree", DENSE_INVX_WIDE_POOL_LDS,
                        DENSE_INVX_WIDE_POOL_LDS)
const SpaceOps &dense_invx_wide_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 {AZD_POOL_SEARCH_OPS(DENSE_INVX_WIDE_WAVES)}};
    return ops;
}

void launch_probe_invx_cost_wide(const uint64_t *d_adj, int n, int count, int reps, const DenseInvxRecipe *d_recipe, DenseInvxCost *d_out, void *stream) {
    k_probe_invx_cost<DENSE_INVX_WIDE_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, d_recipe, d_out);
}

} // namespace azd
