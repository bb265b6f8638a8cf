// dense_invx_kernels.hip -- translation unit of the dense-graph space's extended invariant cost (dense_invx_cost.inc: sixteen
// invariants of a connected graph -- the weighted-invariant cost's ten, one eigenvalue each of the Laplacian and the signless
// Laplacian, the Randic index, the Zagreb indices, the triangle count -- combined by weights and up to four products or quotients
// given at run time; one wave per graph): tree_core.inc instantiated with DenseSpace<KW, DenseCostInvX> for key widths 2 / 4 / 10
// (AZD_ENGINE_DENSE_INVX engines: n <= 32, so max_slots <= E <= 496) -- launch-per-phase kernels, the device root policy, the pool
// step's searchers -- built like dense_inv_kernels.hip, which this unit does not touch; the evaluator side of the pool step
// (k_ext_*) and the recovery kernels are dense_kernels.hip's; and the probe that runs the cost outside any engine.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_invx_cost on the host.
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

// a wave's block is the AH tier's at 32 rows, whatever the cost keeps in registers: the pool step's plan depends on it
static_assert(sizeof(DenseSpace<2, DenseCostInvX>::Lds) == sizeof(DenseAhSpaceLdsT<2, DENSE_INVX_MAX_N>) &&
                  sizeof(DenseSpace<4, DenseCostInvX>::Lds) == sizeof(DenseAhSpaceLdsT<4, DENSE_INVX_MAX_N>) &&
                  sizeof(DenseSpace<10, DenseCostInvX>::Lds) == sizeof(DenseAhSpaceLdsT<10, DENSE_INVX_MAX_N>),
              "the extended invariant cost adds nothing to a wave's LDS block: the pool step plans the INV tier's 10 / 9 / 7 waves");

#define DISPATCH_DINVXKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostInvX, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DINVXKW)
AZD_DENSE_NO_RESIDENT_ENTRIES
// pool step, searchers only.  A wave's block is the 32-row AH block, so the engine plans the AH tier's wave counts (ext_plan counts
// down from 16): 10 at key width 2, 9 at 4, 7 at 10.
#define DENSE_INVX_POOL_LDS "pool step (extended invariant cost): the searcher waves' blocks and scratch do not fit the CU's 160 KB of LDS"
AZD_POOL_SEARCH_ENTRIES(DISPATCH_DINVXKW, PERSIST_WAVES, "pool step: more than 65536 agents or nodes per tree", DENSE_INVX_POOL_LDS, DENSE_INVX_POOL_LDS)
const SpaceOps &dense_invx_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 {AZD_POOL_SEARCH_OPS(PERSIST_WAVES)}};
    return ops;
}

void launch_probe_invx_cost(const uint64_t *d_adj, int n, int count, int reps, const DenseInvxRecipe *d_recipe, DenseInvxCost *d_out, void *stream) {
    k_probe_invx_cost<DENSE_INVX_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, d_recipe, d_out);
}

} // namespace azd
