// dense_inv_kernels.hip -- translation unit of the dense-graph space's third objective, the weighted-invariant cost
// (dense_inv_cost.inc: ten invariants of a connected graph -- degrees, eccentricities, transmissions, one eigenvalue each of the
// adjacency and the distance matrix -- combined with weights given at run time; one wave per graph): tree_core.inc instantiated
// with DenseSpace<KW, DenseCostInv> for key widths 2 / 4 / 10 (AZD_ENGINE_DENSE_INV engines: n <= 32, so max_slots <= E <= 496) --
// launch-per-phase kernels, the device root policy, the pool step's searchers -- built like dense_ah_kernels.hip, which this unit
// does not touch; the evaluator side of the pool step (k_ext_*) and the recovery kernels are dense_kernels.hip's; and the probe
// that runs the cost outside any engine.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_inv_cost on the host.
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

#define DISPATCH_DINVKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostInv, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DINVKW)
AZD_DENSE_NO_RESIDENT_ENTRIES
// pool step, searchers only.  A wave's block is the 32-row AH block, so the engine plans the AH tier's wave counts (ext_plan counts
// down from 16): 10 at key width 2, 9 at 4, 7 at 10.
#define DENSE_INV_POOL_LDS "pool step (weighted-invariant cost): the searcher waves' blocks and scratch do not fit the CU's 160 KB of LDS"
AZD_POOL_SEARCH_ENTRIES(DISPATCH_DINVKW, PERSIST_WAVES, "pool step: more than 65536 agents or nodes per tree", DENSE_INV_POOL_LDS, DENSE_INV_POOL_LDS)
const SpaceOps &dense_inv_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 {AZD_POOL_SEARCH_OPS(PERSIST_WAVES)}};
    return ops;
}

void launch_probe_inv_cost(const uint64_t *d_adj, int n, int count, int reps, const DenseInvRecipe *d_recipe, DenseInvCost *d_out, void *stream) {
    k_probe_inv_cost<DENSE_INV_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, d_recipe, d_out);
}

} // namespace azd
