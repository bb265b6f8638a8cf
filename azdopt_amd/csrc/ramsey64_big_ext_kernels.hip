// ramsey64_big_ext_kernels.hip -- the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP) of the 64-bit Ramsey tier with forbidden
// cliques up to K8 (AZD_ENGINE_RAMSEY_BIG_CLIQUES beside AZD_ENGINE_RAMSEY_U64): pool_step.inc's k_pool_search instantiated with
// RamseyExtSpace over space_ramsey.inc at a clique depth of 6, under the names ramsey64_big_kernels.hip gives it.  The evaluator's
// side (k_ext_take, the gathered GEMMs, k_ext_deliver) is shared with every other tier: dense_kernels.hip, mlp_kernels.hip.
// Built with -ffp-contract=off like the other search units.
#define AZD_TU_ASYNC 1 // (no launch-per-phase kernel is built here)
#define AZD_TU_POOL_SEARCH 1
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"

#define RAMSEY_CLIQUE_DEPTH 6
#define RamseyU64Space RamseyU64BigSpace
#define cliques_inside cliques_inside_big
#define ramsey_adjust ramsey_adjust_big
#include "space_ramsey.inc"

#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"
#include "ramsey_ext.inc"
#include "launchers.inc"

#define DISPATCH_RX64B(A, FN, ...) FN<RamseyExtSpace<RamseyU64BigSpace>>(__VA_ARGS__)
RAMSEY_EXT_POOL_SEARCH_ENTRIES(DISPATCH_RX64B, RAMSEY64_EXT_WAVES)
const PoolSearchOps &ramsey64_big_pool_search_ops() {
    static const PoolSearchOps ops = {AZD_POOL_SEARCH_OPS(RAMSEY64_EXT_WAVES)};
    return ops;
}

} // namespace azd
