// ramsey64_ext_kernels.hip -- the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP) of the 64-bit Ramsey tier
// (AZD_ENGINE_RAMSEY_U64: N <= 64, E*C <= 2304): pool_step.inc's k_pool_search_w instantiated with RamseyExtSpace<RamseyU64Space>
// (ramsey_ext.inc) in a translation unit of its own, apart from ramsey64_kernels.hip's launch-per-phase kernels.  The evaluator's
// side (k_ext_take, the gathered GEMMs, k_ext_deliver) is the dense-graph space's: dense_kernels.hip, mlp_kernels.hip.
// Built with -ffp-contract=off like the other search units.
#define AZD_TU_ASYNC 1 // (no launch-per-phase kernel is built here)
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"
#include "ramsey_ext.inc"

using RamseyU64ExtSpace = RamseyExtSpace<RamseyU64Space>;

bool ramsey64_ext_pool_plan(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return rx_pool_plan<RamseyU64ExtSpace, RAMSEY64_EXT_WAVES>(a, waves, dyn_stride, dyn_bytes, why);
}
void ramsey64_ext_launch_pool_search(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves, uint32_t dyn_stride,
                                     size_t dyn_bytes, void *stream) {
    rx_pool_search<RamseyU64ExtSpace, RAMSEY64_EXT_WAVES>(a, d_args, sl, n_blocks, waves, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
int ramsey64_ext_pool_search_resident(const Arenas &, int waves, size_t dyn_bytes) { // workgroups of k_pool_search_w one CU holds
    int nb = 0;
    rx_pool_search_resident<RamseyU64ExtSpace, RAMSEY64_EXT_WAVES>(&nb, waves, dyn_bytes);
    return nb;
}

} // namespace azd
