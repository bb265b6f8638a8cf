// ramsey64_ext_kernels.hip -- the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP) of the 64-bit Ramsey tier
// (AZD_ENGINE_RAMSEY_U64: N <= 64, E*C <= 2304): pool_step.inc's k_pool_search instantiated with RamseyExtSpace<RamseyU64Space>
// (ramsey_ext.inc) in a translation unit of its own, apart from ramsey64_kernels.hip's launch-per-phase kernels.  The evaluator's
// side (k_ext_take, the gathered GEMMs, k_ext_deliver) is the dense-graph space's: dense_kernels.hip, mlp_kernels.hip.
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "ramsey_ext.inc"

#define DISPATCH_RX64(A, FN, ...) FN<RamseyExtSpace<RamseyU64Space>>(__VA_ARGS__)
RAMSEY_EXT_POOL_SEARCH_UNIT(DISPATCH_RX64, RAMSEY64_EXT_WAVES, ramsey64_pool_search_ops)

} // namespace azd
