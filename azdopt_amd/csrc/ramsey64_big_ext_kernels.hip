// ramsey64_big_ext_kernels.hip -- the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP) of the 64-bit Ramsey tier with forbidden
// cliques up to K8 (AZD_ENGINE_RAMSEY_BIG_CLIQUES beside AZD_ENGINE_RAMSEY_U64): pool_step.inc's k_pool_search instantiated with
// RamseyExtSpace<RamseyU64BigSpace> (ramsey_ext.inc; space_ramsey.inc: a clique depth of 6), apart from ramsey64_ext_kernels.hip's
// for sizes up to 5.  The evaluator's side (k_ext_take, the gathered GEMMs, k_ext_deliver) is shared with every other tier:
// dense_kernels.hip, mlp_kernels.hip.
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "ramsey_ext.inc"

#define DISPATCH_RX64B(A, FN, ...) FN<RamseyExtSpace<RamseyU64BigSpace>>(__VA_ARGS__)
RAMSEY_EXT_POOL_SEARCH_UNIT(DISPATCH_RX64B, RAMSEY64_EXT_WAVES, ramsey64_big_pool_search_ops)

} // namespace azd
