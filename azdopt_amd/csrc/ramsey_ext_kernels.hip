// ramsey_ext_kernels.hip -- the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP) of the 32-bit wide Ramsey tier (max_slots > 0:
// N <= 32, E*C <= 1024): pool_step.inc's k_pool_search instantiated with RamseyExtSpace<RamseyWideSpace<10 / 16>> (ramsey_ext.inc)
// in a translation unit of its own, so that the register allocation of the existing Ramsey units stays as it is.  The evaluator's
// side (k_ext_take, the gathered GEMMs, k_ext_deliver) is the dense-graph space's: dense_kernels.hip, mlp_kernels.hip.
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "ramsey_ext.inc"

// key widths of a wide engine: 10 (E*C <= 640) or 16
#define DISPATCH_RXW(A, FN, ...)                                                \
    do {                                                                        \
        if ((A).KW == 10) FN<RamseyExtSpace<RamseyWideSpace<10>>>(__VA_ARGS__); \
        else FN<RamseyExtSpace<RamseyWideSpace<16>>>(__VA_ARGS__);              \
    } while (0)
RAMSEY_EXT_POOL_SEARCH_UNIT(DISPATCH_RXW, RAMSEY_EXT_WAVES, ramsey_pool_search_ops)

} // namespace azd
