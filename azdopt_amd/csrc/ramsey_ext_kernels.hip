// ramsey_ext_kernels.hip -- the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP) of the 32-bit wide Ramsey tier (max_slots > 0:
// N <= 32, E*C <= 1024): pool_step.inc's k_pool_search_w instantiated with RamseyExtSpace<RamseyWideSpace<10 / 16>> (ramsey_ext.inc)
// in a translation unit of its own, so that the register allocation of the existing Ramsey units stays as it is.  The evaluator's
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

// key widths of a wide engine: 10 (E*C <= 640) or 16
#define DISPATCH_RXW(A, FN, ...)                                                                  \
    do {                                                                                          \
        if ((A).KW == 10) FN<RamseyExtSpace<RamseyWideSpace<10>>, RAMSEY_EXT_WAVES>(__VA_ARGS__); \
        else FN<RamseyExtSpace<RamseyWideSpace<16>>, RAMSEY_EXT_WAVES>(__VA_ARGS__);              \
    } while (0)

bool ramsey_ext_pool_plan(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return a.KW == 10 ? rx_pool_plan<RamseyExtSpace<RamseyWideSpace<10>>, RAMSEY_EXT_WAVES>(a, waves, dyn_stride, dyn_bytes, why)
                      : rx_pool_plan<RamseyExtSpace<RamseyWideSpace<16>>, RAMSEY_EXT_WAVES>(a, waves, dyn_stride, dyn_bytes, why);
}
void ramsey_ext_launch_pool_search(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves, uint32_t dyn_stride,
                                   size_t dyn_bytes, void *stream) {
    DISPATCH_RXW(a, rx_pool_search, a, d_args, sl, n_blocks, waves, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
int ramsey_ext_pool_search_resident(const Arenas &a, int waves, size_t dyn_bytes) { // workgroups of k_pool_search_w one CU holds
    int nb = 0;
    DISPATCH_RXW(a, rx_pool_search_resident, &nb, waves, dyn_bytes);
    return nb;
}

} // namespace azd
