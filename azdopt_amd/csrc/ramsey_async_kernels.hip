// ramsey_async_kernels.hip -- the asynchronous CU-resident step (async_step.inc) for the Ramsey space, in
// its own translation unit like the c21 one (async_kernels.hip): co-compiled with k_persist the shared
// device functions are register-allocated worse.
#define AZD_TU_ASYNC 1
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "async_step.inc"
#include "launchers.inc"

// the per-wave region holds the search scratch + the clique counts during a call
static bool e_async_plan(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return async_plan_common(a, ev, dyn_stride, dyn_bytes, why, ramsey_dyn_bytes(a), ramsey_lds_bytes(a));
}
static void e_launch_async(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl,
                           const float *params, const void *wpk, uint32_t dyn_stride, size_t dyn_bytes, void *stream) {
    DISPATCH_RKW(a, l_async, a, d_args, sl, params, wpk, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
const AsyncOps &ramsey_async_ops() {
    static const AsyncOps ops = {e_async_plan, e_launch_async};
    return ops;
}

} // namespace azd
