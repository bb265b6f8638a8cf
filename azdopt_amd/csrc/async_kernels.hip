// async_kernels.hip -- the asynchronous CU-resident step (async_step.inc) for the c21 space in its own translation
// unit.  Co-compiled with k_persist in tree_kernels.hip, the shared device functions
// (rollout_agent, add_actions_agent) got different inlining/register allocation and k_persist's
// scratch use rose from 128 to 392 B/lane (-12 % end to end); separate TUs keep both at their own optimum.
#define AZD_TU_ASYNC 1
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_c21.inc"
#include "persistent_step.inc"
#include "async_step.inc"
#include "launchers.inc"

static bool e_async_plan(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return async_plan_common(a, ev, dyn_stride, dyn_bytes, why, dyn_lds_bytes(a.n), sizeof(WaveLds));
}
static void e_launch_async(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl,
                           const float *params, const void *wpk, uint32_t dyn_stride, size_t dyn_bytes, void *stream) {
    DISPATCH_KW(a, l_async, a, d_args, sl, params, wpk, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
const AsyncOps &c21_async_ops() {
    static const AsyncOps ops = {e_async_plan, e_launch_async};
    return ops;
}

} // namespace azd
