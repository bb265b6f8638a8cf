// ramsey_pool_kernels.hip -- the pool step (pool_step.inc) for the Ramsey space, in its own translation unit.
#define AZD_TU_ASYNC 1
#define AZD_TU_POOL 1
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"
#include "launchers.inc"

static bool e_pool_plan(const Arenas &a, const FusedEval &ev, PoolArgs *pool, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return pool_plan_common(a, ev, pool, dyn_stride, dyn_bytes, why, ramsey_pool_dyn_bytes(a), ramsey_lds_bytes(a));
}
static void e_launch_pool(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, const float *params,
                          const void *wpk, int n_blocks, uint32_t dyn_stride, size_t dyn_bytes, void *stream) {
    DISPATCH_RKW(a, l_pool, a, d_args, sl, params, wpk, n_blocks, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
static int e_pool_max_resident(const Arenas &a, size_t dyn_bytes, int n_cus) {
    int nb = 0;
    DISPATCH_RKW(a, q_pool_resident, &nb, dyn_bytes);
    return nb * n_cus;
}
const PoolOps &ramsey_pool_ops() {
    static const PoolOps ops = {e_pool_plan, e_launch_pool, e_pool_max_resident};
    return ops;
}

} // namespace azd
