// ramsey_kernels.hip -- Ramsey translation unit of the data-parallel tree-search step on gfx950:
// tree_core.inc instantiated with the RamseySpace policy (space_ramsey.inc), narrow and wide, the CU-resident
// persistent step, the device root policy and this unit's part of the Ramsey table (space_ops.h).
// Built with -ffp-contract=off like the c21 unit.
#include <hip/hip_runtime.h>

#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "root_policy.inc"
#include "launchers.inc"

AZD_PHASE_ENTRIES(DISPATCH_RKW)
static void e_argmin_one(const Arenas &a, int agent, uint32_t node, void *stream) {
    DISPATCH_RKW(a, l_argmin_one, a, agent, node, (hipStream_t)stream);
}
// LDS plan of the persistent step; false when the workgroup does not fit a CU or the in-kernel MLP
// cannot take the layer widths (it loads rows as float4)
static bool e_persist_plan(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return persist_plan_common(a, ev, dyn_stride, dyn_bytes, why, ramsey_dyn_bytes(a), ramsey_lds_bytes(a));
}
static void e_launch_persist(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl,
                             uint32_t *log_node, uint32_t dyn_stride, size_t dyn_bytes, void *stream) {
    DISPATCH_RKW(a, l_persist, a, d_args, sl, log_node, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
const PhaseOps &ramsey_phase_ops() {
    static const PhaseOps ops = {AZD_PHASE_OPS, e_argmin_one, e_persist_plan, e_launch_persist};
    return ops;
}

} // namespace azd
