// ramsey64_kernels.hip -- the 64-bit tier of the Ramsey space (AZD_ENGINE_RAMSEY_U64: N <= 64 over uint64_t neighbourhood rows,
// E*C <= 2304, keys of 36 words): tree_core.inc instantiated with RamseyU64Space (space_ramsey.inc) in a translation unit of its
// own, so that its kernels' register allocation and build time stay apart from the 32-bit tiers'.  Launch-per-phase kernels and the
// device root policy, and the tier's table (space_ops.h).
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "root_policy.inc"
#include "launchers.inc"

AZD_PHASE_ENTRIES(DISPATCH_RU64)
static void e_argmin_one(const Arenas &a, int agent, uint32_t node, void *stream) {
    DISPATCH_RU64(a, l_argmin_one, a, agent, node, (hipStream_t)stream);
}
// The tier runs the launch-per-phase form only: a workgroup of the CU-resident forms keeps 16 waves' clique counts in LDS,
// 144 KB of the CU's 160 at the reference's R(3,3,3,3) shape before anything else.
#define RAMSEY_U64_NO_RESIDENT(FORM) FORM ": not built for the 64-bit Ramsey tier (it runs one launch per phase)"
static bool no_persist(const Arenas &, const FusedEval &, uint32_t *, size_t *, const char **why) {
    *why = RAMSEY_U64_NO_RESIDENT("barrier step");
    return false;
}
static bool no_async(const Arenas &, const FusedEval &, uint32_t *, size_t *, const char **why) {
    *why = RAMSEY_U64_NO_RESIDENT("asynchronous step");
    return false;
}
static bool no_pool(const Arenas &, const FusedEval &, PoolArgs *, uint32_t *, size_t *, const char **why) {
    *why = RAMSEY_U64_NO_RESIDENT("pool step");
    return false;
}
const SpaceOps &ramsey64_ops() { // (the searcher-only part stays null here: ramsey64_ext_kernels.hip exports it, engine.hip joins the two)
    static const SpaceOps ops = {{AZD_PHASE_OPS, e_argmin_one, no_persist, nullptr}, {no_async, nullptr}, {no_pool, nullptr, nullptr}};
    return ops;
}

} // namespace azd
