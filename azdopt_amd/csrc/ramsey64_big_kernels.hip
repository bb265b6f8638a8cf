// ramsey64_big_kernels.hip -- the 64-bit tier of the Ramsey space with forbidden cliques up to K8 (AZD_ENGINE_RAMSEY_BIG_CLIQUES beside
// AZD_ENGINE_RAMSEY_U64): space_ramsey.inc with a clique depth of 6 -- count_cliques_inside as fixed-depth nests for sizes up to
// AZD_RAMSEY_BIG_CLIQUE_MAX -- under names of its own, and tree_core.inc instantiated with that space: launch-per-phase kernels,
// the device root policy and the tier's table (space_ops.h), as ramsey64_kernels.hip has them for sizes up to 5.  That unit is
// not touched by this one: an engine without the flag runs the kernels it ran before.
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "space_ops.h"

namespace azd {

#include "tree_core.inc"

#define RAMSEY_CLIQUE_DEPTH 6
#define RamseyU64Space RamseyU64BigSpace
#define cliques_inside cliques_inside_big
#define ramsey_adjust ramsey_adjust_big
#include "space_ramsey.inc"

#include "persistent_step.inc"
#include "root_policy.inc"
#include "launchers.inc"

AZD_PHASE_ENTRIES(DISPATCH_RU64)
static void e_argmin_one(const Arenas &a, int agent, uint32_t node, void *stream) {
    DISPATCH_RU64(a, l_argmin_one, a, agent, node, (hipStream_t)stream);
}
// The launch-per-phase form only, for the 64-bit tier's reason (ramsey64_kernels.hip: 16 waves' clique counts do not fit a CU's LDS)
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
const SpaceOps &ramsey64_big_ops() { // (the searcher-only part stays null here: ramsey64_big_ext_kernels.hip exports it, engine.hip joins the two)
    static const SpaceOps ops = {{AZD_PHASE_OPS, e_argmin_one, no_persist, nullptr}, {no_async, nullptr}, {no_pool, nullptr, nullptr}};
    return ops;
}

} // namespace azd
