// ramsey64_phase.inc -- a launch-per-phase unit of the 64-bit Ramsey tier, but for its space: the search core, the space policies,
// the launchers, and the unit's table (space_ops.h) as a template over the space.  ramsey64_kernels.hip builds it with
// RamseyU64Space, ramsey64_big_kernels.hip with RamseyU64BigSpace.  Included inside namespace azd after space_ops.h.
#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "root_policy.inc"
#include "launchers.inc"

// A unit instantiates it explicitly (`template struct Ramsey64Phase<SP>;`), so that the entries come into being in the order written
// here, as plain functions would: that order is the order in which hipcc instantiates the kernels, and the kernels' code depends on
// it (launchers.inc).  (Hidden: the entries stay inside the library, as static functions would.)
template <class SP>
struct __attribute__((visibility("hidden"))) Ramsey64Phase {
#define DISPATCH_SP(A, FN, ...) FN<SP>(__VA_ARGS__)
    AZD_PHASE_ENTRIES(DISPATCH_SP)
    static void e_argmin_one(const Arenas &a, int agent, uint32_t node, void *stream) {
        DISPATCH_SP(a, l_argmin_one, a, agent, node, (hipStream_t)stream);
    }
#undef DISPATCH_SP
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
    // (the searcher-only part stays null here: the tier's *_ext_kernels.hip exports it, engine.hip joins the two)
    static const SpaceOps &ops() {
        static const SpaceOps ops = {{AZD_PHASE_OPS, e_argmin_one, no_persist, nullptr}, {no_async, nullptr}, {no_pool, nullptr, nullptr}};
        return ops;
    }
};
