// dense_invs_wide_kernels.hip -- the spectrum invariant cost of the dense-graph space up to 64 vertices (AZD_ENGINE_DENSE_INVS_WIDE beside
// AZD_ENGINE_DENSE_INVS): dense_invs_cost.inc's DenseCostInvSWide, the cost at a row limit of 64 -- the packed triangle is 2080 doubles,
// 16.6 KB a wave, shared by the distance, adjacency, Laplacian and signless-Laplacian passes; at n = 64 every lane of the wave owns a
// row of the reduction and an eigenvalue of the whole-spectrum finisher -- and tree_core.inc instantiated with
// DenseSpace<KW, DenseCostInvSWide> for key widths 2 / 4 / 10 (max_slots <= min(E, 640)): launch-per-phase kernels, the device root
// policy and the cost probe, as dense_invs_kernels.hip has them for 32 rows.  That unit, the INVX, INV and AH units and
// dense_kernels.hip are not touched by this one.
// The pool step's searchers are NOT built for this tier, as they are not for the narrow one (DESIGN.md "No pool step on this tier":
// the narrow tier's searchers hung on their first run on a device, cause not found): its engines run one launch per phase at every
// population.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_invs_cost_wide on the host.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_dense.inc"
#include "dense_spectral.inc"
#include "dense_invs_cost.inc"

#include "root_policy.inc"

#define AZD_TU_POOL_SEARCH 1
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

#include "launchers.inc"

// a wave's block is the AH-wide tier's, whatever the cost keeps in registers
static_assert(sizeof(DenseSpace<2, DenseCostInvSWide>::Lds) == sizeof(DenseAhSpaceLdsT<2, 64>) &&
                  sizeof(DenseSpace<4, DenseCostInvSWide>::Lds) == sizeof(DenseAhSpaceLdsT<4, 64>) &&
                  sizeof(DenseSpace<10, DenseCostInvSWide>::Lds) == sizeof(DenseAhSpaceLdsT<10, 64>),
              "the spectrum invariant cost adds nothing to a wave's LDS block");
static_assert(DENSE_INVS_WIDE_MAX_N == DENSE_AH_WIDE_MAX_N, "the host side of this cost is sized by DENSE_AH_WIDE_MAX_N");

#define DISPATCH_DINVSWKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostInvSWide, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DINVSWKW)
AZD_DENSE_NO_RESIDENT_ENTRIES
const SpaceOps &dense_invs_wide_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 PoolSearchOps{}}; // (no searcher-only pool step: the tier's TierDesc::ext is null)
    return ops;
}

void launch_probe_invs_cost_wide(const uint64_t *d_adj, int n, int count, int reps, const DenseInvsRecipe *d_recipe, DenseInvsCost *d_out, void *stream) {
    k_probe_invs_cost<DENSE_INVS_WIDE_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, d_recipe, d_out);
}

} // namespace azd
