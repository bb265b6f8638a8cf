// dense_invs_kernels.hip -- translation unit of the dense-graph space's spectrum invariant cost (dense_invs_cost.inc: twenty-one
// invariants of a connected graph -- the extended invariant cost's sixteen, the energies of the adjacency, distance, Laplacian and
// signless-Laplacian matrices and the adjacency spread, each a function of a matrix's WHOLE spectrum -- combined by weights and up
// to four products or quotients given at run time; one wave per graph): tree_core.inc instantiated with
// DenseSpace<KW, DenseCostInvS> for key widths 2 / 4 / 10 (AZD_ENGINE_DENSE_INVS engines: n <= 32, so max_slots <= E <= 496) --
// launch-per-phase kernels and the device root policy -- built like dense_invx_kernels.hip, which this unit does not touch; and the
// probe that runs the cost outside any engine.  The pool step's searchers are NOT built for this tier (DESIGN.md "The spectrum
// invariant cost": their first run on a device ended in the step's own no-progress abort, cause not found): its engines run one
// launch per phase at every population.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_invs_cost on the host.
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

// a wave's block is the AH tier's at 32 rows, whatever the cost keeps in registers: the pool step's plan depends on it
static_assert(sizeof(DenseSpace<2, DenseCostInvS>::Lds) == sizeof(DenseAhSpaceLdsT<2, 32>) &&
                  sizeof(DenseSpace<4, DenseCostInvS>::Lds) == sizeof(DenseAhSpaceLdsT<4, 32>) &&
                  sizeof(DenseSpace<10, DenseCostInvS>::Lds) == sizeof(DenseAhSpaceLdsT<10, 32>),
              "the spectrum invariant cost adds nothing to a wave's LDS block");

#define DISPATCH_DINVSKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostInvS, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DINVSKW)
AZD_DENSE_NO_RESIDENT_ENTRIES
const SpaceOps &dense_invs_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 PoolSearchOps{}}; // (no searcher-only pool step: the tier's TierDesc::ext is null)
    return ops;
}

void launch_probe_invs_cost(const uint64_t *d_adj, int n, int count, int reps, const DenseInvsRecipe *d_recipe, DenseInvsCost *d_out, void *stream) {
    k_probe_invs_cost<DENSE_INVS_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, d_recipe, d_out);
}

} // namespace azd
