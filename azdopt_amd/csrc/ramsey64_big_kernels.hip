// ramsey64_big_kernels.hip -- the 64-bit tier of the Ramsey space with forbidden cliques up to K8 (AZD_ENGINE_RAMSEY_BIG_CLIQUES beside
// AZD_ENGINE_RAMSEY_U64): ramsey64_kernels.hip's unit built with RamseyU64BigSpace (space_ramsey.inc: a clique depth of 6 --
// count_cliques_inside as fixed-depth nests for sizes up to AZD_RAMSEY_BIG_CLIQUE_MAX) in place of RamseyU64Space.  A translation
// unit of its own: with both spaces in one the kernels come out different, and an engine without the flag runs the kernels it ran
// before.
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "space_ops.h"

namespace azd {

#include "ramsey64_phase.inc"

template struct Ramsey64Phase<RamseyU64BigSpace>;
const SpaceOps &ramsey64_big_ops() { return Ramsey64Phase<RamseyU64BigSpace>::ops(); }

} // namespace azd
