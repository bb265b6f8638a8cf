// ramsey64_kernels.hip -- the 64-bit tier of the Ramsey space (AZD_ENGINE_RAMSEY_U64: N <= 64 over uint64_t neighbourhood rows,
// E*C <= 2304, keys of 36 words): tree_core.inc instantiated with RamseyU64Space (space_ramsey.inc) in a translation unit of its
// own, so that its kernels' register allocation and build time stay apart from the 32-bit tiers'.  Launch-per-phase kernels and the
// device root policy, and the tier's table (ramsey64_phase.inc).
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "space_ops.h"

namespace azd {

#include "ramsey64_phase.inc"

template struct Ramsey64Phase<RamseyU64Space>;
const SpaceOps &ramsey64_ops() { return Ramsey64Phase<RamseyU64Space>::ops(); }

} // namespace azd
