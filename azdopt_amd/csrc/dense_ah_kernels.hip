// dense_ah_kernels.hip -- translation unit of the dense-graph space's second objective, the Aouchiche-Hansen cost
// (dense_ah_cost.inc: all-sources BFS, Householder tridiagonalisation in LDS, Sturm-count multisection; one wave per graph):
// tree_core.inc instantiated with DenseSpace<KW, DenseCostAH> for key widths 2 / 4 / 10 (AZD_ENGINE_DENSE_AH engines: n <= 32, so
// max_slots <= E <= 496) -- launch-per-phase kernels, the device root policy, the pool step's searchers -- built like
// dense_kernels.hip, whose evaluator side (k_ext_*) and recovery kernels serve these engines too; and the probes that run the cost
// and its f64 primitives outside any engine.
// Built with -ffp-contract=off like the other tree units: the cost is bit-identical to azd_dense_ah_cost on the host.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_dense.inc"
#include "dense_spectral.inc"
#include "dense_ah_cost.inc"

#include "root_policy.inc"

#define AZD_TU_POOL_SEARCH 1
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

#include "launchers.inc"

#define DISPATCH_DAHKW(A, FN, ...) DISPATCH_DKW_COST(DenseCostAH, A, FN, __VA_ARGS__)
AZD_PHASE_ENTRIES(DISPATCH_DAHKW)
AZD_DENSE_NO_RESIDENT_ENTRIES
// pool step, searchers only (dense_kernels.hip has the default cost's).  A wave's block carries the cost's working set (4.1 KB of
// matrix): sixteen blocks and sixteen scratch regions are beyond a CU's LDS, so the engine plans fewer waves per workgroup (ext_plan
// counts down from 16): 10 at key width 2, 9 at 4, 7 at 10.
#define DENSE_AH_POOL_LDS "pool step (Aouchiche-Hansen cost): the searcher waves' blocks and scratch do not fit the CU's 160 KB of LDS"
AZD_POOL_SEARCH_ENTRIES(DISPATCH_DAHKW, PERSIST_WAVES, "pool step: more than 65536 agents or nodes per tree", DENSE_AH_POOL_LDS, DENSE_AH_POOL_LDS)
const SpaceOps &dense_ah_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 {AZD_POOL_SEARCH_OPS(PERSIST_WAVES)}};
    return ops;
}

void launch_probe_ah_cost(const uint64_t *d_adj, int n, int count, int reps, DenseAhCost *d_out, void *stream) {
    k_probe_ah_cost<DENSE_AH_MAX_N><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, reps, dense_ah_eval_slope(n), d_out);
}

// parity probe of the f64 primitives the cost depends on bit for bit: out[3 i] = x / y, [3 i + 1] = sqrt(|x|), [3 i + 2] = x - x / y * y
__global__ void k_probe_math_f64(const double *__restrict__ in, double *__restrict__ out, const int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = in[2 * i], y = in[2 * i + 1];
    const double q = x / y;
    out[3 * i] = q;
    out[3 * i + 1] = sqrt(fabs(x));
    const double m = q * y;
    out[3 * i + 2] = x - m;
}
void launch_probe_math_f64(const double *d_in, double *d_out, int n, void *stream) {
    k_probe_math_f64<<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(d_in, d_out, n);
}

} // namespace azd
