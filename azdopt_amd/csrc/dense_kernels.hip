// dense_kernels.hip -- dense-graph translation unit of the data-parallel tree-search step on gfx950: tree_core.inc
// instantiated with the DenseSpace policy (space_dense.inc) for key widths 2 / 4 / 10 / 16: launch-per-phase kernels, the
// device root policy, and the pool step's searchers (pool_step.inc: k_pool_search) with the evaluator OUTSIDE the kernel --
// the space's model (3676-512-512-512-2450 at N = 50) does not fit an evaluator workgroup's LDS, its rows are served by
// batched GEMM launches over what the searchers have posted (k_ext_take / k_ext_deliver).
// Built with -ffp-contract=off like the other tree units.
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_dense.inc"

#include "root_policy.inc"

#define AZD_TU_POOL_EXT 1
#define AZD_TU_POOL_SEARCH 1
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"

#include "launchers.inc"

AZD_PHASE_ENTRIES(DISPATCH_DKW)
AZD_DENSE_NO_RESIDENT_ENTRIES
// pool step, searchers only: 16 waves per workgroup, or as many as the LDS holds (the engine's knob: fewer leave registers and LDS
// on the CU for the evaluator's GEMM blocks)
#define DENSE_POOL_LDS "pool step: 16 searcher waves' blocks and scratch do not fit the CU's 160 KB of LDS (more than 640 slots per root)"
AZD_POOL_SEARCH_ENTRIES(DISPATCH_DKW, PERSIST_WAVES, "pool step: more than 65536 agents or nodes per tree", DENSE_POOL_LDS, DENSE_POOL_LDS)
const SpaceOps &dense_ops() {
    static const SpaceOps ops = {{AZD_PHASE_OPS, no_argmin_one, no_resident, nullptr}, {no_resident, nullptr}, {no_pool, nullptr, nullptr},
                                 {AZD_POOL_SEARCH_OPS(PERSIST_WAVES)}};
    return ops;
}

// ---------------------------------------------------------------- the evaluator's side of the searcher-only pool step
void launch_ext_take(const PoolArgs &pool, uint32_t *rows, uint32_t *home, uint32_t *n, unsigned long long *t0, void *stream) {
    k_ext_take<<<dim3(1), dim3(POOL_XCDS * 64), 0, (hipStream_t)stream>>>(pool, rows, home, n, t0);
}
// ---------------------------------------------------------------- recovery of an aborted pool launch by the launch-per-phase kernels
// resume[t] = calls agent t has completed | 1u << 31 if its last call ended on a node whose prediction row is still due (k_pool_resume_scan)
__global__ void k_park(Arenas a, const uint32_t *__restrict__ resume, const int n_calls, const int round, const int park) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.B) return;
    uint32_t f = a.flags[t] & ~(uint32_t)FLAG_PARKED;
    if (park) {
        const uint32_t r = resume[t];
        const bool sits_out = round < 0 ? (r >> 31) == 0u : (int)(r & 0x7FFFFFFFu) + round >= n_calls;
        if (sits_out) f |= (uint32_t)FLAG_PARKED;
    }
    a.flags[t] = f;
}
void launch_park(const Arenas &a, const uint32_t *resume, int n_calls, int round, int park, void *stream) {
    k_park<<<dim3((a.B + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(a, resume, n_calls, round, park);
}
// the candidates of the agents that took part in round r, each under the call it really was (optimizer/mod.rs:194-246 up to the choice among trees)
__global__ void k_log_candidates_resume(Arenas a, unsigned long long *__restrict__ log_key, const uint32_t *__restrict__ resume, const int n_calls,
                                        const int round) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.B) return;
    const uint32_t node = a.cand_node[t];
    const int call = (int)(resume[t] & 0x7FFFFFFFu) + round;
    if (node != NONE && a.flags[t] == 0 && call < n_calls) {
        const unsigned long long key = ((unsigned long long)ordf(a.cand_c[t]) << 32) | ((unsigned long long)((uint32_t)t & 0xFFFFu) << 16) |
                                       (unsigned long long)(node & 0xFFFFu);
        atomicMin(&log_key[call], key);
        a.cand_node[t] = NONE; // num_inspected_nodes = nodes.len()
    }
}
void launch_log_candidates_resume(const Arenas &a, unsigned long long *log_key, const uint32_t *resume, int n_calls, int round, void *stream) {
    k_log_candidates_resume<<<dim3((a.B + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(a, log_key, resume, n_calls, round);
}
void launch_ext_hash_rows(const PersistArgs *d_args, const uint32_t *rows, const uint32_t *n, uint32_t cap, float *h_theta, void *stream) {
    k_ext_hash_rows<<<dim3(cap), dim3(256), 0, (hipStream_t)stream>>>(d_args, rows, n, h_theta);
}
void launch_ext_deliver(const PoolArgs &pool, const Arenas &a, const uint32_t *rows, const uint32_t *home, const uint32_t *n, uint32_t cap,
                        const unsigned long long *t0, void *stream) {
    k_ext_deliver<<<dim3((cap + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(pool, a, rows, home, n, t0);
}
// ---------------------------------------------------------------- the default cost outside any engine (tests)
void launch_probe_dense_cost(const uint64_t *d_adj, int n, int count, const uint16_t *d_toggles, int n_toggles, double *d_lam, int *d_mu,
                             uint8_t *d_mate, int *d_hooks, void *stream) {
    k_probe_dense_cost<2><<<dim3(count), dim3(64), 0, (hipStream_t)stream>>>(d_adj, n, count, d_toggles, n_toggles, d_lam, d_mu, d_mate, d_hooks);
}

} // namespace azd
