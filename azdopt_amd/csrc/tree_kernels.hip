// tree_kernels.hip -- c21 translation unit of the data-parallel tree-search step on gfx950:
// tree_core.inc (space-independent search) instantiated with the C21Space policy (space_c21.inc),
// the CU-resident persistent step, the device root policy, the probes and this unit's part of the
// c21 table (space_ops.h).  (async_kernels.hip and pool_kernels.hip hold the other two parts;
// ramsey_kernels.hip is the same core with the Ramsey policy.)
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_c21.inc"

__global__ void k_hash_predictions(float *out, int batch, int action_dim, uint64_t seed, uint64_t first_agent,
                                   uint64_t call) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)batch * action_dim;
    if (i >= total) return;
    uint64_t agent = first_agent + i / action_dim, act = i % action_dim;
    uint64_t r = splitmix(splitmix(splitmix(splitmix(seed ^ 0x70726564ull) ^ agent) ^ call) ^ act);
    out[i] = (float)(r >> 40) * (1.0f / 16777216.0f);
}

#include "persistent_step.inc"
#include "root_policy.inc"
#include "launchers.inc"

// parity probe for the f32 primitives the selection rule depends on; four outputs per input pair:
//   [0] the kernel's own sqrt(|x - y|) (azd_sqrt)   [1] sqrtf   [2] __fsqrt_rn   [3] x - (x - y)
__global__ void k_probe_math(const float *in, float *out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = in[2 * i], y = in[2 * i + 1];
    float d = fabsf(x - y);
    out[4 * i] = azd_sqrt(d);
    float g = x - y;
    out[4 * i + 3] = x - g;
}

// the alternatives, in a kernel of their own so that nothing is shared with azd_sqrt above
__global__ void k_probe_sqrt_alt(const float *in, float *out, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float d = fabsf(in[2 * i] - in[2 * i + 1]);
    out[4 * i + 1] = sqrtf(d);
    out[4 * i + 2] = (float)sqrt((double)d);
}

// lambda_1 / matching probe: one wave per tree, `reps` repetitions (timing), result of the last one
__global__ __launch_bounds__(64) void k_probe_cost(const uint8_t *__restrict__ parents, int n, int count, int reps,
                                                   int full, double *__restrict__ lam_out, int *__restrict__ mu_out, double lo0, double hi0) {
    __shared__ WaveLds s;
    const uint32_t dyn = 0;
    const int t = blockIdx.x;
    if (t >= count) return;
    if (LANE < PARENTS_STRIDE) s.par[LANE] = LANE < n ? parents[(size_t)t * n + LANE] : 0;
    WAVE_SYNC();
    double lam = 0.0;
    int mu = 0;
    for (int r = 0; r < reps; ++r) {
        const PackedTree pt = pack_tree(s, n);
        lam = full ? lambda1_wave<true>(pt, n, dyn, lo0, hi0) : lambda1_wave<false>(pt, n, dyn, lo0, hi0);
        mu = full ? matching_wave(s, n, nullptr) : matching_size_wave(pt, n);
        WAVE_SYNC();
    }
    if (LANE == 0) {
        lam_out[t] = lam;
        mu_out[t] = mu;
    }
}

AZD_PHASE_ENTRIES(DISPATCH_KW)
static void e_argmin_one(const Arenas &a, int agent, uint32_t node, void *stream) {
    DISPATCH_KW(a, l_argmin_one, a, agent, node, (hipStream_t)stream);
}
// LDS plan of the persistent step; returns false when the workgroup does not fit a CU
static bool e_persist_plan(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return persist_plan_common(a, ev, dyn_stride, dyn_bytes, why, dyn_lds_bytes(a.n), sizeof(WaveLds));
}
static void e_launch_persist(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl,
                             uint32_t *log_node, uint32_t dyn_stride, size_t dyn_bytes, void *stream) {
    DISPATCH_KW(a, l_persist, a, d_args, sl, log_node, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
const PhaseOps &c21_phase_ops() {
    static const PhaseOps ops = {AZD_PHASE_OPS, e_argmin_one, e_persist_plan, e_launch_persist};
    return ops;
}

void launch_log_candidates(const Arenas &a, unsigned long long *log_key, uint32_t *call_ctr, void *stream) {
    k_log_candidates<<<dim3(1), dim3(1024), 0, (hipStream_t)stream>>>(a, log_key, call_ctr);
}
void launch_hash_predictions(float *d_out, int batch, int action_dim, uint64_t seed, uint64_t first_agent,
                             uint64_t call, void *stream) {
    size_t total = (size_t)batch * action_dim;
    int threads = 256;
    int blocks = (int)((total + threads - 1) / threads);
    hipLaunchKernelGGL(k_hash_predictions, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, d_out, batch, action_dim,
                       seed, first_agent, call);
}
void launch_probe_cost(const uint8_t *d_parents, int n, int count, int reps, int full, double *d_lam, int *d_mu,
                       void *stream) {
    double lo0, hi0;
    c21_lambda_bracket(n, &lo0, &hi0);
    k_probe_cost<<<dim3(count), dim3(64), dyn_lds_bytes(n), (hipStream_t)stream>>>(d_parents, n, count, reps, full, d_lam, d_mu, lo0, hi0);
}
void launch_probe_math(const float *d_in, float *d_out, int n, void *stream) {
    hipLaunchKernelGGL(k_probe_math, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_out, n);
    hipLaunchKernelGGL(k_probe_sqrt_alt, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_in, d_out, n);
}

} // namespace azd
