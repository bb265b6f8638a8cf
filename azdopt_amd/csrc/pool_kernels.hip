// pool_kernels.hip -- the pool step (pool_step.inc: agents multiplexed over searcher waves, evaluator workgroups on
// CUs of their own) for the c21 space, in its own translation unit like the asynchronous step (async_kernels.hip);
// also the pool step's helpers that are the same for every space (resume scan, tile-forward test entry, XCC probe).
#define AZD_TU_ASYNC 1
#define AZD_TU_POOL 1
#include <hip/hip_runtime.h>

#include "bf16.h"
#include "c21_host.h"
#include "space_ops.h"

namespace azd {

#include "tree_core.inc"
#include "space_c21.inc"
#include "persistent_step.inc"
#include "async_step.inc"
#include "pool_step.inc"
#include "launchers.inc"

// LDS plan of the pool step: a searcher wave's scratch (with room to build its state-vector row) or an evaluator's
// batch of 16 rows [x][h0][h1][out], whichever is larger
static bool e_pool_plan(const Arenas &a, const FusedEval &ev, PoolArgs *pool, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {
    return pool_plan_common(a, ev, pool, dyn_stride, dyn_bytes, why, C21Space<1>::pool_dyn_bytes(a), sizeof(WaveLds));
}
static void e_launch_pool(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, const float *params,
                          const void *wpk, int n_blocks, uint32_t dyn_stride, size_t dyn_bytes, void *stream) {
    DISPATCH_KW(a, l_pool, a, d_args, sl, params, wpk, n_blocks, dyn_stride, dyn_bytes, (hipStream_t)stream);
}
static int e_pool_max_resident(const Arenas &a, size_t dyn_bytes, int n_cus) {
    int nb = 0;
    DISPATCH_KW(a, q_pool_resident, &nb, dyn_bytes);
    return nb * n_cus;
}
const PoolOps &c21_pool_ops() {
    static const PoolOps ops = {e_pool_plan, e_launch_pool, e_pool_max_resident};
    return ops;
}

// Test entry (azd_engine_debug_tile_forward): the forward of the IN-KERNEL evaluator -- pool_eval's staging and mlp_tile_task's
// sums, 16 rows per workgroup -- for rows the host hands over.  A prediction row does not depend on the batch it travels in
// (every output element is its own chain of sums), so these are the rows k_pool's evaluator workgroups hand their agents: the
// oracle is fed with them, call by call, to check a whole launch of the PRODUCT kernel k_pool<SP, 0> with the real model
// (tests/test_gpu_pool.py).  f32 or bf16 storage, as the engine's evaluator has it.
__global__ __launch_bounds__(PERSIST_WAVES * 64) void k_tile_forward(const FusedEval ev, const float *__restrict__ params, const void *__restrict__ wpk,
                                                                     const uint32_t stride, const uint32_t out_off, const int n_rows,
                                                                     const float *__restrict__ states, float *__restrict__ out) {
    __shared__ uint32_t agents[PERSIST_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, first = blockIdx.x * PERSIST_WAVES;
    const int n = n_rows - first < PERSIST_WAVES ? n_rows - first : PERSIST_WAVES;
    const int S = ev.dims[0], S16 = (S + 15) & ~15, L = ev.n_layers, A = ev.dims[L];
    if (tid < PERSIST_WAVES) agents[tid] = (uint32_t)(first + tid);
    PoolRows rows;
    rows.stride = stride;
    rows.out_off = out_off;
    rows.agents = agents;
    rows.n = n;
    EvalPtrs gp;
    gp.params = params;
    gp.wpk = wpk;
    gp.state_vecs = states;
    gp.h_theta = out;
    for (int idx = tid; idx < n * S16; idx += PERSIST_WAVES * 64) {
        const int r = idx / S16, c = idx - r * S16;
        const float v = c < S ? states[(size_t)(first + r) * S + c] : 0.f;
        if (ev.bf16) reinterpret_cast<uint16_t *>(rows.row(r))[c] = (uint16_t)bf16_bits(v);
        else rows.row(r)[c] = v;
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
        const int nt = (ev.dims[l + 1] + 15) >> 4;
        for (int tile = wave; tile < nt; tile += PERSIST_WAVES) {
            unsigned long long ph[3];
            mlp_tile_task<PoolRows, true>(ev, rows, gp, l, tile, ph);
        }
        __syncthreads();
    }
    for (int idx = tid; idx < n * A; idx += PERSIST_WAVES * 64) {
        const int r = idx / A, c = idx - r * A;
        out[(size_t)(first + r) * A + c] = rows.out(r)[c];
    }
}
hipError_t launch_tile_forward(const FusedEval &ev, const PoolArgs &pool, int n_rows, const float *states, float *out, void *stream) {
    const size_t dyn_bytes = (size_t)pool.eval_stride * sizeof(float) * PERSIST_WAVES;
    hipError_t he = hipFuncSetAttribute((const void *)k_tile_forward, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes);
    if (he != hipSuccess) return he;
    k_tile_forward<<<dim3((n_rows + PERSIST_WAVES - 1) / PERSIST_WAVES), dim3(PERSIST_WAVES * 64), dyn_bytes, (hipStream_t)stream>>>(
        ev, ev.params, ev.wpk, pool.eval_stride, pool.eval_out_off, n_rows, states, out);
    return hipGetLastError(); // (a launch that was refused -- LDS, grid -- must not leave the caller copying an unwritten buffer back)
}
// After an aborted pool launch (PoolCtl::abort: a wait ran into its bound): where every agent stands, for the asynchronous
// step that takes over (StepLaunch::resume).  A wave never leaves an agent inside a call, so an agent is in one of three
// states: never taken (index >= claimed: no call made), waiting for the prediction row of its last call's new node (the node
// it stands on has no actions yet; PendRec::call = calls completed), or through all its calls.
__global__ void k_pool_resume_scan(Arenas a, const PendRec *__restrict__ pend, const uint32_t *__restrict__ claim_next, const int n_calls,
                                   uint32_t *__restrict__ resume) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.B) return;
    const uint32_t claimed = *claim_next; // claims handed out (it runs past B once every agent is taken)
    uint32_t r = 0u;
    if ((uint32_t)t < claimed) {
        const NodeRec nd = a.nodes[(size_t)t * a.node_cap + a.state_pos[t]];
        const bool pending = a.flags[t] == 0u && nd.act_end == 0u;
        r = pending ? (pend[t].call | 0x80000000u) : (uint32_t)n_calls;
    }
    resume[t] = r;
}
void launch_pool_resume_scan(const Arenas &a, const PoolArgs &pool, int n_calls, uint32_t *resume, void *stream) {
    k_pool_resume_scan<<<dim3((a.B + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(a, pool.pend, &pool.ctl->claim_next, n_calls, resume);
}
__global__ void k_probe_xcc(uint32_t *out) {
    if (threadIdx.x == 0) out[blockIdx.x] = pool_xcc_id();
}
void launch_probe_xcc(uint32_t *d_out, int n_blocks, void *stream) {
    k_probe_xcc<<<dim3(n_blocks), dim3(64), 0, (hipStream_t)stream>>>(d_out);
}

} // namespace azd
