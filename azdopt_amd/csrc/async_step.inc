// async_step.inc -- included by the asynchronous and pool units (inside namespace azd), after persistent_step.inc.
//
// Asynchronous CU-resident form of NablaOptimizer::par_roll_out_episodes.  As in k_persist one
// workgroup = 16 wavefronts = 16 agents lives on one CU for `n_calls` calls, but the agents are
// NOT kept in lock-step: within an epoch the model is constant and trees never exchange data, so
// agent i's k-th call depends on nothing but agent i -- the reference's barrier between the two
// rayon sections (optimizer/mod.rs:159-189) is an artefact of batching the model call, not of the
// algorithm.  Here an agent that needs a prediction row posts a request and, while it waits,
// SERVES the workgroup's evaluator: waiting waves form batches of the posted rows (<= 16 = one
// v_mfma_f32_16x16x4_f32 tile of M) and pull (layer, column-tile) tasks from LDS tickets; weights
// stream from L2, a row's activations live in the LDS region of the agent that posted it (idle while
// it waits), so the evaluator runs concurrently with the agents that are still searching.
// Effect: a launch lasts as long as the slowest agent's SUM over n_calls calls (which
// concentrates), not n_calls times the slowest single call.
// Results are bit-identical to k_persist: same per-agent call sequence, same MFMA k-order per
// output element.  The per-call argmin (optimizer/mod.rs:190,194-246) is replayed afterwards from
// log_key[call] = min over agents of (ord(c), agent, node), kept by a 64-bit atomic min.

struct AsyncCtl {
    uint32_t req[PERSIST_WAVES];   // 0 idle, 1 posted, 2 in batch, 3 done
    uint32_t rows[PERSIST_WAVES];  // wave ids of the active batch's rows
    uint32_t nrows;
    uint32_t lock;                 // batch-creation lock
    uint32_t active;               // 1 while a batch is in flight
    uint32_t gen;                  // number of batches created so far
    uint32_t tile_next[8];         // per layer: tickets handed out, monotonic over batches
    uint32_t tile_done[8];         // per layer: tiles completed, monotonic over batches
    uint32_t finished;             // waves that completed all their calls
    uint32_t prog[PERSIST_WAVES];  // calls completed per wave (the launch ends with the slowest chain)
    unsigned long long t_open;     // diagnostic: time the active batch was opened
};

#define LDS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define LDS_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define WG_RELEASE() __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup")
#define WG_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup")

// Global pointers the evaluator streams from.  They are passed down from KERNEL ARGUMENTS (not
// read out of the argument block in memory) so that the compiler knows their address space and
// emits global_load (vmcnt only) instead of flat_load.
struct EvalPtrs {
    const void *__restrict__ wpk; // fragment-major weights (FusedEval::wpk): f32 words, or bf16 halves under FusedEval::bf16
    const float *__restrict__ params;
    const float *state_vecs; // aliased by Arenas::state_vecs / h_theta inside the same kernel
    float *h_theta;
};

// Where a posted row keeps its activations: in the dynamic LDS region of the agent that posted it.
// That agent is waiting for this very batch, so its search scratch (selection lists, cascade
// frontier, lambda_1 columns) is dead until the batch closes.  Layout inside the region, skewed by
// 16 B per wave so that the 16 rows of a tile hit different banks:  [x: S][h0: hid[0]][h1: hid[1]] (FusedEval::hid).
__device__ __forceinline__ float *row_lds(const uint32_t owner_wave, const uint32_t dyn_stride) {
    return reinterpret_cast<float *>(lds_base(owner_wave * dyn_stride) + 16u * owner_wave);
}

typedef short bf16x4 __attribute__((ext_vector_type(4)));

// Where a batch of rows lives, for mlp_tile_task: the asynchronous step keeps row r in the LDS region of the agent
// that posted it (the pool step, pool_step.inc, keeps its batch in the evaluator workgroup's own LDS).
struct AsyncRows {
    AsyncCtl &ctl;
    uint32_t dyn_stride;
    int t0;
    __device__ __forceinline__ int count() const { return (int)LDS_LOAD(&ctl.nrows); }
    __device__ __forceinline__ float *row(const int r) const { return row_lds(LDS_LOAD(&ctl.rows[r]), dyn_stride); }
    __device__ __forceinline__ int agent(const int r) const { return t0 + (int)LDS_LOAD(&ctl.rows[r]); }
    __device__ __forceinline__ float *out(const int) const { return nullptr; } // unused: the head's rows go straight to h_theta
};

// one (layer, column-tile) task of a batch: A rows from LDS (see row_lds), weights from L2.
// MLP_PF weight quads are requested together before the first is used.
// LAST_TO_LDS: the head's rows go to LDS too (Rows::out, f32 whatever the storage) instead of to h_theta: the pool
// step stores them from there with whole-row write-through stores.
#ifndef AZD_MLP_PF
#define AZD_MLP_PF 8 // (4 / 6 / 12 / 16 measured in the pool step, round 5: profiles/r05_group_exchange.txt)
#endif
constexpr int MLP_PF = AZD_MLP_PF;
template <class Rows, bool LAST_TO_LDS = false>
__device__ void mlp_tile_task(const FusedEval &ev, const Rows &rows, const EvalPtrs &gp, const int l, const int tile,
                              unsigned long long *ph) {
    ph[0] = PH_NOW();
    const int lane = LANE;
    const int L = ev.n_layers;
    const int K = ev.dims[l], N = ev.dims[l + 1];
    const int S4 = (ev.dims[0] + 15) & ~15, H = ev.hid[0]; // x padded with zeros to whole k-steps; buffer 1 starts H after buffer 0
    const int nrows = rows.count();
    const int n0 = tile * 16;
    // A rows: batch row r = lane & 15
    const int r = lane & 15;
    const int rr = r < nrows ? r : 0;
    float *const rbase = rows.row(rr);
    const float *arow = rbase + (l == 0 ? 0 : S4 + ((l - 1) & 1) * H);
    const float *ap = arow + 4 * (lane >> 4);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // Weights come in fragment order: k-step s of this tile is one contiguous piece, lane l's quad at
    // [(tile * steps + s) * 64 + l] (zeros outside the matrix, so ragged widths need no special case:
    // the last k-step of a ragged input multiplies x's zero padding, the columns past N are not stored).
    // Row-major weights gave every k-step 16 pieces of 64 B; a round of 16 tile tasks on a CU then took
    // 7.0 us whatever the number of serving waves, i.e. the evaluator was bound by its weight stream;
    // in this order it takes 4.4 us, the MFMA time (tools/probes/tile_probe.hip).
    const int steps = (K + 15) >> 4;
    const size_t frag = (size_t)ev.p_off[l] + ((size_t)tile * steps * 64 + lane) * 4;
    ph[1] = PH_NOW();
    if (ev.bf16) {
        // bf16 weight storage: one v_mfma_f32_16x16x16_bf16 per k-step (lane l: A[row l&15][k0 + 4(l>>4) + i],
        // B[k0 + 4(l>>4) + i][col l&15], i = 0..3) takes the place of four f32 MFMAs; the A quad is
        // rounded to bf16 as it is read, products are exact in f32, accumulation is f32
        // the rows are kept in LDS as bf16 halves in this mode (rounded once, where they are written: the row copy
        // and the epilogue below), same layout in units of 2 bytes
        const uint16_t *wq = reinterpret_cast<const uint16_t *>(gp.wpk) + frag;
        const uint16_t *ap16 = reinterpret_cast<const uint16_t *>(rbase) + (l == 0 ? 0 : S4 + ((l - 1) & 1) * H) + 4 * (lane >> 4);
        // whole groups of MLP_PF k-steps without a branch inside: the weight requests, then the rows' LDS reads
        // (their latency passes under the weights'), then the MFMAs; the remaining steps one by one
        int s0 = 0;
        for (; s0 + MLP_PF <= steps; s0 += MLP_PF) {
            uint2 bq[MLP_PF], aq[MLP_PF];
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j) bq[j] = *reinterpret_cast<const uint2 *>(wq + 256 * (s0 + j));
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j) aq[j] = *reinterpret_cast<const uint2 *>(ap16 + 16 * (s0 + j));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j) {
                bf16x4 a4, b4;
                __builtin_memcpy(&a4, &aq[j], 8);
                __builtin_memcpy(&b4, &bq[j], 8);
                acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a4, b4, acc, 0, 0, 0);
            }
        }
        if (s0 < steps) {
            uint2 bq[MLP_PF];
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (s0 + j < steps) bq[j] = *reinterpret_cast<const uint2 *>(wq + 256 * (s0 + j));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (s0 + j < steps) {
                    const uint2 bv = bq[j];
                    const uint2 ab = *reinterpret_cast<const uint2 *>(ap16 + 16 * (s0 + j));
                    bf16x4 a4, b4;
                    __builtin_memcpy(&a4, &ab, 8);
                    __builtin_memcpy(&b4, &bv, 8);
                    acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a4, b4, acc, 0, 0, 0);
                }
        }
    } else {
        const float *wp = reinterpret_cast<const float *>(gp.wpk) + frag;
        int s0 = 0;
        for (; s0 + MLP_PF <= steps; s0 += MLP_PF) {
            float4 bq[MLP_PF];
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j) bq[j] = *reinterpret_cast<const float4 *>(wp + 256 * (s0 + j));
            // the rows' quads two steps ahead of their use (three live instead of all eight: registers)
            float4 a0 = *reinterpret_cast<const float4 *>(ap + 16 * s0);
            float4 a1 = *reinterpret_cast<const float4 *>(ap + 16 * (s0 + 1));
            __builtin_amdgcn_sched_barrier(0); // keep the requests together: the scheduler otherwise sinks them to their uses
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j) {
                float4 a2 = a1;
                if (j + 2 < MLP_PF) a2 = *reinterpret_cast<const float4 *>(ap + 16 * (s0 + j + 2));
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bq[j].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bq[j].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bq[j].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bq[j].w, acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                a0 = a1;
                a1 = a2;
            }
        }
        if (s0 < steps) {
            float4 bq[MLP_PF];
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (s0 + j < steps) bq[j] = *reinterpret_cast<const float4 *>(wp + 256 * (s0 + j));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (s0 + j < steps) {
                    const float4 bv = bq[j];
                    const float4 av = *reinterpret_cast<const float4 *>(ap + 16 * (s0 + j));
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
                }
        }
    }
    ph[2] = PH_NOW();
    const int col = n0 + (lane & 15);
    if (col < N) {
        const float bj = gp.params[ev.b_off[l] + col];
        const int act = (l == L - 1) ? ev.final_act : 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 4 * (lane >> 4) + i;
            if (row < nrows) {
                const float v = act_apply(acc[i] + bj, act);
                if (l == L - 1 && !LAST_TO_LDS) gp.h_theta[(size_t)rows.agent(row) * N + col] = v;
                else if (l == L - 1) rows.out(row)[col] = v;
                else if (ev.bf16) reinterpret_cast<uint16_t *>(rows.row(row))[S4 + (l & 1) * H + col] = (uint16_t)bf16_bits(v);
                else rows.row(row)[S4 + (l & 1) * H + col] = v;
            }
        }
    }
}

// Serve the evaluator until `done()` holds: create a batch if none is active and requests are
// posted, otherwise pull tile tasks of the active batch.  Wave-uniform; lane 0 owns the LDS atomics.
// Batching policy: a batch costs the same whether it carries 1 row or 16 (one MFMA row tile, the
// whole weight set streamed once), so opening one greedily for whatever is posted made the evaluator
// the bottleneck (5 rows per batch, 12 us of evaluator time per row).  A batch is opened when
// AZD_ASYNC_MIN_ROWS requests are posted, when nobody is left searching (every live agent is posted or
// through), or at once when the agent furthest behind posts.  With that last rule in place the threshold
// wants to be high (2: 22.0, 4: 22.3, 6: 22.7, 8: 22.9, 10: 23.0, 12: 22.9 M expansions/s): everyone but the
// slowest agent can afford to wait for company, and fuller batches stream the weights less often.
#ifndef AZD_ASYNC_LAG_SLACK
#define AZD_ASYNC_LAG_SLACK 0
#endif
#ifndef AZD_ASYNC_BASE_PRIO
#define AZD_ASYNC_BASE_PRIO 0
#endif
#ifndef AZD_ASYNC_LAG_PRIO
#define AZD_ASYNC_LAG_PRIO 8 // agents within this many calls of the slowest one search at raised wave priority (+4.5 %; 0..32 alike)
#endif
#ifndef AZD_ASYNC_MIN_ROWS
#define AZD_ASYNC_MIN_ROWS 10
#endif
template <class LDS, typename DoneFn>
__device__ __forceinline__ void serve_evaluator(const FusedEval &ev, AsyncCtl &ctl, const EvalPtrs &gp, const int t0, LDS &s, const int n_live,
                                const uint32_t dyn_stride, DoneFn done) {
    const int L = ev.n_layers;
    for (;;) {
        if (done()) return;
        const uint32_t active = uni(LDS_LOAD(&ctl.active));
        if (!active) {
            // try to open a batch
            uint32_t got = 0;
            if (LANE == 0) got = atomicCAS(&ctl.lock, 0u, 1u) == 0u ? 1u : 0u;
            got = uni(got);
            if (got) {
                if (LANE == 0) {
                    uint32_t n = 0;
                    uint32_t posted = 0, searching = 0;
                    uint32_t min_prog = 0xFFFFFFFFu, min_posted = 0xFFFFFFFFu;
                    for (int w = 0; w < n_live; ++w) {
                        const uint32_t st = LDS_LOAD(&ctl.req[w]);
                        const uint32_t pr = LDS_LOAD(&ctl.prog[w]);
                        posted += st == 1u ? 1u : 0u;
                        searching += (st == 0u || st == 3u) ? 1u : 0u; // 3: served, about to go on
                        min_prog = pr < min_prog ? pr : min_prog;
                        if (st == 1u) min_posted = pr < min_posted ? pr : min_posted;
                    }
                    searching -= LDS_LOAD(&ctl.finished) < searching ? LDS_LOAD(&ctl.finished) : searching;
                    // the launch lasts as long as the slowest agent's chain of calls: the agent that is
                    // furthest behind never waits for company
                    const bool urgent = posted > 0u && min_posted <= min_prog + (uint32_t)AZD_ASYNC_LAG_SLACK;
                    const bool open = posted >= (uint32_t)AZD_ASYNC_MIN_ROWS || (posted > 0u && searching == 0u) || urgent;
                    if (open && LDS_LOAD(&ctl.active) == 0u) {
                        for (int w = 0; w < PERSIST_WAVES; ++w) {
                            if (LDS_LOAD(&ctl.req[w]) == 1u) {
                                LDS_STORE(&ctl.rows[n], (uint32_t)w);
                                LDS_STORE(&ctl.req[w], 2u);
                                ++n;
                            }
                        }
                        if (n) {
                            LDS_STORE(&ctl.nrows, n);
                            LDS_STORE(&ctl.gen, LDS_LOAD(&ctl.gen) + 1u);
                            ctl.t_open = PH_NOW();
                            WG_RELEASE();
                            LDS_STORE(&ctl.active, 1u);
                            CTR_ADD(25, 1);
                            CTR_ADD(26, n);
                        }
                    }
                    WG_RELEASE();
                    LDS_STORE(&ctl.lock, 0u);
                }
            }
            if (!uni(LDS_LOAD(&ctl.active))) {
                __builtin_amdgcn_s_sleep(8);
                continue;
            }
        }
        // ---- work on the active batch g (tickets are monotonic: layer l of batch g owns
        //      [g*nt, (g+1)*nt) of tile_next[l] / tile_done[l])
        WG_ACQUIRE();
        const uint32_t g = uni(LDS_LOAD(&ctl.gen)) - 1u;
        for (int l = 0; l < L; ++l) {
            const uint32_t nt = (uint32_t)((ev.dims[l + 1] + 15) / 16);
            const uint32_t lim = (g + 1u) * nt;
            if (l > 0) { // inputs of layer l are complete once every tile of layer l-1 is
                const uint32_t need = (g + 1u) * (uint32_t)((ev.dims[l] + 15) / 16);
                while (uni(LDS_LOAD(&ctl.tile_done[l - 1])) < need) __builtin_amdgcn_s_sleep(1);
                WG_ACQUIRE();
            }
            for (;;) {
                uint32_t ticket = 0xFFFFFFFFu;
                if (LANE == 0) {
                    uint32_t cur = LDS_LOAD(&ctl.tile_next[l]);
                    while (cur < lim) {
                        const uint32_t prev = atomicCAS(&ctl.tile_next[l], cur, cur + 1u);
                        if (prev == cur) {
                            ticket = cur;
                            break;
                        }
                        cur = prev;
                    }
                }
                ticket = uni(ticket);
                if (ticket == 0xFFFFFFFFu) break;
                const unsigned long long tt0 = PH_NOW();
                unsigned long long ph[3];
                mlp_tile_task(ev, AsyncRows{ctl, dyn_stride, t0}, gp, l, (int)(ticket - g * nt), ph);
                CTR_ADD(27, 1);
                CTR_ADD(28, PH_NOW() - tt0);
                CTR_ADD(30, ph[1] - ph[0]); // diagnostic build: set-up / k loop split of a tile task
                CTR_ADD(31, ph[2] - ph[1]);
                WG_RELEASE(); // the tile's stores are complete before it is counted
                uint32_t fin = 0;
                if (LANE == 0) fin = atomicAdd(&ctl.tile_done[l], 1u) + 1u;
                fin = uni(fin);
                if (l == L - 1 && fin == lim) {
                    // last tile of the last layer: hand the rows back and close the batch
                    if (LANE == 0) {
                        const uint32_t n = LDS_LOAD(&ctl.nrows);
                        for (uint32_t r = 0; r < n; ++r) LDS_STORE(&ctl.req[LDS_LOAD(&ctl.rows[r])], 3u);
                        CTR_ADD(29, PH_NOW() - ctl.t_open);
                        WG_RELEASE();
                        LDS_STORE(&ctl.active, 0u);
                    }
                }
            }
        }
        // the batch may still be finishing in other waves; loop (done() / next batch / short sleep)
        if (uni(LDS_LOAD(&ctl.active)) && uni(LDS_LOAD(&ctl.gen)) - 1u == g) __builtin_amdgcn_s_sleep(2);
    }
}

template <class SP>
__global__ __launch_bounds__(PERSIST_WAVES * 64) void k_async(const PersistArgs *__restrict__ pa, int n_calls,
                                                              unsigned long long *__restrict__ log_key,
                                                              uint32_t dyn_stride,
                                                              const float *__restrict__ params,
                                                              const float *state_vecs, // also written through pa->a.state_vecs (write_vec): no __restrict__
                                                              float *h_theta,          // also read through pa->a.h_theta (add_actions)
                                                              const void *__restrict__ wpk, const uint32_t *__restrict__ resume) {
    const Arenas &a = pa->a;
    const TolTable &tol = pa->tol;
    const FusedEval &ev = pa->ev;
    __shared__ typename SP::Lds sw[PERSIST_WAVES];
    __shared__ AsyncCtl ctl;
    const int wave = threadIdx.x >> 6;
    const int t0 = blockIdx.x * PERSIST_WAVES;
    const int t = t0 + wave;
    const bool active = t < a.B;
    typename SP::Lds &s = sw[wave];
    const uint32_t dyn = (uint32_t)wave * dyn_stride;
    EvalPtrs gp;
    gp.params = params;
    gp.wpk = wpk;
    gp.state_vecs = state_vecs;
    gp.h_theta = h_theta;
    if (threadIdx.x < sizeof(AsyncCtl) / 4) reinterpret_cast<uint32_t *>(&ctl)[threadIdx.x] = 0u;
    SP::prepare(a, s);
    if (LANE < NUM_COUNTERS) s.ctr[LANE] = 0;
    __syncthreads();
    const int n_live = (a.B - t0) < PERSIST_WAVES ? (a.B - t0) : PERSIST_WAVES;
    if (active) {
        // the evaluator for this agent's posted row + add_actions (optimizer/mod.rs:175-189 for one agent)
        auto predict_and_add = [&](const RolloutOut &ro, const int call) __attribute__((always_inline)) {
            if (ev.kind == 3) {
                const unsigned long long w0 = PH_NOW();
                // the state vector row moves into this wave's (now idle) LDS region, where the batch reads it
                WG_RELEASE();
                {
                    const int S = ev.dims[0], S16 = (S + 15) & ~15;
                    const float *src = state_vecs + (size_t)t * S;
                    float *dst = row_lds((uint32_t)wave, dyn_stride);
                    if (ev.bf16) {
                        uint16_t *dst16 = reinterpret_cast<uint16_t *>(dst);
                        for (int i = LANE; i < S16; i += 64) dst16[i] = i < S ? (uint16_t)bf16_bits(src[i]) : (uint16_t)0;
                    } else
                        for (int i = LANE; i < S16; i += 64) dst[i] = i < S ? src[i] : 0.f;
                }
                WG_RELEASE(); // the row is in place before the request is visible
                if (LANE == 0) LDS_STORE(&ctl.req[wave], 1u);
                serve_evaluator(ev, ctl, gp, t0, s, n_live, dyn_stride, [&]() { return uni(LDS_LOAD(&ctl.req[wave])) == 3u; });
                WG_ACQUIRE();
                if (LANE == 0) LDS_STORE(&ctl.req[wave], 0u);
                CTR_ADD(24, PH_NOW() - w0);
            } else if (ev.kind == 2 || ev.kind == 4) {
                float *h = a.h_theta + (size_t)t * a.A;
                const uint64_t agent = ev.first_agent + (uint64_t)t, cidx = ev.call_base + (uint64_t)call;
                for (int i = LANE; i < a.A; i += 64) {
                    uint64_t r = splitmix(splitmix(splitmix(splitmix(ev.seed ^ 0x70726564ull) ^ agent) ^ cidx) ^ (uint64_t)i);
                    h[i] = (float)(r >> 40) * (1.0f / 16777216.0f);
                }
                WAVE_SYNC();
            }
            add_actions_agent<SP>(a, s, t, 0, &ro);
        };
        // Taking over from an aborted pool launch (StepLaunch::resume): the agent has completed `call` calls of this launch; if the
        // last of them ended on a new node, its prediction row and add_actions are still due (PoolArgs::pend was not served):
        // the loop is entered at its second half.  (One loop, so that the evaluator's code is in the kernel once.)
        int call = 0;
        bool due = false;
        RolloutOut ro;
        if (resume) {
            const uint32_t rs = resume[t];
            call = (int)(rs & 0x7FFFFFFFu);
            if (rs >> 31) {
                due = true;
                call -= 1;
                ro.flags = 0;
                ro.cand_c = 0.f;
                ro.cand_node = NONE;
                ro.pos = a.state_pos[t];
                ro.c = a.nodes[(size_t)t * a.node_cap + ro.pos].c;
                ro.n_preds = a.n_preds[t];
            }
        }
        for (; call < n_calls; ++call) {
            if (LANE == 0) LDS_STORE(&ctl.prog[wave], (uint32_t)call);
            if (!due) {
                {   // the agents furthest behind win issue arbitration against their neighbours
                    uint32_t mn = 0xFFFFFFFFu;
                    for (int w = 0; w < n_live; ++w) {
                        const uint32_t pr = LDS_LOAD(&ctl.prog[w]);
                        mn = pr < mn ? pr : mn;
                    }
                    if ((uint32_t)call <= mn + (uint32_t)AZD_ASYNC_LAG_PRIO) __builtin_amdgcn_s_setprio(3);
                    else __builtin_amdgcn_s_setprio(AZD_ASYNC_BASE_PRIO);
                }
                // the agent stays on this wave: its counters accumulate in LDS until the launch ends, and what the
                // call leaves in registers (candidate, node, cost) is not read back from HBM
                const bool expanded = rollout_agent<SP, true>(a, tol, s, dyn, t, &ro);
                __builtin_amdgcn_s_setprio(0);
                // candidate of this call for the argmin replay (first-min over this tree's new nodes)
                if (LANE == 0 && ro.flags == 0) {
                    const uint32_t node = ro.cand_node;
                    if (node != NONE) {
                        const unsigned long long key = ((unsigned long long)ordf(ro.cand_c) << 32) |
                                                       ((unsigned long long)((uint32_t)t & 0xFFFFu) << 16) | (unsigned long long)(node & 0xFFFFu);
                        if (key < __hip_atomic_load(&log_key[call], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&log_key[call], key);
                        a.cand_node[t] = NONE;
                    }
                }
                if (!expanded) continue; // root exhausted (or stopped): no prediction, no add_actions
            }
            due = false;
            predict_and_add(ro, call);
        }
        WAVE_SYNC();
        flush_counters(a, s, t);
        if (LANE == 0) {
            LDS_STORE(&ctl.prog[wave], 0xFFFFFFFFu); // through: no longer the slowest
            atomicAdd(&ctl.finished, 1u);
        }
    }
    // keep serving until every agent of the workgroup is through (nobody is left to wait alone)
    if (ev.kind == 3 && active) {
        serve_evaluator(ev, ctl, gp, t0, s, n_live, dyn_stride, [&]() { return uni(LDS_LOAD(&ctl.finished)) >= (uint32_t)n_live; });
        // the evaluator-service counters of the whole launch (slots 24..), like the others, go out once
        if (LANE == 0) {
            unsigned long long *ctr = a.counters + (size_t)t * NUM_COUNTERS;
            for (int k = 24; k < NUM_COUNTERS; ++k) ctr[k] += s.ctr[k];
        }
    }
}

// ---------------------------------------------------------------- host: LDS plan shared by the spaces
// No evaluator buffers in LDS: a wave's region (wave_dyn_bytes: SP::dyn_bytes) holds its search scratch during a call and its
// row's activations [x][h0][h1] while the agent waits.  wave_lds_bytes: a wave's static block (SP::Lds).
static bool async_plan_common(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why,
                              const size_t wave_dyn_bytes, const size_t wave_lds_bytes) {
    if (a.B > 65536 || a.node_cap > 65536) { // (agent, node) are packed 16 + 16 bits in the argmin log
        *why = "asynchronous step: more than 65536 agents or nodes per tree";
        return false;
    }
    size_t stride = (wave_dyn_bytes + 15) & ~(size_t)15;
    if (ev.kind == 3) {
        for (int l = 0; l < ev.n_layers; ++l)
            if (ev.dims[l] % (l == 0 ? 4 : 16) != 0) { // tile tasks walk K in steps of 16; x is zero-padded
                *why = "asynchronous step: hidden widths must be multiples of 16 and the input width a multiple of 4";
                return false;
            }
        // + the 16-B-per-wave skew
        size_t rows = ((size_t)((ev.dims[0] + 15) & ~15) + (size_t)ev.hid[0] + (size_t)ev.hid[1]) * sizeof(float) + 16 * PERSIST_WAVES;
        if (rows > stride) stride = (rows + 15) & ~(size_t)15;
    }
    const size_t total = stride * PERSIST_WAVES;
    const size_t static_lds = PERSIST_WAVES * (wave_lds_bytes + 16) + sizeof(AsyncCtl) + 256;
    if (total + static_lds > 160 * 1024) {
        *why = "asynchronous step: 16 rows of activations do not fit the CU's 160 KB of LDS";
        return false;
    }
    *dyn_stride = (uint32_t)stride;
    *dyn_bytes = total;
    return true;
}
