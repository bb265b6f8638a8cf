// pool_step.inc -- included after async_step.inc (inside namespace azd) by pool_kernels.hip / ramsey_pool_kernels.hip.
//
// Third CU-resident form of NablaOptimizer::par_roll_out_episodes (optimizer/mod.rs:121-191), with the same results as
// k_persist / k_async: agents are NOT bound to wavefronts, and the evaluator has workgroups (CUs) of its own.
//
//   searcher workgroups   16 wavefronts, each an independent worker: take a ready agent, finish its previous call
//                         (add_actions with the prediction row that has arrived), run its next call
//                         (roll_out_episodes), post the new state vector to the evaluator, take the next ready agent.
//                         A wave never waits for a prediction row; what waits is the agent.
//   evaluator workgroups  blocks [0, n_eval): pull up to 16 posted rows -- 32 where they fit the LDS and that many wait --, run
//                         the MLP on them (one or two v_mfma_f32_16x16x4_f32 / 16x16x16_bf16 row tiles per weight fragment; all
//                         16 waves share the column tiles of a layer; weights stream from L2 in fragment order with nothing
//                         else on the CU's memory path), store the prediction rows, put the agents back on their ready queue.
//   early post            the request for a row may leave the moment the row is stored, before the wave computes the new node's
//                         cost and writes the tree back (rollout_agent, RolloutOut::post_*): the evaluator then works while the
//                         wave still does, and the agent is queued again by whoever is later (PoolArgs::join).  Always for
//                         populations that fit the searching waves; otherwise for agents behind the mean progress of their XCD
//                         and for waves that stood idle (PoolArgs::early_post).
//
// Why (profiles/r01_*): in k_async a launch lasts as long as the slowest agent's chain of calls, 92 us of search + 52 us
// waiting for a row whose batch carried 7 rows on average and streamed the whole weight set past the searchers' dependent
// loads; and a population larger than the resident waves ran as serial rounds of workgroups.  Here a batch costs the MFMA
// time of one full tile, a searching wave's loads queue behind other searchers only, and 8192 agents share 3000 waves.
//
// Memory model (MI355X_MICROARCH.md, "inter-workgroup visibility"): per-XCD L2s are not coherent with each other and a
// CU's L1 is never refreshed by another CU's stores.
//   * A TREE never leaves its XCD: an agent is taken ("claimed") on first touch by a searcher of some XCD and from then on
//     lives on that XCD's ready queue.  Its arenas and per-agent state are plain loads / stores; a wave that takes an agent
//     invalidates its CU's L1 first (agent-scope acquire), and a wave that lets an agent go has drained its stores into
//     the XCD's L2 (s_waitcnt vmcnt(0)) before the agent becomes visible on any queue.
//   * What crosses XCDs -- state-vector rows to the evaluator, prediction rows back, queue words -- is stored and loaded
//     with the sc1 bit only (write-through stores, L1-bypassing loads), the producer drains (vmcnt(0)) before it
//     signals, the consumer loads after its poll has matched: the guide's validated hand-off.
// Every wait has an exit every wave reaches: a wait that runs into its bound raises PoolCtl::abort, which every loop tests (the
// host then reports AZD_ERR_UNREACHABLE) -- a searcher waiting for its ticket only if the population has made no call since
// its last look --, and searchers / evaluators leave when PoolCtl::done_agents reaches the population.  Nothing depends on dispatch order or placement: any searcher can
// take any unclaimed agent, any evaluator can serve any XCD's queue.

// A wait gives up (raises PoolCtl::abort) after this long without success: wall-clock ticks of the constant 100 MHz
// counter, looked at every 256 polls.  Far beyond any wait of a healthy launch (an epoch lasts ~0.1 s).
constexpr unsigned long long POOL_WAIT_TICKS = 400000000ull; // 4 s
struct PoolWait {
    unsigned long long t0;
    uint32_t polls;
    __device__ __forceinline__ PoolWait() : t0(0), polls(0) {}
    __device__ __forceinline__ bool expired() { // call once per unsuccessful poll
        if ((++polls & 255u) != 0u) return false;
        const unsigned long long now = (unsigned long long)wall_clock64();
        if (t0 == 0) t0 = now;
        return now - t0 > POOL_WAIT_TICKS;
    }
};

__device__ __forceinline__ uint32_t pool_xcc_id() {
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 7u;
}

// An evaluator that finds fewer than 16 rows posted looks again after ~1 us, at most this many times, before it takes
// what is there: a batch costs the same with 1 row or 16 (0: 28.2 M expansions/s at 4096 agents, 1: 28.9, 3: 28.6;
// 8192 agents: 33.4 / 33.8 / 34.5; gpurun sweep r2c/fw_*)
#ifndef AZD_POOL_FILL_WAIT
#define AZD_POOL_FILL_WAIT 2
#endif
#ifndef AZD_POOL_FILL_SLEEP
#define AZD_POOL_FILL_SLEEP 32
#endif
#ifndef AZD_POOL_POLL_SLEEP
// x 64 clocks between two looks of a waiting searcher wave at its ticket's slot: 127 = 3.4 us.  Shorter naps find the agent
// sooner but cost the running waves more than that gains: 16 / 32 / 64 / 96 / 127 / 190 / 254 -> 31.9 / 32.2 / 32.6 / 33.0 / 33.0 /
// 33.3 / 33.2 M expansions/s at 4096 agents, 19.7 / 19.9 / 20.4 / 20.6 / 20.8 / 21.0 / 20.8 at 2048 (gpurun r2n)
#define AZD_POOL_POLL_SLEEP 127
#endif
#ifndef AZD_POOL_EVAL_IDLE_SLEEP
#define AZD_POOL_EVAL_IDLE_SLEEP 32 // x 64 clocks between two scans of the evaluator queues by an evaluator that found them all empty
#endif
#ifndef AZD_POOL_BEHIND_SLACK
#define AZD_POOL_BEHIND_SLACK 2 // an agent posts early when its call count + SLACK + mean >> SHIFT is below the mean of its XCD
#endif
#ifndef AZD_POOL_BEHIND_SHIFT
#define AZD_POOL_BEHIND_SHIFT 5
#endif
#ifndef AZD_POOL_TWO_TILES
#define AZD_POOL_TWO_TILES 1
#endif
#include "tile_task_asm.inc"
#include "pool_diag.inc"
#ifndef AZD_POOL_EXPRESS_SLACK
#define AZD_POOL_EXPRESS_SLACK 2 // an agent lags when its calls + SLACK + (ref >> express_shift) < ref (1 / 0 measured: no better, also in 20-call launches)
#endif
#ifndef AZD_POOL_STANDBY
#define AZD_POOL_STANDBY 4
#endif
constexpr int POOL_BATCH_MAX = 32; // two 16-row MFMA tiles
struct PoolBatch { // LDS block of an evaluator workgroup
    uint32_t agent[POOL_BATCH_MAX];
    uint32_t home[POOL_BATCH_MAX];
    uint32_t n, first[2], cnt[2], q, leave;
};

struct PoolRows { // an evaluator batch: row r at byte r * stride * 4 of the dynamic LDS, [x][h0][h1] as in row_lds, then the head's output
    uint32_t stride, out_off; // floats
    const uint32_t *agents;
    int n;
    __device__ __forceinline__ int count() const { return n; }
    // through lds_base, so that the compiler knows the address space (a generic pointer makes every row access a flat
    // load that counts on vmcnt AND lgkmcnt, which serialises the weight stream behind the LDS reads)
    __device__ __forceinline__ float *row(const int r) const { return reinterpret_cast<float *>(lds_base((uint32_t)r * stride * 4u)); }
    __device__ __forceinline__ int agent(const int r) const { return (int)agents[r]; }
    __device__ __forceinline__ float *out(const int r) const { return reinterpret_cast<float *>(lds_base(((uint32_t)r * stride + out_off) * 4u)); }
};

// ---------------------------------------------------------------- a tile task over TWO row tiles (batches of 17..32 rows)
// The same arithmetic per output element as mlp_tile_task (same MFMA sequence over k), for rows 0..15 and 16..31 at once:
// every weight fragment is requested once and feeds both row tiles.  A 16-row batch costs an evaluator 25 us of which 14
// are MFMAs; a 32-row batch costs the MFMAs twice and the rest once.
template <bool BF16>
__device__ void pool_tile2(const FusedEval &ev, const PoolRows &rows, const EvalPtrs &gp, const int l, const int tile) {
    const int lane = LANE;
    const int L = ev.n_layers;
    const int K = ev.dims[l], N = ev.dims[l + 1];
    const int S4 = (ev.dims[0] + 15) & ~15, H = ev.hid[0];
    const int nrows = rows.count();
    const int n0 = tile * 16;
    const int r = lane & 15;
    float *const base0 = rows.row(r < nrows ? r : 0);
    float *const base1 = rows.row(16 + r < nrows ? 16 + r : 0);
    const int in_off = (l == 0 ? 0 : S4 + ((l - 1) & 1) * H) + 4 * (lane >> 4);
    const int steps = (K + 15) >> 4;
    const size_t frag = (size_t)ev.p_off[l] + ((size_t)tile * steps * 64 + lane) * 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (BF16) {
        const uint16_t *wq = reinterpret_cast<const uint16_t *>(gp.wpk) + frag;
        const uint16_t *p0 = reinterpret_cast<const uint16_t *>(base0) + in_off, *p1 = reinterpret_cast<const uint16_t *>(base1) + in_off;
        for (int s0 = 0; s0 < steps; s0 += MLP_PF) {
            uint2 bq[MLP_PF];
            const bool full = s0 + MLP_PF <= steps;
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (full || s0 + j < steps) bq[j] = *reinterpret_cast<const uint2 *>(wq + 256 * (s0 + j));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (full || s0 + j < steps) {
                    const uint2 a0 = *reinterpret_cast<const uint2 *>(p0 + 16 * (s0 + j)), a1 = *reinterpret_cast<const uint2 *>(p1 + 16 * (s0 + j));
                    bf16x4 x0, x1, b4;
                    __builtin_memcpy(&x0, &a0, 8);
                    __builtin_memcpy(&x1, &a1, 8);
                    __builtin_memcpy(&b4, &bq[j], 8);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(x0, b4, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(x1, b4, acc1, 0, 0, 0);
                }
        }
    } else {
        const float *wp = reinterpret_cast<const float *>(gp.wpk) + frag;
        const float *p0 = base0 + in_off, *p1 = base1 + in_off;
        for (int s0 = 0; s0 < steps; s0 += MLP_PF) {
            float4 bq[MLP_PF];
            const bool full = s0 + MLP_PF <= steps;
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (full || s0 + j < steps) bq[j] = *reinterpret_cast<const float4 *>(wp + 256 * (s0 + j));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < MLP_PF; ++j)
                if (full || s0 + j < steps) {
                    const float4 a0 = *reinterpret_cast<const float4 *>(p0 + 16 * (s0 + j)), a1 = *reinterpret_cast<const float4 *>(p1 + 16 * (s0 + j));
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, bq[j].x, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, bq[j].x, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, bq[j].y, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, bq[j].y, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, bq[j].z, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, bq[j].z, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, bq[j].w, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, bq[j].w, acc1, 0, 0, 0);
                }
        }
    }
    const int col = n0 + (lane & 15);
    if (col < N) {
        const float bj = gp.params[ev.b_off[l] + col];
        const int act = (l == L - 1) ? ev.final_act : 1;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 16 * h + 4 * (lane >> 4) + i;
                if (row < nrows) {
                    const float v = act_apply((h ? acc1[i] : acc0[i]) + bj, act);
                    if (l == L - 1) rows.out(row)[col] = v;
                    else if (BF16) reinterpret_cast<uint16_t *>(rows.row(row))[S4 + (l & 1) * H + col] = (uint16_t)bf16_bits(v);
                    else rows.row(row)[S4 + (l & 1) * H + col] = v;
                }
            }
    }
}

// FusedEval kind 4 (test harness): h(agent, call, a) of the call each agent posted (PoolArgs::post_call, stored sc1 ahead of the
// request) instead of the MLP.  Only in the harness' instantiation of the kernel (k_pool<SP, true>): the product kernel is
// compiled without a trace of it.
__device__ __forceinline__ void pool_hash_rows(const FusedEval &ev, const PoolArgs &pl, const PoolBatch &bt, const PoolRows &rows, const int n,
                                            const int A) {
    for (int idx = threadIdx.x; idx < n * A; idx += PERSIST_WAVES * 64) {
        const int r = idx / A, i = idx - r * A;
        const uint64_t agent = ev.first_agent + (uint64_t)bt.agent[r], cidx = ev.call_base + (uint64_t)ld_sc1(pl.post_call + bt.agent[r]);
        const uint64_t h = splitmix(splitmix(splitmix(splitmix(ev.seed ^ 0x70726564ull) ^ agent) ^ cidx) ^ (uint64_t)i);
        rows.out(r)[i] = (float)(h >> 40) * (1.0f / 16777216.0f);
    }
}

// ---------------------------------------------------------------- evaluator workgroup
template <bool HASHED>
__device__ __forceinline__ void pool_eval(const PersistArgs *pa, const EvalPtrs &gp, PoolBatch &bt, const uint32_t xcc) {
    const Arenas &a = pa->a;
    const FusedEval &ev = pa->ev;
    const PoolArgs &pl = pa->pool;
    PoolCtl *ctl = pl.ctl;
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint32_t B = (uint32_t)a.B, qmask = pl.qcap - 1u;
    constexpr bool hashed = HASHED; // the fixed prediction stream, served here (FusedEval kind 4: test harness of the queues / early post / join)
    const int S = ev.dims[0], S16 = (S + 15) & ~15, L = hashed ? 0 : ev.n_layers, A = hashed ? a.A : ev.dims[L];
    PoolRows rows;
    rows.stride = pl.eval_stride;
    rows.out_off = pl.eval_out_off;
    rows.agents = bt.agent;
    unsigned long long n_batches = 0, n_rows = 0, n_tiles = 0, busy = 0, t_stage = 0, t_layers = 0, c_layers = 0;
    for (;;) {
        if (tid == 0) { // form a batch: the own XCD's queue first, then the others (any evaluator may serve any queue)
            uint32_t n = 0, first0 = 0, first1 = 0, cnt0 = 0, cnt1 = 0, q = 0, leave = 0;
            PoolWait wt;
            int fill_waits = AZD_POOL_FILL_WAIT;
            for (;;) {
                for (uint32_t k = 0; k < (uint32_t)POOL_XCDS && n == 0u; ++k) {
                    const uint32_t x = (xcc + k) & (uint32_t)(POOL_XCDS - 1);
                    const uint32_t h0 = 0u, t0 = 0u; // (lane 0, once the lagging agents' queue: nothing posts to it, so it is not looked at)
                    const uint32_t h1 = ld_sc1(&ctl->evalq[1][x].head), t1 = ld_sc1(&ctl->evalq[1][x].tail);
                    const int a0 = (int)(t0 - h0) > 0 ? (int)(t0 - h0) : 0, a1 = (int)(t1 - h1) > 0 ? (int)(t1 - h1) : 0;
                    if (a0 + a1 == 0) continue;
                    // a batch costs the same with 1 row or 16: give it a moment to fill -- unless a lagging agent waits
                    // 16 rows, or 32 (two row tiles per weight fragment) where they fit the LDS AND that many are waiting: a
                    // 32-row batch takes 39 us against 25, which only pays when the evaluators are the bottleneck (config C
                    // with 40 evaluator workgroups: 29.0 -> 40.4 M; at 4096 agents taking 17..31 rows cost 29.3 -> 26.4 M)
                    const int cap = ((int)pl.eval_rows > PERSIST_WAVES && a0 + a1 >= (int)pl.eval_rows) ? (int)pl.eval_rows : PERSIST_WAVES;
                    if (a0 == 0 && a1 < PERSIST_WAVES && fill_waits > 0) {
                        --fill_waits;
                        __builtin_amdgcn_s_sleep(AZD_POOL_FILL_SLEEP);
                        k = (uint32_t)POOL_XCDS; // look again from the own queue
                        continue;
                    }
                    uint32_t c0 = 0, c1 = 0;
                    if (a0 > 0) {
                        const uint32_t take = a0 < cap ? (uint32_t)a0 : (uint32_t)cap;
                        if (atomicCAS(&ctl->evalq[0][x].head, h0, h0 + take) == h0) c0 = take;
                    }
                    if (a1 > 0 && c0 < (uint32_t)cap) {
                        const uint32_t room = (uint32_t)cap - c0;
                        const uint32_t take = (uint32_t)a1 < room ? (uint32_t)a1 : room;
                        if (atomicCAS(&ctl->evalq[1][x].head, h1, h1 + take) == h1) c1 = take;
                    }
                    if (c0 + c1) {
                        n = c0 + c1;
                        first0 = h0;
                        first1 = h1;
                        cnt0 = c0;
                        cnt1 = c1;
                        q = x;
                    } else k = (uint32_t)POOL_XCDS; // lost both races: look again
                }
                if (n) break;
                if (ld_sc1(&ctl->done_agents) >= B || ld_sc1(&ctl->abort) != 0u) {
                    leave = 1;
                    break;
                }
                __builtin_amdgcn_s_sleep(AZD_POOL_EVAL_IDLE_SLEEP);
                if (wt.expired()) {
                    atomicExch(&ctl->abort, 1u);
                    leave = 1;
                    break;
                }
            }
            bt.n = n;
            bt.first[0] = first0;
            bt.first[1] = first1;
            bt.cnt[0] = cnt0;
            bt.cnt[1] = cnt1;
            bt.q = q;
            bt.leave = leave;
        }
        __syncthreads();
        if (bt.leave) break;
        const int n = (int)bt.n;
        const unsigned long long tb0 = (unsigned long long)wall_clock64();
        if (tid < n) { // the slot of ticket first + tid: its producer's store may still be on its way
            const uint32_t lane_q = (uint32_t)tid < bt.cnt[0] ? 0u : 1u; // the lagging agents' lane first
            const uint32_t ticket = lane_q == 0u ? bt.first[0] + (uint32_t)tid : bt.first[1] + (uint32_t)tid - bt.cnt[0];
            uint32_t *slot = pl.eval_slots + ((size_t)lane_q * POOL_XCDS + bt.q) * pl.qcap + (ticket & qmask);
            uint32_t v = 0;
            PoolWait wt;
            while ((v = ld_sc1(slot)) == 0u) {
                __builtin_amdgcn_s_sleep(1);
                if (wt.expired() || ld_sc1(&ctl->abort) != 0u) {
                    atomicExch(&ctl->abort, 1u);
                    bt.leave = 1u; // through LDS and the barrier below: the whole workgroup leaves together
                    break;
                }
            }
            st_sc1(slot, 0u);
            bt.agent[tid] = v ? (v & 0xFFFFFFu) - 1u : 0u;
            bt.home[tid] = v >> 24; // bits 0-2: home XCD, bit 6: posted early (join), bit 7: the agent is behind the mean progress
            if (v) diag_row_waited_for_evaluator(a, pl, bt.agent[tid]);
        }
        __syncthreads();
        if (bt.leave) break;
        rows.n = n;
        // ---- the rows' state vectors: sc1 loads (their agents' waves stored them sc1 and drained before posting)
        if (hashed) pool_hash_rows(ev, pl, bt, rows, n, A);
        else {
            const int q4 = S16 >> 2;
            for (int idx = tid; idx < n * q4; idx += PERSIST_WAVES * 64) {
                const int r = idx / q4, c4 = idx - r * q4;
                azd_f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (4 * c4 < S) v = ld_sc1_x4(gp.state_vecs + (size_t)bt.agent[r] * S + 4 * c4);
                if (ev.bf16) {
                    uint16_t *d = reinterpret_cast<uint16_t *>(rows.row(r)) + 4 * c4;
                    d[0] = (uint16_t)bf16_bits(v[0]);
                    d[1] = (uint16_t)bf16_bits(v[1]);
                    d[2] = (uint16_t)bf16_bits(v[2]);
                    d[3] = (uint16_t)bf16_bits(v[3]);
                } else *reinterpret_cast<azd_f32x4 *>(rows.row(r) + 4 * c4) = v;
            }
        }
        __syncthreads();
        const unsigned long long tb1 = (unsigned long long)wall_clock64();
        const unsigned long long cb1 = (unsigned long long)__builtin_amdgcn_s_memtime(); // shader clocks (the chip lowers its clock under load)
        // ---- dfdx.rs:69-84: layer by layer, the 16 waves share the column tiles (tile j -> wave j mod 16).
        // Measured and discarded (profiles/r02_pool_probe.txt): rotating-register prefetch of the next 8 k-steps of
        // weights, across tiles and across the layer barrier -- 25.6 us per batch of layers against 22.6 us for the
        // plain tile task, whose requests-then-MFMAs groups the four waves of a SIMD already overlap among themselves.
        for (int l = 0; l < L; ++l) {
            const int nt = (ev.dims[l + 1] + 15) >> 4;
            for (int tile = wave; tile < nt; tile += PERSIST_WAVES) {
                if (n > PERSIST_WAVES) { // 17..32 rows: both row tiles per weight fragment
                    if (ev.bf16) pool_tile2<true>(ev, rows, gp, l, tile);
                    else pool_tile2<false>(ev, rows, gp, l, tile);
                } else {
                    unsigned long long ph[3];
                    mlp_tile_task<PoolRows, true>(ev, rows, gp, l, tile, ph);
                }
            }
            __syncthreads();
        }
        for (int l = 0; l < L; ++l) n_tiles += (unsigned long long)((ev.dims[l + 1] + 15) >> 4);
        const unsigned long long tb2 = (unsigned long long)wall_clock64();
        t_stage += tb1 - tb0;
        t_layers += tb2 - tb1;
        c_layers += (unsigned long long)__builtin_amdgcn_s_memtime() - cb1;
        // ---- prediction rows out: whole 16-byte write-through stores (A is a multiple of 4: pool plan)
        {
            const int a4 = A >> 2;
            for (int idx = tid; idx < n * a4; idx += PERSIST_WAVES * 64) {
                const int r = idx / a4, c4 = idx - r * a4;
                st_sc1_x4(gp.h_theta + (size_t)bt.agent[r] * A + 4 * c4, *reinterpret_cast<const azd_f32x4 *>(rows.out(r) + 4 * c4));
            }
        }
        VM_DRAIN(); // every storing wave drains before the barrier behind which the agents are released
        __syncthreads();
        // the agent goes back to its XCD's ready queue once the wave that posted it is through with it too (it posts before it
        // computes the new node's cost): whoever comes second queues it
        // (bit 6 of the request: posted early.  A request posted after the call needs no join: its wave was through first.)
        if (tid < n && ((bt.home[tid] & 0x40u) == 0u || (atomicAdd(&pl.join[bt.agent[tid]], 1u) & 1u))) {
            diag_stamp_handed_over(pl.stamp + bt.agent[tid]);
            const uint32_t x = bt.home[tid] & (uint32_t)(POOL_XCDS - 1);
            const uint32_t rl = (pl.ready_lanes && (bt.home[tid] & 0x80u)) ? 0u : 1u;
            const uint32_t i = atomicAdd(&ctl->ready[rl][x].tail, 1u);
            st_sc1(pl.ready_slots + ((size_t)rl * POOL_XCDS + x) * pl.qcap + (i & qmask), bt.agent[tid] + 1u);
        }
        n_batches += 1;
        n_rows += (unsigned long long)n;
        // test hook (AZD_POOL_DEBUG_ABORT_CALL = k): evaluator workgroup 0 raises the abort flag after its k-th batch
        if (tid == 0 && blockIdx.x == 0 && pl.debug_abort_call != 0u && n_batches == (unsigned long long)pl.debug_abort_call) atomicExch(&ctl->abort, 1u);
        busy += (unsigned long long)wall_clock64() - tb0;
        // bt.agent / bt.home are rewritten only behind the next batch's first barrier
    }
    if (tid == 0) { // evaluator service counters (AZD_CTR_EVAL_*): summed over agents by the host, any agent's block will do
        atomicAdd(&ctl->eval_busy, busy);
        atomicMax(&ctl->t_last, (unsigned long long)wall_clock64());
        unsigned long long *ctr = a.counters + (size_t)(blockIdx.x % (uint32_t)a.B) * NUM_COUNTERS;
        atomicAdd(&ctr[25], n_batches);
        atomicAdd(&ctr[26], n_rows);
        atomicAdd(&ctr[27], n_tiles);
        atomicAdd(&ctr[29], busy); // 100 MHz ticks from batch taken to batch released (AZD_CTR_TICKS_BATCH)
        pool_eval_stage_ticks(ctr, t_stage, t_layers); // ... of which: slots + state-vector rows in, the layers
        atomicAdd(&ctr[13], c_layers);     // the layers in SHADER clocks (AZD_CTR_EVAL_LAYER_CLOCKS): / ticks of 10 ns = the clock the evaluator CUs held
    }
}

// ---------------------------------------------------------------- evaluator GROUP (round 5)
// dfdx.rs:69-84 for a batch of <= 16 rows by g workgroups together: member j keeps the weight fragments of ITS column tiles of every
// layer in LDS for the whole launch (weights change only between launches), so a batch streams no weights at all; what travels
// between the layers is the batch's activations -- 16 rows x the layer's width, fragment-major, through device memory: sc1
// write-through stores, the storing wave's vmcnt(0), one agent-scope add on the layer's arrival counter; consumers poll the counter
// with sc1 loads and read their A operands with sc1 buffer loads straight into the MFMA registers (the hand-off the guide validates;
// placement-independent: a group may span XCDs).  A workgroup's 16 waves are 16 / W batch SLOTS of W waves (W = the most column tiles
// a member holds of one layer): a slot of a group = W waves on each member, walking one batch through the layers; the slots run
// batches independently and share the LDS weights.  Per output element the MFMA sequence is mlp_tile_task's (k ascending, per
// k-step the quads' x, y, z, w): rows are bit-identical to the classic form's.
// For what: a model too large for one CU's stream -- config A, the reference's own 304-512-1024-512-152 (5.1 MB of fp32 weights
// per batch through ONE CU: 86 us per batch of 2.7 rows, the evaluator round trip two thirds of an agent's cycle).  Measured first
// (tools/probes/group_exchange.hip, profiles/r05_group_exchange.txt): a layer edge costs ~3 us, so config B's model (1 MB, 23 us
// classic) gains nothing at the concurrency its row rate needs -- the engine forms groups only where the classic batch is long.
struct GroupTile { // one (layer, column tile) task of a slot's batch
    int tile;      // -1: this wave has none in this layer
    uint32_t lds;  // byte offset of the tile's weight fragments in this workgroup's LDS
};
__device__ __forceinline__ azd_f32x4 grp_buf_ld(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 16); // aux 16 = sc1: L1 bypassed
    azd_f32x4 f;
    __builtin_memcpy(&f, &v, 16);
    return f;
}
__device__ __forceinline__ void pool_eval_group(const PersistArgs *pa, const EvalPtrs &gp, const uint32_t xcc) {
    const Arenas &a = pa->a;
    const FusedEval &ev = pa->ev;
    const PoolArgs &pl = pa->pool;
    PoolCtl *ctl = pl.ctl;
    const int lane = LANE, wave = threadIdx.x >> 6;
    const int g = pl.grp_g, W = pl.grp_w, NS = PERSIST_WAVES / W;
    const int group = (int)blockIdx.x / g, member = (int)blockIdx.x % g;
    const int L = ev.n_layers, S = ev.dims[0], A = ev.dims[L];
    const uint32_t B = (uint32_t)a.B, qmask = pl.qcap - 1u;
    // ---- this member's weight fragments into LDS, once per launch
    for (int l = 0; l < L; ++l) {
        const int steps = (ev.dims[l] + 15) >> 4;
        for (int w = 0; w < W; ++w) {
            const int tile = (int)pl.grp_tile[((size_t)l * g + member) * W + w];
            if (tile < 0) continue;
            const uint32_t off = pl.grp_lds[((size_t)l * g + member) * W + w];
            const float *src = reinterpret_cast<const float *>(gp.wpk) + (size_t)ev.p_off[l] + (size_t)tile * steps * 256;
            for (int i = threadIdx.x; i < steps * 64; i += PERSIST_WAVES * 64)
                *reinterpret_cast<azd_f32x4 *>(lds_base(off + (uint32_t)i * 16u)) = *reinterpret_cast<const azd_f32x4 *>(src + (size_t)i * 4);
        }
    }
    __syncthreads();
    const int slot = wave / W, tw = wave % W;
    if (slot >= NS) return;
    const size_t si = (size_t)group * NS + slot;
    uint32_t *const desc = pl.grp_desc + si * 64;
    uint32_t *const cnt = pl.grp_cnt + si * 8 * 32;
    float *const xb = pl.grp_x + si * 2 * pl.grp_xstride;
    uint32_t *const flags = pl.grp_flag + si * (size_t)g * 16;       // this slot's flag lines, one per member
    uint32_t *const my_flag = flags + (size_t)member * 16;
    // one wave tells every member (a line each: a counter polled by all 80 waves of a slot saturated its line -- 62 us per config A batch)
    auto tell_all = [&](const int word, const uint32_t value) __attribute__((always_inline)) {
        for (int m = lane; m < g; m += 64) st_sc1(flags + (size_t)m * 16 + word, value);
    };
    const bool leader = member == 0 && tw == 0;
    // buffer resources (base, no stride, bytes, raw 32-bit data): reads past the end return zero
    azd_tile_u4 rs_states, rs_x;
    rs_states[0] = (uint32_t)(uintptr_t)gp.state_vecs;
    rs_states[1] = (uint32_t)((uintptr_t)gp.state_vecs >> 32) & 0xFFFFu;
    rs_states[2] = (uint32_t)((size_t)a.B * S * 4);
    rs_states[3] = 0x00020000u;
    rs_x[0] = (uint32_t)(uintptr_t)xb;
    rs_x[1] = (uint32_t)((uintptr_t)xb >> 32) & 0xFFFFu;
    rs_x[2] = 2u * pl.grp_xstride * 4u;
    rs_x[3] = 0x00020000u;
    const int r = lane & 15, q = lane >> 4;
    unsigned long long n_batches = 0, n_rows = 0, n_tiles = 0, busy = 0;
    bool leave = false;
    for (uint32_t gen = 1; !leave; ++gen) {
        unsigned long long tb0 = 0;
        uint32_t n = 0;
        if (leader) { // form a batch: the own XCD's queue first, then the others (pool_eval's rule, one row tile)
            uint32_t first1 = 0, cnt1 = 0, qx = 0, go = 0;
            {   // all eight queues in ONE look (a lane each), starting from a queue of this slot's own: the leaders of a launch sit on a
                // handful of CUs (member 0 of every group), and looking queue by queue from the CU's XCD made them all start on the
                // same queue, sixteen dependent round trips to reach the last (config A: 110 us of an agent's 190-us cycle)
                const uint32_t x0 = (uint32_t)si & (uint32_t)(POOL_XCDS - 1);
                PoolWait wt;
                int fill_waits = AZD_POOL_FILL_WAIT;
                for (;;) {
                    uint32_t h1 = 0, t1 = 0;
                    const uint32_t xq = (x0 + (uint32_t)lane) & (uint32_t)(POOL_XCDS - 1);
                    if (lane < POOL_XCDS) {
                        h1 = ld_sc1(&ctl->evalq[1][xq].head);
                        t1 = ld_sc1(&ctl->evalq[1][xq].tail);
                    }
                    const int a1 = (lane < POOL_XCDS && (int)(t1 - h1) > 0) ? (int)(t1 - h1) : 0;
                    const uint64_t nonempty = __ballot(a1 > 0);
                    if (nonempty) {
                        const int pick = first_lane(nonempty); // the first non-empty queue from x0 on
                        const int ap = (int)rdlane((uint32_t)a1, pick);
                        if (ap < PERSIST_WAVES && fill_waits > 0) { // a batch costs the same with 1 row or 16: give it a moment to fill
                            --fill_waits;
                            __builtin_amdgcn_s_sleep(AZD_POOL_FILL_SLEEP);
                            continue;
                        }
                        const uint32_t hp = rdlane(h1, pick), take = ap < PERSIST_WAVES ? (uint32_t)ap : (uint32_t)PERSIST_WAVES;
                        const uint32_t xp = (x0 + (uint32_t)pick) & (uint32_t)(POOL_XCDS - 1);
                        uint32_t won = 0;
                        if (lane == 0) won = atomicCAS(&ctl->evalq[1][xp].head, hp, hp + take) == hp ? 1u : 0u;
                        if (uni(won)) {
                            cnt1 = take;
                            first1 = hp;
                            qx = xp;
                            go = 1;
                            break;
                        }
                        continue; // lost the race: look again
                    }
                    uint32_t over = 0;
                    if (lane == 0) over = (ld_sc1(&ctl->done_agents) >= B || ld_sc1(&ctl->abort) != 0u) ? 1u : 0u;
                    if (uni(over)) break;
                    __builtin_amdgcn_s_sleep(AZD_POOL_EVAL_IDLE_SLEEP);
                    if (wt.expired()) {
                        if (lane == 0) atomicExch(&ctl->abort, 1u);
                        break;
                    }
                }
            }
            go = uni(go);
            n = uni(cnt1);
            first1 = uni(first1);
            qx = uni(qx);
            if (go) {
                tb0 = (unsigned long long)wall_clock64();
                uint32_t agent_r = 0, home_r = 0;
                if ((uint32_t)lane < n) { // the slot of ticket first + lane: its producer's store may still be on its way
                    uint32_t *tslot = pl.eval_slots + ((size_t)POOL_XCDS + qx) * pl.qcap + ((first1 + (uint32_t)lane) & qmask);
                    uint32_t v = 0;
                    PoolWait wt;
                    while ((v = ld_sc1(tslot)) == 0u) {
                        __builtin_amdgcn_s_sleep(1);
                        if (wt.expired() || ld_sc1(&ctl->abort) != 0u) {
                            atomicExch(&ctl->abort, 1u);
                            break;
                        }
                    }
                    st_sc1(tslot, 0u);
                    agent_r = v ? (v & 0xFFFFFFu) - 1u : 0u;
                    home_r = v >> 24;
                    if (v == 0u) go = 0; // (aborted: the batch is dropped, everybody leaves)
                }
                go = __ballot(go == 0) ? 0u : 1u;
                if (go) {
                    if (lane < 16) {
                        st_sc1(desc + 16 + lane, (uint32_t)lane < n ? agent_r : 0u);
                        st_sc1(desc + 32 + lane, (uint32_t)lane < n ? home_r : 0u);
                    }
                    if (lane == 0) st_sc1(desc + 1, n);
                    VM_DRAIN(); // the batch's description is in memory before its number is
                    tell_all(7, gen);
                }
            }
            if (!go) {
                tell_all(7, 0xFFFFFFFFu); // the slot's other waves leave with this one
                break;
            }
        } else { // the slot's batch number gen, or the word to leave
            PoolWait wt;
            uint32_t v = 0;
            for (;;) {
                v = ld_sc1(my_flag + 7);
                if (v == 0xFFFFFFFFu || v >= gen) break;
                __builtin_amdgcn_s_sleep(4);
                if (wt.expired() || ((wt.polls & 63u) == 0u && ld_sc1(&ctl->abort) != 0u)) {
                    v = 0xFFFFFFFFu;
                    break;
                }
            }
            if (v == 0xFFFFFFFFu) break;
            asm volatile("" ::: "memory");
            n = ld_sc1(desc + 1);
        }
        const uint32_t agent_r = ld_sc1(desc + 16 + r); // row r's agent (rows past the batch's: agent 0's, computed and dropped)
        const uint32_t home_r = ld_sc1(desc + 32 + r);
        for (int l = 0; l < L && !leave; ++l) {
            const int K = ev.dims[l], N = ev.dims[l + 1];
            const int steps = (K + 15) >> 4, nt = (N + 15) >> 4;
            const int tile = (int)pl.grp_tile[((size_t)l * g + member) * W + tw];
            if (tile < 0) continue; // (a wave without a tile in this layer does not wait for its input either)
            if (l > 0) { // every column tile of the layer before is in memory: its last arriver has told this member
                PoolWait wt;
                for (;;) {
                    const uint32_t v = ld_sc1(my_flag + (l - 1));
                    if (v >= gen && v != 0xFFFFFFFFu) break;
                    __builtin_amdgcn_s_sleep(2);
                    if (wt.expired() || ((wt.polls & 63u) == 0u && ld_sc1(&ctl->abort) != 0u)) {
                        atomicExch(&ctl->abort, 1u);
                        leave = true;
                        break;
                    }
                }
                if (leave) break;
                asm volatile("" ::: "memory"); // (the A operands below are loaded behind the poll, for the compiler too)
            }
            const uint32_t woff = pl.grp_lds[((size_t)l * g + member) * W + tw];
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            // A operand of k-step s: rows' quads.  Layer 0: from the agents' state vectors (their waves stored them sc1 and drained before
            // posting); else from the exchange buffer the layer before filled, fragment-major: one contiguous KB per k-step
            const uint32_t a_base = l == 0 ? (agent_r * (uint32_t)S + 4u * (uint32_t)q) * 4u : ((uint32_t)((l - 1) & 1) * pl.grp_xstride + (uint32_t)lane * 4u) * 4u;
            {   // the k loop (tile_task_asm.inc: the next group of 8 k-steps of rows' quads requested before the current group's MFMAs;
                // the compiler's own schedule of this loop -- requests, wait for all, MFMAs -- made a config A batch 78 us)
                azd_tile_acc ac = {0.f, 0.f, 0.f, 0.f};
                const uint32_t bp = (uint32_t)(uintptr_t)lds_base(woff) + (uint32_t)lane * 16u;
                if (l == 0) tile_k_loop_f32_ga64(ac, rs_states, a_base, bp, steps);
                else tile_k_loop_f32_ga1024(ac, rs_x, a_base, bp, steps);
                acc[0] = ac[0]; acc[1] = ac[1]; acc[2] = ac[2]; acc[3] = ac[3];
            }
            const int col = tile * 16 + r;
            const float bj = col < N ? gp.params[ev.b_off[l] + col] : 0.f;
            const int act = (l == L - 1) ? ev.final_act : 1;
            // The tile leaves as whole 16-byte stores (the hand-off the guide validates for a wave that signals for its own stores:
            // every line written whole by one instruction): lane (q, r) holds rows 4q .. 4q + 3 of column r; lane d = (q', R) takes
            // row R's columns 4q' .. 4q' + 3 -- for the next layer that is exactly its quad of k-step `tile` (fragment-major: one
            // contiguous KB per wave instruction), for the head 16 consecutive bytes of the agent's prediction row.
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = act_apply(acc[i] + bj, act);
            const int qd = lane >> 4, Rd = lane & 15;
            azd_f32x4 o;
#pragma unroll
            for (int ik = 0; ik < 4; ++ik) {
                const int src = (Rd >> 2) * 16 + 4 * qd + ik; // the lane that holds row Rd (in its register Rd & 3) of column 4 qd + ik
                const float t0 = __shfl(v[0], src), t1 = __shfl(v[1], src), t2 = __shfl(v[2], src), t3 = __shfl(v[3], src);
                const int rho = Rd & 3;
                o[ik] = rho == 0 ? t0 : rho == 1 ? t1 : rho == 2 ? t2 : t3;
            }
            if (l == L - 1) { // the head's rows: straight to h_theta, write-through (A is a multiple of 4: pool plan)
                const uint32_t ag_row = (uint32_t)__shfl((int)agent_r, Rd);
                const int c0 = tile * 16 + 4 * qd;
                if (c0 < N && (uint32_t)Rd < n) st_sc1_x4(gp.h_theta + (size_t)ag_row * A + c0, o);
            } else {
                float *xo = xb + (size_t)(l & 1) * pl.grp_xstride;
                st_sc1_x4(xo + ((size_t)tile * 64 + (size_t)lane) * 4, o);
            }
            VM_DRAIN(); // this tile's stores are in memory before its arrival counts
            uint32_t arrived = 0;
            if (lane == 0) arrived = __hip_atomic_fetch_add(cnt + l * 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            arrived = uni(arrived);
            if (arrived + 1u == gen * (uint32_t)nt) { // the layer's last tile of this batch (every other tile's stores were in memory before its add)
                if (l < L - 1) tell_all(l, gen);
                else {
                    // every prediction row is out -- the agents go back to their XCD's ready queue, or are queued by their waves where
                    // those are still busy with them (early post: join); then the leader may form the slot's next batch
                    if ((uint32_t)lane < n && lane < 16 && ((home_r & 0x40u) == 0u || (atomicAdd(&pl.join[agent_r], 1u) & 1u))) {
                        const uint32_t x = home_r & (uint32_t)(POOL_XCDS - 1);
                        const uint32_t rl = (pl.ready_lanes && (home_r & 0x80u)) ? 0u : 1u;
                        const uint32_t i = atomicAdd(&ctl->ready[rl][x].tail, 1u);
                        st_sc1(pl.ready_slots + ((size_t)rl * POOL_XCDS + x) * pl.qcap + (i & qmask), agent_r + 1u);
                    }
                    if (lane == 0) st_sc1(flags + (L - 1), gen); // (member 0's line: the leader's)
                }
            }
        }
        if (leave) {
            if (leader) tell_all(7, 0xFFFFFFFFu);
            break;
        }
        if (leader) { // the batch is through when the head's tiles are all in: only then may the slot's buffers be reused
            PoolWait wt;
            for (;;) {
                const uint32_t v = ld_sc1(my_flag + (L - 1));
                if (v >= gen && v != 0xFFFFFFFFu) break;
                __builtin_amdgcn_s_sleep(2);
                if (wt.expired() || ((wt.polls & 63u) == 0u && ld_sc1(&ctl->abort) != 0u)) {
                    atomicExch(&ctl->abort, 1u);
                    leave = true;
                    break;
                }
            }
            if (leave) {
                tell_all(7, 0xFFFFFFFFu);
                break;
            }
            n_batches += 1;
            n_rows += (unsigned long long)n;
            for (int l = 0; l < L; ++l) n_tiles += (unsigned long long)((ev.dims[l + 1] + 15) >> 4);
            busy += (unsigned long long)wall_clock64() - tb0;
            // test hook (AZD_POOL_DEBUG_ABORT_CALL = k): the first slot's leader raises the abort flag after its k-th batch
            if (lane == 0 && si == 0 && pl.debug_abort_call != 0u && n_batches == (unsigned long long)pl.debug_abort_call) atomicExch(&ctl->abort, 1u);
        }
    }
    if (leader && lane == 0) { // evaluator service counters, as pool_eval's (a slot counts as one evaluator)
        atomicAdd(&ctl->eval_busy, busy);
        atomicMax(&ctl->t_last, (unsigned long long)wall_clock64());
        unsigned long long *ctr = a.counters + (size_t)((blockIdx.x * PERSIST_WAVES + (uint32_t)wave) % (uint32_t)a.B) * NUM_COUNTERS;
        atomicAdd(&ctr[25], n_batches);
        atomicAdd(&ctr[26], n_rows);
        atomicAdd(&ctr[27], n_tiles);
        atomicAdd(&ctr[29], busy);
    }
}

// ---------------------------------------------------------------- searcher wavefront
struct PoolIdle { // LDS block of a searcher workgroup: what its waves need not ask device memory again
    uint32_t leave;       // population through, or abort: every wave leaves
    uint32_t claims_done; // no unclaimed agent is left
    uint32_t mean_calls;  // calls completed per agent of this XCD, refreshed by every 8th ticket (early post of the agents behind it)
};

// Run-ahead window: agent t is through call `call` (its candidate, if any, has been performed at the log: the caller drained).
// The wave that counts the last agent hands the call's log entry to the host.
__device__ __forceinline__ void pool_window_count(const PoolArgs &pl, const unsigned long long *log_key, const uint32_t call, const uint32_t B) {
    if (atomicAdd(pl.win_count + call, 1u) + 1u != B) return;
    const unsigned long long key = __hip_atomic_load(log_key + call, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(pl.win_log + call, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(pl.win_flag + call, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// MODE: bit 0 -- hashed rows (the test harness' evaluator, FusedEval kind 4); bit 1 -- run-ahead window (every completed call is
// published to the host).  The product kernel is MODE 0; the others are instantiations of their own so that nothing they need
// costs the product kernel a register.
template <class SP, int MODE>
__device__ __forceinline__ void pool_search(const PersistArgs *pa, const int n_calls, unsigned long long *__restrict__ log_key, typename SP::Lds &s,
                            const uint32_t dyn, const uint32_t xcc, PoolIdle &idle, const bool express) {
    const Arenas &a = pa->a;
    const TolTable &tol = pa->tol;
    const FusedEval &ev = pa->ev;
    const PoolArgs &pl = pa->pool;
    PoolCtl *ctl = pl.ctl;
    constexpr bool HASHED = (MODE & 1) != 0, WINDOW = (MODE & 2) != 0; // (bit 2: evaluator groups compiled in -- nothing of the searchers')
    const uint32_t B = (uint32_t)a.B, qmask = pl.qcap - 1u;
    uint32_t *rslots[2] = {pl.ready_slots + (size_t)xcc * pl.qcap, pl.ready_slots + ((size_t)POOL_XCDS + xcc) * pl.qcap};
    uint32_t *eslots[2] = {pl.eval_slots + (size_t)xcc * pl.qcap, pl.eval_slots + ((size_t)POOL_XCDS + xcc) * pl.qcap};
    for (;;) {
        // ---- take an agent: one whose prediction row has arrived, else one nobody has touched in this launch
        const unsigned long long wp_take0 = WAVE_NOW();
        uint32_t t = NONE, pending = 0, waited = 0;
        if (LANE == 0) {
            // 1) an agent nobody has touched in this launch, while there is one (first come, first served: an XCD gets
            //    agents in proportion to the waves it has free)
            if (!express && LDS_LOAD(&idle.claims_done) == 0u) {
                const uint32_t c = atomicAdd(&ctl->claim_next, 1u);
                if (c < B) {
                    t = c;
                    atomicAdd(&ctl->claimed[xcc].v, 1u);
                    diag_first_touch(a, c);
                } else LDS_STORE(&idle.claims_done, 1u);
            }
            // 2) else the next agent to come back from the evaluator on this XCD: take a ticket (fetch-add: a CAS on
            //    the head made 30 pollers per XCD retry each other and capped the whole chip at ~8 M pops/s) and wait
            //    for its slot.  Waiting waves poll a word of their own, ~1 MHz each.
            if (t == NONE && LDS_LOAD(&idle.leave) == 0u) {
                // Lane mode: the queue of the agents behind the mean progress first -- while it holds agents, or has fewer
                // than AZD_POOL_STANDBY waves standing by (tickets beyond its tail), so that a lagging agent that arrives
                // finds a wave waiting for it.  Fetch-add tickets in both lanes: no CAS, nothing to retry.
                uint32_t rl = 1u;
                if (pl.ready_lanes == 1 && (int)(ld_sc1(&ctl->ready[0][xcc].head) - ld_sc1(&ctl->ready[0][xcc].tail)) < AZD_POOL_STANDBY) rl = 0u;
                // express mode: the express waves serve the lagging agents only; the others take one of them first when more of them
                // wait than express waves stand by (agents queued beyond the tickets taken), so that a lagging agent never waits longer
                // for a wave than it would without the lane
                if (express) rl = 0u;
                else if (pl.ready_lanes == 2 && (int)(ld_sc1(&ctl->ready[0][xcc].tail) - ld_sc1(&ctl->ready[0][xcc].head)) > 0) rl = 0u;
                const uint32_t h = atomicAdd(&ctl->ready[rl][xcc].head, 1u);
                uint32_t *slot = rslots[rl] + (h & qmask);
                PoolWait wt;
                uint32_t v = 0, polls = 0, seen_progress = 0xFFFFFFFFu;
                while ((v = ld_sc1(slot)) == 0u) {
                    if ((++polls & 15u) == 0u) {
                        if (LDS_LOAD(&idle.leave) != 0u) break;
                        if (ld_sc1(&ctl->done_agents) >= B || ld_sc1(&ctl->abort) != 0u) { // nothing will ever fill this ticket
                            LDS_STORE(&idle.leave, 1u);
                            break;
                        }
                    }
                    __builtin_amdgcn_s_sleep(AZD_POOL_POLL_SLEEP);
                    if (wt.expired()) {
                        // A ticket can legitimately wait this long: in a launch of seconds the agents of this XCD may all be
                        // through while others still run.  Only a population that has made no call since the last look is stuck.
                        uint32_t progress = 0u;
                        for (int x = 0; x < POOL_XCDS; ++x) progress += ld_sc1(&ctl->sum_calls[x].v);
                        if (progress != seen_progress) {
                            seen_progress = progress;
                            wt = PoolWait();
                        } else {
                            atomicExch(&ctl->abort, 1u);
                            LDS_STORE(&idle.leave, 1u);
                            break;
                        }
                    }
                }
                if (v) {
                    st_sc1(slot, 0u);
                    if ((h & 7u) == 0u || express) { // mean progress of the agents living on this XCD (express mode: of the unfinished ones)
                        const uint32_t cl = ld_sc1(&ctl->claimed[xcc].v), sc = ld_sc1(&ctl->sum_calls[xcc].v);
                        if (pl.ready_lanes == 2) {
                            const uint32_t dn = ld_sc1(&ctl->done_x[xcc].v), spent = dn * (uint32_t)n_calls;
                            LDS_STORE(&idle.mean_calls, (sc > spent ? sc - spent : 0u) / (cl > dn ? cl - dn : 1u));
                        } else LDS_STORE(&idle.mean_calls, sc / (cl ? cl : 1u));
                    }
                    t = v - 1u;
                    pending = t != NONE ? 1u : 0u;
                    waited = polls > 1u ? 1u : 0u; // this wave stood idle: agents are not queueing for waves right now
                }
            }
        }
        t = uni(t);
        pending = uni(pending);
        waited = uni(waited);
        if (t == NONE) break;
        // another CU of this XCD may have run this agent since this CU last held lines of it
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        diag_per_agent_counters_reset(s);
        if (LANE == 0) s.ctr[31] = (unsigned long long)wall_clock64(); // the wave has an agent in hand from here (slots 30 / 31: busy ticks, stamp)
        diag_wave_take(s, wp_take0); // ticket + wait for its slot
        const unsigned long long wp_add0 = WAVE_NOW();
        WAVE_SYNC();
        uint32_t call = 0u;   // calls of this launch the agent has completed (travels with the agent in PendRec)
        RolloutOut first;     // next_action's choice on the node add_actions fills below, if it does
        first.first_nact = 0u;
        if (pending) { // graph_operations.rs:32-56 for the node the previous call ended on; its row came from an evaluator CU
            diag_agent_waited_for_wave(s, pl, t);
            const PendRec pr = pl.pend[t];
            RolloutOut ro;
            ro.flags = 0;
            ro.cand_c = 0.f;
            ro.cand_node = NONE;
            ro.pos = pr.pos;
            ro.c = pr.c;
            ro.n_preds = pr.n_preds;
            call = pr.call;
            add_actions_agent<SP, true>(a, s, (int)t, 0, &ro, &first);
            diag_wave_add(s, wp_add0); // acquire fence + PendRec + add_actions with the arrived row
        }
        bool posted = false;
        for (;; ++call) {
            if (call >= (uint32_t)n_calls) {
                if (LANE == 0) {
                    atomicAdd(&ctl->done_agents, 1u);
                    if (pl.ready_lanes == 2) atomicAdd(&ctl->done_x[xcc].v, 1u);
                    pool_last_call_done(a, pl, ctl, t);
                }
                break;
            }
            RolloutOut ro;
            ro.post_tail = nullptr;
            ro.posted = 0u;
            // the first call after add_actions: the agent is live and stands on the node just filled
            ro.known_live = first.first_nact != 0u ? 1u : 0u;
            ro.first_nact = first.first_nact;
            ro.first_pp = first.first_pp;
            ro.first_aid = first.first_aid;
            ro.first_g = first.first_g;
            first.first_nact = 0u;
            uint32_t behind = 0u, lane_q = 1u;
            if (HASHED || ev.kind == 3) { // where rollout_agent posts the request the moment the row is out
                if (pl.ready_lanes == 2) { // express mode: does this agent lag behind the unfinished agents of its XCD?
                    const uint32_t ref = LDS_LOAD(&idle.mean_calls);
                    if (call + (uint32_t)AZD_POOL_EXPRESS_SLACK + (ref >> pl.express_shift) < ref) behind = 0x80u;
                } else if (pl.ready_lanes) { // is this agent behind the mean progress of the agents living on this XCD?
                    const uint32_t cl = ld_sc1(&ctl->claimed[xcc].v);
                    const uint32_t mean = ld_sc1(&ctl->sum_calls[xcc].v) / (cl ? cl : 1u);
                    behind = call + 1u < mean ? 0x80u : 0u;
                }
                // early (PoolArgs::early_post): always, or -- mode 2 -- while waves stand idle waiting for agents (the end of a launch, when
                // the slow chains are all that is left: their latency is the launch's, and a wave's time costs nothing)
                // ... or for an agent behind the mean progress (the slow chains are known long before the end: roots in small, dense
                // parts of the space, where a call meets three or four transpositions, take 125 us per call against 92)
                bool early = pl.early_post == 1;
                if (pl.early_post == 2) {
                    const uint32_t mean = LDS_LOAD(&idle.mean_calls);
                    early = waited || behind != 0u || call + (uint32_t)AZD_POOL_BEHIND_SLACK + (mean >> AZD_POOL_BEHIND_SHIFT) < mean;
                }
                ro.post_tail = early ? &ctl->evalq[lane_q][xcc].tail : nullptr;
                ro.post_slots = eslots[lane_q];
                ro.post_mask = qmask;
                ro.post_word = (t + 1u) | ((xcc | behind | 0x40u) << 24);
                ro.post_stamp = pl.stamp + t;
                // hashed rows (test harness): the call whose row this will be, out before the request can be (both posts drain first)
                if (HASHED && LANE == 0) st_sc1(pl.post_call + t, call);
            }
            const unsigned long long wp_roll0 = WAVE_NOW();
            const bool expanded = rollout_agent<SP, true, true>(a, tol, s, dyn, (int)t, &ro);
            diag_wave_rollout(s, wp_roll0); // the whole of rollout_agent, its loading of the agent and its write-back included
            // candidate of this call for the argmin replay (first-min over this tree's new nodes)
            if (LANE == 0 && ro.flags == 0) {
                const uint32_t node = ro.cand_node;
                if (node != NONE) {
                    const unsigned long long key = ((unsigned long long)ordf(ro.cand_c) << 32) |
                                                   ((unsigned long long)(t & 0xFFFFu) << 16) | (unsigned long long)(node & 0xFFFFu);
                    atomicMin(&log_key[call], key); // unconditionally, result unused: a look first would be a round trip of the wave's time
                    a.cand_node[t] = NONE;
                }
            }
            if (LANE == 0) atomicAdd(&ctl->sum_calls[xcc].v, 1u);
            if (!expanded) { // root exhausted (or stopped): no prediction, no add_actions
                if (WINDOW) {
                    VM_DRAIN();
                    if (LANE == 0) pool_window_count(pl, log_key, call, B);
                }
                continue;
            }
            if (HASHED || ev.kind == 3) {
                if (LANE == 0) {
                    PendRec pr;
                    pr.pos = ro.pos;
                    pr.c = ro.c;
                    pr.n_preds = ro.n_preds;
                    pr.call = call + 1u;
                    pl.pend[t] = pr;
                }
                WAVE_SYNC();
                diag_per_agent_counters_flush(a, s, (int)t);
                VM_DRAIN(); // the tree's stores are in this XCD's L2 (and the row's in memory) before the agent can move on
                if (LANE == 0) {
                    if (!ro.posted) { // (rollout_agent posts every row it writes; kept for a caller that passes no queue)
                        diag_stamp_handed_over(pl.stamp + t);
                        const uint32_t i = atomicAdd(&ctl->evalq[lane_q][xcc].tail, 1u);
                        st_sc1(eslots[lane_q] + (i & qmask), (t + 1u) | ((xcc | behind) << 24));
                    }
                    // posted early: this wave is through with the agent now; if the prediction row is out already, queue the agent here
                    else if (atomicAdd(&pl.join[t], 1u) & 1u) {
                        diag_stamp_handed_over(pl.stamp + t);
                        const uint32_t rl = (pl.ready_lanes && behind) ? 0u : 1u;
                        const uint32_t i = atomicAdd(&ctl->ready[rl][xcc].tail, 1u);
                        st_sc1(rslots[rl] + (i & qmask), t + 1u);
                    }
                    if (WINDOW) pool_window_count(pl, log_key, call, B); // (behind the drain above, and off the agent's path)
                }
                posted = true;
                break;
            }
            if (ev.kind == 2) {
                float *h = a.h_theta + (size_t)t * a.A;
                const uint64_t agent = ev.first_agent + (uint64_t)t, cidx = ev.call_base + (uint64_t)call;
                for (int i = LANE; i < a.A; i += 64) {
                    uint64_t r = splitmix(splitmix(splitmix(splitmix(ev.seed ^ 0x70726564ull) ^ agent) ^ cidx) ^ (uint64_t)i);
                    h[i] = (float)(r >> 40) * (1.0f / 16777216.0f);
                }
                WAVE_SYNC();
            }
            add_actions_agent<SP, false>(a, s, (int)t, 0, &ro, &first);
        }
        if (!posted) {
            WAVE_SYNC();
            diag_per_agent_counters_flush(a, s, (int)t);
        }
        if (LANE == 0) s.ctr[30] += (unsigned long long)wall_clock64() - s.ctr[31];
    }
    if (LANE == 0) {
        atomicAdd(&ctl->search_busy, s.ctr[30]);
        atomicMax(&ctl->t_last, (unsigned long long)wall_clock64());
    }
    POOL_SEARCH_FLUSH(a, s, B);
}

// MODE: see pool_search (1: the test harness' hashed rows, FusedEval kind 4 / pool_hash_rows; 2: run-ahead window)
template <class SP, int MODE>
__global__ __launch_bounds__(PERSIST_WAVES * 64) void k_pool(const PersistArgs *__restrict__ pa, int n_calls,
                                                             unsigned long long *__restrict__ log_key, uint32_t dyn_stride,
                                                             const float *__restrict__ params, const float *state_vecs,
                                                             float *h_theta, const void *__restrict__ wpk) {
    // The searcher waves' LDS blocks open the dynamic region (the waves' scratch regions follow them); an evaluator
    // workgroup has no use for them and lays its batch over the whole of it.
    constexpr uint32_t SW_BYTES = (uint32_t)((PERSIST_WAVES * sizeof(typename SP::Lds) + 15) & ~(size_t)15);
    typename SP::Lds *const sw = reinterpret_cast<typename SP::Lds *>(lds_base(0u));
    __shared__ PoolBatch bt;
    __shared__ PoolIdle idle;
    const uint32_t xcc = pool_xcc_id();
    if (threadIdx.x == 0) atomicCAS(&pa->pool.ctl->t_first, 0ull, (unsigned long long)wall_clock64());
    if ((int)blockIdx.x < pa->pool.n_eval) {
        EvalPtrs gp;
        gp.params = params;
        gp.wpk = wpk;
        gp.state_vecs = state_vecs;
        gp.h_theta = h_theta;
        // MODE bit 2: the instantiation that carries the evaluator groups (launched only when the engine has formed groups: their code in
        // the product kernel k_pool<SP, 0> cost every searcher a few spilled registers -- config C 54.2 -> 52.1 M expansions/s, round 5)
        if constexpr ((MODE & 4) != 0) {
            if (pa->pool.grp_g > 0 && (int)blockIdx.x < pa->pool.grp_groups * pa->pool.grp_g) {
                pool_eval_group(pa, gp, xcc);
                return;
            }
        }
        pool_eval<(MODE & 1) != 0>(pa, gp, bt, xcc);
        return;
    }
    const int wave = threadIdx.x >> 6;
    typename SP::Lds &s = sw[wave];
    if (threadIdx.x == 0) {
        idle.leave = 0u;
        idle.claims_done = 0u;
        idle.mean_calls = 0u;
    }
    SP::prepare(pa->a, s);
    if (LANE < NUM_COUNTERS) s.ctr[LANE] = 0;
    __syncthreads();
    // express mode: the last n_express searcher workgroups keep express_waves waves (one per SIMD) and serve the lagging agents
    const bool express = pa->pool.ready_lanes == 2 && (int)blockIdx.x >= (int)gridDim.x - pa->pool.n_express;
    if (express && (uint32_t)wave >= pa->pool.express_waves) return;
    pool_search<SP, MODE>(pa, n_calls, log_key, s, SW_BYTES + (uint32_t)wave * dyn_stride, xcc, idle, express);
}

// ---------------------------------------------------------------- searchers only: the evaluator is a stream of batched GEMM launches
// A model too large for an evaluator workgroup's LDS (config E: 3676-512-512-512-2450, 7.3 MB of bf16 weights) is served from
// OUTSIDE the kernel: the searchers post their requests as above; on a second stream the host replays, until the launch is over,
// a graph of k_ext_take (collect what is posted: one list of agents), the layers' GEMMs over the gathered rows
// (gemm_bf16_glds.inc: k_gemm16 with row lists) and k_ext_deliver (the agents go back on their ready queues).  The searchers'
// grid leaves CUs free for those launches.  Rows and requests are written through (sc1) and a kernel's launch acquires, its end
// releases: the same hand-off as inside k_pool, with a kernel boundary in place of the evaluator's polls.
// WAVES bounds a workgroup three ways: it lays out WAVES static blocks ahead of the waves' scratch regions (SW_BYTES, which the
// host's plan repeats: launchers.inc), it is launch-bounded for WAVES * 64 threads, and hence sets the registers a wave may keep.
// The dense-graph space launches it with PERSIST_WAVES, and fewer where a wave's block is large: six for the 64-row
// Aouchiche-Hansen cost (20-KB blocks), eight for the Ramsey tiers with max_slots > 0 (ramsey_ext.inc) -- sixteen RamseyU64Lds
// blocks are 79 KB before any wave's clique counts, and eight waves may keep 256 registers each.
template <class SP, int MODE, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_pool_search(const PersistArgs *__restrict__ pa, int n_calls,
                                                            unsigned long long *__restrict__ log_key, uint32_t dyn_stride) {
    constexpr uint32_t SW_BYTES = (uint32_t)((WAVES * sizeof(typename SP::Lds) + 15) & ~(size_t)15);
    typename SP::Lds *const sw = reinterpret_cast<typename SP::Lds *>(lds_base(0u));
    __shared__ PoolIdle idle;
    const uint32_t xcc = pool_xcc_id();
    if (threadIdx.x == 0) atomicCAS(&pa->pool.ctl->t_first, 0ull, (unsigned long long)wall_clock64());
    const int wave = threadIdx.x >> 6;
    typename SP::Lds &s = sw[wave];
    if (threadIdx.x == 0) {
        idle.leave = 0u;
        idle.claims_done = 0u;
        idle.mean_calls = 0u;
    }
    SP::prepare(pa->a, s);
    if (LANE < NUM_COUNTERS) s.ctr[LANE] = 0;
    __syncthreads();
    pool_search<SP, MODE>(pa, n_calls, log_key, s, SW_BYTES + (uint32_t)wave * dyn_stride, xcc, idle, false);
}

#ifdef AZD_TU_POOL_EXT
// What the searchers have posted, XCD by XCD (wave x of the block takes queue x): the tickets whose slot is filled, in order, up
// to the first that is not (its producer has taken the ticket and not stored yet: next time).  Several collectors may run at once
// (the host keeps two evaluator streams going): a run of tickets belongs to whoever moves the queue's head over it (CAS).
// out_rows[i] = agent, out_home[i] = the request's flag byte (home XCD, early post, lagging), *out_n = how many (<= the population:
// an agent has at most one request out).
__global__ __launch_bounds__(POOL_XCDS * 64) void k_ext_take(PoolArgs pl, uint32_t *__restrict__ out_rows, uint32_t *__restrict__ out_home,
                                                             uint32_t *__restrict__ out_n, unsigned long long *__restrict__ t0) {
    __shared__ uint32_t n_sh;
    if (threadIdx.x == 0) n_sh = 0u;
    __syncthreads();
    const uint32_t x = threadIdx.x >> 6, qmask = pl.qcap - 1u;
    PoolCtl *ctl = pl.ctl;
    uint32_t *slots = pl.eval_slots + ((size_t)POOL_XCDS + x) * pl.qcap;
    constexpr int G = 8; // tickets per lane and look: a look costs two queue-word round trips and a CAS whatever it collects (round 4: 8,
                         // so that an XCD's share of a batch of ~3500 requests is one look instead of two)
    for (int tries = 0; tries < 64; ++tries) {
        const uint32_t head = ld_sc1(&ctl->evalq[1][x].head), tail = ld_sc1(&ctl->evalq[1][x].tail);
        if ((int)(tail - head) <= 0) break;
        uint32_t v[G];
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const uint32_t ticket = head + (uint32_t)(LANE + 64 * q);
            v[q] = (int)(tail - ticket) > 0 ? ld_sc1(slots + (ticket & qmask)) : 0u;
        }
        uint32_t run = 0u; // filled slots from the head on
        bool open = true;
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const uint64_t full = __ballot(v[q] != 0u);
            const uint32_t r = full == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~full);
            if (open) run += r;
            open = open && r == 64u;
        }
        if (run == 0u) break;
        uint32_t won = 0u, base = 0u;
        if (LANE == 0) {
            won = atomicCAS(&ctl->evalq[1][x].head, head, head + run) == head ? 1u : 0u;
            if (won) base = atomicAdd(&n_sh, run);
        }
        won = (uint32_t)__shfl((int)won, 0, 64);
        base = (uint32_t)__shfl((int)base, 0, 64);
        if (!won) continue; // another collector took them: look again
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const uint32_t idx = (uint32_t)(LANE + 64 * q);
            if (idx < run) {
                st_sc1(slots + ((head + idx) & qmask), 0u);
                out_rows[base + idx] = (v[q] & 0xFFFFFFu) - 1u;
                out_home[base + idx] = v[q] >> 24;
            }
        }
        if (run < 64u * G) break;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *out_n = n_sh;
        if (n_sh) *t0 = (unsigned long long)wall_clock64(); // the evaluator's side is busy from here to the hand-back (PoolCtl::eval_busy)
    }
}
// The batch's prediction rows are out (the GEMM launches before this one have ended): every agent goes back to its XCD's ready
// queue -- at once, or once the wave that posted it early is through with it too (PoolArgs::join), as in pool_eval.
__global__ void k_ext_deliver(PoolArgs pl, Arenas a, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ home, const uint32_t *__restrict__ n_rows,
                              const unsigned long long *__restrict__ t0) {
    const uint32_t n = *n_rows, i = blockIdx.x * blockDim.x + threadIdx.x, qmask = pl.qcap - 1u;
    PoolCtl *ctl = pl.ctl;
    if (i == 0u && n) { // evaluator service counters (AZD_CTR_EVAL_*), summed over agents by the host
        atomicAdd(&a.counters[25], 1ull);
        atomicAdd(&a.counters[26], (unsigned long long)n);
        atomicAdd(&ctl->eval_busy, (unsigned long long)wall_clock64() - *t0);
        // test hook (AZD_POOL_DEBUG_ABORT_CALL = k): the abort flag is raised behind the k-th batch this engine has handed back
        if (pl.debug_abort_call != 0u && atomicAdd(&a.counters[27], 1ull) + 1ull == (unsigned long long)pl.debug_abort_call) atomicExch(&ctl->abort, 1u);
    }
    // Round 4: one atomic per (wave, queue) instead of one per agent -- 3500 agents adding to the eight XCDs' tails, one after the
    // other, were most of this kernel's 11 us.  The lanes that queue an agent on the same (lane, XCD) queue are counted by ballots,
    // their first lane adds the count and hands out consecutive slots.  (Control flow stays wave-uniform: every lane runs every step.)
    const bool live = i < n;
    const uint32_t t = live ? rows[i] : 0u, hm = live ? home[i] : 0u;
    const bool mine = live && ((hm & 0x40u) == 0u || (atomicAdd(&pl.join[t], 1u) & 1u));
    const uint32_t x = hm & (uint32_t)(POOL_XCDS - 1);
    const uint32_t rl = (pl.ready_lanes && (hm & 0x80u)) ? 0u : 1u;
    const uint32_t q = rl * (uint32_t)POOL_XCDS + x; // which of the 16 ready queues
    const int lane = (int)(threadIdx.x & 63);
    for (uint32_t qq = 0; qq < 2u * (uint32_t)POOL_XCDS; ++qq) {
        const uint64_t m = __ballot(mine && q == qq);
        if (m == 0ull) continue;
        const int leader = __ffsll((unsigned long long)m) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&ctl->ready[qq / (uint32_t)POOL_XCDS][qq % (uint32_t)POOL_XCDS].tail, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, leader, 64);
        if (mine && q == qq) {
            const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            st_sc1(pl.ready_slots + (size_t)qq * pl.qcap + (k & qmask), t + 1u);
        }
    }
}
// FusedEval kind 4 (test harness) outside the kernel: h(agent, call, a) of the call each collected agent posted (pool_hash_rows),
// one block per row of the list
__global__ void k_ext_hash_rows(const PersistArgs *__restrict__ pa, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ n_rows,
                                float *__restrict__ h_theta) {
    if (blockIdx.x >= *n_rows) return;
    const FusedEval &ev = pa->ev;
    const uint32_t t = rows[blockIdx.x];
    const int A = pa->a.A;
    const uint64_t agent = ev.first_agent + (uint64_t)t, cidx = ev.call_base + (uint64_t)ld_sc1(pa->pool.post_call + t);
    for (int i = threadIdx.x; i < A; i += blockDim.x) {
        const uint64_t h = splitmix(splitmix(splitmix(splitmix(ev.seed ^ 0x70726564ull) ^ agent) ^ cidx) ^ (uint64_t)i);
        h_theta[(size_t)t * A + i] = (float)(h >> 40) * (1.0f / 16777216.0f);
    }
}
#endif // AZD_TU_POOL_EXT

// ---------------------------------------------------------------- host: LDS plan shared by the two spaces
static bool pool_plan_common(const Arenas &a, const FusedEval &ev, PoolArgs *pool, uint32_t *dyn_stride, size_t *dyn_bytes,
                             const char **why, const size_t search_bytes, const size_t wave_lds_bytes) {
    if (a.B > 65536 || a.node_cap > 65536) { // (agent, node) are packed 16 + 16 bits in the argmin log
        *why = "pool step: more than 65536 agents or nodes per tree";
        return false;
    }
    if (a.S % 4 != 0) {
        *why = "pool step: STATE_DIM must be a multiple of 4 (rows travel as 16-byte stores)";
        return false;
    }
    const size_t stride = (search_bytes + 15) & ~(size_t)15;
    const size_t sw_bytes = (PERSIST_WAVES * wave_lds_bytes + 15) & ~(size_t)15; // k_pool's SW_BYTES
    size_t total = sw_bytes + stride * PERSIST_WAVES;
    const size_t static_lds = sizeof(PoolBatch) + sizeof(PoolIdle) + 256;
    pool->eval_stride = 0;
    pool->eval_out_off = 0;
    pool->eval_rows = PERSIST_WAVES;
    if (ev.kind == 3) {
        for (int l = 0; l < ev.n_layers; ++l)
            if (ev.dims[l] % (l == 0 ? 4 : 16) != 0) {
                *why = "pool step: hidden widths must be multiples of 16 and the input width a multiple of 4";
                return false;
            }
        const int A = ev.dims[ev.n_layers];
        if (A % 4 != 0) {
            *why = "pool step: ACTION_DIM must be a multiple of 4 (rows travel as 16-byte stores)";
            return false;
        }
        const size_t x_el = (size_t)((ev.dims[0] + 15) & ~15);
        const size_t act = x_el + (size_t)ev.hid[0] + (size_t)ev.hid[1]; // elements: f32, or bf16 halves
        const size_t act_fl = ev.bf16 ? act / 2 : act;                   // floats
        // the head's output (f32) goes over the input x, which is dead once the first layer is through -- where it fits and
        // the model has more than one layer; else behind the activations
        const size_t x_fl = ev.bf16 ? x_el / 2 : x_el;
        const bool alias = ev.n_layers >= 2 && (size_t)A <= x_fl;
        const size_t out_off = alias ? 0 : act_fl;
        const size_t row = act_fl + (alias ? 0 : (size_t)A) + 4; // + 16 B: rows start on different banks
        pool->eval_stride = (uint32_t)row;
        pool->eval_out_off = (uint32_t)out_off;
        // two row tiles per batch where 32 rows fit (the 3 x 256 models do, Ramsey's 680-wide input too; 512-1024-512 does not)
        const bool two = AZD_POOL_TWO_TILES && row * sizeof(float) * POOL_BATCH_MAX + static_lds <= 160 * 1024;
        pool->eval_rows = two ? POOL_BATCH_MAX : PERSIST_WAVES;
        const size_t eval_bytes = row * sizeof(float) * pool->eval_rows;
        if (eval_bytes > total) total = eval_bytes;
    }
    if (ev.kind == 4) { // the hashed rows: just the outputs, 32 rows per batch
        if (a.A % 4 != 0) {
            *why = "pool step: ACTION_DIM must be a multiple of 4 (rows travel as 16-byte stores)";
            return false;
        }
        pool->eval_stride = (uint32_t)a.A + 4u;
        pool->eval_out_off = 0;
        pool->eval_rows = POOL_BATCH_MAX;
        const size_t eval_bytes = (size_t)pool->eval_stride * sizeof(float) * pool->eval_rows;
        if (eval_bytes > total) total = eval_bytes;
    }
    if (total + static_lds > 160 * 1024) {
        *why = "pool step: a batch of 16 rows (or 16 searcher waves' blocks and scratch) does not fit the CU's 160 KB of LDS";
        return false;
    }
    *dyn_stride = (uint32_t)stride;
    *dyn_bytes = total;
    return true;
}
