// persistent_step.inc -- included after tree_core.inc and a space policy (inside namespace azd).
//
// CU-resident form of NablaOptimizer::par_roll_out_episodes (optimizer/mod.rs:121-191): one
// workgroup = 16 wavefronts = 16 agents stays on its CU for `n_calls` calls.  Per call:
//     every wave:   roll_out_episodes for its agent                  (optimizer/mod.rs:159-174)
//     barrier
//     workgroup:    model.write_predictions for its 16 rows          (:175-176)
//                   -- the MLP runs on the matrix cores right here: M = 16 rows is one
//                   v_mfma_f32_16x16x4_f32 tile, activations stay in LDS, the 1 MB of weights
//                   streams from L2 (shared by every CU) --
//     barrier
//     every wave:   add_actions                                      (:177-189)
// There is no grid-wide synchronisation: agents never exchange data during episodes, the model
// is constant within an epoch, and the per-call argmin reduction (:190, :194-246) is replayed
// afterwards, in call order, from a [call][workgroup] log of candidates by k_argmin_log.
// What this buys over the launch-per-phase form: no kernel boundaries inside a call, and a call
// lasts as long as the slowest of 16 agents instead of the slowest of the whole population.

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PERSIST_WAVES = 16;

__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == 1) return v > 0.f ? v : 0.f;
    if (act == 2) return 1.0f / (1.0f + expf(-v));
    return v;
}

#ifndef AZD_TU_ASYNC
// dfdx.rs:69-84 for the workgroup's 16 rows.  x rows come from a.state_vecs (written by the waves
// before the barrier), hidden activations ping-pong in LDS, the head's rows go to a.h_theta.
__device__ void mlp_forward_wg(const Arenas &a, const FusedEval &ev, const int t0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = ev.dims[0];
    const int ldx = S + 4, ldh0 = ev.hid[0] + 4, ldh1 = ev.hid[1] + 4; // the ping-pong buffers are sized independently (FusedEval::hid)
    float *xb = (float *)azd_dyn_lds;
    float *hb0 = xb + PERSIST_WAVES * ldx;
    float *hb1 = hb0 + PERSIST_WAVES * ldh0;
    // stage the 16 input rows (rows beyond the population read as zeros)
    const int q_per_row = S >> 2;
    for (int idx = tid; idx < PERSIST_WAVES * q_per_row; idx += PERSIST_WAVES * 64) {
        const int r = idx / q_per_row, c4 = idx - r * q_per_row;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + r < a.B) v = *reinterpret_cast<const float4 *>(a.state_vecs + (size_t)(t0 + r) * S + 4 * c4);
        *reinterpret_cast<float4 *>(xb + r * ldx + 4 * c4) = v;
    }
    __syncthreads();
    const int L = ev.n_layers;
    for (int l = 0; l < L; ++l) {
        const int K = ev.dims[l], N = ev.dims[l + 1];
        const float *in = (l == 0) ? xb : ((l & 1) ? hb0 : hb1);
        const int ldin = (l == 0) ? ldx : ((l & 1) ? ldh0 : ldh1);
        float *out = (l & 1) ? hb1 : hb0;
        const int ldh = (l & 1) ? ldh1 : ldh0;
        const float *W = ev.params + ev.w_off[l];
        const float *bias = ev.params + ev.b_off[l];
        const int act = (l == L - 1) ? ev.final_act : 1;
        for (int n0 = wave * 16; n0 < N; n0 += PERSIST_WAVES * 16) {
            const int wrow = n0 + (lane & 15);
            const bool wvalid = wrow < N;
            const float *wp = W + (size_t)(wvalid ? wrow : 0) * K + 4 * (lane >> 4);
            const float *ap = in + (lane & 15) * ldin + 4 * (lane >> 4);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int K16 = K & ~15;
            for (int k0 = 0; k0 < K16; k0 += 16) {
                float4 bq = *reinterpret_cast<const float4 *>(wp + k0);
                if (!wvalid) bq = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 aq = *reinterpret_cast<const float4 *>(ap + k0);
                // lane l feeds A[row l&15][k] and B[k][col l&15] with k = k0 + 4*(l>>4) + j
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.x, bq.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.y, bq.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.z, bq.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.w, bq.w, acc, 0, 0, 0);
            }
            if (K16 < K) { // K % 16 in {4, 8, 12}: the quads past the row end enter as zeros
                const bool ok = wvalid && (K16 + 4 * (lane >> 4) < K);
                float4 bq = make_float4(0.f, 0.f, 0.f, 0.f), aq = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) {
                    bq = *reinterpret_cast<const float4 *>(wp + K16);
                    aq = *reinterpret_cast<const float4 *>(ap + K16);
                }
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.x, bq.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.y, bq.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.z, bq.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aq.w, bq.w, acc, 0, 0, 0);
            }
            // D layout: col = lane&15, row = 4*(lane>>4) + r
            const int col = n0 + (lane & 15);
            if (col < N) {
                const float bj = bias[col];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * (lane >> 4) + r;
                    const float v = act_apply(acc[r] + bj, act);
                    if (l == L - 1) {
                        if (t0 + row < a.B) a.h_theta[(size_t)(t0 + row) * N + col] = v;
                    } else {
                        out[row * ldh + col] = v;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// PROFILE=1: agent t's ticks of a k_persist call behind its search -- barrier wait (slot 24), evaluator (28), add_actions (29) --
// from the stamps at the end of the roll-out, behind the barrier and behind the evaluator
__device__ __forceinline__ void diag_persist_agent_ticks(const Arenas &a, const int t, const unsigned long long ph_r1, const unsigned long long ph_b1,
                                                         const unsigned long long ph_m1) {
    if constexpr (DIAG_PROFILE)
        if (LANE == 0) {
            unsigned long long *ctr = a.counters + (size_t)t * NUM_COUNTERS;
            ctr[24] += ph_b1 - ph_r1;
            ctr[28] += ph_m1 - ph_b1;
            ctr[29] += PH_NOW() - ph_m1;
        }
}

// The argument block lives in device memory (not in kernel arguments): ~140 dwords of pointers
// and tables kept in SGPRs for the whole launch cost the kernel 100 spilled scalars; from memory
// they are scalar loads at the point of use.
template <class SP>
__global__ __launch_bounds__(PERSIST_WAVES * 64) void k_persist(const PersistArgs *__restrict__ pa, int n_calls,
                                                                unsigned long long *__restrict__ log_key,
                                                                uint32_t *__restrict__ log_node, uint32_t dyn_stride) {
    const Arenas &a = pa->a;
    const TolTable &tol = pa->tol;
    const FusedEval &ev = pa->ev;
    __shared__ typename SP::Lds sw[PERSIST_WAVES];
    __shared__ unsigned long long s_cand[PERSIST_WAVES];
    __shared__ uint32_t s_cnode[PERSIST_WAVES];
    const int wave = threadIdx.x >> 6;
    const int t0 = blockIdx.x * PERSIST_WAVES;
    const int t = t0 + wave;
    const bool active = t < a.B;
    typename SP::Lds &s = sw[wave];
    const uint32_t dyn = (uint32_t)wave * dyn_stride;
    SP::prepare(a, s);
    WAVE_SYNC();
    for (int call = 0; call < n_calls; ++call) {
        if (active) rollout_agent<SP>(a, tol, s, dyn, t);
        const unsigned long long ph_r1 = PH_NOW();
        // this call's candidate for par_update_argmmim_data: first-min over the nodes this tree
        // created since its last inspection (num_inspected_nodes = nodes.len() afterwards)
        if (LANE == 0) {
            unsigned long long key = ~0ull;
            uint32_t node = NONE;
            if (active && a.flags[t] == 0) {
                node = a.cand_node[t];
                if (node != NONE) key = ((unsigned long long)ordf(a.cand_c[t]) << 32) | (unsigned long long)(uint32_t)t;
                a.cand_node[t] = NONE;
            }
            s_cand[wave] = key;
            s_cnode[wave] = node;
        }
        __syncthreads();
        const unsigned long long ph_b1 = PH_NOW();
        if (wave == 0) {
            unsigned long long k = LANE < PERSIST_WAVES ? s_cand[LANE] : ~0ull;
            const unsigned long long m = wave_min_u64(k);
            const uint64_t who = __ballot(k == m);
            if (LANE == 0) {
                const size_t slot = (size_t)call * gridDim.x + blockIdx.x;
                log_key[slot] = m;
                log_node[slot] = m == ~0ull ? NONE : s_cnode[first_lane(who)];
            }
        }
        // model.write_predictions(state_vecs, h_theta) for this workgroup's rows
        if (ev.kind == 3) {
            mlp_forward_wg(a, ev, t0);
        } else if (ev.kind == 2 || ev.kind == 4) {
            if (active) {
                float *h = a.h_theta + (size_t)t * a.A;
                const uint64_t agent = ev.first_agent + (uint64_t)t, cidx = ev.call_base + (uint64_t)call;
                for (int i = LANE; i < a.A; i += 64) {
                    uint64_t r = splitmix(splitmix(splitmix(splitmix(ev.seed ^ 0x70726564ull) ^ agent) ^ cidx) ^ (uint64_t)i);
                    h[i] = (float)(r >> 40) * (1.0f / 16777216.0f);
                }
            }
        } // kind 1 (TrivialModel): h_theta untouched
        __syncthreads();
        const unsigned long long ph_m1 = PH_NOW();
        if (active) add_actions_agent<SP>(a, s, t, 0);
        if (active) diag_persist_agent_ticks(a, t, ph_r1, ph_b1, ph_m1);
    }
}

// Replays par_update_argmmim_data (optimizer/mod.rs:194-246) for `n_calls` calls, in call order,
// from the candidate log of k_persist, then rebuilds ArgminData for the last improvement (:226-241).
template <class SP>
__global__ __launch_bounds__(64) void k_argmin_log(Arenas a, int n_calls, int n_wg, const unsigned long long *__restrict__ log_key,
                                                   const uint32_t *__restrict__ log_node) {
    __shared__ typename SP::Lds s;
    const uint32_t dyn = 0;
    uint32_t best = ordf(a.argmin->eval);
    int wt = -1;
    uint32_t win_node = NONE;
    unsigned long long improved = 0;
    for (int call = 0; call < n_calls; ++call) {
        unsigned long long m = ~0ull;
        uint32_t m_node = NONE;
        for (int base = 0; base < n_wg; base += 64) {
            const int i = base + LANE;
            unsigned long long k = i < n_wg ? log_key[(size_t)call * n_wg + i] : ~0ull;
            const unsigned long long km = wave_min_u64(k);
            if (km < m) {
                m = km;
                const uint64_t who = __ballot(k == km);
                const int src = first_lane(who);
                const uint32_t nd = i < n_wg ? log_node[(size_t)call * n_wg + i] : NONE;
                m_node = (uint32_t)__shfl((int)nd, src, 64);
            }
        }
        if (m != ~0ull && (uint32_t)(m >> 32) < best) { // strict: n.weight.c < min_eval (:211)
            best = (uint32_t)(m >> 32);
            wt = (int)(m & 0xFFFFFFFFull);
            win_node = m_node;
            improved += 1;
        }
    }
    if (wt < 0) return;
    if (LANE == 0) atomicAdd(&a.status->improved, improved - 1); // argmin_replay adds the last one
    argmin_replay<SP>(a, s, dyn, wt, win_node, 0);
}

// ---------------------------------------------------------------- host: LDS plan shared by the spaces
// wave_dyn_bytes: a wave's dynamic region (SP::dyn_bytes); wave_lds_bytes: its static block (SP::Lds).  False when the workgroup
// does not fit a CU or the in-kernel MLP cannot take the layer widths.
static bool persist_plan_common(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why,
                                const size_t wave_dyn_bytes, const size_t wave_lds_bytes) {
    const size_t stride = (wave_dyn_bytes + 15) & ~(size_t)15;
    size_t total = stride * PERSIST_WAVES;
    if (ev.kind == 3) {
        if (ev.bf16) { // bf16 weight storage is built into the asynchronous step only
            *why = "barrier step: bf16 weight storage is not built into it";
            return false;
        }
        for (int l = 0; l < ev.n_layers; ++l)
            if (ev.dims[l] % 4 != 0) { // the in-kernel MLP loads rows as float4
                *why = "barrier step: layer widths must be multiples of 4";
                return false;
            }
        size_t mlp = (size_t)PERSIST_WAVES * ((size_t)(ev.dims[0] + 4) + (size_t)(ev.hid[0] + 4) + (size_t)(ev.hid[1] + 4)) * sizeof(float);
        if (mlp > total) total = mlp;
    }
    const size_t static_lds = PERSIST_WAVES * (wave_lds_bytes + 16) + 256;
    if (total + static_lds > 160 * 1024) {
        *why = "barrier step: 16 rows of activations do not fit the CU's 160 KB of LDS";
        return false;
    }
    *dyn_stride = (uint32_t)stride;
    *dyn_bytes = total;
    return true;
}
#endif // !AZD_TU_ASYNC
