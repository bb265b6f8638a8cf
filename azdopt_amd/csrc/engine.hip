// engine.hip -- host side of the C ABI (include/azdopt_amd.h): owns the device arenas,
// sequences the kernels of one NablaOptimizer call on a HIP stream, copies results out.
// No CPU fallback: every compute entry point needs a gfx950 device.
#include "engine_impl.h"

namespace azd {
thread_local std::string g_last_error;

int hip_fail(hipError_t e, const char *what) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return AZD_ERR_NO_DEVICE;
    if (e == hipErrorOutOfMemory) return AZD_ERR_OUT_OF_MEMORY;
    return AZD_ERR_HIP;
}

int device_ok(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_last_error = "no HIP device visible (this library has no CPU fallback)";
        return AZD_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        g_last_error = "device ordinal out of range";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    return AZD_OK;
}

// The searcher-only pool step's two forms (ExtPoolForm, engine_impl.h)
static const ExtPoolForm *ext_pool_form(bool dense_space) {
    // the dense-graph space, whatever its cost (the 64-row Aouchiche-Hansen cost has the same knobs and bounds: a setting above the 6
    // wavefronts its kernels are built for runs what fits).  One evaluator stream, for fp32 rows (AZD_ENGINE_EXT_POOL_F32) as for
    // bf16: with the gathered fp32 GEMMs a second stream gave +2..4 % at 512 agents (AH N = 31, AH-wide N = 50) and at config E's
    // shape, and -9 % at AH N = 31 with 4096 agents (5.03 against 5.51 M expansions/s) -- no win across the shapes, so no default
    // of its own (profiles/r16_dense_ext_f32.txt; AZD_DENSE_POOL_STREAMS=2 where it helps)
    static const ExtPoolForm dense =
        {4, 16, true, false, 1, 1, /* the request leaves with the row: the GEMMs run while the wave computes lambda_1 and the matching */
         "AZD_DENSE_NO_POOL", "AZD_DENSE_POOL_WAVES", "AZD_DENSE_POOL_SEARCH_WGS", "AZD_DENSE_POOL_STREAMS", "AZD_DENSE_POOL_ROUNDS", "AZD_DENSE_POOL_DEPTH",
         "AZD_DENSE_POOL_DEBUG", "dense pool",
         "AZD_DENSE_POOL_WAVES must be 4..16 (wavefronts per searcher workgroup of the dense-graph pool step)",
         "dense-graph space: the pool step is not configured for this engine",
         "an earlier pool launch of this engine aborted: launch-per-phase form",
         "dense-graph space: the pool step needs an evaluator that serves gathered bf16 rows (ActionModel with bf16 storage)",
         "dense-graph space: the pool step needs an evaluator that serves gathered rows (ActionModel: bf16 storage, or fp32 storage under "
         "AZD_ENGINE_EXT_POOL_F32)",
         "dense-graph space: the device holds no searcher workgroup of the pool step",
         "dense pool step aborted (a queue wait ran into its bound: the searchers or the evaluator's launches made no "
         "progress); the launch-per-phase kernels completed the launch and serve this engine from here on",
         "dense pool step aborted with the test harness' prediction stream: no recovery"};
    // Ramsey tiers with max_slots > 0 under AZD_ENGINE_EXT_POOL_STEP.  Eight wavefronts per workgroup.  The request
    // leaves with the row (early post): there is no cost to compute behind it, but the tree's write-back and the wave's drain still
    // overlap with the evaluator's round (r3333 1.54 against 1.46 M expansions/s, r45 on the 64-bit tier 0.94 against 0.90).  Two
    // evaluator streams: the evaluator's rounds, not the searchers, bound these engines (its stream is busy 0.8-0.9 of a launch, a
    // searcher wave 0.1-0.2), and a second stream collects and runs its first layer while the first is in its later ones -- r45 on
    // the wide tier 1.26 -> 1.38 M, r3333 and r45 on the 64-bit tier +1..3 % (profiles/r09_ramsey_ext_pool.txt); the dense-graph
    // space, with a population ten times as large, measured the opposite.
    static const ExtPoolForm ramsey =
        {1, 8, false, true, 1, 2, nullptr, "AZD_RAMSEY_EXT_POOL_WAVES", "AZD_RAMSEY_EXT_POOL_SEARCH_WGS",
         "AZD_RAMSEY_EXT_POOL_STREAMS", "AZD_RAMSEY_EXT_POOL_ROUNDS", "AZD_RAMSEY_EXT_POOL_DEPTH", "AZD_RAMSEY_EXT_POOL_DEBUG", "ramsey external pool",
         "AZD_RAMSEY_EXT_POOL_WAVES must be 1..8 (wavefronts per searcher workgroup of the external pool step)",
         "external pool step: not configured for this engine",
         "external pool step: an earlier launch of this engine aborted: launch-per-phase form",
         "external pool step: needs an evaluator that serves gathered bf16 rows (ActionModel with bf16 storage)",
         "external pool step: needs an evaluator that serves gathered rows (ActionModel: bf16 storage, or fp32 storage under AZD_ENGINE_EXT_POOL_F32)",
         "external pool step: the device holds no searcher workgroup",
         "external pool step aborted (a queue wait ran into its bound: the searchers or the evaluator's launches made no "
         "progress); the launch-per-phase kernels completed the launch and serve this engine from here on",
         "external pool step aborted with the test harness' prediction stream: no recovery"};
    return dense_space ? &dense : &ramsey;
}

// The fourteen kinds of engine (engine_impl.h: TierDesc).  The tables of c21 and Ramsey (space_ops.h) are put together from their units'
// parts: c21 has no searcher-only pool step; the 64-bit Ramsey tier's is joined to the three parts of its phase unit's table.
static const TierDesc *tier_desc(Tier t) {
    static const SpaceOps c21 = {c21_phase_ops(), c21_async_ops(), c21_pool_ops(), PoolSearchOps{}};
    static const SpaceOps ramsey = {ramsey_phase_ops(), ramsey_async_ops(), ramsey_pool_ops(), ramsey_pool_search_ops()};
    static const SpaceOps ramsey64 = {ramsey64_ops(), ramsey64_ops(), ramsey64_ops(), ramsey64_pool_search_ops()};
    static const SpaceOps ramsey64_big = {ramsey64_big_ops(), ramsey64_big_ops(), ramsey64_big_ops(), ramsey64_big_pool_search_ops()};
    const ExtPoolForm *const xd = ext_pool_form(true), *const xr = ext_pool_form(false);
    static const TierDesc tiers[TIER_COUNT] = {
        {TIER_C21, SPACE_C21, &c21, nullptr, 0, 0, false, false, false, 1, 1, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr},
        {TIER_RAMSEY, SPACE_RAMSEY, &ramsey, nullptr, sizeof(RamseyArgminRec), 128, false, false, false, 1, 1, 0, AZD_RAMSEY_MAX_N, 256, 64 * MAX_KW, 0, 5, false,
         "unsupported Ramsey space (need 3 <= n, E <= 256, 2..4 colours, clique sizes 2..5, E*C <= 384)", nullptr, nullptr, nullptr},
        // max_slots > 0: the most permitted edges a root may bring; device keys padded to the widths ramsey_kernels.hip is built for
        {TIER_RAMSEY_WIDE, SPACE_RAMSEY, &ramsey, xr, sizeof(RamseyWideArgminRec), 128, true, true, false, 1, 1, 0, AZD_RAMSEY_WIDE_MAX_N, 496, 1024, 0, 5, false,
         "unsupported wide Ramsey space (max_slots > 0: need 3 <= n <= 32, 2..4 colours, clique sizes 2..5, E*C <= 1024)",
         "wide Ramsey space: need 1 <= max_slots <= E (azd_engine_config::max_slots: permitted edges per root)", nullptr,
         // (cur_seq holds MAX_NODE_ACTIONS actions; a wide path can be longer)
         "wide Ramsey space (max_slots > 0): ActionSet paths only (path_kind = AZD_PATH_SET), no Layered wrapper (layers <= 1)"},
        // AZD_ENGINE_RAMSEY_U64: uint64_t neighbourhood rows of 64 vertices, keys of RAMSEY_U64_KW words, its own record
        {TIER_RAMSEY_U64, SPACE_RAMSEY, &ramsey64, xr, sizeof(RamseyU64ArgminRec), 512, true, true, false, 1, 1, 0, AZD_RAMSEY_U64_MAX_N, 2016,
         64 * RAMSEY_U64_KW, AZD_RAMSEY_U64_NODE_ACTIONS, 5, false,
         "unsupported 64-bit Ramsey space (AZD_ENGINE_RAMSEY_U64: need 3 <= n <= 64, 2..4 colours, clique sizes 2..5, E*C <= 2304)",
         "64-bit Ramsey space: need 1 <= max_slots <= E (azd_engine_config::max_slots: permitted edges per root)",
         "64-bit Ramsey space: a node holds 512 actions: need max_slots * (C - 1) <= 512 (azd_engine_config::max_slots)",
         "64-bit Ramsey space (AZD_ENGINE_RAMSEY_U64): ActionSet paths only (path_kind = AZD_PATH_SET), no Layered wrapper (layers <= 1)"},
        // AZD_ENGINE_RAMSEY_BIG_CLIQUES beside AZD_ENGINE_RAMSEY_U64: the same tier over kernels that count cliques up to K8
        // (ramsey64_big_kernels.hip); the record, the limits and the pool step's form are the 64-bit tier's
        {TIER_RAMSEY_U64_BIG, SPACE_RAMSEY, &ramsey64_big, xr, sizeof(RamseyU64ArgminRec), 512, true, true, false, 1, 1, 0, AZD_RAMSEY_U64_MAX_N, 2016,
         64 * RAMSEY_U64_KW, AZD_RAMSEY_U64_NODE_ACTIONS, AZD_RAMSEY_BIG_CLIQUE_MAX, true,
         "unsupported 64-bit Ramsey space (AZD_ENGINE_RAMSEY_U64 with AZD_ENGINE_RAMSEY_BIG_CLIQUES: need 3 <= n <= 64, 2..4 colours, clique "
         "sizes 2..8, E*C <= 2304)",
         "64-bit Ramsey space (AZD_ENGINE_RAMSEY_BIG_CLIQUES): need 1 <= max_slots <= E (azd_engine_config::max_slots: permitted edges per root)",
         "64-bit Ramsey space (AZD_ENGINE_RAMSEY_BIG_CLIQUES): a node holds 512 actions: need max_slots * (C - 1) <= 512 (azd_engine_config::max_slots)",
         "64-bit Ramsey space (AZD_ENGINE_RAMSEY_U64 with AZD_ENGINE_RAMSEY_BIG_CLIQUES): ActionSet paths only (path_kind = AZD_PATH_SET), no "
         "Layered wrapper (layers <= 1)"},
        {TIER_DENSE, SPACE_DENSE, &dense_ops(), xd, sizeof(DenseArgminRec), 0, false, true, false, 1, 1, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr},
        {TIER_DENSE_AH, SPACE_DENSE, &dense_ah_ops(), xd, sizeof(DenseAhArgminRec), 0, false, true, true, 2, 2, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr},
        {TIER_DENSE_AH_WIDE, SPACE_DENSE, &dense_ah_wide_ops(), xd, sizeof(DenseAhWideArgminRec), 0, false, true, true, 2, 2, 0, 0, 0, 0, 0, 0, false, nullptr, nullptr,
         nullptr, nullptr},
        // AZD_ENGINE_DENSE_INV: the weighted-invariant cost (dense_inv_kernels.hip): ten doubles and two ints per agent, the recipe behind the doubles
        {TIER_DENSE_INV, SPACE_DENSE, &dense_inv_ops(), xd, sizeof(DenseInvArgminRec), 0, false, true, false, DENSE_INV_COUNT, 2,
         (int)((sizeof(DenseInvRecipe) + 7) / 8), 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr, &dense_family(DENSE_FAMILY_INV), false},
        // AZD_ENGINE_DENSE_INV_WIDE beside it: the same record per agent over the 64-row kernels (dense_inv_wide_kernels.hip)
        {TIER_DENSE_INV_WIDE, SPACE_DENSE, &dense_inv_wide_ops(), xd, sizeof(DenseInvWideArgminRec), 0, false, true, false, DENSE_INV_COUNT, 2,
         (int)((sizeof(DenseInvRecipe) + 7) / 8), 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr, &dense_family(DENSE_FAMILY_INV), true},
        // AZD_ENGINE_DENSE_INVX: the extended invariant cost (dense_invx_kernels.hip): sixteen doubles and two ints per agent, the recipe behind the doubles
        {TIER_DENSE_INVX, SPACE_DENSE, &dense_invx_ops(), xd, sizeof(DenseInvxArgminRec), 0, false, true, false, DENSE_INVX_COUNT, 2,
         (int)((sizeof(DenseInvxRecipe) + 7) / 8), 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr, &dense_family(DENSE_FAMILY_INVX), false},
        // AZD_ENGINE_DENSE_INVX_WIDE beside it: the same record per agent over the 64-row kernels (dense_invx_wide_kernels.hip)
        {TIER_DENSE_INVX_WIDE, SPACE_DENSE, &dense_invx_wide_ops(), xd, sizeof(DenseInvxWideArgminRec), 0, false, true, false, DENSE_INVX_COUNT, 2,
         (int)((sizeof(DenseInvxRecipe) + 7) / 8), 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr, &dense_family(DENSE_FAMILY_INVX), true},
        // AZD_ENGINE_DENSE_INVS: the spectrum invariant cost (dense_invs_kernels.hip): twenty-one doubles and two ints per agent, the recipe behind the doubles
        // (no searcher-only pool step on this tier yet: ext is null, so its engines run one launch per phase at every population)
        {TIER_DENSE_INVS, SPACE_DENSE, &dense_invs_ops(), nullptr, sizeof(DenseInvsArgminRec), 0, false, true, false, DENSE_INVS_COUNT, 2,
         (int)((sizeof(DenseInvsRecipe) + 7) / 8), 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr, &dense_family(DENSE_FAMILY_INVS), false},
        // AZD_ENGINE_DENSE_INVS_WIDE beside it: the same record per agent over the 64-row kernels (dense_invs_wide_kernels.hip); no pool step either
        {TIER_DENSE_INVS_WIDE, SPACE_DENSE, &dense_invs_wide_ops(), nullptr, sizeof(DenseInvsWideArgminRec), 0, false, true, false, DENSE_INVS_COUNT, 2,
         (int)((sizeof(DenseInvsRecipe) + 7) / 8), 0, 0, 0, 0, 0, false, nullptr, nullptr, nullptr, nullptr, &dense_family(DENSE_FAMILY_INVS), true},
    };
    return &tiers[t];
}
// the tier of a configuration that check_engine_config has accepted: the flags name it, never the sizes
const TierDesc *engine_tier(const azd_engine_config *cfg) {
    if (cfg->space_id == AZD_SPACE_DENSE)
        return tier_desc(cfg->flags & AZD_ENGINE_DENSE_INVS_WIDE ? TIER_DENSE_INVS_WIDE
                         : cfg->flags & AZD_ENGINE_DENSE_INVS    ? TIER_DENSE_INVS
                         : cfg->flags & AZD_ENGINE_DENSE_INVX_WIDE ? TIER_DENSE_INVX_WIDE
                         : cfg->flags & AZD_ENGINE_DENSE_INVX    ? TIER_DENSE_INVX
                         : cfg->flags & AZD_ENGINE_DENSE_INV_WIDE ? TIER_DENSE_INV_WIDE
                         : cfg->flags & AZD_ENGINE_DENSE_INV     ? TIER_DENSE_INV
                         : cfg->flags & AZD_ENGINE_DENSE_AH_WIDE ? TIER_DENSE_AH_WIDE
                         : cfg->flags & AZD_ENGINE_DENSE_AH      ? TIER_DENSE_AH
                                                                 : TIER_DENSE);
    if (cfg->space_id != AZD_SPACE_RAMSEY) return tier_desc(TIER_C21);
    if (cfg->flags & AZD_ENGINE_RAMSEY_U64) return tier_desc(cfg->flags & AZD_ENGINE_RAMSEY_BIG_CLIQUES ? TIER_RAMSEY_U64_BIG : TIER_RAMSEY_U64);
    return tier_desc(cfg->max_slots != 0 ? TIER_RAMSEY_WIDE : TIER_RAMSEY);
}

// ------------------------------------------------------------------ simple evaluators
struct TrivialEvaluator : azd_evaluator { // TrivialModel, model/mod.rs:10-23
    int write_predictions_dev(int, const float *, float *, hipStream_t) override {
        calls += 1;
        return AZD_OK;
    }
    int update_model_dev(int, const float *, const float *, const float *, float *loss, hipStream_t) override {
        if (loss) *loss = 0.f;
        return AZD_OK;
    }
    bool fused_desc(FusedEval *f) override {
        memset(f, 0, sizeof(*f));
        f->kind = 1;
        return true;
    }
};

struct HashStreamEvaluator : azd_evaluator {
    uint64_t seed = 0, first_agent = 0;
    bool via_pool = false; // the pool step serves the rows from its evaluator workgroups (FusedEval kind 4: test harness)
    int debug_serve_from_pool(int on) override {
        via_pool = on != 0;
        return AZD_OK;
    }
    int write_predictions_dev(int batch, const float *, float *d_p, hipStream_t st) override {
        launch_hash_predictions(d_p, batch, action_dim, seed, first_agent, calls, st);
        calls += 1;
        AZD_HIP(hipGetLastError());
        return AZD_OK;
    }
    bool fused_desc(FusedEval *f) override {
        memset(f, 0, sizeof(*f));
        f->kind = via_pool ? 4 : 2;
        f->seed = seed;
        f->first_agent = first_agent;
        return true;
    }
    int update_model_dev(int, const float *, const float *, const float *, float *loss, hipStream_t) override {
        if (loss) *loss = 0.f;
        return AZD_OK;
    }
};

} // namespace azd

int azd_evaluator::ensure_staging(int batch) {
    AZD_HIP(hipSetDevice(device));
    if (!own_stream) AZD_ST(own_stream.create());
    if (batch <= staged_batch) return AZD_OK;
    staged_batch = 0;
    const size_t ns = (size_t)batch * state_dim, na = (size_t)batch * action_dim;
    AZD_ST(alloc_set(d_states, ns, d_preds, na, d_obs, na, d_w, na));
    staged_batch = batch;
    return AZD_OK;
}

namespace azd {

static int next_pow2(int v) {
    int p = 128;
    while (p < v) p <<= 1;
    return p;
}

int fetch_status(azd_engine *e) { // the device's status block -> e->h_status, behind everything queued on the stream
    AZD_HIP(hipMemcpyAsync(e->h_status, e->a.status, sizeof(StatusRec), hipMemcpyDeviceToHost, e->stream));
    AZD_HIP(hipStreamSynchronize(e->stream));
    e->time_collect();
    AZD_HIP(hipGetLastError());
    return AZD_OK;
}
int check_status(azd_engine *e) {
    if (e->h_status->failed != 0) {
        // distinguish capacity from unreachable by reading the flags
        std::vector<uint32_t> fl((size_t)e->a.B);
        AZD_HIP(hipMemcpy(fl.data(), e->a.flags, fl.size() * 4, hipMemcpyDeviceToHost));
        uint32_t all = 0;
        for (uint32_t f : fl) all |= f;
        char buf[128];
        snprintf(buf, sizeof(buf), "%llu agent(s) stopped, flag union 0x%x", e->h_status->failed, all);
        g_last_error = buf;
        return (all & (FLAG_UNREACHABLE | FLAG_LOOP_GUARD)) ? AZD_ERR_UNREACHABLE : AZD_ERR_CAPACITY;
    }
    return AZD_OK;
}
int sync_status(azd_engine *e) {
    const int st = fetch_status(e);
    return st ? st : check_status(e);
}
// how a roll-out call ends: its status, and how many calls improved the argmin since the last one that asked
int report_improved(azd_engine *e, int st, int *improved) {
    if (improved) *improved = (int)(e->h_status->improved - e->seen_improved);
    e->seen_improved = e->h_status->improved;
    return st;
}

// dense-graph space: check the roots and hand the device what it works with -- the modifiable slots ranked by ACTION ID
// (Add(e) = e for an absent edge, Delete(e) = E + e for a present one: adds first, each group ascending), as a
// rank -> action id table, and the mask of ranks still open (all k of them)
static int upload_dense_roots(azd_engine *e, const uint8_t *adj_bytes, const uint64_t *slots) {
    const Arenas &a = e->a;
    const int n = a.n, E = a.E, KWH = e->kw_host, KW = a.KW, MAXS = e->dense_slots;
    const size_t per = (size_t)17 * KW; // [rank mask: KW words][rank -> action id: 64 KW x u16]
    e->dense_packed.assign((size_t)a.B * per, 0ull);
    for (int i = 0; i < a.B; ++i) {
        uint64_t adj[64];
        memcpy(adj, adj_bytes + (size_t)i * n * 8, (size_t)n * 8);
        const uint64_t all = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        for (int v = 0; v < n; ++v) {
            if ((adj[v] & ~all) || ((adj[v] >> v) & 1ull)) {
                g_last_error = "root graph: neighbour out of range or a loop";
                return AZD_ERR_INVALID_ARGUMENT;
            }
            for (int u = 0; u < v; ++u)
                if (((adj[v] >> u) & 1ull) != ((adj[u] >> v) & 1ull)) {
                    g_last_error = "root graph: neighbourhoods are not symmetric";
                    return AZD_ERR_INVALID_ARGUMENT;
                }
        }
        if (!dense_connected(adj, n)) {
            g_last_error = "root graph must be connected";
            return AZD_ERR_INVALID_ARGUMENT;
        }
        const uint64_t *sl = slots + (size_t)i * KWH;
        uint64_t *pk = &e->dense_packed[(size_t)i * per];
        uint16_t *tab = reinterpret_cast<uint16_t *>(pk + KW);
        for (int r = 0; r < MAXS; ++r) tab[r] = 0xFFFFu;
        int k = 0;
        for (int pass = 0; pass < 2; ++pass) { // adds (absent edges), then deletes (present edges)
            int slot = 0;
            for (int v = 1; v < n; ++v)
                for (int u = 0; u < v; ++u, ++slot) {
                    if (!((sl[slot >> 6] >> (slot & 63)) & 1ull)) continue;
                    const bool present = (adj[v] >> u) & 1ull;
                    if (present != (pass == 1)) continue;
                    if (k >= MAXS) {
                        char buf[160];
                        snprintf(buf, sizeof(buf), "a root brings more than %d modifiable slots (azd_engine_config::max_slots sizes the keys)", MAXS);
                        g_last_error = buf;
                        return AZD_ERR_INVALID_ARGUMENT;
                    }
                    tab[k++] = (uint16_t)(pass == 0 ? slot : E + slot);
                }
        }
        for (int w = 0; w < KWH; ++w) {
            const int hi = E - 64 * w;
            if ((hi <= 0 && sl[w] != 0) || (hi > 0 && hi < 64 && (sl[w] >> hi) != 0)) {
                g_last_error = "slot mask has bits beyond the edge count";
                return AZD_ERR_INVALID_ARGUMENT;
            }
        }
        for (int w = 0; w < KW; ++w) {
            const int hi = k - 64 * w;
            pk[w] = hi <= 0 ? 0ull : (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull));
        }
    }
    AZD_HIP(hipMemcpyAsync(e->d_stage_parents, adj_bytes, (size_t)a.B * n * 8, hipMemcpyHostToDevice, e->stream));
    AZD_HIP(hipMemcpyAsync(e->d_stage_perm, e->dense_packed.data(), e->dense_packed.size() * 8, hipMemcpyHostToDevice, e->stream));
    AZD_HIP(hipStreamSynchronize(e->stream)); // the packed block is pageable host memory
    return AZD_OK;
}

static int upload_roots(azd_engine *e, const uint8_t *parents, const uint64_t *permitted) {
    const Arenas &a = e->a;
    if (a.space == SPACE_DENSE) return upload_dense_roots(e, parents, permitted);
    if (a.space == SPACE_RAMSEY) {
        // packed roots: colour of every edge in colex order (E bytes) + permitted edge positions (kw_host words; a wide engine's
        // device masks are a.KW words, zero-padded)
        const int KWH = e->kw_host;
        if (KWH != a.KW) {
            e->ramsey_perm_pad.assign((size_t)a.B * a.KW, 0ull);
            for (int i = 0; i < a.B; ++i) memcpy(&e->ramsey_perm_pad[(size_t)i * a.KW], permitted + (size_t)i * KWH, (size_t)KWH * 8);
        }
        for (int i = 0; i < a.B; ++i) {
            const uint8_t *col = parents + (size_t)i * a.E;
            for (int x = 0; x < a.E; ++x)
                if (col[x] >= a.C) {
                    g_last_error = "root edge colour out of range";
                    return AZD_ERR_INVALID_ARGUMENT;
                }
            int cnt = 0;
            for (int w = 0; w < KWH; ++w) {
                uint64_t m = permitted[(size_t)i * KWH + w];
                int hi = a.E - 64 * w;
                if ((hi <= 0 && m != 0) || (hi > 0 && hi < 64 && (m >> hi) != 0)) {
                    g_last_error = "permitted mask has bits beyond the edge count";
                    return AZD_ERR_INVALID_ARGUMENT;
                }
                cnt += __builtin_popcountll(m);
            }
            if (e->tier->cap_from_slots ? cnt > e->ramsey_slots : cnt * (a.C - 1) > MAX_NODE_ACTIONS) {
                g_last_error = e->tier->cap_from_slots ? "more permitted edges than azd_engine_config::max_slots" : "more permitted actions than a node can hold";
                return AZD_ERR_INVALID_ARGUMENT;
            }
        }
        AZD_HIP(hipMemcpyAsync(e->d_stage_parents, parents, (size_t)a.B * a.E, hipMemcpyHostToDevice, e->stream));
        AZD_HIP(hipMemcpyAsync(e->d_stage_perm, KWH != a.KW ? e->ramsey_perm_pad.data() : permitted, (size_t)a.B * a.KW * 8, hipMemcpyHostToDevice, e->stream));
        if (KWH != a.KW) AZD_HIP(hipStreamSynchronize(e->stream)); // the padded block is pageable host memory
        return AZD_OK;
    }
    // validate on the host what the kernels assume (parents[v] < v; at most MAX_NODE_ACTIONS permitted)
    for (int i = 0; i < a.B; ++i) {
        const uint8_t *p = parents + (size_t)i * a.n;
        // rooted_tree/mod.rs:14-20: parents[0] = parents[1] = parents[N-1] = 0, and no action ever
        // re-parents vertex N-1 (action children are 2..N-2), so N-1 and N-2 stay leaves -- the
        // lambda_1 kernel gives them no accumulator slot
        if (p[0] != 0 || p[a.n - 1] != 0) {
            g_last_error = "root parents[0] and parents[N-1] must be 0";
            return AZD_ERR_INVALID_ARGUMENT;
        }
        for (int v = 1; v < a.n; ++v)
            if (p[v] >= v) {
                g_last_error = "root parents[v] must be < v";
                return AZD_ERR_INVALID_ARGUMENT;
            }
        int cnt = 0;
        for (int w = 0; w < a.KW; ++w) {
            uint64_t m = permitted[(size_t)i * a.KW + w];
            int hi = a.A - 64 * w;
            if (hi < 64 && hi > 0 && (m >> hi) != 0) {
                g_last_error = "permitted mask has bits beyond ACTION_DIM";
                return AZD_ERR_INVALID_ARGUMENT;
            }
            cnt += __builtin_popcountll(m);
        }
        if (cnt > MAX_NODE_ACTIONS) {
            g_last_error = "more permitted actions than a node can hold";
            return AZD_ERR_INVALID_ARGUMENT;
        }
    }
    AZD_HIP(hipMemcpyAsync(e->d_stage_parents, parents, (size_t)a.B * a.n, hipMemcpyHostToDevice, e->stream));
    AZD_HIP(hipMemcpyAsync(e->d_stage_perm, permitted, (size_t)a.B * a.KW * 8, hipMemcpyHostToDevice, e->stream));
    return AZD_OK;
}

int run_evaluator(azd_engine *e) {
    e->time_begin(1);
    int st = e->ev->write_predictions_dev16(e->a.B, e->a.state_vecs, e->a.state_vecs16, e->a.S16, e->a.h_theta, e->stream);
    e->time_end();
    return st;
}

// The argument checks of azd_engine_create, before the device is touched (azd_debug_ext_pool_plan runs them too)
static int refuse(const char *why) {
    g_last_error = why;
    return AZD_ERR_INVALID_ARGUMENT;
}
// ... of a Ramsey configuration, against its tier's limits
static int check_ramsey_config(const azd_engine_config *cfg, const TierDesc &t) {
    bool ok = cfg->batch > 0 && cfg->n >= 3 && cfg->n <= t.max_n && cfg->n_colors >= 2 && cfg->n_colors <= 4;
    if (ok) {
        for (int c = 0; c < cfg->n_colors; ++c) ok = ok && cfg->clique_sizes[c] >= 2 && cfg->clique_sizes[c] <= t.max_clique;
    }
    if (ok && t.clique_overflow_rule) {
        // RamseyCounts::new (ramsey_counts/mod.rs:47-62) adds the per-edge counts of a colour's adjacent pairs into an i32 BEFORE it
        // divides by C(s,2): a root monochromatic in colour c brings C(s,2) * C(n,s)
        for (int c = 0; c < cfg->n_colors; ++c) {
            const int64_t s = cfg->clique_sizes[c];
            int64_t binom = 1; // C(n, s), exact at every step (C(n, k) * (n - k) is divisible by k + 1); <= C(64, 8) = 4.4e9
            for (int64_t k = 0; k < s; ++k) binom = binom * (cfg->n - k) / (k + 1);
            if (s * (s - 1) / 2 * binom > (int64_t)INT32_MAX) {
                char why[256];
                snprintf(why, sizeof(why),
                         "AZD_ENGINE_RAMSEY_BIG_CLIQUES: colour %d (clique size %d at n = %d) is beyond the reference's i32 bound: need "
                         "C(s,2) * C(n,s) <= 2^31 - 1 for every colour (size 7: n <= 50, size 8: n <= 39)",
                         c, (int)s, cfg->n);
                return refuse(why);
            }
        }
    }
    if (ok) ok = ramsey_edges(cfg->n) <= t.max_edges && ramsey_action_dim(cfg->n, cfg->n_colors) <= t.max_actions;
    if (!ok) return refuse(t.e_range);
    if (!t.cap_from_slots) return AZD_OK;
    if (cfg->max_slots < 1 || cfg->max_slots > ramsey_edges(cfg->n)) return refuse(t.e_slots);
    if (t.node_actions && (long)cfg->max_slots * (cfg->n_colors - 1) > t.node_actions) return refuse(t.e_node_actions);
    if (cfg->layers > 1 || cfg->path_kind != AZD_PATH_SET) return refuse(t.e_paths);
    return AZD_OK;
}
// ... of a dense-graph configuration's cost flags: each cost is asked for by name, never chosen from the sizes, and a _WIDE flag is
// a second flag beside its cost's, never a cost of its own.  One row per flag, in the order of precedence; the first flag set is checked.
struct DenseCostFlag {
    uint32_t flag, base, excludes; // base: the flag a _WIDE flag must stand beside (0: a cost's own flag); excludes: flags of other costs
    const char *name;
    int max_n;
    bool cap_640, needs_slot; // max_slots <= min(E, 640), not E; max_slots >= 1
    const char *e_base, *e_excludes, *e_n;
};
static int check_dense_cost_flags(const azd_engine_config *cfg) {
    constexpr uint32_t AH = AZD_ENGINE_DENSE_AH | AZD_ENGINE_DENSE_AH_WIDE, INV = AZD_ENGINE_DENSE_INV | AZD_ENGINE_DENSE_INV_WIDE,
                       INVX = AZD_ENGINE_DENSE_INVX | AZD_ENGINE_DENSE_INVX_WIDE;
    static const DenseCostFlag rows[] = {
        {AZD_ENGINE_DENSE_INVS_WIDE, AZD_ENGINE_DENSE_INVS, AH | INV | INVX, "AZD_ENGINE_DENSE_INVS_WIDE", AZD_DENSE_INVS_WIDE_MAX_N, true, true,
         "flags: AZD_ENGINE_DENSE_INVS_WIDE is valid only beside AZD_ENGINE_DENSE_INVS (the spectrum invariant cost whose 64-row form it asks for)",
         "flags: AZD_ENGINE_DENSE_INVS_WIDE belongs to a cost of its own: it cannot be combined with AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE, "
         "AZD_ENGINE_DENSE_INV, AZD_ENGINE_DENSE_INV_WIDE, AZD_ENGINE_DENSE_INVX or AZD_ENGINE_DENSE_INVX_WIDE (the Aouchiche-Hansen cost, the "
         "weighted-invariant cost and the extended invariant cost are among its recipes)",
         "n: the wide spectrum invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVS_WIDE_MAX_N)"},
        {AZD_ENGINE_DENSE_INVS, 0, AH | INV | INVX, "AZD_ENGINE_DENSE_INVS", AZD_DENSE_INVS_MAX_N, false, false, nullptr,
         "flags: AZD_ENGINE_DENSE_INVS is a cost of its own: it cannot be combined with AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE, "
         "AZD_ENGINE_DENSE_INV, AZD_ENGINE_DENSE_INV_WIDE, AZD_ENGINE_DENSE_INVX or AZD_ENGINE_DENSE_INVX_WIDE (the Aouchiche-Hansen cost, the "
         "weighted-invariant cost and the extended invariant cost are among its recipes)",
         "n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)"},
        {AZD_ENGINE_DENSE_INVX_WIDE, AZD_ENGINE_DENSE_INVX, AH | INV, "AZD_ENGINE_DENSE_INVX_WIDE", AZD_DENSE_INVX_WIDE_MAX_N, true, true,
         "flags: AZD_ENGINE_DENSE_INVX_WIDE is valid only beside AZD_ENGINE_DENSE_INVX (the extended invariant cost whose 64-row form it asks for)",
         "flags: AZD_ENGINE_DENSE_INVX_WIDE belongs to a cost of its own: it cannot be combined with AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE, "
         "AZD_ENGINE_DENSE_INV or AZD_ENGINE_DENSE_INV_WIDE (the Aouchiche-Hansen cost and the weighted-invariant cost are among its recipes)",
         "n: the wide extended invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVX_WIDE_MAX_N)"},
        {AZD_ENGINE_DENSE_INVX, 0, AH | INV, "AZD_ENGINE_DENSE_INVX", AZD_DENSE_INVX_MAX_N, false, false, nullptr,
         "flags: AZD_ENGINE_DENSE_INVX is a cost of its own: it cannot be combined with AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE, "
         "AZD_ENGINE_DENSE_INV or AZD_ENGINE_DENSE_INV_WIDE (the Aouchiche-Hansen cost and the weighted-invariant cost are among its recipes)",
         "n: the extended invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVX_MAX_N)"},
        {AZD_ENGINE_DENSE_INV_WIDE, AZD_ENGINE_DENSE_INV, AH, "AZD_ENGINE_DENSE_INV_WIDE", AZD_DENSE_INV_WIDE_MAX_N, true, true,
         "flags: AZD_ENGINE_DENSE_INV_WIDE is valid only beside AZD_ENGINE_DENSE_INV (the weighted-invariant cost whose 64-row form it asks for)",
         "flags: AZD_ENGINE_DENSE_INV_WIDE belongs to a cost of its own: it cannot be combined with AZD_ENGINE_DENSE_AH or AZD_ENGINE_DENSE_AH_WIDE "
         "(the Aouchiche-Hansen cost is one of its recipes)",
         "n: the wide weighted-invariant cost needs 4 <= n <= 64 (AZD_DENSE_INV_WIDE_MAX_N)"},
        {AZD_ENGINE_DENSE_INV, 0, AH, "AZD_ENGINE_DENSE_INV", AZD_DENSE_INV_MAX_N, false, false, nullptr,
         "flags: AZD_ENGINE_DENSE_INV is a cost of its own: it cannot be combined with AZD_ENGINE_DENSE_AH or AZD_ENGINE_DENSE_AH_WIDE "
         "(the Aouchiche-Hansen cost is one of its recipes)",
         "n: the weighted-invariant cost needs 4 <= n <= 32 (AZD_DENSE_INV_MAX_N)"},
        // (the one 64-row tier whose max_slots has no lower bound)
        {AZD_ENGINE_DENSE_AH_WIDE, AZD_ENGINE_DENSE_AH, 0, "AZD_ENGINE_DENSE_AH_WIDE", AZD_DENSE_AH_WIDE_MAX_N, true, false,
         "flags: AZD_ENGINE_DENSE_AH_WIDE is valid only beside AZD_ENGINE_DENSE_AH (the Aouchiche-Hansen cost whose 64-row form it asks for)", nullptr,
         "n: the wide Aouchiche-Hansen cost needs 4 <= n <= 64 (AZD_DENSE_AH_WIDE_MAX_N)"},
        {AZD_ENGINE_DENSE_AH, 0, 0, "AZD_ENGINE_DENSE_AH", AZD_DENSE_AH_MAX_N, false, false, nullptr, nullptr,
         "n: the Aouchiche-Hansen cost needs 4 <= n <= 32 (AZD_DENSE_AH_MAX_N)"},
    };
    for (const DenseCostFlag &r : rows) {
        if (!(cfg->flags & r.flag)) continue;
        const std::string name = r.name;
        if (r.base && !(cfg->flags & r.base)) return refuse(r.e_base);
        if (cfg->flags & r.excludes) return refuse(r.e_excludes);
        if (cfg->space_id != AZD_SPACE_DENSE) return refuse(("space_id: " + name + " needs the dense-graph space (AZD_SPACE_DENSE)").c_str());
        if (cfg->n < 4 || cfg->n > r.max_n) return refuse(r.e_n);
        if (cfg->layers > 1) return refuse(("layers: " + name + " engines take no Layered wrapper (layers <= 1)").c_str());
        const bool bad_path = cfg->path_kind != AZD_PATH_SET;
        const bool bad_slots = (r.needs_slot && cfg->max_slots < 1) || cfg->max_slots > (r.cap_640 ? std::min(dense_edges(cfg->n), 640) : dense_edges(cfg->n));
        // (a cost's own flag says max_slots before path_kind, a _WIDE flag path_kind before max_slots)
        if (bad_path && (r.base || !bad_slots)) return refuse(("path_kind: " + name + " engines keep ActionSet paths (AZD_PATH_SET)").c_str());
        if (bad_slots)
            return refuse(("max_slots: " + name + " needs " + (r.needs_slot ? "1 <= " : "") + "max_slots <= " +
                           (r.cap_640 ? "min(E, 640), E = n (n - 1) / 2 (key widths 2, 4 and 10)" : "E = n (n - 1) / 2"))
                              .c_str());
        return AZD_OK;
    }
    return AZD_OK;
}
int check_engine_config(const azd_engine_config *cfg) {
    const bool ramsey = cfg->space_id == AZD_SPACE_RAMSEY;
    const bool dense = cfg->space_id == AZD_SPACE_DENSE;
    // clique sizes up to 8: a second flag beside the 64-bit tier's, never a tier chosen from the sizes
    if ((cfg->flags & AZD_ENGINE_RAMSEY_BIG_CLIQUES) && (!ramsey || !(cfg->flags & AZD_ENGINE_RAMSEY_U64)))
        return refuse("flags: AZD_ENGINE_RAMSEY_BIG_CLIQUES is valid only beside AZD_ENGINE_RAMSEY_U64 (the 64-bit tier of the Ramsey space, "
                      "AZD_SPACE_RAMSEY with max_slots > 0, whose kernels for clique sizes up to 8 it asks for)");
    AZD_ST(check_dense_cost_flags(cfg));
    if (dense) {
        if (cfg->n < 4 || cfg->n > AZD_DENSE_MAX_N || cfg->batch <= 0 || cfg->layers > 1 || cfg->max_slots < 0 || cfg->max_slots > AZD_DENSE_MAX_SLOTS ||
            !(cfg->dense_p >= 0.f && cfg->dense_p <= 1.f))
            return refuse("unsupported dense-graph space (need 4 <= n <= 64, no Layered wrapper, max_slots <= 1024, 0 <= dense_p <= 1)");
    } else if (cfg->flags & AZD_ENGINE_RAMSEY_U64) { // the 64-bit tier: asked for by name, never chosen from the sizes
        if (!ramsey || cfg->max_slots == 0) return refuse("AZD_ENGINE_RAMSEY_U64 needs a Ramsey space (AZD_SPACE_RAMSEY) with max_slots > 0");
        AZD_ST(check_ramsey_config(cfg, *engine_tier(cfg))); // (... and its big-clique kernels by a second flag beside the first)
    } else if (ramsey) { // (max_slots != 0: wide)
        AZD_ST(check_ramsey_config(cfg, *tier_desc(cfg->max_slots != 0 ? TIER_RAMSEY_WIDE : TIER_RAMSEY)));
    } else if (cfg->space_id != AZD_SPACE_C21 || cfg->n < 4 || cfg->n > AZD_C21_MAX_N || cfg->batch <= 0) {
        return refuse("unsupported space / n / batch");
    }
    if (cfg->layers < 0 || cfg->layers > 8) return refuse("layers must be 0/1 (plain space) or 2..8");
    if (cfg->path_kind != AZD_PATH_SET && cfg->path_kind != AZD_PATH_SEQUENCE) return refuse("unknown path encoding");
    // the searcher-only pool step of the Ramsey tiers with max_slots > 0: asked for by name, never chosen from the sizes
    if (cfg->flags & AZD_ENGINE_EXT_POOL_STEP) {
        const char *bad = !ramsey || cfg->max_slots <= 0 ? "AZD_ENGINE_EXT_POOL_STEP needs a Ramsey space (AZD_SPACE_RAMSEY) with max_slots > 0 (the wide or the 64-bit tier)"
                          : (cfg->flags & AZD_ENGINE_NO_PERSISTENT_STEP)
                              ? "AZD_ENGINE_EXT_POOL_STEP is a CU-resident step form: it cannot be combined with AZD_ENGINE_NO_PERSISTENT_STEP"
                              : nullptr;
        if (bad) return refuse(bad);
    }
    // ... and its fp32 evaluator: a second flag beside the first, never a form of its own.  The dense-graph space's searcher-only
    // form needs no flag (it is the space's pool step, on all three tiers), so there the flag stands alone: a request to the
    // configured pool step, refused beside the flag that rules every CU-resident form out
    if ((cfg->flags & AZD_ENGINE_EXT_POOL_F32) && dense) {
        if (cfg->flags & AZD_ENGINE_NO_PERSISTENT_STEP)
            return refuse("AZD_ENGINE_EXT_POOL_F32 asks the dense-graph space's pool step, a CU-resident step form, for its fp32 evaluator: it cannot be "
                          "combined with AZD_ENGINE_NO_PERSISTENT_STEP");
    } else if ((cfg->flags & AZD_ENGINE_EXT_POOL_F32) && !(cfg->flags & AZD_ENGINE_EXT_POOL_STEP))
        return refuse("AZD_ENGINE_EXT_POOL_F32 is valid only beside AZD_ENGINE_EXT_POOL_STEP (the searcher-only pool step whose fp32 evaluator it asks for), "
                      "or alone on the dense-graph space (AZD_SPACE_DENSE), whose pool step is that form");
    return AZD_OK;
}
// dense-graph space, device keys: ranks of the root's modifiable slots, in 2 / 4 / 10 / 16 words (the widths dense_kernels.hip is built for)
static int dense_device_key_words(int max_slots) {
    const int ms = max_slots > 0 ? max_slots : 128;
    return ms <= 128 ? 2 : ms <= 256 ? 4 : ms <= 640 ? 10 : 16;
}
// The shape part of an engine's arenas -- what the LDS plans and the allocations read -- for a configuration that check_engine_config
// has accepted.  Everything else in *a is zeroed.
void engine_shape(const azd_engine_config *cfg, const TierDesc *t, Arenas *ap) {
    Arenas &a = *ap;
    memset(&a, 0, sizeof(a));
    a.n = cfg->n;
    a.B = cfg->batch;
    a.space = t->space;
    a.path_kind = cfg->path_kind;
    a.layers = cfg->layers > 1 ? cfg->layers : 1;
    if (t->space == SPACE_DENSE) {
        a.E = dense_edges(cfg->n);
        a.A = dense_action_dim(cfg->n);
        a.S = dense_state_dim(cfg->n);
        a.KW = dense_device_key_words(cfg->max_slots); // (an AH engine: key widths 2, 4 and 10 only: max_slots <= E <= 496)
        a.dense_p24 = (uint32_t)((cfg->dense_p > 0.f ? (double)cfg->dense_p : 0.2) * 16777216.0 + 0.5);
        a.eval_slope = t->ah ? dense_ah_eval_slope(cfg->n) : c21_eval_slope(cfg->n); // (the weighted-invariant cost reads its recipe's scale, not this)
    } else if (t->space == SPACE_RAMSEY) {
        a.C = cfg->n_colors;
        a.E = ramsey_edges(cfg->n);
        a.A = ramsey_action_dim(cfg->n, a.C);
        a.S = ramsey_state_dim(cfg->n, a.C);
        a.KW = ramsey_key_words(cfg->n, a.C);
        if (t->padded_keys) a.KW = t->id == TIER_RAMSEY_U64 || t->id == TIER_RAMSEY_U64_BIG ? RAMSEY_U64_KW : a.A <= 640 ? 10 : 16; // RamseyWideSpace<10 / 16>; one width for the 64-bit tier
        for (int c = 0; c < a.C; ++c) {
            a.sizes[c] = cfg->clique_sizes[c];
            a.cweights[c] = cfg->color_weights[c];
        }
    } else {
        a.A = c21_action_dim(cfg->n);
        a.S = c21_state_dim(cfg->n);
        a.KW = c21_key_words(cfg->n);
        a.eval_slope = c21_eval_slope(cfg->n);
        c21_lambda_bracket(cfg->n, &a.lam_lo, &a.lam_hi);
    }
    a.S_inner = a.S;
    a.S = a.S_inner * a.layers; // Layered<L, Space>::STATE_DIM (nabla/space/mod.rs:53)
    a.node_cap = cfg->node_capacity > 0 ? (uint32_t)cfg->node_capacity : 4096u;
    a.arc_cap = cfg->arc_capacity > 0 ? (uint32_t)cfg->arc_capacity : 8192u;
    a.pred_cap = cfg->prediction_capacity > 0 ? (uint32_t)cfg->prediction_capacity : 32768u;
    a.ht_cap = (uint32_t)next_pow2((int)(2 * a.node_cap));
}

} // namespace azd

extern "C" {

const char *azd_status_string(int s) {
    switch (s) {
    case AZD_OK: return "ok";
    case AZD_ERR_INVALID_ARGUMENT: return "invalid argument";
    case AZD_ERR_NO_DEVICE: return "no gfx950 device (no CPU fallback)";
    case AZD_ERR_HIP: return "HIP runtime error";
    case AZD_ERR_CAPACITY: return "tree arena capacity exceeded";
    case AZD_ERR_UNREACHABLE: return "unreachable selection state";
    case AZD_ERR_NO_EVALUATOR: return "engine has no evaluator";
    case AZD_ERR_OUT_OF_MEMORY: return "out of device memory";
    case AZD_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
    }
}
const char *azd_last_error(void) { return azd::g_last_error.c_str(); }
int azd_version(void) { return 100; }
int azd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int azd_ramsey_state_dim(int n, int n_colors) { return azd::ramsey_state_dim(n, n_colors); }
int azd_ramsey_action_dim(int n, int n_colors) { return azd::ramsey_action_dim(n, n_colors); }
int azd_ramsey_key_words(int n, int n_colors) { return azd::ramsey_key_words(n, n_colors); }
int azd_ramsey_generate_roots_weighted(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int n_colors, int kmin,
                                       int kmax, const double *color_weights, uint8_t *colors, uint64_t *permitted) {
    if (!colors || !permitted || count < 0 || n < 3 || n > AZD_RAMSEY_U64_MAX_N || n_colors < 2 || n_colors > 4) return AZD_ERR_INVALID_ARGUMENT;
    if (kmin < 0 || kmax < kmin || kmax > azd::ramsey_edges(n)) return AZD_ERR_INVALID_ARGUMENT;
    uint64_t thr[azd::RAMSEY_COLOR_THRESHOLDS];
    if (color_weights) {
        if (const char *why = azd::ramsey_check_color_weights(color_weights, n_colors)) {
            azd::g_last_error = why;
            return AZD_ERR_INVALID_ARGUMENT;
        }
        azd::ramsey_color_thresholds(color_weights, n_colors, thr);
    }
    azd::ramsey_generate_roots_weighted(seed, epoch, first_agent, count, n, n_colors, kmin, kmax, color_weights ? thr : nullptr, colors,
                                        permitted);
    return AZD_OK;
}
int azd_ramsey_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int n_colors, int kmin,
                              int kmax, uint8_t *colors, uint64_t *permitted) {
    return azd_ramsey_generate_roots_weighted(seed, epoch, first_agent, count, n, n_colors, kmin, kmax, nullptr, colors, permitted);
}
int azd_dense_state_dim(int n) { return azd::dense_state_dim(n); }
int azd_dense_action_dim(int n) { return azd::dense_action_dim(n); }
int azd_dense_key_words(int n) { return azd::dense_key_words(n); }
int azd_dense_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin, int kmax, double p,
                             uint64_t *adj, uint64_t *slots) {
    if (!adj || !slots || count < 0 || n < 4 || n > AZD_DENSE_MAX_N || !(p > 0.0 && p <= 1.0)) return AZD_ERR_INVALID_ARGUMENT;
    if (kmin < 1 || kmax < kmin || kmax > AZD_DENSE_MAX_SLOTS || kmax > azd::dense_edges(n)) return AZD_ERR_INVALID_ARGUMENT;
    azd::dense_generate_roots(seed, epoch, first_agent, count, n, kmin, kmax, (uint32_t)(p * 16777216.0 + 0.5), adj, slots);
    return AZD_OK;
}
int azd_c21_state_dim(int n) { return azd::c21_state_dim(n); }
int azd_c21_action_dim(int n) { return azd::c21_action_dim(n); }
int azd_c21_key_words(int n) { return azd::c21_key_words(n); }
int azd_c21_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin,
                           int kmax, uint8_t *parents, uint64_t *permitted) {
    if (n < 4 || n > AZD_C21_MAX_N || count < 0 || !parents || !permitted) return AZD_ERR_INVALID_ARGUMENT;
    int A = azd::c21_action_dim(n);
    if (kmin < 0 || kmax < kmin || kmax > A || kmax > azd::MAX_NODE_ACTIONS) return AZD_ERR_INVALID_ARGUMENT;
    azd::c21_generate_roots(seed, epoch, first_agent, count, n, kmin, kmax, parents, permitted);
    return AZD_OK;
}

// ------------------------------------------------------------------ evaluator ABI
int azd_evaluator_create_mlp(azd_evaluator **out, int device, int max_batch, int state_dim, int action_dim,
                             const int *hidden, int n_hidden, int final_act, const azd_adam_config *adam,
                             uint64_t seed) {
    if (!out || max_batch <= 0 || state_dim <= 0 || action_dim <= 0 || n_hidden < 0 || (n_hidden && !hidden) || !adam)
        return AZD_ERR_INVALID_ARGUMENT;
    int st = azd::device_ok(device);
    if (st) return st;
    azd_evaluator *ev = azd::make_mlp_evaluator(device, max_batch, state_dim, action_dim, hidden, n_hidden, final_act, adam, seed, &st);
    if (!ev) return st;
    *out = ev;
    return AZD_OK;
}
int azd_evaluator_create_trivial(azd_evaluator **out, int device, int state_dim, int action_dim) {
    if (!out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd::device_ok(device));
    auto *ev = new (std::nothrow) azd::TrivialEvaluator();
    if (!ev) return AZD_ERR_OUT_OF_MEMORY;
    ev->device = device;
    ev->state_dim = state_dim;
    ev->action_dim = action_dim;
    *out = ev;
    return AZD_OK;
}
int azd_evaluator_create_hash_stream(azd_evaluator **out, int device, int state_dim, int action_dim, uint64_t seed,
                                     uint64_t first_agent) {
    if (!out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd::device_ok(device));
    auto *ev = new (std::nothrow) azd::HashStreamEvaluator();
    if (!ev) return AZD_ERR_OUT_OF_MEMORY;
    ev->device = device;
    ev->state_dim = state_dim;
    ev->action_dim = action_dim;
    ev->seed = seed;
    ev->first_agent = first_agent;
    *out = ev;
    return AZD_OK;
}
int azd_evaluator_destroy(azd_evaluator *ev) {
    delete ev;
    return AZD_OK;
}
int azd_evaluator_write_predictions(azd_evaluator *ev, int batch, const float *states, float *predictions) {
    if (!ev || batch <= 0 || !states || !predictions) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(ev->ensure_staging(batch));
    size_t sb = (size_t)batch * ev->state_dim * 4, pb = (size_t)batch * ev->action_dim * 4;
    AZD_HIP(hipMemcpyAsync(ev->d_states, states, sb, hipMemcpyHostToDevice, ev->own_stream));
    // TrivialModel must leave the caller's buffer untouched: seed the staging copy with it
    AZD_HIP(hipMemcpyAsync(ev->d_preds, predictions, pb, hipMemcpyHostToDevice, ev->own_stream));
    AZD_ST(ev->write_predictions_dev(batch, ev->d_states, ev->d_preds, ev->own_stream));
    AZD_HIP(hipMemcpyAsync(predictions, ev->d_preds, pb, hipMemcpyDeviceToHost, ev->own_stream));
    AZD_HIP(hipStreamSynchronize(ev->own_stream));
    return AZD_OK;
}
int azd_evaluator_update_model(azd_evaluator *ev, int batch, const float *states, const float *observations,
                               const float *action_weights, float *loss) {
    if (!ev || batch <= 0 || !states || !observations || !action_weights) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(ev->ensure_staging(batch));
    size_t sb = (size_t)batch * ev->state_dim * 4, pb = (size_t)batch * ev->action_dim * 4;
    AZD_HIP(hipMemcpyAsync(ev->d_states, states, sb, hipMemcpyHostToDevice, ev->own_stream));
    AZD_HIP(hipMemcpyAsync(ev->d_obs, observations, pb, hipMemcpyHostToDevice, ev->own_stream));
    AZD_HIP(hipMemcpyAsync(ev->d_w, action_weights, pb, hipMemcpyHostToDevice, ev->own_stream));
    return ev->update_model_dev(batch, ev->d_states, ev->d_obs, ev->d_w, loss, ev->own_stream);
}
int azd_evaluator_write_predictions_dev(azd_evaluator *ev, int batch, const float *d_states, float *d_predictions,
                                        void *stream) {
    if (!ev || batch <= 0) return AZD_ERR_INVALID_ARGUMENT;
    AZD_HIP(hipSetDevice(ev->device));
    return ev->write_predictions_dev(batch, d_states, d_predictions, (hipStream_t)stream);
}
int azd_evaluator_update_model_dev(azd_evaluator *ev, int batch, const float *d_states, const float *d_observations,
                                   const float *d_action_weights, float *loss, void *stream) {
    if (!ev || batch <= 0) return AZD_ERR_INVALID_ARGUMENT;
    AZD_HIP(hipSetDevice(ev->device));
    return ev->update_model_dev(batch, d_states, d_observations, d_action_weights, loss, (hipStream_t)stream);
}
int azd_evaluator_set_weight_storage(azd_evaluator *ev, int dtype) { return ev ? ev->set_weight_storage(dtype) : AZD_ERR_INVALID_ARGUMENT; }
int64_t azd_evaluator_num_params(azd_evaluator *ev) { return ev ? ev->num_params() : 0; }
int azd_evaluator_get_params(azd_evaluator *ev, float *out) { return ev && out ? ev->get_params(out) : AZD_ERR_INVALID_ARGUMENT; }
int azd_evaluator_set_params(azd_evaluator *ev, const float *in) { return ev && in ? ev->set_params(in) : AZD_ERR_INVALID_ARGUMENT; }
uint64_t azd_evaluator_calls(azd_evaluator *ev) { return ev ? ev->calls : 0; }

// ------------------------------------------------------------------ engine ABI
int azd_engine_create(azd_engine **out, const azd_engine_config *cfg, azd_evaluator *ev) {
    if (!out || !cfg) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(check_engine_config(cfg));
    const TierDesc *const tier = engine_tier(cfg);
    const bool ramsey = tier->space == azd::SPACE_RAMSEY, dense = tier->space == azd::SPACE_DENSE;
    AZD_ST(azd::device_ok(cfg->device));
    AZD_HIP(hipSetDevice(cfg->device));
    std::unique_ptr<azd_engine> e(new (std::nothrow) azd_engine()); // whatever it holds by then goes with it on every early return
    if (!e) return AZD_ERR_OUT_OF_MEMORY;
    e->cfg = *cfg;
    e->ev = ev;
    e->tier = tier;
    e->ops = tier->ops;
    azd::Arenas &a = e->a;
    engine_shape(cfg, tier, &a);
    if (dense) {
        e->dense_slots = 64 * a.KW;
        e->kw_host = azd::dense_key_words(cfg->n);
    } else if (ramsey) {
        e->kw_host = azd::ramsey_key_words(cfg->n, a.C);
        e->ramsey_slots = tier->cap_from_slots ? cfg->max_slots : azd::MAX_NODE_ACTIONS / (a.C - 1);
    }
    // (the flag decides whether a Ramsey tier has its searcher-only pool step; the dense-graph space always has)
    if (dense || (cfg->flags & AZD_ENGINE_EXT_POOL_STEP)) e->ext = tier->ext;
    e->ext_f32 = (cfg->flags & AZD_ENGINE_EXT_POOL_F32) != 0;
    if (ev && (ev->state_dim != a.S || ev->action_dim != a.A)) {
        azd::g_last_error = "evaluator dimensions do not match the space";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    // what the packed records hold (engine_types.h: PredRec / node_pack): child node 16 bits, arc id 16 (0xFFFF = none), a child's first
    // prediction 20, action id 12, actions per node 11, n_t 20 (one per arc at most), exhausted 12 (one per action at most).  The
    // reference's u32 indices (petgraph NodeIndex / EdgeIndex, tree/mod.rs:28-32) have no such limits: a configuration beyond them is
    // refused here, naming the argument, instead of corrupting a neighbouring bit field later.
    static_assert(AZD_RAMSEY_U64_NODE_ACTIONS == 64 * azd::RAMSEY_U64_CH, "node capacity of the 64-bit Ramsey tier");
    static_assert(AZD_DENSE_MAX_SLOTS <= 2047 && azd::MAX_NODE_ACTIONS <= 2047, "actions per node must fit PredRec's 11-bit count");
    static_assert(AZD_MAX_NODE_CAPACITY == 65536 && AZD_MAX_ARC_CAPACITY == 65535 && AZD_MAX_PREDICTION_CAPACITY == (1 << 20), "limits of the packed records");
    {
        const char *bad = nullptr;
        static thread_local char msg[256];
        const long per_node = dense ? (long)e->dense_slots : ramsey ? (long)std::min(a.E, e->ramsey_slots) * (a.C - 1) : (long)a.A;
        if (a.node_cap > (uint32_t)AZD_MAX_NODE_CAPACITY) snprintf(msg, sizeof msg, "node_capacity %u is beyond the record format (<= %d)", a.node_cap, AZD_MAX_NODE_CAPACITY), bad = msg;
        else if (a.arc_cap > (uint32_t)AZD_MAX_ARC_CAPACITY) snprintf(msg, sizeof msg, "arc_capacity %u is beyond the record format (<= %d)", a.arc_cap, AZD_MAX_ARC_CAPACITY), bad = msg;
        else if (a.pred_cap > (uint32_t)AZD_MAX_PREDICTION_CAPACITY) snprintf(msg, sizeof msg, "prediction_capacity %u is beyond the record format (<= %d)", a.pred_cap, AZD_MAX_PREDICTION_CAPACITY), bad = msg;
        else if (a.A > 4096) snprintf(msg, sizeof msg, "ACTION_DIM %d is beyond the record format (<= 4096)", a.A), bad = msg;
        // (an upper bound of what a node can hold: c21 / Ramsey nodes are further limited to MAX_NODE_ACTIONS at run time, FLAG_NODE_ACTIONS)
        else if (per_node > 2047) snprintf(msg, sizeof msg, "%ld legal actions per node are beyond the record format (<= 2047)", per_node), bad = msg;
        if (bad) {
            azd::g_last_error = bad;
            return AZD_ERR_INVALID_ARGUMENT;
        }
    }
    const size_t B = (size_t)a.B;
    AZD_ST(e->stream.create());
    AZD_ST(e->alloc(&a.nodes, B * a.node_cap));
    AZD_ST(e->alloc(&a.keys, B * a.node_cap * a.KW));
    AZD_ST(e->alloc(&a.arcs, B * a.arc_cap));
    AZD_ST(e->alloc(&a.preds, B * a.pred_cap));
    AZD_ST(e->alloc(&a.pred_g, B * a.pred_cap));
    AZD_ST(e->alloc(&a.ht, B * a.ht_cap));
    AZD_ST(e->alloc(&a.root_parents, B * azd::PARENTS_STRIDE));
    AZD_ST(e->alloc(&a.cur_parents, B * azd::PARENTS_STRIDE));
    AZD_ST(e->alloc(&a.root_perm, B * a.KW));
    AZD_ST(e->alloc(&a.cur_perm, B * a.KW));
    AZD_ST(e->alloc(&a.cur_path, B * a.KW));
    // (an AH dense engine keeps two doubles and two ints per agent there: dense_ah_cost.inc, DenseCostAH; an INV dense engine ten and
    // two, and its recipe behind the doubles: dense_inv_cost.inc, DenseCostInv -- the tier's row says how many)
    AZD_ST(e->alloc(&a.cur_lambda, (size_t)tier->cost_f64 * B + (size_t)tier->cost_tail_f64));
    AZD_ST(e->alloc(&a.cur_mu, (size_t)tier->cost_i32 * B));
    AZD_ST(e->alloc(&a.state_pos, B));
    AZD_ST(e->alloc(&a.n_nodes, B));
    AZD_ST(e->alloc(&a.n_arcs, B));
    AZD_ST(e->alloc(&a.n_preds, B));
    AZD_ST(e->alloc(&a.flags, B));
    a.fr_lds = (uint32_t)azd::FRONTIER_CAP;
    if (const char *v = getenv("AZD_DEBUG_FRONTIER_LDS")) { // test hook: a smaller LDS share, so that small trees reach the spill arena
        const int k = atoi(v);
        if (k >= 64 && k <= azd::FRONTIER_CAP && k % 64 == 0) a.fr_lds = (uint32_t)k;
    }
    if (ramsey) AZD_ST(e->alloc(&a.fr_spill, B * 4 * a.node_cap)); // cascade frontier levels beyond the LDS's FRONTIER_CAP entries: (node, x) x node_cap x 2 levels (RamseySpace::FRONTIER_SPILL)
    AZD_ST(e->alloc(&a.cand_c, B));
    AZD_ST(e->alloc(&a.cand_node, B));
    AZD_ST(e->alloc(&a.counters, B * azd::NUM_COUNTERS));
    AZD_ST(e->alloc(&a.state_vecs, B * a.S));
    AZD_ST(e->alloc(&a.h_theta, B * a.A));
    a.obs = a.h_theta; // the reference reuses h_theta_host as the observation buffer (optimizer/mod.rs:270-277)
    AZD_ST(e->alloc(&a.weights, B * a.A));
    AZD_ST(e->alloc(&a.argmin, 1));
    AZD_ST(e->alloc(&a.status, 1));
    if (a.layers > 1) AZD_ST(e->alloc(&a.cur_seq, B * azd::MAX_NODE_ACTIONS));
    AZD_ST(e->alloc(&a.cur_stack, B * azd::PATH_STACK));
    if (dense) {
        AZD_ST(e->alloc(&a.root_adj, B * 64));
        AZD_ST(e->alloc(&a.cur_adj, B * 64));
        AZD_ST(e->alloc(&a.root_aid, B * (size_t)e->dense_slots));
        AZD_ST(e->alloc(&e->d_stage_slots, B * (size_t)((a.E + 63) / 64)));
        // (a tier's kernels write its own record where argmin_d points, TierDesc::argmin_bytes of it: so many records of the default
        // cost's type, as argmin_r_recs counts them for the Ramsey tiers -- one for every tier but the 64-row invariant
        // ones, whose 64 rows, 32 slot words and ten, sixteen or twenty-one invariants come to 872, 920 and 960 bytes where the default cost's record has 856)
        static_assert(sizeof(azd::DenseAhArgminRec) <= sizeof(azd::DenseArgminRec) && sizeof(azd::DenseAhWideArgminRec) <= sizeof(azd::DenseArgminRec) &&
                          sizeof(azd::DenseInvArgminRec) <= sizeof(azd::DenseArgminRec) && sizeof(azd::DenseInvWideArgminRec) <= 2 * sizeof(azd::DenseArgminRec) &&
                          sizeof(azd::DenseInvxArgminRec) <= sizeof(azd::DenseArgminRec) && sizeof(azd::DenseInvxWideArgminRec) <= 2 * sizeof(azd::DenseArgminRec) &&
                          sizeof(azd::DenseInvsArgminRec) <= sizeof(azd::DenseArgminRec) && sizeof(azd::DenseInvsWideArgminRec) <= 2 * sizeof(azd::DenseArgminRec),
                      "an AH or INV engine's argmin record lives in argmin_d's allocation");
        AZD_ST(e->alloc(&a.argmin_d, (tier->argmin_bytes + sizeof(azd::DenseArgminRec) - 1) / sizeof(azd::DenseArgminRec)));
        if (tier->id == TIER_DENSE) AZD_ST(e->alloc(&a.node_mate, B * (size_t)a.node_cap * 64)); // (the AH and the weighted-invariant cost keep nothing per node)
        // a bf16 evaluator takes the state vectors as bf16 rows: this space's kernels write them beside the f32 rows (write_vec16)
        if (ev && ev->input16_pitch() >= a.S) {
            a.S16 = ev->input16_pitch();
            AZD_ST(e->alloc(&a.state_vecs16, B * (size_t)a.S16));
            if (hipMemset(a.state_vecs16, 0, B * (size_t)a.S16 * 2) != hipSuccess) return AZD_ERR_HIP;
        }
    }
    if (ramsey) {
        AZD_ST(e->alloc(&a.root_nbr, B * tier->nbr_words));
        AZD_ST(e->alloc(&a.cur_nbr, B * tier->nbr_words));
        AZD_ST(e->alloc(&a.root_counts, B * (size_t)a.C * a.E));
        AZD_ST(e->alloc(&a.cur_counts, B * (size_t)a.C * a.E));
        AZD_ST(e->alloc(&a.root_tot, B * 4));
        AZD_ST(e->alloc(&a.cur_tot, B * 4));
        AZD_ST(e->alloc(&a.argmin_r, e->argmin_r_recs()));
        // AZD_ENGINE_EXT_POOL_STEP with a bf16 evaluator: the rows its searchers write beside the f32 rows (azd_engine::ext_s16; the
        // padding between S and the pitch is zeroed here and never written)
        if (e->ext && ev && ev->input16_pitch() >= a.S && ev->input16_pitch() % 8 == 0) {
            e->ext_s16_pitch = ev->input16_pitch();
            AZD_ST(e->alloc(&e->ext_s16, B * (size_t)e->ext_s16_pitch));
            if (hipMemset(e->ext_s16, 0, B * (size_t)e->ext_s16_pitch * 2) != hipSuccess) return AZD_ERR_HIP;
        }
    }
    e->persist_enabled = (cfg->flags & AZD_ENGINE_NO_PERSISTENT_STEP) == 0;
    e->barrier_step = (cfg->flags & AZD_ENGINE_BARRIER_STEP) != 0;
    // default: the pool step for populations of 256 agents and more (below that a row's trip to an evaluator CU and
    // back costs more than the asynchronous step's in-workgroup evaluator: 0.36 against 0.49 M expansions/s at 64 agents,
    // 4.7 against 3.7 at 512); AZD_ENGINE_POOL_STEP / AZD_ENGINE_ASYNC_STEP / AZD_ENGINE_BARRIER_STEP force a form
    e->graph_enabled = getenv("AZD_NO_CALL_GRAPH") == nullptr;
    e->pool_step = (cfg->flags & AZD_ENGINE_POOL_STEP) != 0 ||
                   ((cfg->flags & (AZD_ENGINE_ASYNC_STEP | AZD_ENGINE_BARRIER_STEP)) == 0 && cfg->batch >= 256);
    if (const char *env = getenv("AZD_STEP_FORM")) { // experiments: override the configured form
        if (!strcmp(env, "pool")) e->pool_step = true, e->barrier_step = false;
        else if (!strcmp(env, "async")) e->pool_step = false, e->barrier_step = false;
        else if (!strcmp(env, "barrier")) e->pool_step = false, e->barrier_step = true;
    }
    {
        hipDeviceProp_t prop;
        e->n_cus = hipGetDeviceProperties(&prop, cfg->device) == hipSuccess ? prop.multiProcessorCount : 256;
        uint32_t qcap = 128;
        while (qcap < 2u * (uint32_t)a.B) qcap <<= 1;
        e->pool.qcap = qcap;
        e->pool_slot_words = (size_t)4 * azd::POOL_XCDS * qcap; // two ready lanes + two evaluator lanes
        AZD_ST(e->alloc(&e->pool.ctl, 1));
        AZD_ST(e->alloc(&e->pool.ready_slots, e->pool_slot_words));
        e->pool.eval_slots = e->pool.ready_slots + (size_t)2 * azd::POOL_XCDS * qcap;
        AZD_ST(e->alloc(&e->pool.join, B));
        AZD_ST(e->alloc(&e->pool.pend, B));
        AZD_ST(e->alloc(&e->pool.stamp, B));
        AZD_ST(e->alloc(&e->pool.post_call, B));
        AZD_ST(e->alloc(&e->d_resume, B));
        AZD_ST(e->alloc(&e->d_call_ctr, (size_t)azd_engine::MAX_SUBS));
        if (e->ext) {
            AZD_ST(e->alloc(&e->d_ext_rows, B * azd_engine::EXT_STREAMS));
            AZD_ST(e->alloc(&e->d_ext_home, B * azd_engine::EXT_STREAMS));
            AZD_ST(e->alloc(&e->d_ext_n, (size_t)azd_engine::EXT_STREAMS));
            AZD_ST(e->alloc(&e->d_ext_t0, (size_t)azd_engine::EXT_STREAMS));
        }
    }
    e->log_calls = 1024;
    {
        const size_t n_wg = (B + 15) / 16;
        AZD_ST(e->alloc(&e->d_pargs, 1));
        AZD_ST(e->h_pargs.alloc(1));
        AZD_ST(e->alloc(&e->d_log_key, (size_t)e->log_calls * n_wg));
        AZD_ST(e->alloc(&e->d_log_node, (size_t)e->log_calls * n_wg));
        AZD_ST(e->alloc(&e->pool.win_count, (size_t)e->log_calls));
        AZD_ST(e->alloc(&e->d_argmin_side, 1));
        if (ramsey) AZD_ST(e->alloc(&e->d_argmin_r_side, e->argmin_r_recs()));
        // what the kernel hands the host in the middle of a launch: fine-grained (host-coherent) pinned memory
        AZD_ST(e->h_win_log.alloc((size_t)e->log_calls, hipHostMallocCoherent));
        AZD_ST(e->h_win_flag.alloc((size_t)e->log_calls, hipHostMallocCoherent));
        e->pool.win_log = e->h_win_log;
        e->pool.win_flag = e->h_win_flag;
    }
    AZD_ST(e->alloc(&e->d_stage_parents, B * (size_t)(dense ? 8 * a.n : ramsey ? a.E : a.n)));
    AZD_ST(e->alloc(&e->d_stage_perm, B * (size_t)(dense ? 17 * a.KW : a.KW)));
    if (!dense) e->d_stage_slots = e->d_stage_perm; // (SpaceOps::modify_roots)
    AZD_ST(e->alloc(&e->d_root_report, B * 3));
    e->root_args.report = e->d_root_report;
    AZD_ST(e->h_status.alloc(1));
    AZD_ST(e->root_report.alloc(B * 3));
    AZD_ST(e->h_argmin.alloc(1));
    hipError_t he = hipMemsetAsync(a.counters, 0, B * azd::NUM_COUNTERS * 8, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(a.status, 0, sizeof(azd::StatusRec), e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(a.argmin, 0, sizeof(azd::ArgminRec), e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(a.flags, 0, B * 4, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(a.h_theta, 0, B * a.A * 4, e->stream);
    if (he == hipSuccess) he = hipMemsetAsync(a.state_vecs, 0, B * a.S * 4, e->stream); // vec![0.; ..] (optimizer/mod.rs:65)
    if (he == hipSuccess) he = hipMemsetAsync(a.weights, 0, B * a.A * 4, e->stream);
    // (the argmin kernels write E colours of the record: the entries beyond them are read back as zeros, whatever the memory held before)
    if (he == hipSuccess && ramsey) he = hipMemsetAsync(a.argmin_r, 0, e->argmin_r_recs() * sizeof(azd::RamseyArgminRec), e->stream);
    if (he == hipSuccess && ramsey) he = hipMemsetAsync(e->d_argmin_r_side, 0, e->argmin_r_recs() * sizeof(azd::RamseyArgminRec), e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) return azd::hip_fail(he, "engine init memset");
    *out = e.release();
    return AZD_OK;
}

int azd_engine_destroy(azd_engine *e) {
    if (e) delete e; // (~azd_engine, engine_impl.h: waits for the streams; then the members release what they own)
    return AZD_OK;
}

// optimizer/mod.rs:61-70
int azd_engine_par_new_begin(azd_engine *e, const uint8_t *parents, const uint64_t *permitted) {
    if (!e || !parents || !permitted) return AZD_ERR_INVALID_ARGUMENT;
    if (e->tier->family && !e->inv_recipe_set) {
        const azd::DenseFamilyDesc &f = *e->tier->family;
        azd::g_last_error = std::string("par_new: an ") + f.flag[0] + " engine has no cost before " + f.setter + " has given it its recipe";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    AZD_ENTER(e);
    AZD_ST(upload_roots(e, parents, permitted));
    e->inv_recipe_locked = true;
    const azd::Arenas &a = e->a;
    AZD_HIP(hipMemsetAsync(a.counters, 0, (size_t)a.B * azd::NUM_COUNTERS * 8, e->stream));
    e->counters_by_wave = false;
    AZD_HIP(hipMemsetAsync(a.status, 0, sizeof(azd::StatusRec), e->stream));
    e->seen_improved = 0;
    e->ops->init_roots(a, e->d_stage_parents, e->d_stage_perm, e->stream);
    AZD_HIP(hipMemsetAsync(a.h_theta, 0, (size_t)a.B * a.A * 4, e->stream)); // vec![0.; ..] at :71
    AZD_HIP(hipGetLastError());
    return AZD_OK;
}
static int new_finish(azd_engine *e) {
    e->ops->add_actions(e->a, 1, e->stream);
    e->ops->argmin(e->a, 1, e->stream);
    e->initialised = true;
    return sync_status(e);
}
// optimizer/mod.rs:74-101
int azd_engine_par_new_end(azd_engine *e, const float *h_theta) {
    if (!e || !h_theta) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipMemcpyAsync(e->a.h_theta, h_theta, (size_t)e->a.B * e->a.A * 4, hipMemcpyHostToDevice, e->stream));
    return new_finish(e);
}
int azd_engine_par_new(azd_engine *e, const uint8_t *parents, const uint64_t *permitted) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_ST(azd_engine_par_new_begin(e, parents, permitted));
    AZD_ST(run_evaluator(e)); // :72
    return new_finish(e);
}

int azd_engine_observe_dev(azd_engine *e, uint32_t n_obs_tol, const float **d_state_vecs, const float **d_obs,
                           const float **d_w) {
    if (!e || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    e->ops->observe(e->a, n_obs_tol, e->stream);
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipGetLastError());
    if (d_state_vecs) *d_state_vecs = e->a.state_vecs;
    if (d_obs) *d_obs = e->a.obs;
    if (d_w) *d_w = e->a.weights;
    return AZD_OK;
}
int azd_engine_observe(azd_engine *e, uint32_t n_obs_tol, float *state_vecs, float *observations, float *weights) {
    AZD_ST(azd_engine_observe_dev(e, n_obs_tol, nullptr, nullptr, nullptr));
    const azd::Arenas &a = e->a;
    if (state_vecs) AZD_HIP(hipMemcpy(state_vecs, a.state_vecs, (size_t)a.B * a.S * 4, hipMemcpyDeviceToHost));
    if (observations) AZD_HIP(hipMemcpy(observations, a.obs, (size_t)a.B * a.A * 4, hipMemcpyDeviceToHost));
    if (weights) AZD_HIP(hipMemcpy(weights, a.weights, (size_t)a.B * a.A * 4, hipMemcpyDeviceToHost));
    return AZD_OK;
}
int azd_engine_par_update_model(azd_engine *e, uint32_t n_obs_tol, float *loss) {
    if (!e || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_ENTER(e);
    e->ops->observe(e->a, n_obs_tol, e->stream);
    AZD_HIP(hipGetLastError());
    float l = 0.f;
    AZD_ST(e->ev->update_model_dev(e->a.B, e->a.state_vecs, e->a.obs, e->a.weights, &l, e->stream)); // :279-280
    AZD_HIP(hipStreamSynchronize(e->stream));
    if (loss) *loss = l;
    return AZD_OK;
}

// ---- the epoch exchange of a sharded population, for hosts that are not Python (azdopt_amd/parallel.py does the
// same through torch.distributed): optimizer/mod.rs:249-281 where the batch is the union of all ranks' agents.
// RCCL is bound at first use (dlopen), so the library carries no link-time dependency on it.
namespace {
struct RcclApi {
    void *lib = nullptr;
    int (*allGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*commCount)(void *, int *) = nullptr;
    const char *(*errorString)(int) = nullptr;
    bool tried = false;
};
RcclApi *rccl() {
    static RcclApi api;
    if (!api.tried) {
        api.tried = true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib) break;
        }
        if (api.lib) {
            api.allGather = (decltype(api.allGather))dlsym(api.lib, "ncclAllGather");
            api.commCount = (decltype(api.commCount))dlsym(api.lib, "ncclCommCount");
            api.errorString = (decltype(api.errorString))dlsym(api.lib, "ncclGetErrorString");
        }
    }
    return &api;
}
constexpr int NCCL_FLOAT32 = 7; // ncclFloat32 (rccl.h)
} // namespace

int azd_engine_par_update_model_sharded(azd_engine *e, uint32_t n_obs_tol, void *nccl_comm, float *loss) {
    if (!e || !e->initialised || !nccl_comm) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_ENTER(e);
    RcclApi &api = *rccl();
    if (!api.allGather || !api.commCount) {
        azd::g_last_error = "librccl.so could not be loaded (ncclAllGather / ncclCommCount)";
        return AZD_ERR_UNSUPPORTED;
    }
    int world = 0;
    int rc = api.commCount(nccl_comm, &world);
    if (rc != 0 || world <= 0) {
        azd::g_last_error = std::string("ncclCommCount: ") + (api.errorString ? api.errorString(rc) : "failed");
        return AZD_ERR_INVALID_ARGUMENT;
    }
    const azd::Arenas &a = e->a;
    const size_t B = (size_t)a.B, rows = B * (size_t)world;
    const size_t ns = rows * a.S, na = rows * a.A;
    if (rows > e->pool_rows) {
        e->pool_rows = 0;
        AZD_ST(e->d_pool.alloc(ns + 2 * na));
        e->pool_rows = rows;
    }
    if (rows > e->pool_rows || rows > (size_t)INT32_MAX) { // (the pooled buffers hold `pool_rows` rows: sized just above)
        azd::g_last_error = "pooled batch does not fit its buffers";
        return AZD_ERR_CAPACITY;
    }
    float *g_sv = e->d_pool, *g_obs = g_sv + ns, *g_w = g_obs + na;
    e->ops->observe(a, n_obs_tol, e->stream); // :262-278 on this rank's trees
    AZD_HIP(hipGetLastError());
    // rank order = global agent order (shards are contiguous agent ranges); the collectives run on the engine's
    // stream, behind k_observe and ahead of the optimiser step
    const float *src[3] = {a.state_vecs, a.obs, a.weights};
    float *dst[3] = {g_sv, g_obs, g_w};
    const size_t cnt[3] = {B * (size_t)a.S, B * (size_t)a.A, B * (size_t)a.A};
    for (int i = 0; i < 3; ++i) {
        rc = api.allGather(src[i], dst[i], cnt[i], NCCL_FLOAT32, nccl_comm, e->stream);
        if (rc != 0) {
            (void)hipStreamSynchronize(e->stream); // k_observe and the collectives already queued: nothing of this call is left in flight
            azd::g_last_error = std::string("ncclAllGather: ") + (api.errorString ? api.errorString(rc) : "failed");
            return AZD_ERR_HIP;
        }
    }
    float l = 0.f;
    AZD_ST(e->ev->update_model_dev((int)rows, g_sv, g_obs, g_w, &l, e->stream)); // :279-280, the same step on every rank
    AZD_HIP(hipStreamSynchronize(e->stream));
    if (loss) *loss = l;
    return AZD_OK;
}

// optimizer/mod.rs:317-346
int azd_engine_reset_begin(azd_engine *e, const uint8_t *parents, const uint64_t *permitted) {
    if (!e || !parents || !permitted || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_ST(upload_roots(e, parents, permitted));
    const azd::Arenas &a = e->a;
    AZD_HIP(hipMemsetAsync(&a.status->failed, 0, sizeof(unsigned long long), e->stream));
    e->ops->init_roots(a, e->d_stage_parents, e->d_stage_perm, e->stream);
    AZD_HIP(hipMemsetAsync(a.h_theta, 0, (size_t)a.B * a.A * 4, e->stream)); // h_theta_host.fill(0.) at :347
    AZD_HIP(hipGetLastError());
    return AZD_OK;
}
static int reset_finish(azd_engine *e) {
    e->ops->add_actions(e->a, 1, e->stream); // :350-358; num_inspected_nodes = 0 via cand_* in init_roots
    return sync_status(e);
}
int azd_engine_reset_end(azd_engine *e, const float *h_theta) {
    if (!e || !h_theta) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipMemcpyAsync(e->a.h_theta, h_theta, (size_t)e->a.B * e->a.A * 4, hipMemcpyHostToDevice, e->stream));
    return reset_finish(e);
}
int azd_engine_par_reset_trees(azd_engine *e, const uint8_t *parents, const uint64_t *permitted) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_ST(azd_engine_reset_begin(e, parents, permitted));
    AZD_ST(run_evaluator(e)); // :348
    return reset_finish(e);
}

} // extern "C"
