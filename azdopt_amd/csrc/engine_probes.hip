// engine_probes.hip -- the azd_debug_* entries (probes and test hooks) and the host entries of the Aouchiche-Hansen cost.
#include "engine_impl.h"

// ------------------------------------------------------------------ spectral costs of the dense-graph space: the probes' host side
// One driver around every probe kernel (32 or 64 rows, with a recipe or without).  check(graph, i) refuses graph i, and the recipe
// after it, with the entry's text; launch(d_adj, n, count, reps, d_recipe, d_out, stream) starts the tier's kernel (space_ops.h:
// launch_probe_*_cost): once to warm up, then `reps` repetitions between two events.  recipe: null for a cost that takes none
// (Recipe = char; nothing is allocated for it).
template <class Cost, class Recipe, class Check, class Launch>
static int probe_dense_cost(const char *name, const char *tag, int device, const uint64_t *adj, int n, int count, int reps, const Recipe *recipe,
                            void *out, float *ms, Check check, Launch launch) {
    if (!out || count <= 0 || reps <= 0) {
        azd::g_last_error = std::string(name) + ": out / count / reps";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < count; ++i) // (before the device check, like every limit: the kernel indexes LDS by the bits of adj)
        AZD_ST(check(adj ? adj + (size_t)i * (n > 0 ? n : 0) : nullptr, i));
    AZD_ST(azd::device_ok(device));
    AZD_HIP(hipSetDevice(device));
    azd::DevBuf<uint64_t> d_adj;
    azd::DevBuf<Cost> d_out;
    azd::DevBuf<Recipe> d_recipe;
    azd::Event e0, e1;
    AZD_ST(azd::alloc_set(d_adj, (size_t)count * n, d_out, (size_t)count, d_recipe, (size_t)(recipe ? 1 : 0)));
    AZD_ST(e0.create());
    AZD_ST(e1.create());
    AZD_HIP(hipMemcpy(d_adj, adj, (size_t)count * n * 8, hipMemcpyHostToDevice));
    if (recipe) {
        AZD_HIP(hipMemcpy(d_recipe, recipe, sizeof(Recipe), hipMemcpyHostToDevice));
    }
    launch(d_adj, n, count, 1, d_recipe, d_out, nullptr); // warm-up
    AZD_HIP(hipEventRecord(e0, nullptr));
    launch(d_adj, n, count, reps, d_recipe, d_out, nullptr);
    AZD_HIP(hipEventRecord(e1, nullptr));
    hipError_t he = hipDeviceSynchronize();
    float t = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&t, e0, e1);
    if (he == hipSuccess) he = hipMemcpy(out, d_out, (size_t)count * sizeof(Cost), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return azd::hip_fail(he, tag);
    if (ms) *ms = t;
    return AZD_OK;
}
// The three recipe costs (dense_cost_host.h: DenseFamily) behind one set of entries; the ABI's structs mirror the host's.
// graph `i` (or the only one) and the recipe, checked in this order; the text names `fn` and the argument
template <azd::DenseFamily F>
static int recipe_check(const char *fn, bool wide, const uint64_t *adj, int n, int i, const typename azd::DenseFamilyOf<F>::Recipe *recipe) {
    const azd::DenseFamilyDesc &f = azd::dense_family(F);
    const char *why = azd::dense_check_graph(adj, n, f.max_n[wide], f.bad_n[wide]);
    if (!why) why = azd::dense_check_recipe<F>(recipe, n);
    else if (i >= 0) {
        azd::g_last_error = std::string(fn) + ": graph " + std::to_string(i) + ": " + why;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (why) azd::g_last_error = std::string(fn) + ": " + why;
    return why ? AZD_ERR_INVALID_ARGUMENT : AZD_OK;
}
// the host cost: one host function behind the 32-row and the 64-row check
template <azd::DenseFamily F, class AbiRecipe, class AbiCost>
static int recipe_cost(const char *fn, bool wide, const uint64_t *adj, int n, const AbiRecipe *recipe, AbiCost *out) {
    using T = azd::DenseFamilyOf<F>;
    static_assert(sizeof(AbiRecipe) == sizeof(typename T::Recipe) && sizeof(AbiCost) == sizeof(typename T::Cost), "ABI struct mismatch");
    if (!out) {
        azd::g_last_error = std::string(fn) + ": out: null";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    const auto *r = reinterpret_cast<const typename T::Recipe *>(recipe);
    AZD_ST(recipe_check<F>(fn, wide, adj, n, -1, r));
    T::cost_host(adj, n, *r, reinterpret_cast<typename T::Cost *>(out));
    return AZD_OK;
}
// the probe: the 32-row or the 64-row kernel, as `launch` starts it
template <azd::DenseFamily F, class AbiRecipe, class AbiCost, class Launch>
static int probe_recipe_cost(const char *name, const char *tag, bool wide, int device, const uint64_t *adj, int n, int count, int reps, const AbiRecipe *recipe,
                             AbiCost *out, float *ms, Launch launch) {
    using T = azd::DenseFamilyOf<F>;
    const auto *r = reinterpret_cast<const typename T::Recipe *>(recipe);
    const auto check = [=](const uint64_t *g, int i) { return recipe_check<F>(name, wide, g, n, i, r); };
    return probe_dense_cost<typename T::Cost>(name, tag, device, adj, n, count, reps, r, out, ms, check, launch);
}

extern "C" {

int azd_debug_mlp_gradients(azd_evaluator *ev, int batch, const float *states, const float *observations, const float *action_weights,
                            float *grads_out, float *loss) {
    if (!ev || batch <= 0 || !states || !observations || !action_weights || !grads_out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(ev->ensure_staging(batch));
    size_t sb = (size_t)batch * ev->state_dim * 4, pb = (size_t)batch * ev->action_dim * 4;
    AZD_HIP(hipMemcpyAsync(ev->d_states, states, sb, hipMemcpyHostToDevice, ev->own_stream));
    AZD_HIP(hipMemcpyAsync(ev->d_obs, observations, pb, hipMemcpyHostToDevice, ev->own_stream));
    AZD_HIP(hipMemcpyAsync(ev->d_w, action_weights, pb, hipMemcpyHostToDevice, ev->own_stream));
    return ev->debug_gradients(batch, ev->d_states, ev->d_obs, ev->d_w, grads_out, loss, ev->own_stream);
}
int azd_debug_write_predictions_gathered(azd_evaluator *ev, int max_rows, const uint32_t *rows, int n_rows, const float *states, int n_state_rows,
                                         float *predictions) {
    if (!ev || max_rows < 1 || n_rows < 0 || n_rows > max_rows || (n_rows > 0 && !rows) || !states || n_state_rows < 1 || !predictions)
        return AZD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n_rows; ++i)
        if (rows[i] >= (uint32_t)n_state_rows) {
            azd::g_last_error = "azd_debug_write_predictions_gathered: a row index is not below n_state_rows";
            return AZD_ERR_INVALID_ARGUMENT;
        }
    return ev->debug_write_predictions_gathered(max_rows, rows, n_rows, states, n_state_rows, predictions);
}
int azd_debug_hash_stream_via_evaluators(azd_evaluator *ev, int on) { return ev ? ev->debug_serve_from_pool(on) : AZD_ERR_INVALID_ARGUMENT; }
// Test entry: rows of the evaluator as the CU-resident step forms compute them (mlp_tile_task; k_tile_forward), for `rows` state
// vectors given by the host.  Needs an MLP evaluator the pool step can serve (the plan lays the rows out in LDS).
int azd_engine_debug_tile_forward(azd_engine *e, const float *states, float *predictions, int rows) {
    if (!e || !states || !predictions || rows < 1) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    azd::FusedEval fe;
    azd::PoolArgs pool = e->pool;
    uint32_t dyn_stride = 0;
    size_t dyn_bytes = 0;
    const char *why = "";
    if (e->a.space == azd::SPACE_DENSE || !e->ev->fused_desc(&fe) || fe.kind != 3 || !e->ops->pool_plan(e->a, fe, &pool, &dyn_stride, &dyn_bytes, &why)) {
        azd::g_last_error = "debug_tile_forward: needs the c21 or the Ramsey space with an MLP evaluator the pool step can serve";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::DevBuf<float> d_in, d_out;
    AZD_ST(azd::alloc_set(d_in, (size_t)rows * e->a.S, d_out, (size_t)rows * e->a.A));
    const char *what = "hipMemcpyAsync";
    hipError_t he = hipMemcpyAsync(d_in, states, (size_t)rows * e->a.S * 4, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) what = "k_tile_forward", he = azd::launch_tile_forward(fe, pool, rows, d_in, d_out, e->stream);
    if (he == hipSuccess) what = "hipMemcpyAsync", he = hipMemcpyAsync(predictions, d_out, (size_t)rows * e->a.A * 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) what = "hipStreamSynchronize", he = hipStreamSynchronize(e->stream);
    else (void)hipStreamSynchronize(e->stream); // nothing of this call may still be running on the buffers when they go
    return he == hipSuccess ? AZD_OK : azd::hip_fail(he, what);
}
int azd_debug_probe_xcc(int device, uint32_t *out, int n_blocks) {
    if (!out || n_blocks <= 0) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd::device_ok(device));
    AZD_HIP(hipSetDevice(device));
    azd::DevBuf<uint32_t> d;
    AZD_ST(d.alloc((size_t)n_blocks));
    azd::launch_probe_xcc(d, n_blocks, nullptr);
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(out, d, (size_t)n_blocks * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return azd::hip_fail(he, "probe_xcc");
    return AZD_OK;
}
// The LDS plan of the searcher-only pool step for a configuration (AZD_ENGINE_EXT_POOL_STEP, or a dense-graph engine with
// AZD_ENGINE_DENSE_AH_WIDE, AZD_ENGINE_DENSE_INV_WIDE or AZD_ENGINE_DENSE_INVX_WIDE, whose pool step is planned by what the LDS holds too): wavefronts per
// searcher workgroup and bytes of LDS a workgroup takes, its static blocks included.  Arithmetic only: no device is touched.
int azd_debug_ext_pool_plan(const azd_engine_config *cfg, int *waves, size_t *lds_bytes) {
    if (!cfg || !waves || !lds_bytes) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(check_engine_config(cfg));
    const bool ah_wide = (cfg->flags & (AZD_ENGINE_DENSE_AH_WIDE | AZD_ENGINE_DENSE_INV_WIDE | AZD_ENGINE_DENSE_INVX_WIDE | AZD_ENGINE_DENSE_INVS_WIDE)) != 0; // (the 64-row tiers; the last has no such step and is told so below)
    // (a dense-graph configuration that sets AZD_ENGINE_EXT_POOL_F32 alone asks its pool step for the fp32 evaluator: the plan is
    // that step's, whatever the cost -- the searchers do not know which evaluator serves them)
    const bool dense_f32 = cfg->space_id == AZD_SPACE_DENSE && (cfg->flags & AZD_ENGINE_EXT_POOL_F32) != 0;
    if (!(cfg->flags & AZD_ENGINE_EXT_POOL_STEP) && !ah_wide && !dense_f32) {
        azd::g_last_error = "azd_debug_ext_pool_plan: the configuration does not set AZD_ENGINE_EXT_POOL_STEP";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    const TierDesc *const tier = engine_tier(cfg);
    azd::Arenas a;
    engine_shape(cfg, tier, &a);
    const azd::SpaceOps *ops = tier->ops;
    const ExtPoolForm *xf = tier->ext;
    if (!xf) {
        azd::g_last_error = "azd_debug_ext_pool_plan: the configuration's tier has no searcher-only pool step";
        return AZD_ERR_UNSUPPORTED;
    }
    const char *why = "";
    uint32_t dyn_stride = 0;
    size_t dyn_bytes = 0;
    int w = ops->waves_max;
    while (w > xf->waves_min && !ops->pool_search_plan(a, w, &dyn_stride, &dyn_bytes, &why)) w -= 1;
    if (!ops->pool_search_plan(a, w, &dyn_stride, &dyn_bytes, &why)) {
        azd::g_last_error = why;
        return AZD_ERR_UNSUPPORTED;
    }
    *waves = w;
    *lds_bytes = dyn_bytes + azd::POOL_SEARCH_STATIC_LDS;
    return AZD_OK;
}
int azd_debug_probe_math(int device, const float *in, float *out, int n) {
    if (!in || !out || n <= 0) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd::device_ok(device));
    AZD_HIP(hipSetDevice(device));
    azd::DevBuf<float> d_in, d_out;
    AZD_ST(azd::alloc_set(d_in, (size_t)n * 2, d_out, (size_t)n * 4));
    AZD_HIP(hipMemcpy(d_in, in, (size_t)n * 8, hipMemcpyHostToDevice));
    azd::launch_probe_math(d_in, d_out, n, nullptr);
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return azd::hip_fail(he, "probe_math");
    return AZD_OK;
}

int azd_debug_probe_cost(int device, const uint8_t *parents, int n, int count, int reps, int full, double *lambda_1,
                         int *matching_size, float *ms) {
    if (!parents || !lambda_1 || !matching_size || n < 4 || n > AZD_C21_MAX_N || count <= 0 || reps <= 0)
        return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd::device_ok(device));
    AZD_HIP(hipSetDevice(device));
    for (int i = 0; i < count; ++i) {
        const uint8_t *p = parents + (size_t)i * n;
        if (p[0] != 0 || p[n - 1] != 0) return AZD_ERR_INVALID_ARGUMENT;
        for (int v = 1; v < n; ++v)
            if (p[v] >= v) return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::DevBuf<uint8_t> d_p;
    azd::DevBuf<double> d_l;
    azd::DevBuf<int> d_m;
    azd::Event e0, e1;
    AZD_ST(azd::alloc_set(d_p, (size_t)count * n, d_l, (size_t)count, d_m, (size_t)count));
    AZD_ST(e0.create());
    AZD_ST(e1.create());
    AZD_HIP(hipMemcpy(d_p, parents, (size_t)count * n, hipMemcpyHostToDevice));
    azd::launch_probe_cost(d_p, n, count, 1, full, d_l, d_m, nullptr); // warm-up
    AZD_HIP(hipEventRecord(e0, nullptr));
    azd::launch_probe_cost(d_p, n, count, reps, full, d_l, d_m, nullptr);
    AZD_HIP(hipEventRecord(e1, nullptr));
    hipError_t he = hipDeviceSynchronize();
    float t = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&t, e0, e1);
    if (he == hipSuccess) he = hipMemcpy(lambda_1, d_l, (size_t)count * 8, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(matching_size, d_m, (size_t)count * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return azd::hip_fail(he, "probe_cost");
    if (ms) *ms = t;
    return AZD_OK;
}

// The dense-graph space's default cost outside any engine (space_dense.inc: k_probe_dense_cost).  Everything the kernel indexes
// by -- the bits of adj, the slots -- is checked before the device is looked for.
int azd_debug_probe_dense_cost(int device, const uint64_t *adj, int n, int count, const uint16_t *toggles, int n_toggles, double *lambda_1,
                               int *matching_size, uint8_t *mate, int *hook_calls) {
    const std::string name = "azd_debug_probe_dense_cost: ";
    if (!adj || !lambda_1 || !matching_size || !mate || !hook_calls || count <= 0 || n_toggles < 0 || n_toggles > 64 || (n_toggles > 0 && !toggles)) {
        azd::g_last_error = name + "adj / outputs / count / toggles / n_toggles (0 .. 64)";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (n < 4 || n > 64) {
        azd::g_last_error = name + "n: 4 <= n <= 64";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    const int E = n * (n - 1) / 2;
    const uint64_t beyond = n >= 64 ? 0ull : ~((1ull << n) - 1ull);
    for (int g = 0; g < count; ++g) {
        const uint64_t *a = adj + (size_t)g * n;
        const char *why = nullptr;
        for (int v = 0; v < n && !why; ++v) {
            if ((a[v] >> v) & 1ull) why = "adj: a loop";
            else if (a[v] & beyond) why = "adj: a neighbour at or above n";
            else
                for (int u = 0; u < v && !why; ++u)
                    if (((a[v] >> u) & 1ull) != ((a[u] >> v) & 1ull)) why = "adj: not symmetric";
        }
        uint64_t seen[32] = {};
        for (int j = 0; j < n_toggles && !why; ++j) {
            const int slot = toggles[(size_t)g * n_toggles + j];
            if (slot >= E) why = "toggles: a slot at or above E = n (n - 1) / 2";
            else if ((seen[slot >> 6] >> (slot & 63)) & 1ull) why = "toggles: a slot twice";
            else seen[slot >> 6] |= 1ull << (slot & 63);
        }
        if (why) {
            azd::g_last_error = name + "graph " + std::to_string(g) + ": " + why;
            return AZD_ERR_INVALID_ARGUMENT;
        }
    }
    AZD_ST(azd::device_ok(device));
    AZD_HIP(hipSetDevice(device));
    const size_t rows = (size_t)count * (size_t)(n_toggles + 1);
    azd::DevBuf<uint64_t> d_adj;
    azd::DevBuf<uint16_t> d_tog;
    azd::DevBuf<double> d_l;
    azd::DevBuf<int> d_m, d_h;
    azd::DevBuf<uint8_t> d_mate;
    AZD_ST(azd::alloc_set(d_adj, (size_t)count * n, d_tog, (size_t)count * n_toggles + 1, d_l, rows, d_m, rows, d_h, rows, d_mate, rows * 64));
    AZD_HIP(hipMemcpy(d_adj, adj, (size_t)count * n * 8, hipMemcpyHostToDevice));
    if (n_toggles > 0) AZD_HIP(hipMemcpy(d_tog, toggles, (size_t)count * n_toggles * 2, hipMemcpyHostToDevice));
    azd::launch_probe_dense_cost(d_adj, n, count, d_tog, n_toggles, d_l, d_m, d_mate, d_h, nullptr);
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(lambda_1, d_l, rows * 8, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(matching_size, d_m, rows * 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(hook_calls, d_h, rows * 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(mate, d_mate, rows * 64, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return azd::hip_fail(he, "probe_dense_cost");
    return AZD_OK;
}

// ------------------------------------------------------------------ Aouchiche-Hansen cost of the dense-graph space
static_assert(sizeof(azd_dense_ah_cost_t) == sizeof(azd::DenseAhCost) && offsetof(azd_dense_ah_cost_t, eval) == offsetof(azd::DenseAhCost, eval),
              "azd_dense_ah_cost_t mirrors azd::DenseAhCost");
static_assert(AZD_DENSE_AH_MAX_N == azd::DENSE_AH_MAX_N && AZD_DENSE_AH_WIDE_MAX_N == azd::DENSE_AH_WIDE_MAX_N, "AZD_DENSE_AH_MAX_N, AZD_DENSE_AH_WIDE_MAX_N");
int azd_dense_ah_cost(const uint64_t *adj, int n, azd_dense_ah_cost_t *out) {
    if (!out) {
        azd::g_last_error = "azd_dense_ah_cost: out: null";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (const char *why = azd::dense_ah_check_graph(adj, n)) {
        azd::g_last_error = std::string("azd_dense_ah_cost: ") + why;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::dense_ah_cost_host(adj, n, reinterpret_cast<azd::DenseAhCost *>(out));
    return AZD_OK;
}
int azd_dense_ah_cost_wide(const uint64_t *adj, int n, azd_dense_ah_cost_t *out) {
    if (!out) {
        azd::g_last_error = "azd_dense_ah_cost_wide: out: null";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (const char *why = azd::dense_ah_check_graph_wide(adj, n)) {
        azd::g_last_error = std::string("azd_dense_ah_cost_wide: ") + why;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::dense_ah_cost_host(adj, n, reinterpret_cast<azd::DenseAhCost *>(out));
    return AZD_OK;
}
// the two probes: the 32-row and the 64-row kernel
static int probe_ah_cost(const char *name, bool wide, int device, const uint64_t *adj, int n, int count, int reps, azd_dense_ah_cost_t *out, float *ms) {
    const auto graph_check = wide ? azd::dense_ah_check_graph_wide : azd::dense_ah_check_graph;
    const auto kernel = wide ? azd::launch_probe_ah_cost_wide : azd::launch_probe_ah_cost;
    const auto check = [=](const uint64_t *g, int i) {
        const char *why = graph_check(g, n);
        if (why) azd::g_last_error = std::string(name) + ": graph " + std::to_string(i) + ": " + why;
        return why ? AZD_ERR_INVALID_ARGUMENT : AZD_OK;
    };
    const auto launch = [=](const uint64_t *d_adj, int n_, int count_, int reps_, const char *, azd::DenseAhCost *d_out, void *stream) {
        kernel(d_adj, n_, count_, reps_, d_out, stream);
    };
    return probe_dense_cost<azd::DenseAhCost, char>(name, "probe_ah_cost", device, adj, n, count, reps, (const char *)nullptr, out, ms, check, launch);
}
int azd_debug_probe_ah_cost(int device, const uint64_t *adj, int n, int count, int reps, azd_dense_ah_cost_t *out, float *ms) {
    return probe_ah_cost("azd_debug_probe_ah_cost", false, device, adj, n, count, reps, out, ms);
}
int azd_debug_probe_ah_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, azd_dense_ah_cost_t *out, float *ms) {
    return probe_ah_cost("azd_debug_probe_ah_cost_wide", true, device, adj, n, count, reps, out, ms);
}
// ------------------------------------------------------------------ weighted-invariant cost of the dense-graph space
static_assert(AZD_DENSE_INV_MAX_N == azd::DENSE_INV_MAX_N && AZD_DENSE_INV_WIDE_MAX_N == azd::DENSE_INV_WIDE_MAX_N && AZD_DENSE_INV_COUNT == azd::DENSE_INV_COUNT && AZD_DENSE_INV_INDEX_AH == azd::DENSE_INV_INDEX_AH,
              "AZD_DENSE_INV_*");
int azd_dense_inv_cost(const uint64_t *adj, int n, const azd_dense_inv_recipe *recipe, azd_dense_inv_cost_t *out) {
    return recipe_cost<azd::DENSE_FAMILY_INV>("azd_dense_inv_cost", false, adj, n, recipe, out);
}
int azd_dense_inv_cost_wide(const uint64_t *adj, int n, const azd_dense_inv_recipe *recipe, azd_dense_inv_cost_t *out) {
    return recipe_cost<azd::DENSE_FAMILY_INV>("azd_dense_inv_cost_wide", true, adj, n, recipe, out);
}
int azd_debug_probe_inv_cost(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_inv_recipe *recipe,
                             azd_dense_inv_cost_t *out, float *ms) {
    return probe_recipe_cost<azd::DENSE_FAMILY_INV>("azd_debug_probe_inv_cost", "probe_inv_cost", false, device, adj, n, count, reps, recipe, out, ms, azd::launch_probe_inv_cost);
}
int azd_debug_probe_inv_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_inv_recipe *recipe,
                                  azd_dense_inv_cost_t *out, float *ms) {
    return probe_recipe_cost<azd::DENSE_FAMILY_INV>("azd_debug_probe_inv_cost_wide", "probe_inv_cost", true, device, adj, n, count, reps, recipe, out, ms,
                                                    azd::launch_probe_inv_cost_wide);
}
// ------------------------------------------------------------------ extended invariant cost of the dense-graph space
static_assert(AZD_DENSE_INVX_MAX_N == azd::DENSE_INVX_MAX_N && AZD_DENSE_INVX_WIDE_MAX_N == azd::DENSE_INVX_WIDE_MAX_N && AZD_DENSE_INVX_COUNT == azd::DENSE_INVX_COUNT && AZD_DENSE_INVX_MAX_TERMS == azd::DENSE_INVX_MAX_TERMS &&
                  AZD_DENSE_INVX_MUL == azd::DENSE_INVX_MUL && AZD_DENSE_INVX_DIV == azd::DENSE_INVX_DIV,
              "AZD_DENSE_INVX_*");
int azd_dense_invx_cost(const uint64_t *adj, int n, const azd_dense_invx_recipe *recipe, azd_dense_invx_cost_t *out) {
    return recipe_cost<azd::DENSE_FAMILY_INVX>("azd_dense_invx_cost", false, adj, n, recipe, out);
}
int azd_dense_invx_cost_wide(const uint64_t *adj, int n, const azd_dense_invx_recipe *recipe, azd_dense_invx_cost_t *out) {
    return recipe_cost<azd::DENSE_FAMILY_INVX>("azd_dense_invx_cost_wide", true, adj, n, recipe, out);
}
int azd_debug_probe_invx_cost(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invx_recipe *recipe,
                              azd_dense_invx_cost_t *out, float *ms) {
    return probe_recipe_cost<azd::DENSE_FAMILY_INVX>("azd_debug_probe_invx_cost", "probe_invx_cost", false, device, adj, n, count, reps, recipe, out, ms,
                                                     azd::launch_probe_invx_cost);
}
int azd_debug_probe_invx_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invx_recipe *recipe,
                                   azd_dense_invx_cost_t *out, float *ms) {
    return probe_recipe_cost<azd::DENSE_FAMILY_INVX>("azd_debug_probe_invx_cost_wide", "probe_invx_cost", true, device, adj, n, count, reps, recipe, out, ms,
                                                     azd::launch_probe_invx_cost_wide);
}
// ------------------------------------------------------------------ spectrum invariant cost of the dense-graph space
static_assert(AZD_DENSE_INVS_MAX_N == azd::DENSE_INVS_MAX_N && AZD_DENSE_INVS_WIDE_MAX_N == azd::DENSE_INVS_WIDE_MAX_N && AZD_DENSE_INVS_COUNT == azd::DENSE_INVS_COUNT && AZD_DENSE_INVS_ROUNDS == azd::DENSE_INVS_ROUNDS &&
                  AZD_DENSE_INVS_MATRIX_ADJ == azd::DENSE_INVS_MATRIX_ADJ && AZD_DENSE_INVS_MATRIX_DIST == azd::DENSE_INVS_MATRIX_DIST &&
                  AZD_DENSE_INVS_MATRIX_LAP == azd::DENSE_INVS_MATRIX_LAP && AZD_DENSE_INVS_MATRIX_SLAP == azd::DENSE_INVS_MATRIX_SLAP,
              "AZD_DENSE_INVS_*");
// the two spectrum calls: one host function behind the 32-row and the 64-row check
static int invs_spectrum(const char *fn, bool wide, const uint64_t *adj, int n, int which, double *out) {
    const azd::DenseFamilyDesc &f = azd::dense_family(azd::DENSE_FAMILY_INVS);
    const char *why = !out ? "out: null" : azd::dense_check_graph(adj, n, f.max_n[wide], f.bad_n[wide]);
    if (!why && (which < AZD_DENSE_INVS_MATRIX_ADJ || which > AZD_DENSE_INVS_MATRIX_SLAP))
        why = "which: must be one of AZD_DENSE_INVS_MATRIX_ADJ, _DIST, _LAP, _SLAP (0 .. 3)";
    if (why) {
        azd::g_last_error = std::string(fn) + ": " + why;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::dense_invs_spectrum_host(adj, n, which, out);
    return AZD_OK;
}
int azd_dense_invs_cost(const uint64_t *adj, int n, const azd_dense_invs_recipe *recipe, azd_dense_invs_cost_t *out) {
    return recipe_cost<azd::DENSE_FAMILY_INVS>("azd_dense_invs_cost", false, adj, n, recipe, out);
}
int azd_dense_invs_cost_wide(const uint64_t *adj, int n, const azd_dense_invs_recipe *recipe, azd_dense_invs_cost_t *out) {
    return recipe_cost<azd::DENSE_FAMILY_INVS>("azd_dense_invs_cost_wide", true, adj, n, recipe, out);
}
int azd_dense_invs_spectrum(const uint64_t *adj, int n, int which, double *out) { return invs_spectrum("azd_dense_invs_spectrum", false, adj, n, which, out); }
int azd_dense_invs_spectrum_wide(const uint64_t *adj, int n, int which, double *out) {
    return invs_spectrum("azd_dense_invs_spectrum_wide", true, adj, n, which, out);
}
int azd_debug_probe_invs_cost(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invs_recipe *recipe,
                              azd_dense_invs_cost_t *out, float *ms) {
    return probe_recipe_cost<azd::DENSE_FAMILY_INVS>("azd_debug_probe_invs_cost", "probe_invs_cost", false, device, adj, n, count, reps, recipe, out, ms,
                                                     azd::launch_probe_invs_cost);
}
int azd_debug_probe_invs_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invs_recipe *recipe,
                                   azd_dense_invs_cost_t *out, float *ms) {
    return probe_recipe_cost<azd::DENSE_FAMILY_INVS>("azd_debug_probe_invs_cost_wide", "probe_invs_cost_wide", true, device, adj, n, count, reps, recipe, out, ms,
                                                     azd::launch_probe_invs_cost_wide);
}
int azd_debug_probe_math_f64(int device, const double *in, double *out, int n) {
    if (!in || !out || n <= 0) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd::device_ok(device));
    AZD_HIP(hipSetDevice(device));
    azd::DevBuf<double> d_in, d_out;
    AZD_ST(azd::alloc_set(d_in, (size_t)n * 2, d_out, (size_t)n * 3));
    AZD_HIP(hipMemcpy(d_in, in, (size_t)n * 16, hipMemcpyHostToDevice));
    azd::launch_probe_math_f64(d_in, d_out, n, nullptr);
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(out, d_out, (size_t)n * 24, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return azd::hip_fail(he, "probe_math_f64");
    return AZD_OK;
}
} // extern "C"
