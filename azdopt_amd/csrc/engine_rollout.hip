// engine_rollout.hip -- the roll-out driver: the launch steps the forms share, the searcher-only pool step, the pool step's split
// and evaluator groups, the step plan and its runners, the run-ahead window.
#include "engine_impl.h"

static uint32_t host_ordf(float f) { // tree_core.inc ordf
    f = f + 0.0f;
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static bool pool_feedback_on() { return knob_int("AZD_POOL_FEEDBACK", 1) != 0; }
static int fill_tol(TolTable &t, const uint32_t *tol, int n_tol, uint32_t dflt) {
    if (n_tol < 0 || n_tol > MAX_TOL || (n_tol > 0 && !tol)) return AZD_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < MAX_TOL; ++i) t.tol[i] = i < n_tol ? tol[i] : dflt;
    t.n_tol = n_tol;
    t.tol_default = dflt;
    return AZD_OK;
}

extern "C" {

// optimizer/mod.rs:159-174
int azd_engine_roll_out_begin(azd_engine *e, const uint32_t *tol, int n_tol, uint32_t dflt) {
    if (!e || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    azd::TolTable t;
    AZD_ST(fill_tol(t, tol, n_tol, dflt));
    e->time_begin(0);
    e->ops->rollout(e->a, t, e->stream);
    e->time_end();
    return sync_status(e);
}
// optimizer/mod.rs:177-190
int azd_engine_roll_out_end(azd_engine *e, const float *h_theta, int *improved) {
    if (!e || !h_theta || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipMemcpyAsync(e->a.h_theta, h_theta, (size_t)e->a.B * e->a.A * 4, hipMemcpyHostToDevice, e->stream));
    e->ops->add_actions(e->a, 0, e->stream);
    e->ops->argmin(e->a, 0, e->stream);
    return report_improved(e, sync_status(e), improved);
}
// Evaluator groups (pool_step.inc: pool_eval_group): which member keeps which column tile of which layer in its LDS.
// Greedy by size: the largest tiles first, each to the member that holds the fewest bytes so far and fewer than W tiles of that
// layer.  The smallest group (a multiple of 8 workgroups) and the fewest waves per slot that fit the LDS are taken: a batch's
// latency does not depend on g (a layer is one tile's MFMA chain per wave either way), the number of groups the CUs make does.
struct GroupPlan {
    int g = 0, W = 0;
    size_t lds_bytes = 0;      // the fullest member's
    uint32_t xstride = 0;      // floats per exchange buffer
    std::vector<int16_t> tile; // [L][g][W]
    std::vector<uint32_t> lds; // [L][g][W]
};
static bool plan_groups(const azd::FusedEval &fe, size_t lds_budget, int avail_wgs, int force_g, GroupPlan *out) {
    const int L = fe.n_layers;
    if (L < 1 || L > 7 || fe.bf16) return false;
    std::vector<int> tiles(L), steps(L);
    int max_tiles = 0;
    uint32_t xs = 0;
    for (int l = 0; l < L; ++l) {
        steps[l] = (fe.dims[l] + 15) / 16;
        tiles[l] = (fe.dims[l + 1] + 15) / 16;
        max_tiles = std::max(max_tiles, tiles[l]);
        if (l < L - 1) xs = std::max<uint32_t>(xs, (uint32_t)tiles[l] * 256u);
        if (l < L - 1 && fe.dims[l + 1] % 16 != 0) return false; // a hidden layer's output is the next layer's whole k-steps
    }
    // the fewest waves per slot first (W = 1: sixteen batch slots per group), then the smallest group that fits the LDS and leaves
    // room for two groups (config A: W = 1 needs g = 64 of the 192 CUs the searchers leave: 5.7 M expansions/s against 5.2 at g = 40, W = 2)
    for (int W : {1, 2, 4})
    for (int g = force_g > 0 ? force_g : 8; g <= avail_wgs && g <= 128; g += 8) {
        {
            if (force_g <= 0 && W < 4 && 2 * g > avail_wgs) break; // (a lone group only as the last resort)
            if ((max_tiles + g - 1) / g > W) {
                if (force_g > 0) break; // (a forced size is tried with every W, never enlarged)
                continue;
            }
            struct Item { int l, t; size_t bytes; };
            std::vector<Item> items;
            for (int l = 0; l < L; ++l)
                for (int t = 0; t < tiles[l]; ++t) items.push_back({l, t, (size_t)steps[l] * 1024});
            std::stable_sort(items.begin(), items.end(), [](const Item &x, const Item &y) { return x.bytes > y.bytes; });
            std::vector<size_t> load((size_t)g, 0);
            std::vector<int> cnt((size_t)L * g, 0);
            std::vector<int16_t> tile((size_t)L * g * W, (int16_t)-1);
            std::vector<uint32_t> lds((size_t)L * g * W, 0u);
            bool ok = true;
            for (const Item &it : items) {
                int best = -1;
                for (int m = 0; m < g; ++m)
                    if (cnt[(size_t)it.l * g + m] < W && (best < 0 || load[(size_t)m] < load[(size_t)best])) best = m;
                if (best < 0 || load[(size_t)best] + it.bytes > lds_budget) {
                    ok = false;
                    break;
                }
                const int w = cnt[(size_t)it.l * g + best]++;
                tile[((size_t)it.l * g + best) * W + w] = (int16_t)it.t;
                lds[((size_t)it.l * g + best) * W + w] = (uint32_t)load[(size_t)best];
                load[(size_t)best] += it.bytes;
            }
            if (!ok) {
                if (force_g > 0) break;
                continue;
            }
            out->g = g;
            out->W = W;
            out->lds_bytes = *std::max_element(load.begin(), load.end());
            out->xstride = xs ? xs : 256u;
            out->tile = tile;
            out->lds = lds;
            return true;
        }
        if (force_g > 0) break;
    }
    return false;
}

// ---- launch steps the roll-out forms share
// The argument block of the CU-resident forms, re-sent only when it changed (per-launch values are kernel arguments).
static int send_pargs(azd_engine *e, const azd::Arenas &arenas, const azd::TolTable &tol, const azd::FusedEval &fe, const azd::PoolArgs &pool) {
    azd::PersistArgs now;
    memset(&now, 0, sizeof(now)); // (padding bytes compare equal)
    now.a = arenas;
    now.tol = tol;
    now.ev = fe;
    now.ev.call_base = (fe.kind == 2 || fe.kind == 4) ? e->ev->calls : 0; // hash stream: index of the launch's first call
    now.pool = pool;
    if (e->pargs_valid && memcmp(&e->pargs_sent, &now, sizeof(now)) == 0) return AZD_OK;
    AZD_HIP(hipStreamSynchronize(e->stream)); // the pinned block may still be in flight from the copy before
    memcpy(e->h_pargs, &now, sizeof(now));
    AZD_HIP(hipMemcpyAsync(e->d_pargs, e->h_pargs, sizeof(azd::PersistArgs), hipMemcpyHostToDevice, e->stream));
    memcpy(&e->pargs_sent, &now, sizeof(now));
    e->pargs_valid = true;
    return AZD_OK;
}
// The per-call log starts a launch with all ones; the launches that replay it (k_argmin_log1, argmin_log) leave it so.
static int ensure_log_clean(azd_engine *e) {
    if (e->log_clean) return AZD_OK;
    AZD_HIP(hipMemsetAsync(e->d_log_key, 0xFF, (size_t)e->log_calls * sizeof(unsigned long long), e->stream));
    e->log_clean = true;
    return AZD_OK;
}
static azd::StepLaunch step_launch(const azd_engine *e, int k, azd::PoolCtl *ctl, const uint32_t *resume, bool hashed, bool window = false, bool groups = false) {
    azd::StepLaunch sl;
    sl.n_calls = k;
    sl.log_key = e->d_log_key;
    sl.resume = resume;
    sl.ctl = ctl;
    sl.hashed = hashed ? 1 : 0;
    sl.window = window ? 1 : 0;
    sl.groups = groups ? 1 : 0;
    return sl;
}
// What `body` launches on `stream`, captured and instantiated as *exec; body's own status comes first, the template graph always goes.
static int capture_graph(hipStream_t stream, const std::function<int()> &body, azd::GraphExec *exec) {
    hipGraph_t g = nullptr;
    hipGraphExec_t x = nullptr;
    AZD_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    const int st = body();
    const hipError_t he = hipStreamEndCapture(stream, &g);
    if (st) {
        if (g) (void)hipGraphDestroy(g);
        return st;
    }
    if (he != hipSuccess) return azd::hip_fail(he, "hipStreamEndCapture");
    const hipError_t hi = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (hi != hipSuccess) return azd::hip_fail(hi, "hipGraphInstantiate");
    exec->adopt(x);
    return AZD_OK;
}

static int pool_clear(azd_engine *e, const azd::PoolArgs &pool) { // empty queues, nobody claimed, no call done
    AZD_HIP(hipMemsetAsync(pool.ctl, 0, sizeof(azd::PoolCtl), e->stream));
    AZD_HIP(hipMemsetAsync(pool.ready_slots, 0, e->pool_slot_words * sizeof(uint32_t), e->stream));
    AZD_HIP(hipMemsetAsync(pool.join, 0, (size_t)e->a.B * sizeof(uint32_t), e->stream));
    e->pool_clean = true;
    return AZD_OK;
}

// What follows a pool launch of k calls on the host: its status block (the two sides' busy shares, for the split feedback) and
// -- when a wait ran into its bound -- the take-over.
// A wait that ran into its bound ends a pool launch instead of hanging it (PoolCtl::abort; k_argmin_log1 has put the flag into
// the status block and left the log alone).  The trees are consistent -- a wave never leaves an agent inside a call -- so the
// asynchronous step, whose workgroups need no company, takes the launch over where every agent stands, and this engine stays
// with it (*took_over; the asynchronous step's LDS plan in *as_out / *ab_out).
static int pool_finish_launch(azd_engine *e, const azd::FusedEval &fe, const azd::PoolArgs &pool, int k, bool *took_over,
                              uint32_t *as_out, size_t *ab_out) {
    *took_over = false;
    AZD_ST(fetch_status(e));
    if (e->h_status->pool_ticks > 0 && !e->h_status->pool_abort) {
        const double T = (double)e->h_status->pool_ticks;
        e->pool_util_eval = e->pool_eval_wgs > 0 ? (double)e->h_status->pool_eval_busy / (T * e->pool_eval_wgs) : 0.0;
        e->pool_util_search = e->pool_search_waves > 0 ? (double)e->h_status->pool_search_busy / (T * e->pool_search_waves) : 0.0;
    }
    if (!e->h_status->pool_abort) return AZD_OK;
    e->pool_clean = false;
    e->log_clean = false; // (it holds the aborted launch's candidates, which the take-over's replay needs: not cleared here)
    e->pool_failed = true;
    e->pool_step = false;
    uint32_t as = 0;
    size_t ab = 0;
    const char *why_t = "";
    if (!e->ops->async_plan(e->a, fe, &as, &ab, &why_t)) {
        e->time_collect();
        azd::g_last_error = std::string("pool step: a queue wait ran into its bound, and the asynchronous step cannot take over: ") + why_t;
        return AZD_ERR_UNREACHABLE;
    }
    azd::launch_pool_resume_scan(e->a, pool, k, e->d_resume, e->stream);
    AZD_ST(pool_clear(e, pool));
    const azd::StepLaunch sl = step_launch(e, k, nullptr, e->d_resume, fe.kind == 4);
    e->time_begin(0);
    e->ops->launch_async(e->a, e->d_pargs, sl, fe.params, fe.wpk, as, ab, e->stream);
    e->time_end();
    e->log_clean = true; // k_argmin_log1 has replayed and cleared it
    e->step_form = AZD_STEP_ASYNC;
    e->step_reason = "pool step aborted (a queue wait ran into its bound: no evaluator or searcher workgroup made progress); "
                     "the asynchronous step took the launch over and serves this engine from here on";
    *took_over = true;
    *as_out = as;
    *ab_out = ab;
    return AZD_OK;
}

// The pool step of the dense-graph space (BASELINE configs[4]): searcher workgroups only (k_pool_search) on part of the chip; the
// model -- too large for an evaluator workgroup's LDS -- is served by batched GEMM launches over the rows the searchers have posted,
// replayed from a graph on a second stream for as long as the searchers run.  Agents advance independently, so a launch no longer
// lasts as long as its slowest agent per call (launch-per-phase form: a roll-out launch took 1.2 ms where the mean agent needed 0.06).
// The Ramsey tiers with max_slots > 0 run the same form under AZD_ENGINE_EXT_POOL_STEP: what differs between the engines that have
// it comes from e->ops (PoolSearchOps: the searcher kernel's entries and its wavefronts per workgroup) and e->ext (ExtPoolForm: knobs and reason strings).
struct ExtPlan { // one roll-out of the form, as ext_plan decided it
    azd::Arenas a;     // what the searchers and the evaluator's graph see
    azd::FusedEval fe; // what the searchers look at
    azd::PoolArgs pool;
    bool hashed, f32_rows;
    const char *r_needs_rows;
    int waves, n_search, n_ext;
    uint32_t dyn_stride;
    size_t dyn_bytes;
};
// *runs = false: the form cannot run here (why in e->step_reason).  A knob that asks for what cannot run is an error.
static int ext_plan(azd_engine *e, int n_calls, ExtPlan *out, bool *runs) {
    *runs = false;
    const ExtPoolForm &xf = *e->ext;
    // what the searchers and the evaluator's graph see: a flagged Ramsey engine's bf16 rows exist for this form only (azd_engine::ext_s16)
    azd::Arenas ax = e->a;
    if (e->ext_s16) {
        ax.state_vecs16 = e->ext_s16;
        ax.S16 = e->ext_s16_pitch;
    }
    const azd::Arenas &a = ax;
    // AZD_ENGINE_EXT_POOL_F32: the evaluator's graph may read the f32 rows, which the searchers always write (write_rows_direct), so
    // the form runs without bf16 rows; which of the two gathered forwards is captured is the evaluator's answer (its storage type).
    // On the dense-graph space the flag stands alone and is a request to the configured pool step: the plan below is the one a
    // bf16 model gets (the searchers do not know which evaluator serves them), and where the pool step is not configured
    // (`configured` below) nothing changes.
    const bool f32_rows = e->ext_f32;
    const char *const r_needs_rows = f32_rows ? xf.r_needs_rows : xf.r_needs_bf16;
    if (f32_rows && e->ext_unsupported && e->ext_unsupported_layout != e->ev->layout_version) e->ext_unsupported = false;
    const char *why = "";
    uint32_t dyn_stride = 0;
    size_t dyn_bytes = 0;
    // wavefronts per searcher workgroup: 16, or as many as the LDS holds (roots of more than 640 slots: 12 -- a wave's block and its
    // selection scratch are 12 KB there)
    // (the Ramsey tiers: 8, the bound their kernels are built for -- every shape the tiers accept fits)
    int waves = knob_int(xf.env_waves, e->ops->waves_max);
    if (waves < xf.waves_min || waves > xf.waves_knob_max) { // (round-4 verdict, 7c: a knob out of range is refused, not silently bent)
        azd::g_last_error = xf.e_waves_range;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    const bool knobs = getenv(xf.env_wgs) || getenv(xf.env_waves);
    auto pool_plan = e->ops->pool_search_plan;
    while (waves > xf.waves_min && !pool_plan(a, waves, &dyn_stride, &dyn_bytes, &why)) waves -= 1;
    azd::FusedEval fe;
    const bool hashed = e->ev->fused_desc(&fe) && fe.kind == 4; // the test harness' fixed prediction stream, served like a model's rows
    const bool configured = (e->pool_step || !xf.needs_pool_step) && e->persist_enabled;
    if (!configured || e->pool_failed || e->ext_unsupported || (!a.state_vecs16 && !hashed && !f32_rows) ||
        n_calls < 1 || !pool_plan(a, waves, &dyn_stride, &dyn_bytes, &why)) {
        e->step_reason = !configured       ? xf.r_not_configured
                         : e->pool_failed ? xf.r_failed_before
                         : ((!a.state_vecs16 && !hashed && !f32_rows) || e->ext_unsupported) ? r_needs_rows
                                                                                 : why;
        return AZD_OK;
    }
    const int per_cu = e->ops->pool_search_resident(a, waves, dyn_bytes);
    // searcher workgroups: no more waves than twice the agents, and no more than half the chip's wave slots -- the GEMM launches
    // need the rest
    int n_search = (2 * a.B + waves - 1) / waves;
    if (n_search > e->n_cus * 8 / waves) n_search = e->n_cus * 8 / waves;
    if (xf.keep_quarter_free && n_search > e->n_cus - e->n_cus / 4) n_search = e->n_cus - e->n_cus / 4;
    n_search = knob_pos(xf.env_wgs, n_search);
    // The evaluator of this form is a stream of GEMM LAUNCHES beside the searchers' persistent kernel: they run only where a CU has
    // LDS and registers left, and a searcher workgroup (1024 threads' worth of LDS blocks) leaves none.  A setting of the two knobs
    // that lets the searchers cover more than three quarters of the CUs used to be accepted and then cost a 4-s wait bound, an
    // abort and the engine's demotion to the launch-per-phase form (gpurun_out/ew.txt, round 4): refused up front instead.
    // (workgroups, not wave slots: the dispatcher deals one workgroup to every CU before it doubles up, so 256 workgroups of 8 waves
    // sit on 256 CUs although two would fit one)
    if (per_cu >= 1 && knobs && n_search > e->n_cus - e->n_cus / 4) {
        static thread_local char msg[256];
        snprintf(msg, sizeof msg, "%s / %s: %d searcher workgroups of %d waves would sit on %d of %d CUs; "
                 "the evaluator's GEMM launches need at least a quarter of the chip free (at most %d workgroups)", xf.env_wgs, xf.env_waves, n_search, waves,
                 n_search < e->n_cus ? n_search : e->n_cus, e->n_cus, e->n_cus - e->n_cus / 4);
        azd::g_last_error = msg;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (per_cu < 1 || n_search > e->n_cus * per_cu * 7 / 8) n_search = per_cu < 1 ? 0 : e->n_cus * per_cu * 7 / 8;
    if (n_search < 1) {
        e->step_reason = xf.r_no_wg;
        return AZD_OK;
    }
    // (one stream by default: with two, each batch is half as large and takes as long -- the GEMMs' k loops are latency-bound at these
    // batch sizes and the streams share the same CUs -- so an agent's cycle, which sets the rate, gets no shorter: 18.8 M expansions/s
    // with one stream against 17.8 with two at config E)
    int n_ext = knob_int(xf.env_streams, xf.streams);
    n_ext = n_ext < 1 ? 1 : n_ext > azd_engine::EXT_STREAMS ? azd_engine::EXT_STREAMS : n_ext;
    azd::PoolArgs pool = e->pool;
    pool.n_eval = 0;
    pool.ready_lanes = 0;
    pool.n_express = 0;
    pool.express_waves = 0;
    pool.express_shift = 0;
    pool.early_post = knob_int("AZD_POOL_EARLY_POST", xf.early_post);
    pool.eval_stride = pool.eval_out_off = 0;
    pool.eval_rows = 0;
    pool.debug_abort_call = (uint32_t)knob_int("AZD_POOL_DEBUG_ABORT_CALL", 0); // test hook: k_ext_deliver
    if (!hashed) {
        memset(&fe, 0, sizeof(fe));
        fe.kind = 3; // what the searchers look at: requests are posted for an evaluator
    }
    *out = ExtPlan{ax, fe, pool, hashed, f32_rows, r_needs_rows, waves, n_search, n_ext, dyn_stride, dyn_bytes};
    *runs = true;
    return AZD_OK;
}
// the evaluator's graphs, one per stream: collect, the layers over the collected rows, hand back.  Every stream may find the
// whole population posted, so each has row lists and activation rows of its own.
// *served = false: the evaluator cannot serve gathered rows (why in e->step_reason; asked once per layout).
static int ext_graphs(azd_engine *e, const ExtPlan &xp, bool *served) {
    *served = true;
    if (!xp.hashed) AZD_ST(e->ev->ensure_rows(xp.n_ext * xp.a.B));
    int rounds = knob_int(e->ext->env_rounds, 4); // collect / layers / hand-back rounds per replay of the evaluator's graph
    rounds = rounds < 1 ? 1 : rounds > 16 ? 16 : rounds;
    const uint64_t layout = e->ev->layout_version + (xp.hashed ? 1ull << 63 : 0ull) + ((uint64_t)rounds << 56);
    if (e->ext_graph_n != xp.n_ext || e->ext_graph_layout != layout) {
        for (azd::GraphExec &g : e->ext_graph) g.reset();
        e->ext_graph_n = 0;
        for (int x = 0; x < xp.n_ext; ++x) {
            uint32_t *rows = e->d_ext_rows + (size_t)x * xp.a.B, *home = e->d_ext_home + (size_t)x * xp.a.B, *cnt = e->d_ext_n + x;
            const int st_x = capture_graph(e->ext_stream[x], [&]() -> int {
                int st_g = AZD_OK;
                // several rounds per graph: between two graphs on a stream the GPU idles ~18 us, between two kernels of one graph not at all
                for (int r = 0; r < rounds && st_g == AZD_OK; ++r) {
                    azd::launch_ext_take(xp.pool, rows, home, cnt, e->d_ext_t0 + x, e->ext_stream[x]);
                    if (xp.hashed) azd::launch_ext_hash_rows(e->d_pargs, rows, cnt, (uint32_t)xp.a.B, xp.a.h_theta, e->ext_stream[x]);
                    else {
                        st_g = xp.a.state_vecs16 ? e->ev->write_predictions_gathered(rows, cnt, xp.a.B, xp.a.state_vecs16, xp.a.S16, xp.a.h_theta, e->ext_stream[x], x * xp.a.B)
                                              : AZD_ERR_UNSUPPORTED;
                        if (st_g == AZD_ERR_UNSUPPORTED && xp.f32_rows) // (asked before anything is launched: a refusal leaves the capture empty)
                            st_g = e->ev->write_predictions_gathered_f32(rows, cnt, xp.a.B, xp.a.state_vecs, xp.a.S, xp.a.h_theta, e->ext_stream[x], x * xp.a.B);
                    }
                    azd::launch_ext_deliver(xp.pool, xp.a, rows, home, cnt, (uint32_t)xp.a.B, e->d_ext_t0 + x, e->ext_stream[x]);
                }
                return st_g;
            }, &e->ext_graph[x]);
            if (st_x == AZD_ERR_UNSUPPORTED) {
                e->ext_unsupported = true;
                e->ext_unsupported_layout = e->ev->layout_version;
                e->step_reason = xp.r_needs_rows;
                *served = false;
                return AZD_OK;
            }
            if (st_x) return st_x;
        }
        e->ext_graph_n = xp.n_ext;
        e->ext_graph_layout = layout;
    }
    return AZD_OK;
}
// A wait ran into its bound (nothing made progress for 4 s: the GEMM launches never got CUs, say).  The trees are
// consistent -- a wave never leaves an agent inside a call -- but the agents stand at different calls.  No other
// CU-resident form of this space exists to take the launch over, so the launch-per-phase kernels complete it: agent by
// agent from where each one stands (k_pool_resume_scan), the ones that are through sitting out (FLAG_PARKED), every
// candidate logged under the call it really belongs to, one replay of the log at the end -- the results of an
// undisturbed launch.  This engine stays with the launch-per-phase form.
// (the engine's own arenas from here on: a flagged Ramsey engine's launch-per-phase kernels write no bf16 rows, so the
// evaluator is handed none and converts the f32 rows -- ext_s16 above)
static int ext_recover(azd_engine *e, const azd::TolTable &t, const ExtPlan &xp, int k) {
    const azd::Arenas &a = e->a;
    e->pool_failed = true;
    e->log_clean = false;
    azd::launch_pool_resume_scan(a, xp.pool, k, e->d_resume, e->stream);
    std::vector<uint32_t> res((size_t)a.B);
    AZD_HIP(hipMemcpyAsync(res.data(), e->d_resume, res.size() * 4, hipMemcpyDeviceToHost, e->stream));
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_ST(pool_clear(e, xp.pool));
    int rounds = 0;
    bool any_pending = false;
    for (uint32_t r : res) {
        const int rem = k - (int)(r & 0x7FFFFFFFu);
        rounds = rem > rounds ? rem : rounds;
        any_pending = any_pending || (r >> 31) != 0u;
    }
    auto evaluate_rows = [&]() -> int {
        if (xp.hashed) { // the fixed stream's rows depend on the call: not reproducible outside the launch that posted them
            azd::g_last_error = e->ext->e_abort_hashed;
            return AZD_ERR_UNREACHABLE;
        }
        const uint64_t calls_before = e->ev->calls;
        const int s2 = e->ev->write_predictions_dev16(a.B, a.state_vecs, a.state_vecs16, a.S16, a.h_theta, e->stream);
        e->ev->calls = calls_before;
        return s2;
    };
    if (any_pending) { // the rows that were still due, and add_actions for the nodes waiting for them
        azd::launch_park(a, e->d_resume, k, -1, 1, e->stream);
        AZD_ST(evaluate_rows());
        e->ops->add_actions(a, 0, e->stream);
    }
    for (int r = 0; r < rounds; ++r) {
        azd::launch_park(a, e->d_resume, k, r, 1, e->stream);
        e->ops->rollout(a, t, e->stream);
        AZD_ST(evaluate_rows());
        e->ops->add_actions(a, 0, e->stream);
        azd::launch_log_candidates_resume(a, e->d_log_key, e->d_resume, k, r, e->stream);
    }
    azd::launch_park(a, e->d_resume, k, 0, 0, e->stream); // everyone back
    e->ops->argmin_log(a, k, e->d_log_key, e->stream);  // replays the k calls and leaves the log clean
    e->log_clean = true;
    AZD_HIP(hipGetLastError());
    AZD_ST(fetch_status(e));
    e->step_form = AZD_STEP_PER_CALL;
    e->step_reason = e->ext->r_aborted;
    return AZD_OK;
}
// The launches of one roll-out and, beside each, the replays of the evaluator's graphs.  *left_out: see ext_pool_run.
static int ext_run_launches(azd_engine *e, const azd::TolTable &t, int n_calls, const ExtPlan &xp, int *left_out) {
    const ExtPoolForm &xf = *e->ext;
    int depth = knob_int(xf.env_depth, e->ext_depth);
    depth = depth < 1 ? 1 : depth > azd_engine::EXT_IN_FLIGHT ? azd_engine::EXT_IN_FLIGHT : depth;
    int left = n_calls;
    while (left > 0) {
        const int k = left < e->log_calls ? left : e->log_calls;
        AZD_ST(send_pargs(e, xp.a, t, xp.fe, xp.pool));
        AZD_ST(pool_clear(e, xp.pool)); // (always: a collect that ran past the end of the last launch may have touched the control block)
        AZD_ST(ensure_log_clean(e));
        AZD_HIP(hipMemsetAsync(e->d_ext_n, 0, sizeof(uint32_t) * azd_engine::EXT_STREAMS, e->stream));
        AZD_HIP(hipEventRecord(e->ext_fork, e->stream));
        for (int x = 0; x < xp.n_ext; ++x) AZD_HIP(hipStreamWaitEvent(e->ext_stream[x], e->ext_fork, 0)); // the first collect sees the cleared queues
        const azd::StepLaunch sl = step_launch(e, k, xp.pool.ctl, nullptr, xp.hashed);
        e->time_begin(0);
        e->ops->launch_pool_search(xp.a, e->d_pargs, sl, xp.n_search, xp.waves, xp.dyn_stride, xp.dyn_bytes, e->stream);
#ifndef AZD_PHASE_PROFILE
        e->counters_by_wave = true;
#endif
        e->time_end();
        AZD_HIP(hipGetLastError());
        AZD_HIP(hipEventRecord(e->ext_done, e->stream));
        e->pool_clean = false;
        // the evaluator: replayed, stream after stream, until the searchers (and the argmin replay behind them) are through; ext_depth
        // replays queued per stream at a time -- a replay that finds nothing posted costs a few microseconds
        unsigned long long it = 0;
        for (;;) {
            const hipError_t q = hipEventQuery(e->ext_done);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) return azd::hip_fail(q, "hipEventQuery");
            const int x = (int)(it % (unsigned long long)xp.n_ext);
            const unsigned long long round = it / (unsigned long long)xp.n_ext;
            hipEvent_t slot = e->ext_ring[x][round % (unsigned long long)depth];
            if (round >= (unsigned long long)depth) AZD_HIP(hipEventSynchronize(slot));
            AZD_HIP(hipGraphLaunch(e->ext_graph[x], e->ext_stream[x]));
            AZD_HIP(hipEventRecord(slot, e->ext_stream[x]));
            it += 1;
        }
        for (int x = 0; x < xp.n_ext; ++x) AZD_HIP(hipStreamSynchronize(e->ext_stream[x]));
        e->ext_iterations += it;
        if (getenv(xf.env_debug)) fprintf(stderr, "%s: %d calls, %d searcher workgroups, %llu evaluator replays\n", xf.debug_tag, k, xp.n_search, it);
        left -= k;
        e->ev->calls += (uint64_t)k;
        AZD_ST(fetch_status(e));
        if (e->h_status->pool_ticks > 0) {
            const double T = (double)e->h_status->pool_ticks;
            e->pool_util_eval = (double)e->h_status->pool_eval_busy / (T * xp.n_ext); // the share of the launch an evaluator stream held a batch
            e->pool_util_search = (double)e->h_status->pool_search_busy / (T * e->pool_search_waves);
            // (A controller on these two shares, as for the in-kernel evaluator, was measured and not kept: over whole epochs the rate is flat
            // between 112 and 160 searcher workgroups -- config E 19.7-20.0 M expansions/s, 612-slot roots 10.2-10.3 M.)
        }
        if (e->h_status->pool_abort) {
            *left_out = left;
            return ext_recover(e, t, xp, k);
        }
    }
    return AZD_OK;
}
// *ran = false: the form cannot run here (why in e->step_reason) and the caller takes the launch-per-phase form.
// *left_out: calls still to run when an aborted launch had to be completed by the launch-per-phase kernels (the caller runs them).
static int ext_pool_run(azd_engine *e, const azd::TolTable &t, int n_calls, bool *ran, int *left_out) {
    *ran = false;
    *left_out = 0;
    ExtPlan xp;
    bool go = false; // (the plan runs / the evaluator serves its rows)
    int st = ext_plan(e, n_calls, &xp, &go);
    if (st || !go) return st;
    if (!e->ext_done) AZD_ST(e->ext_done.create(hipEventDisableTiming));
    if (!e->ext_fork) AZD_ST(e->ext_fork.create(hipEventDisableTiming));
    for (int x = 0; x < xp.n_ext; ++x) {
        if (!e->ext_stream[x]) AZD_ST(e->ext_stream[x].create(hipStreamNonBlocking));
        for (int i = 0; i < azd_engine::EXT_IN_FLIGHT; ++i)
            if (!e->ext_ring[x][i]) AZD_ST(e->ext_ring[x][i].create(hipEventDisableTiming));
    }
    st = ext_graphs(e, xp, &go);
    if (st || !go) return st;
    e->step_form = AZD_STEP_POOL;
    e->step_reason.clear();
    e->pool_eval_wgs = 0;
    e->pool_search_wgs = xp.n_search;
    e->pool_search_waves = xp.n_search * xp.waves;
    e->ext_iterations = 0;
    AZD_ST(ext_run_launches(e, t, n_calls, xp, left_out));
    *ran = true;
    return AZD_OK;
}
// The AZD_POOL_* knobs of the split (read in plan_step).  0: not set, where a positive value overrides; KNOB_UNSET where any integer does.
struct PoolKnobs { int eval_wgs, search_wgs, ready_lanes, express_wgs, express_waves, express_shift, early_post; };
// Split of the CUs between the two roles, in proportion to the CU time a row costs an evaluator and a call costs
// the searchers.  AZD_POOL_EVAL_WGS / AZD_POOL_SEARCH_WGS override (experiments).
// A function of its arguments alone (tests/test_gpu_pool_split.py pins what it gives on an MI355X): capacity = the workgroups the device holds at once,
// fb_n_eval = the feedback controller's wish (0: none).  Returns the searcher workgroups (none: no room for one of each); everything else goes into *pool.
static int pool_split(int n_cus, const azd::Arenas &a, const azd::FusedEval &fe, int n_calls, int capacity, int fb_n_eval, const PoolKnobs &k, azd::PoolArgs *pool) {
    const int B = a.B;
    int cap = 0; // (set below, with the measurement behind it)
    auto clamp_eval = [&](int v) { // at most `cap`; at most half the chip, or whatever the searchers of a small population leave; one at least
        const int want_search = (B + 7) / 8;
        const int most = want_search < n_cus / 2 ? n_cus - want_search : n_cus / 2;
        v = v > cap ? cap : v;
        v = v > most ? most : v;
        return v < 1 ? 1 : v;
    };
    int n_eval = 0;
    if (fe.kind >= 3) {
        double flop = 0;
        if (fe.kind == 3)
            for (int l = 0; l < fe.n_layers; ++l) flop += 2.0 * fe.dims[l] * fe.dims[l + 1];
        else flop = 2.0 * 256.0 * (a.S + 512.0 + a.A); // hashed rows (test harness): the split a 3 x 256 model would get
        // measured (profiles/r02_pool_probe.txt): a 16-row fp32 batch of the 3 x 256 MLP takes 25 us of an evaluator
        // CU, bf16 storage 16 us; pure search 4.65 us of a CU per call on young trees.  Whole epochs (older, larger
        // trees) want a few more evaluators than that ratio says: best 88-100 of 256 at 4096 agents fp32, 80 at 8192,
        // 56 at 8192 bf16 (gpurun sweeps r2c/sw_*), which the constants below reproduce
        const double eval_us_per_row = flop / (256.0 * 2400.0) / (fe.bf16 ? 1.85 : 1.0) / 0.33;
        // (a Ramsey call costs the searchers less: no lambda_1, five selections per expansion against eleven; best 126 of 256
        // for config D, 113 cost 10 %, 134 5 % -- gpurun sweep r2m/D_*)
        // (round 4: a c21 call costs the searchers a quarter less -- one round trip per selection level, 3.6 rounds of lambda_1 -- and the
        // measured-feedback split settles at 100-105 of 256 where it used to settle at 89-96; a first guess of 88 cost a process that
        // makes few launches -- the bench's 20-call window -- 8 %: 27.0 against 29.4 M expansions/s at 88 / 104 evaluator workgroups)
        const double search_us_per_call = a.space == azd::SPACE_RAMSEY ? 3.6 : 3.65;
        n_eval = (int)(n_cus * eval_us_per_row / (eval_us_per_row + search_us_per_call) + 0.5);
        // populations well beyond the searching waves keep the evaluator queues deep enough for 32-row batches (two row
        // tiles per weight fragment, where they fit the LDS), which cost an evaluator 1.2 us per row instead of 1.6:
        // best 76-84 of 256 at 8192 agents fp32 (88-92 at 4096), 50-58 at 8192 bf16 (gpurun sweeps r2m/B8_*, C_*)
        if (pool->eval_rows > 16 && B >= 6144) n_eval = (int)(n_eval * 0.91 + 0.5);
        // small populations leave CUs free (the searchers need no more waves than twice the agents): evaluators may take
        // them down to ~4 rows per batch -- rows then rarely queue behind a running batch (config A, 512 agents and a
        // 2.5 MFLOP model: 33 / 64 / 128 evaluator workgroups -> 2.70 / 2.92 / 3.09 M expansions/s; gpurun r2t/A_*)
        cap = (B + 3) / 4 + 1;
        n_eval = clamp_eval(n_eval);
        if (fb_n_eval > 0) n_eval = clamp_eval(fb_n_eval); // the split the last launches' busy shares ask for, under the same caps
        // a SHORT launch is fill and drain (its length is its slowest agents' few calls, each with an evaluator round trip in it): a seventh
        // more evaluator workgroups than the busy shares of whole epochs ask for -- bench.py --steps 20, 4096 agents, same box, four
        // alternating runs each: 104 workgroups 27.7 / 28.6 / 30.1 / 29.4 M expansions/s, 116: 29.9 / 29.2 / 29.3 / 29.8, 124: 29.5 / 29.8 /
        // 29.6 / 29.6 (round 5; the launch over its median agent 1.50 -> 1.44 -> 1.37)
        if (n_calls <= 64 && fe.kind == 3) n_eval = clamp_eval(n_eval + n_eval / 7);
        if (k.eval_wgs > 0) n_eval = k.eval_wgs;
    }
    int n_search = n_cus - n_eval;
    const int want = (B + 7) / 8; // no more waves than twice the agents: a wave without an agent only polls
    n_search = n_search > want ? want : n_search;
    n_search = n_search < 1 ? 1 : n_search;
    if (k.search_wgs > 0) n_search = k.search_wgs;
    // Searcher and evaluator workgroups spin-wait on each other: every one of them must be RESIDENT, whatever the overrides
    // above ask for and whatever the device can hold (a CU mask, a partition, another kernel's LDS).  Clamp the grid to the
    // co-resident capacity the runtime reports, evaluators first (they are dispatched first: a grid of evaluators alone
    // would never let a searcher in); with no room for one of each the call takes the asynchronous step instead.
    if (fe.kind < 3) n_eval = 0; // TrivialModel / in-wave hash stream: nothing to serve
    if (n_eval + n_search > capacity) {
        if (n_eval > capacity / 2) n_eval = capacity / 2;
        if (fe.kind >= 3 && n_eval < 1) n_eval = 1;
        n_search = capacity - n_eval;
    }
    pool->n_eval = n_eval;
    // With more agents than searching waves an agent's cycle is mostly waiting for a wave (92 of 179 us at 8192 agents);
    // in lane mode the agents behind the mean progress are taken first, so that the slow chains do not also queue.
    // (lane mode: measured +4 % at 8192 agents fp32, -4 % at config C, +-0 at config D -- within run-to-run noise: those
    // populations are bound by the searchers' capacity, not by the order they are served in.  Off unless asked for.)
    pool->ready_lanes = k.ready_lanes;
    // Express mode (default with a model evaluator and a chip-sized grid): one searcher workgroup per XCD serves only the
    // agents that lag behind the progress of their XCD's unfinished agents (by more than 1/16 of it), and every other wave
    // takes one of those first when more of them wait than express waves stand by.  A launch lasts as long as its slowest
    // agent's chain of calls; in that chain ~10 us per call were the agent waiting for a wave.  4096 agents fp32: 32.7-33.3
    // -> 34.1-34.6 M expansions/s over whole epochs, 25.4-25.7 -> 26.0 in a 20-call launch (gpurun r3 sweeps: 8 / 16 / 24
    // express workgroups, thresholds 1/4 .. 1/64, 4 / 8 / 16 waves each: 8-16 workgroups and 1/16-1/32 are the flat optimum,
    // the waves per workgroup do not matter -- what helps is the place in the queue, not the emptier CU).
    pool->n_express = (fe.kind >= 3 && n_search >= 64) ? 8 : 0;
    if (k.express_wgs != KNOB_UNSET) pool->n_express = k.express_wgs;
    int express_waves = k.express_waves;
    pool->express_shift = (uint32_t)k.express_shift;
    if (pool->n_express > n_search / 2) pool->n_express = n_search / 2;
    if (pool->n_express < 0) pool->n_express = 0;
    if (pool->ready_lanes != 1) pool->ready_lanes = (pool->n_express > 0 && fe.kind >= 3) ? 2 : 0;
    if (pool->ready_lanes != 2) pool->n_express = 0;
    if (express_waves < 1 || express_waves > 16) express_waves = 4;
    pool->express_waves = (uint32_t)express_waves;
    // Early post: the row leaves, and the evaluator is asked, before the wave computes the new node's cost and writes the
    // tree back (the agent is queued again by whoever is later, PoolArgs::join).  That takes ~15 us off an agent's cycle
    // and costs the wave a second drain of its stores (~1.5 us): +10 % where agents rarely wait for a wave (512..2048
    // agents, gpurun r2k/e_*), -3 % where the searchers' capacity is the bound (4096 agents and beyond).
    // Larger populations: only by a wave that had to wait for its agent (mode 2), which is the state of the last fifth of a
    // launch, when the slowest chains are all that is left.
    pool->early_post = (double)B <= 1.25 * n_search * 16 ? 1 : 2; // 16 waves per searcher workgroup
    // (a SHORT launch is fill and drain: its length is its slowest agent's few calls, not the searchers' capacity -- always early
    // there: 28.4 -> 29.05 M expansions/s in the driver's 20-call window, same-box A/B of two runs each, round 5)
    if (n_calls <= 64) pool->early_post = 1;
    if (k.early_post != KNOB_UNSET) pool->early_post = k.early_post;
    return n_search;
}

// ---- evaluator groups (pool_eval_group): where a classic batch is long -- a model whose weights one CU streams in tens of
// microseconds -- and the population small enough that a few groups carry its rows.  AZD_POOL_EVAL_GROUP = 0: never;
// = g: groups of g workgroups whatever the model (tests, experiments).  f32 weight storage only.
// `avail`: what the searchers leave of the resident capacity (>= n_eval: idle CUs of a small population included); with groups, pool->n_eval and *dyn_bytes are theirs.
static int ensure_eval_groups(azd_engine *e, const azd::FusedEval &fe, bool enabled, int avail, int force_knob, azd::PoolArgs *pool, size_t *dyn_bytes) {
    const int B = e->a.B;
    pool->grp_g = pool->grp_w = pool->grp_groups = 0;
    pool->grp_tile = nullptr;
    pool->grp_lds = nullptr;
    pool->grp_desc = pool->grp_cnt = nullptr;
    pool->grp_x = nullptr;
    pool->grp_flag = nullptr;
    pool->grp_xstride = 0;
    if (!enabled || fe.kind != 3 || fe.bf16 || e->a.space != azd::SPACE_C21 || (size_t)B * (size_t)e->a.S * 4 >= (1ull << 31)) return AZD_OK;
    double wbytes = 0;
    for (int l = 0; l < fe.n_layers; ++l) wbytes += 4.0 * fe.dims[l] * fe.dims[l + 1];
    int force_g = 0;
    bool want = wbytes > 2.5e6 && B <= 1536; // (measured with config A's model: groups 5.7 / 9.8 / 11.0 M expansions/s at 512 / 1024 / 2048 agents, the classic form 3.5 / 6.8 / 13.2)
    if (force_knob != KNOB_UNSET) {
        force_g = force_knob;
        want = force_g > 0;
    }
    GroupPlan gpl;
    if (!want || !plan_groups(fe, (size_t)160 * 1024 - 2048, avail, force_g, &gpl)) return AZD_OK;
    const int n_groups = std::max(1, avail / gpl.g);
    const int NS = 16 / gpl.W;
    const size_t slots = (size_t)n_groups * NS;
    EvalGroupMem &m = e->grp;
    // the groups' device memory and the two tables of the plan
    AZD_ST(m.ensure(e->stream, slots, slots * 2 * gpl.xstride, slots * gpl.g * 16));
    if (gpl.tile != m.tile_host || gpl.lds != m.lds_host) {
        AZD_HIP(hipStreamSynchronize(e->stream));
        AZD_HIP(hipMemcpy(m.tile, gpl.tile.data(), gpl.tile.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        AZD_HIP(hipMemcpy(m.lds, gpl.lds.data(), gpl.lds.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        m.tile_host = gpl.tile;
        m.lds_host = gpl.lds;
    }
    pool->grp_g = gpl.g;
    pool->grp_w = gpl.W;
    pool->grp_groups = n_groups;
    pool->grp_tile = m.tile;
    pool->grp_lds = m.lds;
    pool->grp_desc = m.desc;
    pool->grp_cnt = m.cnt;
    pool->grp_x = m.x;
    pool->grp_flag = m.flag;
    pool->grp_xstride = gpl.xstride;
    pool->n_eval = n_groups * gpl.g; // every evaluator workgroup is a group member
    if (gpl.lds_bytes > *dyn_bytes) *dyn_bytes = gpl.lds_bytes;
    return AZD_OK;
}

// What a runner needs of plan_step's decision, beside e->step_form.  Which form runs is part of the result a caller may want to check
// (azd_engine_step_form): the launch-per-phase form is several times slower than the CU-resident ones
struct StepPlan {
    azd::FusedEval fe;
    uint32_t dyn_stride;
    size_t dyn_bytes;
    azd::PoolArgs pool;
    int pool_blocks;
    bool feedback; // the pool step's controller acts on this engine's launches (pool_feedback_update)
};

// Pool, asynchronous, lock-step or launch-per-phase form, with the step down from a pool step that cannot be resident: writes
// e->step_form and e->step_reason and fills *out, which comes zeroed.
static int plan_step(azd_engine *e, int n_calls, StepPlan *out) {
    StepPlan &p = *out;
    const std::string dense_reason = e->a.space == azd::SPACE_DENSE ? e->step_reason : std::string();
    // a Ramsey engine under AZD_ENGINE_EXT_POOL_STEP whose form did not run takes what it would have taken without the flag; the
    // reason opens with why the form did not run.  After an aborted launch of the form it stays with the launch-per-phase kernels
    // that completed it.
    const bool ext_ramsey = e->ext && e->a.space == azd::SPACE_RAMSEY;
    const std::string ext_reason = ext_ramsey ? e->step_reason : std::string();
    const bool ext_demoted = ext_ramsey && e->pool_failed;
    p.pool = e->pool;
    const bool fusable = e->persist_enabled && !ext_demoted && e->ev->fused_desc(&p.fe);
    const bool pool_wanted = fusable && e->pool_step;
    const char *why_a = "", *why_b = "", *why_p = "";
    const bool pool_planned = pool_wanted && e->ops->pool_plan(e->a, p.fe, &p.pool, &p.dyn_stride, &p.dyn_bytes, &why_p);
    bool use_pool = pool_planned, use_async = false, use_barrier = false;
    e->step_reason.clear();
    if (pool_planned) { // the launch: the split, the evaluator groups, and what azd_engine_pool_split / azd_engine_pool_groups report
        const int capacity = knob_int("AZD_POOL_MAX_RESIDENT", e->ops->pool_max_resident(e->a, p.dyn_bytes, e->n_cus)); // (the knob: tests -- a device that holds fewer workgroups)
        PoolKnobs k;
        k.eval_wgs = knob_pos("AZD_POOL_EVAL_WGS", 0);
        k.search_wgs = knob_pos("AZD_POOL_SEARCH_WGS", 0);
        k.ready_lanes = knob_int("AZD_POOL_READY_LANES", 0);
        k.express_wgs = knob_int("AZD_POOL_EXPRESS_WGS", KNOB_UNSET);
        k.express_waves = knob_int("AZD_POOL_EXPRESS_WAVES", 8);
        k.express_shift = knob_int("AZD_POOL_EXPRESS_SHIFT", 4);
        k.early_post = knob_int("AZD_POOL_EARLY_POST", KNOB_UNSET);
        const int n_search = pool_split(e->n_cus, e->a, p.fe, n_calls, capacity, pool_feedback_on() ? e->pool_fb.n_eval : 0, k, &p.pool);
        if (n_search < 1 || capacity < 1) {
            use_pool = false;
            char buf[160];
            snprintf(buf, sizeof(buf), "pool step: the device holds %d of its workgroups at once; it needs an evaluator and a searcher resident together; ", capacity);
            e->step_reason = buf;
        }
        p.pool.debug_abort_call = (uint32_t)knob_int("AZD_POOL_DEBUG_ABORT_CALL", 0);
        AZD_ST(ensure_eval_groups(e, p.fe, use_pool, capacity - n_search, knob_int("AZD_POOL_EVAL_GROUP", KNOB_UNSET), &p.pool, &p.dyn_bytes));
        p.pool_blocks = p.pool.n_eval + n_search;
        e->pool_grp_g = p.pool.grp_g;
        e->pool_grp_groups = p.pool.grp_groups;
        e->pool_grp_w = p.pool.grp_w;
        e->pool_eval_wgs = p.pool.n_eval;
        e->pool_search_wgs = n_search;
        e->pool_search_waves = (n_search - p.pool.n_express) * 16 + p.pool.n_express * (int)p.pool.express_waves;
    }
    auto step_down = [&]() { // the forms below the pool step, in order; what each of them says goes behind the reason so far
        use_async = !e->barrier_step && e->ops->async_plan(e->a, p.fe, &p.dyn_stride, &p.dyn_bytes, &why_a);
        use_barrier = !use_async && e->ops->persist_plan(e->a, p.fe, &p.dyn_stride, &p.dyn_bytes, &why_b);
        if (!use_async) e->step_reason += why_a;
        if (!use_async && !use_barrier && *why_b) e->step_reason += std::string("; ") + why_b;
    };
    if (!e->persist_enabled) e->step_reason = "AZD_ENGINE_NO_PERSISTENT_STEP";
    else if (!fusable) e->step_reason = "the evaluator cannot run inside the kernel (external model, more than 7 layers, or a layer width that is not a multiple of 4)";
    else if (pool_planned && !use_pool) step_down(); // the pool step was wanted and cannot be resident: the next form down
    else if (!use_pool) {
        if (pool_wanted) e->step_reason = std::string(why_p) + "; ";
        if (e->barrier_step) e->step_reason = "AZD_ENGINE_BARRIER_STEP";
        step_down();
        if (e->pool_failed && use_async)
            e->step_reason = "an earlier pool launch of this engine aborted (a queue wait ran into its bound): asynchronous step";
        // (a pool step that was wanted and could not be planned has always asked the forms below it twice: where the asynchronous
        // step cannot run either, the reason names what was said about it and the lock-step form a second time.  Kept as it is.)
        if (pool_wanted) step_down();
    }
    e->step_form = use_pool ? AZD_STEP_POOL : use_async ? AZD_STEP_ASYNC : use_barrier ? AZD_STEP_BARRIER : AZD_STEP_PER_CALL;
    p.feedback = use_pool && p.fe.kind == 3 && pool_feedback_on() && !getenv("AZD_POOL_EVAL_WGS");
    if (e->a.space == azd::SPACE_DENSE) // why the space's pool step did not run: the launch-per-phase form follows
        e->step_reason = dense_reason.empty() ? "AZD_DENSE_NO_POOL: the dense-graph space's pool step was switched off" : dense_reason;
    if (ext_ramsey) e->step_reason = ext_demoted || e->step_reason.empty() ? ext_reason : ext_reason + "; " + e->step_reason;
    return AZD_OK;
}
// From the busy shares of a launch that is over: the evaluator workgroups the next launch's pool_split is given (fb_n_eval).
static void pool_feedback_update(azd_engine *e) {
    // where the best split sits: at equal shares when the agents hardly outnumber the searching waves (their cycle, not the
    // chip, sets the pace: configs A, B, the 384 x 384 model), at u_e - u_s = +0.06 when they queue for waves (8192 agents:
    // a slightly starved evaluator side fills 32-row batches, which cost it a quarter less per row)
    const double crowd = e->pool_search_waves > 0 ? (double)e->a.B / e->pool_search_waves - 1.5 : 0.0;
    const double d = e->pool_util_eval - e->pool_util_search - 0.06 * (crowd < 0 ? 0.0 : crowd > 1 ? 1.0 : crowd);
    // (large steps while the first guess is being corrected; afterwards at most 6 workgroups per launch, so that one disturbed
    // launch -- another tenant's burst on the box, a first dispatch under a profiler -- cannot carry the split far: a run whose
    // warm-up launch moved it from 89 to 102 evaluators stayed 7 % low for the two launches it had left to walk back)
    const int cur = e->pool_eval_wgs, lim = e->pool_fb.updates < 2 ? (cur / 4 > 4 ? cur / 4 : 4) : 6;
    e->pool_fb.updates += 1;
    int mv = (int)(100.0 * d + (d >= 0 ? 0.5 : -0.5));
    mv = mv > lim ? lim : mv < -lim ? -lim : mv;
    int next = cur + mv;
    next = next > e->n_cus / 2 ? e->n_cus / 2 : next < 1 ? 1 : next;
    e->pool_fb.n_eval = next;
}
// CU-resident forms: the whole call chain, n_calls times, in one launch per <= log_calls calls.  What a launch costs
// the host: the argument block is re-sent only when it changed (per-launch values are kernel arguments), the log and
// the pool's control block are left clean by k_argmin_log1, the abort flag comes back with the status block.
// ahead: one launch, left running behind an open window.  *fresh: h_status already holds the status behind the last launch.
static int run_resident(azd_engine *e, const azd::TolTable &t, int n_calls, StepPlan p, bool ahead, bool *fresh) {
    int left = n_calls;
    while (left > 0) {
        const int k = left < e->log_calls ? left : e->log_calls;
        const bool use_pool = e->step_form == AZD_STEP_POOL, use_async = e->step_form == AZD_STEP_ASYNC, use_barrier = e->step_form == AZD_STEP_BARRIER;
        *fresh = false;
        AZD_ST(send_pargs(e, e->a, t, p.fe, p.pool));
        if (use_pool && !e->pool_clean) AZD_ST(pool_clear(e, p.pool));
        if (use_pool && p.pool.grp_g > 0) { // batch numbers and arrival counts of the groups' slots start from zero in every launch
            const size_t slots = (size_t)p.pool.grp_groups * (16 / p.pool.grp_w);
            AZD_HIP(hipMemsetAsync(p.pool.grp_desc, 0, slots * 64 * 4, e->stream));
            AZD_HIP(hipMemsetAsync(p.pool.grp_cnt, 0, slots * 8 * 32 * 4, e->stream));
            AZD_HIP(hipMemsetAsync(p.pool.grp_flag, 0, slots * p.pool.grp_g * 16 * 4, e->stream));
        }
        if (!use_barrier) AZD_ST(ensure_log_clean(e));
        if (ahead) {
            // the window's hand-over words (no launch that writes them is in flight: a window is drained before the next opens),
            // and the argmin record the window starts from: its cost for the host's per-call compare, a copy for argmin_data
            AZD_HIP(hipMemsetAsync(p.pool.win_count, 0, (size_t)e->log_calls * sizeof(uint32_t), e->stream));
            AZD_HIP(hipMemcpyAsync(e->d_argmin_side, e->a.argmin, sizeof(azd::ArgminRec), hipMemcpyDeviceToDevice, e->stream));
            if (e->d_argmin_r_side)
                AZD_HIP(hipMemcpyAsync(e->d_argmin_r_side, e->a.argmin_r, e->tier->argmin_bytes, hipMemcpyDeviceToDevice, e->stream));
            AZD_HIP(hipMemcpyAsync(e->h_argmin, e->a.argmin, sizeof(azd::ArgminRec), hipMemcpyDeviceToHost, e->stream));
            AZD_ST(fetch_status(e)); // (synchronises)
            memset(e->h_win_flag, 0, (size_t)e->log_calls * sizeof(uint32_t));
            __atomic_thread_fence(__ATOMIC_SEQ_CST);
        }
        const azd::StepLaunch sl = step_launch(e, k, use_pool ? p.pool.ctl : nullptr, nullptr, p.fe.kind == 4, ahead, use_pool && p.pool.grp_g > 0);
        e->time_begin(0);
        if (use_pool) {
            e->ops->launch_pool(e->a, e->d_pargs, sl, p.fe.params, p.fe.wpk, p.pool_blocks, p.dyn_stride, p.dyn_bytes, e->stream);
#ifndef AZD_PHASE_PROFILE
            e->counters_by_wave = true;
#endif
        } else if (use_async) e->ops->launch_async(e->a, e->d_pargs, sl, p.fe.params, p.fe.wpk, p.dyn_stride, p.dyn_bytes, e->stream);
        else {
            e->ops->launch_persist(e->a, e->d_pargs, sl, e->d_log_node, p.dyn_stride, p.dyn_bytes, e->stream);
            e->log_clean = false;
        }
        e->time_end();
        left -= k;
        if (ahead) { // the launch is on its way; window_serve / window_drain do the rest
            AZD_HIP(hipGetLastError());
            e->ev->calls += (uint64_t)k;
            azd_engine::Window &w = e->win;
            w = azd_engine::Window();
            w.open = true;
            w.n = k;
            w.tol = t;
            w.best_ord = host_ordf(e->h_argmin->eval);
            w.base_improved = e->h_status->improved;
            w.fe = p.fe;
            w.pool = p.pool;
            return AZD_OK;
        }
        if (use_pool) {
            bool took_over = false;
            AZD_ST(pool_finish_launch(e, p.fe, p.pool, k, &took_over, &p.dyn_stride, &p.dyn_bytes));
            *fresh = left == 0 && !took_over; // the last launch's status is in, and nothing ran behind it
        }
        e->ev->calls += (uint64_t)k;
    }
    AZD_HIP(hipGetLastError());
    if (p.feedback && n_calls >= 100 && e->step_form == AZD_STEP_POOL && *fresh && e->h_status->pool_ticks > 0) pool_feedback_update(e); // the launch is over and its busy shares are in
    return AZD_OK;
}
// One launch-per-phase call per sub-population, captured in a graph each and replayed on streams of their own.
static int run_per_call_subs(azd_engine *e, const azd::TolTable &t, int n_calls, int n_subs) {
    const int per = (e->a.B + n_subs - 1) / n_subs;
    if (!e->sub_fork) AZD_ST(e->sub_fork.create(hipEventDisableTiming));
    for (int i = 0; i < n_subs; ++i) {
        if (!e->sub_stream[i]) AZD_ST(e->sub_stream[i].create(hipStreamNonBlocking));
        if (!e->sub_join[i]) AZD_ST(e->sub_join[i].create(hipEventDisableTiming));
    }
    int st = AZD_OK;
    if (e->sub_graph_n != n_subs || memcmp(&e->call_graph_tol, &t, sizeof(t)) != 0 || e->call_graph_layout != e->ev->layout_version) {
        for (azd::GraphExec &g : e->sub_graph) g.reset();
        e->sub_graph_n = 0;
        for (int i = 0; i < n_subs; ++i) {
            azd::Arenas as = e->a;
            as.t0 = i * per;
            as.tn = e->a.B - as.t0 < per ? e->a.B - as.t0 : per;
            if (as.tn <= 0) continue;
            st = capture_graph(e->sub_stream[i], [&]() -> int {
                e->ops->rollout(as, t, e->sub_stream[i]);
                const int st_w = e->ev->write_predictions_rows(as.t0, as.tn, e->a.state_vecs, e->a.state_vecs16, e->a.S16, e->a.h_theta, e->sub_stream[i]);
                e->ops->add_actions(as, 0, e->sub_stream[i]);
                azd::launch_log_candidates(as, e->d_log_key, e->d_call_ctr + i, e->sub_stream[i]);
                return st_w;
            }, &e->sub_graph[i]);
            if (st) return st;
        }
        e->sub_graph_n = n_subs;
        e->call_graph_tol = t;
        e->call_graph_layout = e->ev->layout_version;
        e->call_graph.reset(); // (the single-stream graph was captured for another tol table or layout)
    }
    int left = n_calls;
    while (left > 0) {
        const int k = left < e->log_calls ? left : e->log_calls;
        AZD_ST(ensure_log_clean(e));
        AZD_HIP(hipMemsetAsync(e->d_call_ctr, 0, sizeof(uint32_t) * azd_engine::MAX_SUBS, e->stream));
        AZD_HIP(hipEventRecord(e->sub_fork, e->stream));
        for (int i = 0; i < n_subs; ++i)
            if (e->sub_graph[i]) AZD_HIP(hipStreamWaitEvent(e->sub_stream[i], e->sub_fork, 0));
        for (int c = 0; c < k; ++c)
            for (int i = 0; i < n_subs; ++i)
                if (e->sub_graph[i]) AZD_HIP(hipGraphLaunch(e->sub_graph[i], e->sub_stream[i]));
        for (int i = 0; i < n_subs; ++i)
            if (e->sub_graph[i]) {
                AZD_HIP(hipEventRecord(e->sub_join[i], e->sub_stream[i]));
                AZD_HIP(hipStreamWaitEvent(e->stream, e->sub_join[i], 0));
            }
        e->ops->argmin_log(e->a, k, e->d_log_key, e->stream); // replays the k calls and leaves the log clean
        left -= k;
    }
    e->ev->calls += (uint64_t)n_calls;
    e->step_form = AZD_STEP_PER_CALL_GRAPH;
    return AZD_OK;
}
// One call captured once into a hipGraph and replayed per call.
static int run_per_call_graph(azd_engine *e, const azd::TolTable &t, int n_calls) {
    if (!e->call_graph || e->sub_graph_n != 0 || memcmp(&e->call_graph_tol, &t, sizeof(t)) != 0 || e->call_graph_layout != e->ev->layout_version) {
        e->sub_graph_n = 0; // (the sub-population graphs, if any, belong to another tol table or layout from here on)
        e->call_graph.reset();
        const int st = capture_graph(e->stream, [&]() -> int {
            e->ops->rollout(e->a, t, e->stream);
            const uint64_t calls_before = e->ev->calls;
            const int st_w = e->ev->write_predictions_dev16(e->a.B, e->a.state_vecs, e->a.state_vecs16, e->a.S16, e->a.h_theta, e->stream);
            e->ev->calls = calls_before;
            e->ops->add_actions(e->a, 0, e->stream);
            e->ops->argmin(e->a, 0, e->stream);
            return st_w;
        }, &e->call_graph);
        if (st) return st;
        e->call_graph_tol = t;
        e->call_graph_layout = e->ev->layout_version;
    }
    for (int c = 0; c < n_calls; ++c) AZD_HIP(hipGraphLaunch(e->call_graph, e->stream));
    e->ev->calls += (uint64_t)n_calls;
    e->step_form = AZD_STEP_PER_CALL_GRAPH;
    return AZD_OK;
}

// optimizer/mod.rs:159-190, n_calls times.  ahead: azd_engine_run_ahead -- the launch is left running and its calls are handed
// out by window_serve; *accepted = 0 when this engine's step form cannot do that (nothing is launched then).
static int roll_out_impl(azd_engine *e, const azd::TolTable &t, int n_calls, int *improved, bool ahead, int *accepted) {
    if (accepted) *accepted = 0;
    if (e->ext && !(e->ext->env_off && getenv(e->ext->env_off))) {
        if (ahead) return AZD_OK; // (the evaluator's launches need this thread: nothing can run ahead of the host; a hint, declined)
        bool ran = false;
        int left_after = 0;
        AZD_ST(ext_pool_run(e, t, n_calls, &ran, &left_after));
        if (ran && left_after == 0) return report_improved(e, check_status(e), improved);
        if (ran) n_calls = left_after; // (an aborted launch was completed call by call: what is left runs the same way, below)
    }
    StepPlan p{};
    AZD_ST(plan_step(e, n_calls, &p));
    if (ahead) { // only the pool step publishes its calls while it runs, one launch's worth of them
        const bool ok = e->step_form == AZD_STEP_POOL && p.fe.kind >= 3 && n_calls >= 1 && n_calls <= e->log_calls && !e->timing;
        if (!ok) return AZD_OK; // a hint: the calls run when they are asked for
        *accepted = 1;
    }
    bool status_fresh = false; // h_status already holds the status behind the last launch
    if (e->step_form != AZD_STEP_PER_CALL) {
        AZD_ST(run_resident(e, t, n_calls, p, ahead, &status_fresh));
        if (ahead) { // the launch is on its way; window_serve / window_drain do the rest
            if (improved) *improved = 0;
            return AZD_OK;
        }
    } else {
        // One call = roll-out, model call, add_actions, argmin: four to eight launches.  With the MLP evaluator (whose
        // launches take no per-call arguments) the sequence is captured once into a hipGraph and replayed per call, so
        // a call costs one graph launch instead of a launch per phase (BASELINE configs[4]: "hipGraph-captured episode
        // step").  Not while per-launch timing is on (the events would be captured too), nor for evaluators whose
        // kernels take the call index.
        const bool graphable = e->graph_enabled && !e->timing && n_calls >= 2 && e->ev->replayable(e->a.B);
        // Sub-populations: a roll-out launch lasts as long as its slowest agent (config E: 1.2 ms against a mean agent's 0.06), so
        // the population is cut into S parts, each with a stream and a graph of its own (roll-out, model rows, add_actions,
        // candidates into the per-call log); the parts run n_calls calls independently -- trees never exchange data and the
        // model is constant -- and one part's kernels fill the CUs another part's stragglers leave idle.  The per-call argmin
        // is replayed from the log afterwards, as in the CU-resident forms.  Needs an evaluator whose rows may run concurrently.
        // (Config E, 8192 agents: 1 / 2 / 4 / 8 parts -> 11.7 / 12.4 / 8.0 / 6.0 M expansions/s: every part adds seven graph nodes per
        // call for the host to enqueue, and beyond two parts the host, not the GPU, sets the pace.)
        int n_subs = (e->a.B >= 2048 && e->ev->rows_concurrent()) ? 2 : 1;
        n_subs = knob_int("AZD_PER_CALL_STREAMS", n_subs);
        if (n_subs > azd_engine::MAX_SUBS) n_subs = azd_engine::MAX_SUBS;
        if (n_subs > 1 && (!e->ev->rows_concurrent() || e->a.B > 65536 || e->a.node_cap > 65536)) n_subs = 1;
        if (graphable && n_subs > 1) AZD_ST(run_per_call_subs(e, t, n_calls, n_subs));
        else if (graphable) AZD_ST(run_per_call_graph(e, t, n_calls));
        else
            for (int c = 0; c < n_calls; ++c) {
                e->time_begin(0);
                e->ops->rollout(e->a, t, e->stream);
                e->time_end();
                AZD_ST(run_evaluator(e)); // :175-176
                e->ops->add_actions(e->a, 0, e->stream);
                e->ops->argmin(e->a, 0, e->stream); // :190
            }
    }
    return report_improved(e, status_fresh ? check_status(e) : sync_status(e), improved);
}

} // extern "C"

// ---------------------------------------------------------------- run-ahead window
namespace azd {
// The launch behind the window is over (or is waited for here): status in, busy shares noted, an aborted launch taken over.
static int window_drain(azd_engine *e) {
    azd_engine::Window &w = e->win;
    if (w.drained) return AZD_OK;
    bool took_over = false;
    uint32_t as = 0;
    size_t ab = 0;
    AZD_ST(pool_finish_launch(e, w.fe, w.pool, w.n, &took_over, &as, &ab));
    if (took_over) AZD_ST(fetch_status(e));
    w.drained = true;
    return check_status(e);
}
// The window ends: every call it ran is accounted for, whether handed out or not.
int window_close(azd_engine *e) {
    azd_engine::Window &w = e->win;
    if (!w.open) return AZD_OK;
    const int st = window_drain(e);
    w.open = false;
    if (st) return st;
    // every improvement the host was told of, call by call, is one the device's replay of the same log counted
    const unsigned long long total = e->h_status->improved - w.base_improved;
    if (w.consumed == w.n && !w.lumped && w.reported != total) {
        char buf[160];
        snprintf(buf, sizeof(buf), "run-ahead window: %llu improvements handed out call by call, %llu in the device's replay", w.reported, total);
        azd::g_last_error = buf;
        e->seen_improved = e->h_status->improved;
        return AZD_ERR_UNREACHABLE;
    }
    e->seen_improved = e->h_status->improved;
    return AZD_OK;
}
// k calls of the window, in order: each is waited for (the kernel publishes a call once its last agent is through it) and
// compared with the best cost so far exactly as k_argmin_log1 will compare it (strict, optimizer/mod.rs:211).
static int window_serve(azd_engine *e, int k, int *improved) {
    azd_engine::Window &w = e->win;
    int imp = 0;
    for (int i = w.consumed; i < w.consumed + k; ++i) {
        uint32_t spins = 0;
        while (!w.drained && __atomic_load_n(&e->h_win_flag[i], __ATOMIC_ACQUIRE) == 0u) {
            if ((++spins & 255u) == 0u) {
                const hipError_t q = hipStreamQuery(e->stream);
                if (q == hipSuccess) { // the launch is over: whatever it has not published it will not (an abort)
                    const int st = window_drain(e);
                    if (st) {
                        w.open = false;
                        e->seen_improved = e->h_status->improved;
                        return st;
                    }
                } else if (q != hipErrorNotReady) return azd::hip_fail(q, "hipStreamQuery");
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
        if (__atomic_load_n(&e->h_win_flag[i], __ATOMIC_ACQUIRE) != 0u) {
            const unsigned long long key = e->h_win_log[i];
            if (key != ~0ull && (uint32_t)(key >> 32) < w.best_ord) {
                w.best_ord = (uint32_t)(key >> 32);
                w.best_key = key;
                imp += 1;
            }
        } else if (!w.lumped) {
            // an aborted launch: the take-over completed the calls from here on and does not publish them one by one -- what they
            // improved is reported with this call, and the argmin record is the one the launch ended with
            const unsigned long long total = e->h_status->improved - w.base_improved;
            imp += (int)(total - w.reported - (unsigned long long)imp);
            w.lumped = true;
        }
    }
    w.consumed += k;
    w.reported += (unsigned long long)imp;
    if (improved) *improved = imp;
    if (w.consumed == w.n) return window_close(e);
    return AZD_OK;
}
// argmin_data inside a window: the record as of the calls handed out.  The winner's replay reads its tree, so the launch is
// waited for; the calls not yet handed out stay in the window.
int window_argmin_side(azd_engine *e, bool *side) {
    azd_engine::Window &w = e->win;
    *side = false;
    if (!w.open) return AZD_OK;
    const int st = window_drain(e);
    if (st) {
        w.open = false;
        e->seen_improved = e->h_status->improved;
        return st;
    }
    if (w.lumped) return AZD_OK; // (the device's record is all there is)
    if (w.best_key != w.side_key) {
        azd::Arenas a2 = e->a;
        a2.argmin = e->d_argmin_side;
        a2.argmin_r = e->d_argmin_r_side;
        e->ops->argmin_one(a2, (int)((w.best_key >> 16) & 0xFFFFull), (uint32_t)(w.best_key & 0xFFFFull), e->stream);
        AZD_HIP(hipGetLastError());
        w.side_key = w.best_key;
    }
    *side = true;
    return AZD_OK;
}
} // namespace azd

extern "C" {

int azd_engine_par_roll_out_episodes(azd_engine *e, const uint32_t *tol, int n_tol, uint32_t dflt, int n_calls,
                                     int *improved) {
    if (!e || n_calls < 0 || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_HIP(hipSetDevice(e->cfg.device));
    azd::TolTable t;
    AZD_ST(fill_tol(t, tol, n_tol, dflt));
    if (e->win.open) {
        // calls that were run ahead: handed out without a launch.  Other calls (another tolerance table, more calls than the
        // window has left) close the window and run as usual.
        if (memcmp(&e->win.tol, &t, sizeof(t)) == 0 && n_calls <= e->win.n - e->win.consumed) {
            if (n_calls == 0) {
                if (improved) *improved = 0;
                return AZD_OK;
            }
            return window_serve(e, n_calls, improved);
        }
        AZD_ST(window_close(e));
    }
    return roll_out_impl(e, t, n_calls, improved, false, nullptr);
}

// Run-ahead window: the next n_calls calls of par_roll_out_episodes(tol, ...) are started now, in one launch, and the calls
// that ask for them -- one by one, or in any chunks -- are answered from what the kernel publishes as it goes.
int azd_engine_run_ahead(azd_engine *e, const uint32_t *tol, int n_tol, uint32_t dflt, int n_calls, int *accepted) {
    if (accepted) *accepted = 0;
    if (!e || n_calls < 0 || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_ENTER(e);
    azd::TolTable t;
    int st = fill_tol(t, tol, n_tol, dflt);
    if (st) return st;
    if (n_calls == 0) return AZD_OK;
    int ok = 0;
    st = roll_out_impl(e, t, n_calls, nullptr, true, &ok);
    if (accepted) *accepted = ok;
    return st;
}
} // extern "C"
