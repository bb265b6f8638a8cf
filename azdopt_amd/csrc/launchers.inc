// launchers.inc -- host side of a search translation unit: the launcher templates, once for every space.  Included (inside
// namespace azd) after tree_core.inc, the space policy and the step includes; a unit sees the launchers of the kernels it is built
// with -- the phase units those of the launch-per-phase kernels, the root policy and the barrier step, the AZD_TU_ASYNC units
// l_async, the AZD_TU_POOL units l_pool, and beside any of these the AZD_TU_POOL_SEARCH units the searcher-only pool step's plan,
// launch and residency query -- and builds the instantiations that its table entries (space_ops.h) name, no others.
//
// Dynamic LDS beyond the default 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize, which is per DEVICE (the current one): the
// CU-resident launchers set it on every launch -- a host-side call, once per <= 1024 search calls -- so that engines on several
// devices in one process all get it; the plans have already checked that the request fits beside the kernel's static LDS.  A
// failure is sticky: the caller's hipGetLastError reports it.

#if defined(AZD_TU_POOL)
template <class SP>
static void l_pool(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, const float *params,
                   const void *wpk, int n_blocks, uint32_t dyn_stride, size_t dyn_bytes, hipStream_t st) {
    constexpr bool GROUPS = SP::POOL_EVAL_GROUPS; // (the instantiations with evaluator groups are built for such a space only)
    const int mode = (sl.hashed ? 1 : 0) | (sl.window ? 2 : 0) | ((GROUPS && sl.groups && !sl.hashed) ? 4 : 0);
#define AZD_LAUNCH_POOL(M)                                                                                                          \
    case M:                                                                                                                         \
        if (hipFuncSetAttribute((const void *)k_pool<SP, M>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return; \
        k_pool<SP, M><<<dim3(n_blocks), dim3(PERSIST_WAVES * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, dyn_stride, params, a.state_vecs, a.h_theta, wpk); \
        break;
    switch (mode) {
        AZD_LAUNCH_POOL(0)
        AZD_LAUNCH_POOL(1)
        AZD_LAUNCH_POOL(2)
        AZD_LAUNCH_POOL(3)
    default:
        if constexpr (GROUPS) switch (mode) {
            AZD_LAUNCH_POOL(4) // evaluator groups (pool_eval_group) ...
            AZD_LAUNCH_POOL(6) // ... and inside a run-ahead window
        }
    }
#undef AZD_LAUNCH_POOL
    k_argmin_log1<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, sl.n_calls, sl.log_key, sl.ctl);
}
template <class SP>
static void q_pool_resident(int *out, size_t dyn_bytes) {
    int nb = 0;
    if (hipFuncSetAttribute((const void *)k_pool<SP, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_pool<SP, 0>, PERSIST_WAVES * 64, dyn_bytes) != hipSuccess) {
        (void)hipGetLastError();
        nb = 0;
    }
    *out = nb;
}

#elif defined(AZD_TU_ASYNC)
template <class SP>
static void l_async(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl,
                    const float *params, const void *wpk, uint32_t dyn_stride, size_t dyn_bytes, hipStream_t st) {
    if (hipFuncSetAttribute((const void *)k_async<SP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return;
    const int n_wg = (a.B + PERSIST_WAVES - 1) / PERSIST_WAVES;
    k_async<SP><<<dim3(n_wg), dim3(PERSIST_WAVES * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, dyn_stride, params, a.state_vecs, a.h_theta, wpk, sl.resume);
    k_argmin_log1<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, sl.n_calls, sl.log_key, nullptr);
}

#else // a phase unit
template <class SP>
static void l_init_roots(const Arenas &a, const uint8_t *p, const uint64_t *m, hipStream_t st) {
    k_init_roots<SP><<<dim3(a.B), dim3(64), SP::dyn_bytes(a), st>>>(a, p, m);
}
template <class SP>
static void l_add_actions(const Arenas &a, int root_mode, hipStream_t st) {
    k_add_actions<SP><<<dim3(a.tn ? a.tn : a.B), dim3(64), SP::dyn_bytes(a), st>>>(a, root_mode);
}
template <class SP>
static void l_rollout(const Arenas &a, const TolTable &tol, hipStream_t st) {
    k_rollout<SP><<<dim3(a.tn ? a.tn : a.B), dim3(64), SP::dyn_bytes(a), st>>>(a, tol);
}
template <class SP>
static void l_argmin(const Arenas &a, int init_mode, hipStream_t st) {
    k_argmin<SP><<<dim3(1), dim3(1024), SP::dyn_bytes(a), st>>>(a, init_mode);
}
template <class SP>
static void l_argmin_log(const Arenas &a, int n_calls, unsigned long long *log_key, hipStream_t st) {
    k_argmin_log1<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, n_calls, log_key, nullptr);
}
template <class SP>
static void l_observe(const Arenas &a, uint32_t tol, hipStream_t st) {
    k_observe<SP><<<dim3(a.B), dim3(64), SP::dyn_bytes(a), st>>>(a, tol);
}
template <class SP>
static void l_modify_roots(const Arenas &a, uint64_t seed, uint64_t epoch, uint64_t first_agent, int kmin, int kmax, uint8_t *d_roots,
                           uint64_t *d_perm, uint64_t *d_slots, const RootPolicyArgs &rp, hipStream_t st) {
    k_modify_roots<SP><<<dim3(a.B), dim3(64), SP::dyn_bytes(a), st>>>(a, seed, epoch, first_agent, kmin, kmax, d_roots, d_perm, d_slots, rp);
}
template <class SP>
static void l_argmin_one(const Arenas &a, int agent, uint32_t node, hipStream_t st) {
    k_argmin_one<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, agent, node);
}
template <class SP>
static void l_persist(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl,
                      uint32_t *log_node, uint32_t dyn_stride, size_t dyn_bytes, hipStream_t st) {
    if (hipFuncSetAttribute((const void *)k_persist<SP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return;
    const int n_wg = (a.B + PERSIST_WAVES - 1) / PERSIST_WAVES;
    k_persist<SP><<<dim3(n_wg), dim3(PERSIST_WAVES * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, log_node, dyn_stride);
    k_argmin_log<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, sl.n_calls, n_wg, sl.log_key, log_node);
}

// The table entries every phase unit has, for the unit's key-width switch D (DISPATCH_KW and its like, beside the space policies).
// (The order of the definitions is the order in which the kernels are instantiated; with k_modify_roots behind the others the
// Ramsey policies' k_modify_roots comes out a few instructions different.  It stays where the Ramsey units had it: first.)
#define AZD_PHASE_ENTRIES(D)                                                                                                          \
    static void e_modify_roots(const Arenas &a, uint64_t seed, uint64_t epoch, uint64_t first_agent, int kmin, int kmax,              \
                               uint8_t *d_roots, uint64_t *d_perm, uint64_t *d_slots, const RootPolicyArgs &rp, void *stream) {       \
        D(a, l_modify_roots, a, seed, epoch, first_agent, kmin, kmax, d_roots, d_perm, d_slots, rp, (hipStream_t)stream);             \
    }                                                                                                                                 \
    static void e_init_roots(const Arenas &a, const uint8_t *d_roots, const uint64_t *d_permitted, void *stream) {                    \
        D(a, l_init_roots, a, d_roots, d_permitted, (hipStream_t)stream);                                                             \
    }                                                                                                                                 \
    static void e_add_actions(const Arenas &a, int root_mode, void *stream) { D(a, l_add_actions, a, root_mode, (hipStream_t)stream); } \
    static void e_rollout(const Arenas &a, const TolTable &tol, void *stream) { D(a, l_rollout, a, tol, (hipStream_t)stream); }       \
    static void e_argmin(const Arenas &a, int init_mode, void *stream) { D(a, l_argmin, a, init_mode, (hipStream_t)stream); }         \
    static void e_argmin_log(const Arenas &a, int n_calls, unsigned long long *log_key, void *stream) {                               \
        D(a, l_argmin_log, a, n_calls, log_key, (hipStream_t)stream);                                                                 \
    }                                                                                                                                 \
    static void e_observe(const Arenas &a, uint32_t n_obs_tol, void *stream) { D(a, l_observe, a, n_obs_tol, (hipStream_t)stream); }
#define AZD_PHASE_OPS e_init_roots, e_add_actions, e_rollout, e_argmin, e_argmin_log, e_observe, e_modify_roots
// What the dense-graph units put in their tables for the forms they do not build: the space's state vector (3E + 1 floats) does not
// fit the CU-resident forms' LDS plans, so it runs one launch per phase, or its searcher-only pool step (hence no run-ahead window)
#define DENSE_NO_RESIDENT "dense-graph space: its CU-resident form is the pool searchers with the evaluator outside the kernel (engine.hip: dense_pool_run)"
#define AZD_DENSE_NO_RESIDENT_ENTRIES                                                                                                 \
    static void no_argmin_one(const Arenas &, int, uint32_t, void *) {}                                                               \
    static bool no_resident(const Arenas &, const FusedEval &, uint32_t *, size_t *, const char **why) {                              \
        *why = DENSE_NO_RESIDENT;                                                                                                     \
        return false;                                                                                                                 \
    }                                                                                                                                 \
    static bool no_pool(const Arenas &, const FusedEval &, PoolArgs *, uint32_t *, size_t *, const char **why) {                      \
        *why = DENSE_NO_RESIDENT;                                                                                                     \
        return false;                                                                                                                 \
    }
#endif

#if defined(AZD_TU_POOL_SEARCH)
// ---------------------------------------------------------------- pool step, searchers only (pool_step.inc: k_pool_search<SP, MODE, WAVES>)
// WAVES: the wavefronts per workgroup the unit's kernels are built and launch-bounded for.  The Ramsey tiers' (ramsey_ext_kernels.hip,
// ramsey64_ext_kernels.hip; DESIGN.md section 3 says why eight):
constexpr int RAMSEY_EXT_WAVES = 8, RAMSEY64_EXT_WAVES = 8;
static_assert(RAMSEY_EXT_WAVES == 8 && RAMSEY64_EXT_WAVES == 8, "AZD_RAMSEY_EXT_POOL_WAVES' range is spelled out in its error text (engine.hip)");
static_assert(sizeof(PoolIdle) <= POOL_SEARCH_STATIC_LDS, "space_ops.h: POOL_SEARCH_STATIC_LDS");
template <int WAVES>
struct PoolSearch { // (a class over WAVES, so that a unit's key-width switch can name its members as templates over SP alone)
    // LDS of a searcher workgroup: WAVES blocks (the kernel's SW_BYTES), then a scratch region per wave that runs (no row is staged:
    // SP::write_rows_direct).  Arithmetic only.  *bad: one of the unit's three refusals, or left as it was.
    template <class SP>
    static void plan(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **bad, const char *r_agents,
                     const char *r_waves, const char *r_lds) {
        if (a.B > 65536 || a.node_cap > 65536) { // (agent, node) are packed 16 + 16 bits in the argmin log
            *bad = r_agents;
            return;
        }
        const size_t stride = (SP::dyn_bytes(a) + 15) & ~(size_t)15;
        const size_t sw_bytes = (WAVES * sizeof(typename SP::Lds) + 15) & ~(size_t)15;
        *dyn_stride = (uint32_t)stride;
        *dyn_bytes = sw_bytes + stride * (size_t)waves;
        if (waves < 1 || waves > WAVES) *bad = r_waves;
        else if (*dyn_bytes + sizeof(PoolIdle) + 256 > 160 * 1024) *bad = r_lds;
    }
    template <class SP>
    static void launch(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves, uint32_t dyn_stride,
                       size_t dyn_bytes, hipStream_t st) {
        if (waves < 1 || waves > WAVES) return; // (the plan refuses it)
        if (sl.hashed) { // the test harness' evaluator (FusedEval kind 4): the searchers note the call of every row they post
            if (hipFuncSetAttribute((const void *)k_pool_search<SP, 1, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return;
            k_pool_search<SP, 1, WAVES><<<dim3(n_blocks), dim3(waves * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, dyn_stride);
        } else {
            if (hipFuncSetAttribute((const void *)k_pool_search<SP, 0, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess) return;
            k_pool_search<SP, 0, WAVES><<<dim3(n_blocks), dim3(waves * 64), dyn_bytes, st>>>(d_args, sl.n_calls, sl.log_key, dyn_stride);
        }
        k_argmin_log1<SP><<<dim3(1), dim3(64), SP::dyn_bytes(a), st>>>(a, sl.n_calls, sl.log_key, sl.ctl);
    }
    template <class SP>
    static void resident(int *out, int waves, size_t dyn_bytes) { // workgroups of the kernel one CU holds
        int nb = 0;
        if (waves < 1 || waves > WAVES ||
            hipFuncSetAttribute((const void *)k_pool_search<SP, 0, WAVES>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_bytes) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)k_pool_search<SP, 0, WAVES>, waves * 64, dyn_bytes) != hipSuccess) {
            (void)hipGetLastError();
            nb = 0;
        }
        *out = nb;
    }
};
// A unit's PoolSearchOps (space_ops.h) for its key-width switch D, and its refusals: more than 65536 agents or nodes, more wavefronts
// than WAVES, more LDS than a CU has.
#define AZD_POOL_SEARCH_ENTRIES(D, WAVES, R_AGENTS, R_WAVES, R_LDS)                                                                   \
    static bool e_pool_search_plan(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why) {           \
        const char *bad = nullptr;                                                                                                    \
        D(a, PoolSearch<WAVES>::plan, a, waves, dyn_stride, dyn_bytes, &bad, R_AGENTS, R_WAVES, R_LDS);                               \
        if (bad) *why = bad;                                                                                                          \
        return bad == nullptr;                                                                                                        \
    }                                                                                                                                 \
    static void e_launch_pool_search(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves,       \
                                     uint32_t dyn_stride, size_t dyn_bytes, void *stream) {                                           \
        D(a, PoolSearch<WAVES>::launch, a, d_args, sl, n_blocks, waves, dyn_stride, dyn_bytes, (hipStream_t)stream);                  \
    }                                                                                                                                 \
    static int e_pool_search_resident(const Arenas &a, int waves, size_t dyn_bytes) {                                                 \
        int nb = 0;                                                                                                                   \
        D(a, PoolSearch<WAVES>::resident, &nb, waves, dyn_bytes);                                                                     \
        return nb;                                                                                                                    \
    }
#define AZD_POOL_SEARCH_OPS(WAVES) e_pool_search_plan, e_launch_pool_search, e_pool_search_resident, WAVES
#endif
