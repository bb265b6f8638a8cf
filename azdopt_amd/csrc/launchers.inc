// launchers.inc -- host side of a search translation unit: the launcher templates, once for every space.  Included (inside
// namespace azd) after tree_core.inc, the space policy and the step includes; a unit sees the launchers of the kernels it is built
// with -- the phase units those of the launch-per-phase kernels, the root policy and the barrier step, the AZD_TU_ASYNC units
// l_async, the AZD_TU_POOL units l_pool -- and builds the instantiations that its table entries (space_ops.h) name, no others.
//
// Dynamic LDS beyond the default 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize, which is per DEVICE (the current one): the
// CU-resident launchers set it on every launch -- a host-side call, once per <= 1024 search calls -- so that engines on several
// devices in one process all get it; the plans have already checked that the request fits beside the kernel's static LDS.  A
// failure is sticky: the caller's hipGetLastError reports it.

#if defined(AZD_TU_POOL)
template <class SP, class = void>
struct SpacePoolEvalGroups { static constexpr bool value = false; };
template <class SP>
struct SpacePoolEvalGroups<SP, decltype((void)SP::POOL_EVAL_GROUPS)> { static constexpr bool value = SP::POOL_EVAL_GROUPS; };

template <class SP>
static void l_pool(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, const float *params,
                   const void *wpk, int n_blocks, uint32_t dyn_stride, size_t dyn_bytes, hipStream_t st) {
    constexpr bool GROUPS = SpacePoolEvalGroups<SP>::value; // (the instantiations with evaluator groups are built for such a space only)
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
#endif
