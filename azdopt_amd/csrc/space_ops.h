// space_ops.h -- what the host engine calls in the search translation units: one table of launchers and LDS plans per space
// and tier (SpaceOps, in four parts: launch-per-phase and barrier step, asynchronous step, pool step, searcher-only pool step;
// azd_engine_create picks it once), and the helpers that are the same for every space.  Everything is asynchronous on `stream`.
#pragma once
#include "engine_types.h"

namespace azd {

// A *_plan lays out the LDS of a CU-resident step; when the model or the population does not fit, or the space does not build
// the form, it returns false and says why in *why.  The launch entries of a form whose plan always refuses are null; a space
// without the searcher-only pool step (c21) has that whole part null.
struct PhaseOps { // a space's phase unit (tree_kernels.hip, ramsey_kernels.hip, ramsey64_kernels.hip, dense_kernels.hip and its AH siblings)
    void (*init_roots)(const Arenas &a, const uint8_t *d_roots, const uint64_t *d_permitted, void *stream);
    void (*add_actions)(const Arenas &a, int root_mode, void *stream);
    void (*rollout)(const Arenas &a, const TolTable &tol, void *stream);
    void (*argmin)(const Arenas &a, int init_mode, void *stream);
    // replays the candidates launch_log_candidates (or a CU-resident step) left in log_key, in call order
    void (*argmin_log)(const Arenas &a, int n_calls, unsigned long long *log_key, void *stream);
    void (*observe)(const Arenas &a, uint32_t n_obs_tol, void *stream);
    // device root policy.  d_perm: what k_init_roots takes; d_slots: the drawn slot masks of the dense-graph space ((E + 63) / 64
    // words per root), d_perm again for the other spaces; rp: the engine's root policy (azd_engine_set_root_policy) and its report
    void (*modify_roots)(const Arenas &a, uint64_t seed, uint64_t epoch, uint64_t first_agent, int kmin, int kmax, uint8_t *d_roots,
                         uint64_t *d_perm, uint64_t *d_slots, const RootPolicyArgs &rp, void *stream);
    // one candidate (agent, node) replayed into the argmin records `a` points at; StatusRec untouched (run-ahead window, engine_rollout.hip)
    void (*argmin_one)(const Arenas &a, int agent, uint32_t node, void *stream);
    bool (*persist_plan)(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why);
    void (*launch_persist)(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, uint32_t *log_node, uint32_t dyn_stride,
                           size_t dyn_bytes, void *stream);
};
struct AsyncOps { // async_kernels.hip, ramsey_async_kernels.hip
    bool (*async_plan)(const Arenas &a, const FusedEval &ev, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why);
    void (*launch_async)(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, const float *params, const void *wpk,
                         uint32_t dyn_stride, size_t dyn_bytes, void *stream);
};
struct PoolOps { // pool_kernels.hip, ramsey_pool_kernels.hip
    // the plan also lays out an evaluator batch (pool->eval_*)
    bool (*pool_plan)(const Arenas &a, const FusedEval &ev, PoolArgs *pool, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why);
    void (*launch_pool)(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, const float *params, const void *wpk,
                        int n_blocks, uint32_t dyn_stride, size_t dyn_bytes, void *stream);
    // workgroups of k_pool the device can hold at once with this much dynamic LDS (occupancy query x CUs): the pool step's
    // searcher and evaluator workgroups spin-wait on each other, so all of them must be resident together
    int (*pool_max_resident)(const Arenas &a, size_t dyn_bytes, int n_cus);
};
struct PoolSearchOps { // the pool step with searcher workgroups only (pool_step.inc: k_pool_search; launchers.inc): the evaluator is a stream
                       // of batched GEMM launches over the rows the searchers have posted (launch_ext_* below).  Null where a space has none.
    // waves: wavefronts per searcher workgroup; the plan is arithmetic and touches no device
    bool (*pool_search_plan)(const Arenas &a, int waves, uint32_t *dyn_stride, size_t *dyn_bytes, const char **why);
    void (*launch_pool_search)(const Arenas &a, const PersistArgs *d_args, const StepLaunch &sl, int n_blocks, int waves, uint32_t dyn_stride,
                               size_t dyn_bytes, void *stream);
    int (*pool_search_resident)(const Arenas &a, int waves, size_t dyn_bytes); // workgroups of the kernel one CU holds
    // the wavefronts the unit's kernels lay out blocks and are launch-bounded for; the plan refuses more, and more than the LDS holds
    // (the engine counts down from here: 16 for the dense-graph space -- 10, 9 or 7 fit with the Aouchiche-Hansen cost --, 6 for that
    // cost's 64-row form, 8 for the Ramsey tiers)
    int waves_max;
};
struct SpaceOps : PhaseOps, AsyncOps, PoolOps, PoolSearchOps {};

// what the units export: c21 and Ramsey (narrow and wide) build each form in a unit of its own, the 64-bit Ramsey tier and the
// dense-graph space run one launch per phase and refuse the CU-resident forms in their tables; the dense-graph units build their
// searcher-only pool step themselves, the Ramsey tiers with max_slots > 0 have it in units of their own (AZD_ENGINE_EXT_POOL_STEP:
// ramsey_ext_kernels.hip the 32-bit wide tier, ramsey64_ext_kernels.hip the 64-bit tier)
// (functions, not objects: a const object of a .hip file is compiled for the device too, where its entries do not exist)
const PhaseOps &c21_phase_ops(), &ramsey_phase_ops();
const AsyncOps &c21_async_ops(), &ramsey_async_ops();
const PoolOps &c21_pool_ops(), &ramsey_pool_ops();
const PoolSearchOps &ramsey_pool_search_ops(), &ramsey64_pool_search_ops();
// the 64-bit tier with forbidden cliques up to K8 (AZD_ENGINE_RAMSEY_BIG_CLIQUES: ramsey64_big_kernels.hip, ramsey64_big_ext_kernels.hip)
const SpaceOps &ramsey64_big_ops();
const PoolSearchOps &ramsey64_big_pool_search_ops();
const SpaceOps &ramsey64_ops(), &dense_ops(), &dense_ah_ops(); // dense_ah_ops: DenseSpace with the Aouchiche-Hansen cost (dense_ah_kernels.hip)
const SpaceOps &dense_ah_wide_ops();                            // ... with its 64-row form (dense_ah_wide_kernels.hip: AZD_ENGINE_DENSE_AH_WIDE)
const SpaceOps &dense_inv_ops();                                // ... with the weighted-invariant cost (dense_inv_kernels.hip: AZD_ENGINE_DENSE_INV)
const SpaceOps &dense_inv_wide_ops();                           // ... with its 64-row form (dense_inv_wide_kernels.hip: AZD_ENGINE_DENSE_INV_WIDE)
const SpaceOps &dense_invx_ops();                               // ... with the extended invariant cost (dense_invx_kernels.hip: AZD_ENGINE_DENSE_INVX)
const SpaceOps &dense_invx_wide_ops();                          // ... with its 64-row form (dense_invx_wide_kernels.hip: AZD_ENGINE_DENSE_INVX_WIDE)
constexpr size_t POOL_SEARCH_STATIC_LDS = 16; // k_pool_search's static LDS (PoolIdle) beside the dynamic region the plans lay out

// ---- the same for every space
// launch-per-phase form over sub-populations on streams of their own (engine_rollout.hip): the candidates of agents a.t0 .. a.t0 + a.tn - 1
// since their last inspection go into log_key[*call_ctr] (atomic min), the counter is bumped; replayed by SpaceOps::argmin_log
void launch_log_candidates(const Arenas &a, unsigned long long *log_key, uint32_t *call_ctr, void *stream);
// after an aborted pool launch: resume[t] for k_async (StepLaunch::resume) from the trees and PoolArgs::pend
void launch_pool_resume_scan(const Arenas &a, const PoolArgs &pool, int n_calls, uint32_t *resume, void *stream);
// test entry: the in-kernel evaluator's forward (pool_eval's staging + mlp_tile_task) for rows given by the host
hipError_t launch_tile_forward(const FusedEval &ev, const PoolArgs &pool, int n_rows, const float *states, float *out, void *stream);
void launch_probe_xcc(uint32_t *d_out, int n_blocks, void *stream); // HW_REG_XCC_ID of every block of a launch (tests)
void launch_hash_predictions(float *d_out, int batch, int action_dim, uint64_t seed, uint64_t first_agent,
                             uint64_t call, void *stream);
void launch_probe_cost(const uint8_t *d_parents, int n, int count, int reps, int full, double *d_lam, int *d_mu,
                       void *stream);
void launch_probe_math(const float *d_in, float *d_out, int n, void *stream); // sqrtf / sub parity probe (tests)
// dense_kernels.hip: the dense-graph space's default cost (lambda_1 + matching number) of `count` graphs on n vertices, one wave
// each: from nothing, then after each of n_toggles edge toggles with the matching repaired (outputs [count][n_toggles + 1])
void launch_probe_dense_cost(const uint64_t *d_adj, int n, int count, const uint16_t *d_toggles, int n_toggles, double *d_lam, int *d_mu,
                             uint8_t *d_mate, int *d_hooks, void *stream);
// dense_ah_kernels.hip: the Aouchiche-Hansen cost of `count` graphs on n vertices, one wave each (dense_cost_host.h: DenseAhCost), and the
// f64 division / sqrt parity probe (tests)
struct DenseAhCost;
void launch_probe_ah_cost(const uint64_t *d_adj, int n, int count, int reps, DenseAhCost *d_out, void *stream);
void launch_probe_math_f64(const double *d_in, double *d_out, int n, void *stream);
void launch_probe_ah_cost_wide(const uint64_t *d_adj, int n, int count, int reps, DenseAhCost *d_out, void *stream); // n <= 64 (dense_ah_wide_kernels.hip)
// dense_inv_kernels.hip: the weighted-invariant cost of `count` graphs on n vertices under the recipe at d_recipe (device memory), one
// wave each (dense_cost_host.h: DenseInvRecipe, DenseInvCost)
struct DenseInvRecipe;
struct DenseInvCost;
void launch_probe_inv_cost(const uint64_t *d_adj, int n, int count, int reps, const DenseInvRecipe *d_recipe, DenseInvCost *d_out, void *stream);
void launch_probe_inv_cost_wide(const uint64_t *d_adj, int n, int count, int reps, const DenseInvRecipe *d_recipe, DenseInvCost *d_out, void *stream); // n <= 64 (dense_inv_wide_kernels.hip)
const SpaceOps &dense_invs_ops();                               // ... with the spectrum invariant cost (dense_invs_kernels.hip: AZD_ENGINE_DENSE_INVS)
const SpaceOps &dense_invs_wide_ops();                          // ... with its 64-row form (dense_invs_wide_kernels.hip: AZD_ENGINE_DENSE_INVS_WIDE)
struct DenseInvxRecipe;
struct DenseInvxCost;
void launch_probe_invx_cost(const uint64_t *d_adj, int n, int count, int reps, const DenseInvxRecipe *d_recipe, DenseInvxCost *d_out, void *stream); // (dense_invx_kernels.hip)
void launch_probe_invx_cost_wide(const uint64_t *d_adj, int n, int count, int reps, const DenseInvxRecipe *d_recipe, DenseInvxCost *d_out, void *stream); // n <= 64 (dense_invx_wide_kernels.hip)
struct DenseInvsRecipe;
struct DenseInvsCost;
void launch_probe_invs_cost(const uint64_t *d_adj, int n, int count, int reps, const DenseInvsRecipe *d_recipe, DenseInvsCost *d_out, void *stream); // n <= 32 (dense_invs_kernels.hip)
void launch_probe_invs_cost_wide(const uint64_t *d_adj, int n, int count, int reps, const DenseInvsRecipe *d_recipe, DenseInvsCost *d_out, void *stream); // n <= 64 (dense_invs_wide_kernels.hip)

// ---- the evaluator's side of the searcher-only pool step and the recovery of an aborted launch (dense_kernels.hip; for every space that has the form)
void launch_ext_take(const PoolArgs &pool, uint32_t *rows, uint32_t *home, uint32_t *n, unsigned long long *t0, void *stream);
// recovery of an aborted launch (engine_rollout.hip): park (round >= 0: the agents whose calls are through by that round; -1: the
// agents that are not waiting for a row) / unpark (mode 0), and the candidates of round r under the call each agent is really in
void launch_park(const Arenas &a, const uint32_t *resume, int n_calls, int round, int park, void *stream);
void launch_log_candidates_resume(const Arenas &a, unsigned long long *log_key, const uint32_t *resume, int n_calls, int round, void *stream);
void launch_ext_hash_rows(const PersistArgs *d_args, const uint32_t *rows, const uint32_t *n, uint32_t cap, float *h_theta, void *stream);
void launch_ext_deliver(const PoolArgs &pool, const Arenas &a, const uint32_t *rows, const uint32_t *home, const uint32_t *n, uint32_t cap,
                        const unsigned long long *t0, void *stream);

} // namespace azd
