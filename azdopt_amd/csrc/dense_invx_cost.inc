// dense_invx_cost.inc -- the extended invariant cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_spectral.inc, whose stages it is composed of).
//
// BUILD-DEFINED (dense_cost_host.h: DenseInvxRecipe; DESIGN.md "The extended invariant cost"): sixteen invariants in a fixed order --
//   0 edges  1 max_degree  2 min_degree  3 diameter  4 radius  5 proximity  6 remoteness  7 avg_distance  8 adj_eig  9 dist_eig
//   10 lap_eig  11 slap_eig  12 randic  13 zagreb1  14 zagreb2  15 triangles
// -- combined by a recipe the caller gives at RUN time: c = bias, then c = c + weight[i] * I_i for every i whose weight is not zero,
// in order, then c = c + coef_t * (I_a * I_b or I_a / I_b) for every pair term whose coefficient is not zero, in order;
// cost = (f32)c; eval = eval_scale * (cost + eval_offset).  The first ten are dense_inv_cost.inc's, and with weights 10 .. 15 zero
// and no pair term the sequence of operations is that unit's: the weighted-invariant cost, and so the Aouchiche-Hansen cost, are
// recipes of this one and come out bit for bit.
//
// One triangle serves up to four spectral passes, one after the other: the DISTANCE pass first, on the rows the BFS left; then the
// ADJACENCY, LAPLACIAN (D - A) and SIGNLESS-LAPLACIAN (D + A) passes, each refilling the triangle from the bitsets, which are still
// in LDS, and the lane's degree.  So the wave's LDS block is the AH block.  Every reduction deflates.
// The degree-based invariants run after the passes (dense_degree_sums_wave), so that nothing of them is held across the reductions.
// Each of the invariants 8 .. 15 is computed only when its weight is not zero or a pair term with a non-zero coefficient names it
// (wave-uniform branches: the recipe is the same for all lanes): otherwise 0.0, and its bit of `computed` is clear.
//
// The row limit ROWS is a template parameter of everything here that depends on it: 32 (DenseCostInvX: dense_invx_kernels.hip,
// AZD_ENGINE_DENSE_INVX) or 64 (DenseCostInvXWide: dense_invx_wide_kernels.hip, AZD_ENGINE_DENSE_INVX_WIDE beside the first flag),
// and the engine's argmin record follows from it.
//
// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  rc: the recipe in device memory, the same address in
// every lane.  hook: called once, after the BFS (the pool step's deferred post).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_invx_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const DenseInvxRecipe *rc,
                                                     Hook &&hook, DenseInvxCost &out) {
    static_assert(ROWS == DENSE_INVX_MAX_N || ROWS == DENSE_INVX_WIDE_MAX_N, "the row limits that are built");
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const uint64_t all = dense_vertex_mask<ROWS>(n);
    const uint32_t need = uni(dense_invx_needed(*rc));
    const auto has = [need](const int i) { return ((need >> i) & 1u) != 0u; };
    const int dist_index = (int)uni((uint32_t)rc->dist_index);
    int t, d, deg;
    dense_bfs_wave(adj, w, lane, row, in, all, has(DENSE_INV_DIST_EIG), t, d, deg);
    const DenseBfsSums s = dense_bfs_sums_wave(in, t, d, deg);
    hook();
    const int dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : dense_ah_index(s.diam, n);
    double eig[4] = {0.0, 0.0, 0.0, 0.0}; // by pass
    // ---- the spectral passes: 0 = distance matrix (the BFS's rows), then refilled from the bitsets: 1 = adjacency matrix,
    // 2 = Laplacian D - A, 3 = signless Laplacian D + A
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int which = pass == 0 ? DENSE_INV_DIST_EIG : pass == 1 ? DENSE_INV_ADJ_EIG : pass == 2 ? DENSE_INVX_LAP_EIG : DENSE_INVX_SLAP_EIG;
        if (!has(which)) continue;
        if (pass > 0) dense_refill_wave(adj, w, lane, row, in, pass == 2 ? -1.0 : 1.0, pass == 1 ? 0.0 : (double)deg);
        const int k = pass == 0   ? dist_k
                      : pass == 1 ? (int)uni((uint32_t)rc->adj_index)
                      : pass == 2 ? (int)uni((uint32_t)rc->lap_index)
                                  : (int)uni((uint32_t)rc->slap_index);
        const double R = dense_tridiag_wave<ROWS, true>(w, n, lane, row, in);
        dense_set_by_pass(eig, pass, dense_multisection_wave(w, n, lane, n - 1 - k, R)); // ascending index j = n - 1 - k
    }
    double randic = 0.0;
    int z1 = 0, z2 = 0, tri = 0;
    if (need >> DENSE_INVX_RANDIC) dense_degree_sums_wave(adj, n, lane, in, all, deg, randic, z1, z2, tri);
    dense_bfs_invariants(s, n, out.inv);
    out.inv[DENSE_INV_ADJ_EIG] = eig[1];
    out.inv[DENSE_INV_DIST_EIG] = eig[0];
    out.inv[DENSE_INVX_LAP_EIG] = eig[2];
    out.inv[DENSE_INVX_SLAP_EIG] = eig[3];
    out.inv[DENSE_INVX_RANDIC] = has(DENSE_INVX_RANDIC) ? randic : 0.0;
    out.inv[DENSE_INVX_ZAGREB1] = has(DENSE_INVX_ZAGREB1) ? (double)z1 : 0.0;
    out.inv[DENSE_INVX_ZAGREB2] = has(DENSE_INVX_ZAGREB2) ? (double)z2 : 0.0;
    out.inv[DENSE_INVX_TRIANGLES] = has(DENSE_INVX_TRIANGLES) ? (double)(tri / 3) : 0.0;
    double c = dense_weighted_sum<DENSE_INVX_COUNT>(rc->bias, rc->weight, out.inv);
    // the pair terms pick their invariants by a run-time index: from w.v, which the passes are done with (the host has checked 0 <= a, b < 16)
    const int n_terms = (int)uni((uint32_t)rc->n_terms);
    if (n_terms > 0) {
        LDS_SYNC();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < DENSE_INVX_COUNT; ++i) w.v[i] = out.inv[i];
        }
        LDS_SYNC();
    }
#pragma unroll 1
    for (int tt = 0; tt < n_terms; ++tt) {
        const double coef = rc->term[tt].coef;
        if (coef == 0.0) continue;
        const double ia = w.v[uni((uint32_t)rc->term[tt].a) & (DENSE_INVX_COUNT - 1)], ib = w.v[uni((uint32_t)rc->term[tt].b) & (DENSE_INVX_COUNT - 1)];
        const double v = uni((uint32_t)rc->term[tt].op) == (uint32_t)DENSE_INVX_DIV ? ia / ib : ia * ib;
        const double term = coef * v;
        c = c + term;
    }
    out.dist_k = dist_k;
    out.computed = DENSE_INV_ALWAYS | need;
    out.cost = (float)c;
    out.eval = rc->eval_scale * (out.cost + rc->eval_offset);
}

// ---------------------------------------------------------------- the extended invariant cost as a DenseSpace's cost policy
// (dense_spectral.inc: DenseCostRecipeT -- a wave's block is the AH block of the same row limit, so the pool step plans the INV
// tiers' waves; the recipe lies behind sixteen doubles per agent).  Named structs, not aliases: the kernels' names carry them
// (k_rollout<DenseSpace<2, DenseCostInvX>>)
struct DenseInvxCostFn {
    template <class W, class Hook>
    __device__ static __forceinline__ void run(const uint64_t *adj, W &w, const int n, const DenseInvxRecipe *rc, Hook &&hook, DenseInvxCost &out) {
        dense_invx_cost_wave(adj, w, n, rc, hook, out);
    }
};
struct DenseCostInvX : DenseCostRecipeT<DenseInvxCost, DenseInvxRecipe, DENSE_INVX_COUNT, DENSE_INVX_MAX_N, DenseInvxArgminRec, DenseInvxCostFn> {};
struct DenseCostInvXWide : DenseCostRecipeT<DenseInvxCost, DenseInvxRecipe, DENSE_INVX_COUNT, DENSE_INVX_WIDE_MAX_N, DenseInvxWideArgminRec, DenseInvxCostFn> {};

// The cost outside any engine (space_ops.h: launch_probe_invx_cost, launch_probe_invx_cost_wide): one wave per graph, `reps`
// repetitions (timing), the result of the last one.  Each unit launches the instantiation of its own row limit.  The host has
// checked the graphs and the recipe (engine_probes.hip): LDS is indexed by the bits of adj, and the pair terms' indices pick among
// sixteen registers.
template <int ROWS>
__global__ __launch_bounds__(64) void k_probe_invx_cost(const uint64_t *__restrict__ adj, const int n, const int count, const int reps,
                                                        const DenseInvxRecipe *__restrict__ recipe, DenseInvxCost *__restrict__ out) {
    __shared__ uint64_t s_adj[ROWS];
    __shared__ DenseAhLdsT<ROWS> w;
    const int g = blockIdx.x;
    if (g >= count) return;
    if (LANE < ROWS) s_adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    DenseInvxCost c;
    for (int r = 0; r < reps; ++r) {
        dense_invx_cost_wave(s_adj, w, n, recipe, DenseNoHook{}, c);
        LDS_SYNC();
    }
    if (LANE == 0) out[g] = c;
}
