// dense_inv_cost.inc -- the weighted-invariant cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_spectral.inc, whose stages it is composed of).
//
// BUILD-DEFINED (dense_cost_host.h: DenseInvRecipe; DESIGN.md "The invariant cost"): ten invariants in a fixed order --
//   0 edges  1 max_degree  2 min_degree  3 diameter  4 radius  5 proximity  6 remoteness  7 avg_distance  8 adj_eig  9 dist_eig
// -- combined with weights the caller gives at RUN time: c = bias, then c = c + weight[i] * I_i for every i whose weight is not
// zero, in order; cost = (f32)c; eval = eval_scale * (cost + eval_offset).  One build serves a family of objectives of the
// AutoGraphiX shape; the Aouchiche-Hansen cost is one recipe among them (weight[5] = weight[9] = 1, the AH index rule, offset 2,
// scale 1 / (2 n + 2)) and comes out bit for bit as dense_ah_cost_wave gives it.  The matching number is deliberately not in the
// list: it needs the default cost's per-node matching arena and its repair, and lambda_1 + mu stays DenseCostC21's objective.
//
// One triangle serves both spectral invariants, one after the other.  The BFS leaves the distances in it, so the DISTANCE pass
// runs first, on those rows; the ADJACENCY pass then refills the triangle with 0 / 1 from the bitsets, which are still in LDS.
// So the BFS neither runs again nor keeps its rows anywhere else, and the wave's LDS block is the AH block's size at either row limit.  The
// two values do not depend on the order they are computed in; the cost takes them in index order (adj_eig, then dist_eig).
// A spectral invariant whose weight is zero is not computed (a wave-uniform branch: the recipe is the same for all lanes): its
// value is 0.0 and its bit of `computed` is clear.  Both reductions deflate (dense_spectral.inc: dense_tridiag_wave).
//
// The row limit ROWS is a template parameter of everything here that depends on it: 32 (DenseCostInv: dense_inv_kernels.hip,
// AZD_ENGINE_DENSE_INV) or 64 (DenseCostInvWide: dense_inv_wide_kernels.hip, AZD_ENGINE_DENSE_INV_WIDE beside the first flag),
// and the engine's argmin record follows from it.
//
// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  rc: the recipe in device memory, the same address in
// every lane.  hook: called once, after the BFS (the pool step's deferred post).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_inv_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const DenseInvRecipe *rc,
                                                    Hook &&hook, DenseInvCost &out) {
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const bool need_adj = uni(rc->weight[DENSE_INV_ADJ_EIG] != 0.0 ? 1u : 0u) != 0u;
    const bool need_dist = uni(rc->weight[DENSE_INV_DIST_EIG] != 0.0 ? 1u : 0u) != 0u;
    const int adj_index = (int)uni((uint32_t)rc->adj_index), dist_index = (int)uni((uint32_t)rc->dist_index);
    int t, d, deg;
    dense_bfs_wave(adj, w, lane, row, in, dense_vertex_mask<ROWS>(n), need_dist, t, d, deg);
    const DenseBfsSums s = dense_bfs_sums_wave(in, t, d, deg);
    hook();
    const int dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : dense_ah_index(s.diam, n);
    double eig_adj = 0.0, eig_dist = 0.0;
    // ---- the spectral passes: 0 = distance matrix (the BFS's rows), 1 = adjacency matrix (refilled from the bitsets)
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !need_dist : !need_adj) continue;
        if (pass == 1) dense_refill_wave(adj, w, lane, row, in, 1.0, 0.0);
        const int k = pass == 0 ? dist_k : adj_index;
        const double R = dense_tridiag_wave<ROWS, true>(w, n, lane, row, in);
        const double eig = dense_multisection_wave(w, n, lane, n - 1 - k, R); // ascending index j = n - 1 - k
        if (pass == 0) eig_dist = eig;
        else eig_adj = eig;
    }
    dense_bfs_invariants(s, n, out.inv);
    out.inv[DENSE_INV_ADJ_EIG] = eig_adj;
    out.inv[DENSE_INV_DIST_EIG] = eig_dist;
    const double c = dense_weighted_sum<DENSE_INV_COUNT>(rc->bias, rc->weight, out.inv);
    out.dist_k = dist_k;
    out.computed = DENSE_INV_ALWAYS | (need_adj ? 1u << DENSE_INV_ADJ_EIG : 0u) | (need_dist ? 1u << DENSE_INV_DIST_EIG : 0u);
    out.cost = (float)c;
    out.eval = rc->eval_scale * (out.cost + rc->eval_offset);
}

// ---------------------------------------------------------------- the weighted-invariant cost as a DenseSpace's cost policy
// (dense_spectral.inc: DenseCostRecipeT -- a wave's block is the AH block of the same row limit, the recipe lies behind ten
// doubles per agent).  Named structs, not aliases: the kernels' names carry them (k_rollout<DenseSpace<2, DenseCostInv>>)
struct DenseInvCostFn {
    template <class W, class Hook>
    __device__ static __forceinline__ void run(const uint64_t *adj, W &w, const int n, const DenseInvRecipe *rc, Hook &&hook, DenseInvCost &out) {
        dense_inv_cost_wave(adj, w, n, rc, hook, out);
    }
};
struct DenseCostInv : DenseCostRecipeT<DenseInvCost, DenseInvRecipe, DENSE_INV_COUNT, DENSE_INV_MAX_N, DenseInvArgminRec, DenseInvCostFn> {};
struct DenseCostInvWide : DenseCostRecipeT<DenseInvCost, DenseInvRecipe, DENSE_INV_COUNT, DENSE_INV_WIDE_MAX_N, DenseInvWideArgminRec, DenseInvCostFn> {};

// The cost outside any engine (space_ops.h: launch_probe_inv_cost, launch_probe_inv_cost_wide): one wave per graph, `reps`
// repetitions (timing), the result of the last one.  Each unit launches the instantiation of its own row limit.  The host has
// checked the graphs and the recipe (engine_probes.hip): LDS is indexed by the bits of adj.
template <int ROWS>
__global__ __launch_bounds__(64) void k_probe_inv_cost(const uint64_t *__restrict__ adj, const int n, const int count, const int reps,
                                                       const DenseInvRecipe *__restrict__ recipe, DenseInvCost *__restrict__ out) {
    __shared__ uint64_t s_adj[ROWS];
    __shared__ DenseAhLdsT<ROWS> w;
    const int g = blockIdx.x;
    if (g >= count) return;
    if (LANE < ROWS) s_adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    DenseInvCost c;
    for (int r = 0; r < reps; ++r) {
        dense_inv_cost_wave(s_adj, w, n, recipe, DenseNoHook{}, c);
        LDS_SYNC();
    }
    if (LANE == 0) out[g] = c;
}
