// dense_invs_cost.inc -- the spectrum invariant cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_spectral.inc, whose stages it is composed of).
//
// BUILD-DEFINED (dense_cost_host.h: DenseInvsRecipe; DESIGN.md "The spectrum invariant cost"): twenty-one invariants in a fixed order --
//   0 .. 15 the extended invariant cost's (dense_invx_cost.inc)
//   16 adj_energy  17 dist_energy  18 lap_energy  19 slap_energy  20 adj_spread
// -- combined by a recipe the caller gives at RUN time, by the extended cost's rule over twenty-one weights and up to four pair
// terms.  With weights 16 .. 20 zero and no term naming 16 .. 20 the sequence of operations is dense_invx_cost_wave's, and the
// first sixteen invariants, dist_k, computed, cost and eval come out bit for bit.
//
// Beside the extended cost's stages this one uses the second finisher on the tridiagonal form that every spectral pass leaves in
// w.diag / w.sub2: dense_multisection_wave gives one eigenvalue by index, dense_bisect_all_wave all eigenvalues at once.
// An energy is the xor-butterfly over |theta_l| (adjacency, distance) or |theta_l - s| (Laplacians, s the mean degree), lanes >= n
// holding 0.0; the spread is theta_{n-1} - theta_0 by two shuffles.  Each is folded into its pass: nothing of the finisher but
// its one result is held across the next reduction.
// A matrix is reduced at most once per cost: a pass runs when its *_eig, its energy or (adjacency) the spread is needed; after the
// reduction the multisection runs only for the *_eig, the bisections only for the energy or the spread (wave-uniform branches).
// The row limit ROWS is a template parameter of everything here that depends on it, as in dense_invx_cost.inc: 32 (DenseCostInvS:
// dense_invs_kernels.hip, AZD_ENGINE_DENSE_INVS) or 64 (DenseCostInvSWide: dense_invs_wide_kernels.hip, AZD_ENGINE_DENSE_INVS_WIDE
// beside the first flag: a triangle of 2080 doubles serves the four passes), and the engine's argmin record follows from it.  At 64
// rows and n = 64 every lane owns an eigenvalue of the whole-spectrum finisher, the spread's upper shuffle reads lane 63, and the
// vertex mask is formed without a shift by 64 (dense_vertex_mask).  Order of operations, lane roles and reductions do not depend on
// ROWS: at n <= 32 the two compute the same bits.
//
// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  rc: the recipe in device memory, the same address in
// every lane.  hook: called once, after the BFS (the pool step's deferred post).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_invs_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const DenseInvsRecipe *rc,
                                                     Hook &&hook, DenseInvsCost &out) {
    static_assert(ROWS == DENSE_INVS_MAX_N || ROWS == DENSE_INVS_WIDE_MAX_N, "the row limits that are built");
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const uint64_t all = dense_vertex_mask<ROWS>(n);
    const uint32_t need = uni(dense_invs_needed(*rc));
    const auto has = [need](const int i) { return ((need >> i) & 1u) != 0u; };
    const int dist_index = (int)uni((uint32_t)rc->dist_index);
    int t, d, deg;
    dense_bfs_wave(adj, w, lane, row, in, all, has(DENSE_INV_DIST_EIG) || has(DENSE_INVS_DIST_ENERGY), t, d, deg);
    const DenseBfsSums s = dense_bfs_sums_wave(in, t, d, deg);
    hook();
    const int dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : dense_ah_index(s.diam, n);
    double eig[4] = {0.0, 0.0, 0.0, 0.0}, energy[4] = {0.0, 0.0, 0.0, 0.0}, spread = 0.0; // by pass
    // ---- the spectral passes: 0 = distance matrix (the BFS's rows), then refilled from the bitsets: 1 = adjacency matrix,
    // 2 = Laplacian D - A, 3 = signless Laplacian D + A
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int which = pass == 0 ? DENSE_INV_DIST_EIG : pass == 1 ? DENSE_INV_ADJ_EIG : pass == 2 ? DENSE_INVX_LAP_EIG : DENSE_INVX_SLAP_EIG;
        const int which_energy = pass == 0   ? DENSE_INVS_DIST_ENERGY
                                 : pass == 1 ? DENSE_INVS_ADJ_ENERGY
                                 : pass == 2 ? DENSE_INVS_LAP_ENERGY
                                             : DENSE_INVS_SLAP_ENERGY;
        const bool want_eig = has(which), want_energy = has(which_energy), want_spread = pass == 1 && has(DENSE_INVS_ADJ_SPREAD);
        if (!(want_eig || want_energy || want_spread)) continue;
        if (pass > 0) dense_refill_wave(adj, w, lane, row, in, pass == 2 ? -1.0 : 1.0, pass == 1 ? 0.0 : (double)deg);
        const double R = dense_tridiag_wave<ROWS, true>(w, n, lane, row, in);
        if (want_eig) {
            const int k = pass == 0   ? dist_k
                          : pass == 1 ? (int)uni((uint32_t)rc->adj_index)
                          : pass == 2 ? (int)uni((uint32_t)rc->lap_index)
                                      : (int)uni((uint32_t)rc->slap_index);
            dense_set_by_pass(eig, pass, dense_multisection_wave(w, n, lane, n - 1 - k, R)); // ascending index j = n - 1 - k
        }
        if (want_energy || want_spread) {
            const double theta = dense_bisect_all_wave(w, n, lane, R);
            if (want_energy) {
                const double shift = (double)s.m2 / (double)n; // the mean degree: the centre of the Laplacian energies
                const double a = !in ? 0.0 : pass >= 2 ? fabs(theta - shift) : fabs(theta);
                dense_set_by_pass(energy, pass, dense_tree_sum(a));
            }
            if (want_spread) spread = __shfl(theta, n - 1, 64) - __shfl(theta, 0, 64);
        }
    }
    double randic = 0.0;
    int z1 = 0, z2 = 0, tri = 0;
    if ((need >> DENSE_INVX_RANDIC) & 0xFu) dense_degree_sums_wave(adj, n, lane, in, all, deg, randic, z1, z2, tri);
    dense_bfs_invariants(s, n, out.inv);
    out.inv[DENSE_INV_ADJ_EIG] = eig[1];
    out.inv[DENSE_INV_DIST_EIG] = eig[0];
    out.inv[DENSE_INVX_LAP_EIG] = eig[2];
    out.inv[DENSE_INVX_SLAP_EIG] = eig[3];
    out.inv[DENSE_INVX_RANDIC] = has(DENSE_INVX_RANDIC) ? randic : 0.0;
    out.inv[DENSE_INVX_ZAGREB1] = has(DENSE_INVX_ZAGREB1) ? (double)z1 : 0.0;
    out.inv[DENSE_INVX_ZAGREB2] = has(DENSE_INVX_ZAGREB2) ? (double)z2 : 0.0;
    out.inv[DENSE_INVX_TRIANGLES] = has(DENSE_INVX_TRIANGLES) ? (double)(tri / 3) : 0.0;
    out.inv[DENSE_INVS_ADJ_ENERGY] = energy[1];
    out.inv[DENSE_INVS_DIST_ENERGY] = energy[0];
    out.inv[DENSE_INVS_LAP_ENERGY] = energy[2];
    out.inv[DENSE_INVS_SLAP_ENERGY] = energy[3];
    out.inv[DENSE_INVS_ADJ_SPREAD] = spread;
    double c = dense_weighted_sum<DENSE_INVS_COUNT>(rc->bias, rc->weight, out.inv);
    // the pair terms pick their invariants by a run-time index: from w.v, which the passes are done with (the host has checked
    // 0 <= a, b < 21; the bound below keeps an unchecked index inside w.v all the same)
    const int n_terms = (int)uni((uint32_t)rc->n_terms);
    if (n_terms > 0) {
        LDS_SYNC();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < DENSE_INVS_COUNT; ++i) w.v[i] = out.inv[i];
        }
        LDS_SYNC();
    }
    static_assert(DENSE_INVS_COUNT <= ROWS, "the pair terms' operands lie in w.v");
#pragma unroll 1
    for (int tt = 0; tt < n_terms; ++tt) {
        const double coef = rc->term[tt].coef;
        if (coef == 0.0) continue;
        const uint32_t ta = uni((uint32_t)rc->term[tt].a), tb = uni((uint32_t)rc->term[tt].b);
        const double ia = w.v[ta < (uint32_t)DENSE_INVS_COUNT ? ta : 0u], ib = w.v[tb < (uint32_t)DENSE_INVS_COUNT ? tb : 0u];
        const double v = uni((uint32_t)rc->term[tt].op) == (uint32_t)DENSE_INVX_DIV ? ia / ib : ia * ib;
        const double term = coef * v;
        c = c + term;
    }
    out.dist_k = dist_k;
    out.computed = DENSE_INV_ALWAYS | need;
    out.cost = (float)c;
    out.eval = rc->eval_scale * (out.cost + rc->eval_offset);
}

// ---------------------------------------------------------------- the spectrum invariant cost as a DenseSpace's cost policy
// (dense_spectral.inc: DenseCostRecipeT -- a wave's block is the AH block of the same row limit, the recipe lies behind twenty-one
// doubles per agent).  No pool searchers are built with these policies: dense_invs_kernels.hip, dense_invs_wide_kernels.hip.
struct DenseInvsCostFn {
    template <class W, class Hook>
    __device__ static __forceinline__ void run(const uint64_t *adj, W &w, const int n, const DenseInvsRecipe *rc, Hook &&hook, DenseInvsCost &out) {
        dense_invs_cost_wave(adj, w, n, rc, hook, out);
    }
};
// Named structs, not aliases: the kernels' names carry them (k_rollout<DenseSpace<2, DenseCostInvS>>)
struct DenseCostInvS : DenseCostRecipeT<DenseInvsCost, DenseInvsRecipe, DENSE_INVS_COUNT, DENSE_INVS_MAX_N, DenseInvsArgminRec, DenseInvsCostFn> {};
struct DenseCostInvSWide : DenseCostRecipeT<DenseInvsCost, DenseInvsRecipe, DENSE_INVS_COUNT, DENSE_INVS_WIDE_MAX_N, DenseInvsWideArgminRec, DenseInvsCostFn> {};

// The cost outside any engine (space_ops.h: launch_probe_invs_cost, launch_probe_invs_cost_wide): one wave per graph, `reps`
// repetitions (timing), the result of the last one.  Each unit launches the instantiation of its own row limit.  The host has
// checked the graphs and the recipe (engine_probes.hip): LDS is indexed by the bits of adj.
template <int ROWS>
__global__ __launch_bounds__(64) void k_probe_invs_cost(const uint64_t *__restrict__ adj, const int n, const int count, const int reps,
                                                        const DenseInvsRecipe *__restrict__ recipe, DenseInvsCost *__restrict__ out) {
    __shared__ uint64_t s_adj[ROWS];
    __shared__ DenseAhLdsT<ROWS> w;
    const int g = blockIdx.x;
    if (g >= count) return;
    if (LANE < ROWS) s_adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    DenseInvsCost c;
    for (int r = 0; r < reps; ++r) {
        dense_invs_cost_wave(s_adj, w, n, recipe, DenseNoHook{}, c);
        LDS_SYNC();
    }
    if (LANE == 0) out[g] = c;
}
