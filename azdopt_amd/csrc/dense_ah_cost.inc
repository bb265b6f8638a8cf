// dense_ah_cost.inc -- the Aouchiche-Hansen cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_spectral.inc, whose stages it is composed of).
//
// The objective is the reference's ConnectedBitsetGraph::ah_cost (graph-state/src/simple_graph/connected_bitset_graph/
// mod.rs:156-198; the objective of examples/05-ah.rs), restated:
//   BFS from every vertex over the bitsets -> distance matrix d(u, v), transmissions t(u) = sum_v d(u, v), diameter D
//   proximity pi = min_u t(u) / (n - 1);  k = 2D/3 - 1, or n - 1 when 2D/3 = 0 (checked_sub(1).unwrap_or(N - 1))
//   cost = (f32)(pi + entry k of the distance matrix's eigenvalues sorted descending)
// and, BUILD-DEFINED in the image of the dense space's squish, eval = slope (cost + 2) with slope = 1 / (2 n + 2).
//
// The eigenvalue procedure stands in for faer's (as the power iteration does for lambda_1): Householder reduction of the
// distance matrix to tridiagonal form in LDS, then a Sturm-count multisection for the ONE eigenvalue wanted -- DENSE_AH_ROUNDS
// rounds from the Gershgorin radius (dense_spectral.inc).  dense_cost_host.cpp dense_ah_cost_host and tests/dense_ah_ref.py run the same
// sequence and agree bit for bit.  The reduction does not deflate: distance matrices of connected graphs are what it has always
// reduced, to these bits.
//
// The row limit ROWS is a template parameter of everything here that depends on it: 32 (DenseCostAH: dense_ah_kernels.hip,
// AZD_ENGINE_DENSE_AH) or 64 (DenseCostAhWide: dense_ah_wide_kernels.hip, AZD_ENGINE_DENSE_AH_WIDE), and the engine's argmin
// record follows from it -- one library may instantiate both.
//
// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  hook: called once, after the BFS (the pool
// step's deferred post, as in dense_lambda1_wave).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_ah_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const float slope, Hook &&hook, DenseAhCost &out) {
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    int t, d, deg;
    dense_bfs_wave(adj, w, lane, row, in, dense_vertex_mask<ROWS>(n), true, t, d, deg);
    const int min_t = (int)wave_min_u32(in ? (uint32_t)t : 0xFFFFFFFFu);
    const int diam = (int)wave_max_u32(in ? (uint32_t)d : 0u);
    hook();
    const double prox = (double)min_t / (double)(n - 1);
    const int k = dense_ah_index(diam, n);
    const double R = dense_tridiag_wave<ROWS, false>(w, n, lane, row, in);
    const double eig = dense_multisection_wave(w, n, lane, n - 1 - k, R); // ascending index j = n - 1 - k
    out.proximity = prox;
    out.eigenvalue = eig;
    out.diameter = diam;
    out.k = k;
    out.cost = (float)(prox + eig);
    out.eval = slope * (out.cost + 2.0f);
}

// ---------------------------------------------------------------- the AH cost as a DenseSpace's cost policy (space_dense.inc)
// A wave's block is DenseAhSpaceLdsT<KW, ROWS> (dense_spectral.inc).
// An agent's record between launches lives in the arrays the default cost uses, twice as long (engine.hip allocates 2 B entries):
// cur_lambda[t] = pi, cur_lambda[B + t] = eigenvalue, cur_mu[t] = D, cur_mu[B + t] = k.  No per-node arena: node_mate is null.
template <int ROWS>
struct DenseCostAhT {
    using ArgminRec = std::conditional_t<ROWS == DENSE_AH_MAX_N, DenseAhArgminRec, DenseAhWideArgminRec>; // (what engine.hip sizes argmin_d for)
    template <int KW_>
    using Lds = DenseAhSpaceLdsT<KW_, ROWS>;
    template <int KW_>
    struct St {
        uint64_t rem[KW_];
        double pi, eig;
        int diam, k;
    };
    struct Replay {
        DenseAhCost c;
        float ev;
    };
    template <class S>
    __device__ static __forceinline__ void new_node_begin(S &, const uint32_t, const uint32_t) {}
    template <class L>
    __device__ static __forceinline__ void new_node_end(const Arenas &, const int, L &, const uint32_t) {}
    template <class S>
    __device__ static __forceinline__ void load_cost(const Arenas &a, const int t, S &st) {
        st.pi = a.cur_lambda[t];
        st.eig = a.cur_lambda[a.B + t];
        st.diam = a.cur_mu[t];
        st.k = a.cur_mu[a.B + t];
    }
    template <class S>
    __device__ static __forceinline__ void store_cost(const Arenas &a, const int t, const S &st) { // (one lane)
        a.cur_lambda[t] = st.pi;
        a.cur_lambda[a.B + t] = st.eig;
        a.cur_mu[t] = st.diam;
        a.cur_mu[a.B + t] = st.k;
    }
    template <class S>
    __device__ static __forceinline__ void keep(S &st, const DenseAhCost &c) {
        st.pi = c.proximity;
        st.eig = c.eigenvalue;
        st.diam = c.diameter;
        st.k = c.k;
    }
    template <class L, class S, class Hook>
    __device__ static __forceinline__ float evaluate(const Arenas &a, L &s, S &st, const int, Hook &&hook) {
        const unsigned long long ph0 = PH_NOW();
        DenseAhCost c;
        dense_ah_cost_wave(s.adj, s.ah, a.n, a.eval_slope, hook, c);
        keep(st, c);
        CTR_ADD(22, PH_NOW() - ph0);
        return c.eval;
    }
    template <class L, class S>
    __device__ static __forceinline__ float root_cost(const Arenas &a, const int t, L &s, S &st) {
        DenseAhCost c;
        dense_ah_cost_wave(s.adj, s.ah, a.n, a.eval_slope, DenseNoHook{}, c);
        keep(st, c);
        if (LANE == 0) store_cost(a, t, st);
        return c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_cost(const Arenas &a, L &s, Replay &r) {
        dense_ah_cost_wave(s.adj, s.ah, a.n, a.eval_slope, DenseNoHook{}, r.c);
        r.ev = r.c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_write(const Arenas &a, L &s, const Replay &r, const int wt, const uint32_t win_node) {
        ArgminRec *out = reinterpret_cast<ArgminRec *>(a.argmin_d);
        if (LANE < ROWS) out->adj[LANE] = LANE < a.n ? s.adj[LANE] : 0ull;
        if (LANE < (int)(sizeof(out->permitted) / sizeof(uint64_t))) out->permitted[LANE] = s.slotmask[LANE];
        if (LANE == 0) {
            out->proximity = r.c.proximity;
            out->eigenvalue = r.c.eigenvalue;
            out->diameter = r.c.diameter;
            out->k = r.c.k;
            out->cost = r.c.cost;
            out->eval = r.c.eval;
            out->agent = wt;
            out->node = win_node;
        }
    }
};
// Named structs, not aliases: the kernels' names carry them (k_rollout<DenseSpace<2, DenseCostAH>>)
struct DenseCostAH : DenseCostAhT<DENSE_AH_MAX_N> {};
struct DenseCostAhWide : DenseCostAhT<DENSE_AH_WIDE_MAX_N> {};

// The cost outside any engine (space_ops.h: launch_probe_ah_cost, launch_probe_ah_cost_wide): one wave per graph, `reps` repetitions
// (timing), the result of the last one.  Each AH unit launches the instantiation of its own row limit.
template <int ROWS>
__global__ __launch_bounds__(64) void k_probe_ah_cost(const uint64_t *__restrict__ adj, const int n, const int count, const int reps,
                                                      const float slope, DenseAhCost *__restrict__ out) {
    __shared__ uint64_t s_adj[ROWS];
    __shared__ DenseAhLdsT<ROWS> w;
    const int g = blockIdx.x;
    if (g >= count) return;
    if (LANE < ROWS) s_adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    DenseAhCost c;
    for (int r = 0; r < reps; ++r) {
        dense_ah_cost_wave(s_adj, w, n, slope, DenseNoHook{}, c);
        LDS_SYNC();
    }
    if (LANE == 0) out[g] = c;
}
