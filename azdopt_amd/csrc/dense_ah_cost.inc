// dense_ah_cost.inc -- the Aouchiche-Hansen cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc and space_dense.inc).
//
// The objective is the reference's ConnectedBitsetGraph::ah_cost (graph-state/src/simple_graph/connected_bitset_graph/
// mod.rs:156-198; the objective of examples/05-ah.rs), restated:
//   BFS from every vertex over the bitsets -> distance matrix d(u, v), transmissions t(u) = sum_v d(u, v), diameter D
//   proximity pi = min_u t(u) / (n - 1);  k = 2D/3 - 1, or n - 1 when 2D/3 = 0 (checked_sub(1).unwrap_or(N - 1))
//   cost = (f32)(pi + entry k of the distance matrix's eigenvalues sorted descending)
// and, BUILD-DEFINED in the image of the dense space's squish, eval = slope (cost + 2) with slope = 1 / (2 n + 2).
//
// The eigenvalue procedure stands in for faer's (as the power iteration does for lambda_1): Householder reduction of the
// distance matrix to tridiagonal form in LDS, then a Sturm-count multisection for the ONE eigenvalue wanted -- 64 lanes count at
// 64 shifts, the bracket shrinks by 65 a round, DENSE_AH_ROUNDS rounds from the Gershgorin radius.  Every step is one IEEE f64
// operation (-ffp-contract=off; f64 division and sqrt are correctly rounded on gfx950), every reduction an xor-butterfly = a
// balanced binary tree: c21_host.cpp dense_ah_cost_host and tests/dense_ah_ref.py run the same sequence and agree bit for bit.
//
// Lanes: BFS -- lane u is source u.  Householder -- lane r owns row r of the working matrix.  Multisection -- lane l owns shift l;
// the tridiagonal entries are LDS broadcasts.
// The working matrix is kept as its LOWER TRIANGLE, packed (row r at r (r + 1) / 2: 4.1 KB a wave where the square is 8.3 KB --
// sixteen waves' blocks of the pool step's searchers have to share a CU's 160 KB).  The host form keeps the square; the values are
// the same to the bit, because the rank-two update A_rc - (v_r q_c + q_r v_c) is symmetric in (r, c) operation by operation
// (products and the sum commute), so the square's two triangles never differ.
//
// The row limit ROWS is a template parameter of everything here that depends on it: 32 (DenseCostAH: dense_ah_kernels.hip,
// AZD_ENGINE_DENSE_AH) or 64 (DenseCostAhWide: dense_ah_wide_kernels.hip, AZD_ENGINE_DENSE_AH_WIDE: a triangle of 2080 doubles,
// 16.6 KB a wave), and the engine's argmin record follows from it -- one library may instantiate both.  Order of operations, lane
// roles and reductions do not depend on it: at n <= 32 the two compute the same bits.
__device__ __forceinline__ int dense_ah_at(const int r, const int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }
template <int ROWS>
struct DenseAhLdsT {
    static_assert(ROWS == 32 || ROWS == 64, "the lanes of one wave own the rows");
    static constexpr int TRI = ROWS * (ROWS + 1) / 2;
    double A[TRI]; // distance matrix (lower triangle, packed), reduced in place
    double v[ROWS], q[ROWS]; // Householder vector and its companion, by row
    double diag[ROWS], sub2[ROWS]; // the tridiagonal form: diagonal, squared subdiagonal
};
using DenseAhLds = DenseAhLdsT<DENSE_AH_MAX_N>;
using DenseAhWideLds = DenseAhLdsT<DENSE_AH_WIDE_MAX_N>;

// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  hook: called once, after the BFS (the pool
// step's deferred post, as in dense_lambda1_wave).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_ah_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const float slope, Hook &&hook, DenseAhCost &out) {
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const uint64_t all = ROWS < 64 ? (1ull << n) - 1ull : ~0ull >> (64 - n); // (64 rows: n = 64 must not shift by 64; n >= 4)
    // ---- BFS from every vertex at once
    int t = 0, d = 0;
    if (in) {
        w.A[row + lane] = 0.0;
        uint64_t seen = 1ull << lane, frontier = seen;
        for (;;) {
            uint64_t next = 0;
            for (uint64_t f = frontier; f; f &= f - 1ull) next |= adj[__ffsll((unsigned long long)f) - 1];
            next &= ~seen & all;
            if (!next) break;
            ++d;
            for (uint64_t m = next & ((1ull << lane) - 1ull); m; m &= m - 1ull) w.A[row + __ffsll((unsigned long long)m) - 1] = (double)d;
            t += d * __popcll(next);
            seen |= next;
            frontier = next;
        }
    }
    const int min_t = (int)wave_min_u32(in ? (uint32_t)t : 0xFFFFFFFFu);
    const int diam = (int)wave_max_u32(in ? (uint32_t)d : 0u);
    hook();
    const double prox = (double)min_t / (double)(n - 1);
    const int q23 = (2 * diam) / 3, k = q23 >= 1 ? q23 - 1 : n - 1;
    // ---- Householder reduction: step i clears column i below row i + 1; lane i keeps (diag_i, sub_i)
    double dg = 0.0, sb = 0.0;
#pragma unroll 1
    for (int i = 0; i + 2 < n; ++i) {
        LDS_SYNC();
        const bool act = in && lane > i;
        const double x = act ? w.A[row + i] : 0.0;
        const double tail = dense_tree_sum(lane > i + 1 ? x * x : 0.0);
        const double x1 = __shfl(x, i + 1, 64);
        if (lane == i) dg = w.A[row + i];
        if (tail == 0.0) { // the column is tridiagonal already
            if (lane == i) sb = x1;
            continue;
        }
        const double sigma = tail + x1 * x1;
        const double s = sqrt(sigma);
        const double alpha = x1 >= 0.0 ? -s : s;
        const double v1 = x1 - alpha;
        const double v = lane == i + 1 ? v1 : x;
        const double beta = 2.0 / (tail + v1 * v1);
        if (lane < ROWS) w.v[lane] = v;
        LDS_SYNC();
        double acc = 0.0;
        if (act)
            for (int c = i + 1; c < n; ++c) acc = acc + w.A[dense_ah_at(lane, c)] * w.v[c];
        const double p = act ? beta * acc : 0.0;
        const double vp = dense_tree_sum(v * p);
        const double K = (0.5 * beta) * vp;
        const double q = act ? p - K * v : 0.0;
        if (lane < ROWS) w.q[lane] = q;
        LDS_SYNC();
        if (act)
            for (int c = i + 1; c <= lane; ++c) w.A[row + c] = w.A[row + c] - (v * w.q[c] + q * w.v[c]);
        if (lane == i) sb = alpha;
    }
    LDS_SYNC();
    if (lane == n - 2) {
        dg = w.A[row + lane];
        sb = w.A[dense_ah_at(n - 1, n - 2)];
    }
    if (lane == n - 1) dg = w.A[row + lane];
    // ---- multisection for the eigenvalue of ascending index j = n - 1 - k
    const int j = n - 1 - k;
    const double sb_below = __shfl(sb, lane > 0 ? lane - 1 : 0, 64);
    const double g = (fabs(dg) + (lane > 0 ? fabs(sb_below) : 0.0)) + fabs(sb); // Gershgorin; >= 0: the bit patterns order like the numbers
    const double R = __longlong_as_double((long long)wave_max_u64(in ? (uint64_t)__double_as_longlong(g) : 0ull));
    if (lane < ROWS) {
        w.diag[lane] = dg;
        w.sub2[lane] = sb * sb;
    }
    LDS_SYNC();
    double hi = R + 1.0, lo = -hi;
#pragma unroll 1
    for (int round = 0; round < DENSE_AH_ROUNDS; ++round) {
        const double wd = hi - lo;
        const double x = lo + (wd * (double)(lane + 1)) / 65.0;
        double qq = w.diag[0] - x;
        if (fabs(qq) < DENSE_AH_TINY) qq = -DENSE_AH_TINY;
        int c = qq < 0.0 ? 1 : 0;
        for (int i = 1; i < n; ++i) { // eigenvalues below x = negative pivots of T - x
            const double r = w.sub2[i - 1] / qq;
            qq = (w.diag[i] - x) - r;
            if (fabs(qq) < DENSE_AH_TINY) qq = -DENSE_AH_TINY;
            c += qq < 0.0 ? 1 : 0;
        }
        const int m = __popcll(__ballot(c <= j));
        const double x_lo = __shfl(x, m > 0 ? m - 1 : 0, 64), x_hi = __shfl(x, m < 64 ? m : 63, 64);
        lo = m > 0 ? x_lo : lo;
        hi = m < 64 ? x_hi : hi;
    }
    const double eig = (lo + hi) * 0.5;
    out.proximity = prox;
    out.eigenvalue = eig;
    out.diameter = diam;
    out.k = k;
    out.cost = (float)(prox + eig);
    out.eval = slope * (out.cost + 2.0f);
}

// ---------------------------------------------------------------- the AH cost as a DenseSpace's cost policy (space_dense.inc)
// A wave's block: DenseLds without the matching, with the cost's working set.  4 <= n <= ROWS, so E <= 496 or 2016.
template <int KW_, int ROWS>
struct DenseAhSpaceLdsT {
    uint64_t adj[DENSE_MAX_N];
    double x[32];                    // write_rows_direct's scratch (the present edges as a bitmap: 8 words at 32 rows, 32 at 64, read one past)
    uint64_t slotmask[32];
    uint16_t aid[64 * KW_];
    unsigned long long ctr[NUM_COUNTERS];
    uint16_t seq[4];
    uint32_t stack[PATH_STACK];
    DenseAhLdsT<ROWS> ah;
};
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
