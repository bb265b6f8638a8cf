// dense_inv_cost.inc -- the weighted-invariant cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_ah_cost.inc, whose LDS layout and constants it uses).
//
// BUILD-DEFINED (c21_host.h: DenseInvRecipe; DESIGN.md "The invariant cost"): ten invariants in a fixed order --
//   0 edges  1 max_degree  2 min_degree  3 diameter  4 radius  5 proximity  6 remoteness  7 avg_distance  8 adj_eig  9 dist_eig
// -- combined with weights the caller gives at RUN time: c = bias, then c = c + weight[i] * I_i for every i whose weight is not
// zero, in order; cost = (f32)c; eval = eval_scale * (cost + eval_offset).  One build serves a family of objectives of the
// AutoGraphiX shape; the Aouchiche-Hansen cost is one recipe among them (weight[5] = weight[9] = 1, the AH index rule, offset 2,
// scale 1 / (2 n + 2)) and comes out bit for bit as dense_ah_cost_wave gives it.  The matching number is deliberately not in the
// list: it needs the default cost's per-node matching arena and its repair, and lambda_1 + mu stays DenseCostC21's objective.
//
// Stages and lane roles are dense_ah_cost_wave's: all-sources BFS (lane u is source u; it also yields the degree, eccentricity and
// transmission of u, reduced over the wave), Householder reduction in the packed lower triangle (lane r owns row r), Sturm-count
// multisection for ONE eigenvalue by index (lane l owns shift l), every f64 step one IEEE operation, every f64 reduction the
// xor-butterfly.  They are written out again here instead of being shared with dense_ah_cost.inc, so that the AH units compile
// to the code they compiled to before.
// One triangle serves both spectral invariants, one after the other.  The BFS leaves the distances in it, so the DISTANCE pass
// runs first, on those rows; the ADJACENCY pass then refills the triangle with 0 / 1 from the bitsets, which are still in LDS.
// So the BFS neither runs again nor keeps its rows anywhere else, and the wave's LDS block is the AH block's size at either row limit.  The
// two values do not depend on the order they are computed in; the cost takes them in index order (adj_eig, then dist_eig).
// A spectral invariant whose weight is zero is not computed (a wave-uniform branch: the recipe is the same for all lanes): its
// value is 0.0 and its bit of `computed` is clear.
//
// The row limit ROWS is a template parameter of everything here that depends on it, as in dense_ah_cost.inc: 32 (DenseCostInv:
// dense_inv_kernels.hip, AZD_ENGINE_DENSE_INV) or 64 (DenseCostInvWide: dense_inv_wide_kernels.hip, AZD_ENGINE_DENSE_INV_WIDE beside
// the first flag: a triangle of 2080 doubles), and the engine's argmin record follows from it.  Order of operations, lane roles
// and reductions do not depend on it: at n <= 32 the two compute the same bits.  At every n and either row limit a Householder step
// whose column tail is below DENSE_INV_DEFLATE is skipped like one whose tail is zero (c21_host.h: a rank-deficient adjacency
// matrix otherwise runs the reduction into subnormal squares and NaN -- after some 20 steps on K(10,11) or a double broom with
// the heavier end first; from 19 vertices on).
__device__ __forceinline__ uint32_t dense_inv_sum_u32(uint32_t v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v += (uint32_t)__shfl_xor((int)v, w, 64);
    return uni(v);
}

// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  rc: the recipe in device memory, the same address in
// every lane.  hook: called once, after the BFS (the pool step's deferred post).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_inv_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const DenseInvRecipe *rc,
                                                    Hook &&hook, DenseInvCost &out) {
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const uint64_t all = ROWS < 64 ? (1ull << n) - 1ull : ~0ull >> (64 - n); // (64 rows: n = 64 must not shift by 64; n >= 4)
    const bool need_adj = uni(rc->weight[DENSE_INV_ADJ_EIG] != 0.0 ? 1u : 0u) != 0u;
    const bool need_dist = uni(rc->weight[DENSE_INV_DIST_EIG] != 0.0 ? 1u : 0u) != 0u;
    const int adj_index = (int)uni((uint32_t)rc->adj_index), dist_index = (int)uni((uint32_t)rc->dist_index);
    // ---- BFS from every vertex at once
    int t = 0, d = 0, deg = 0;
    if (in) {
        deg = __popcll(adj[lane] & all);
        if (need_dist) w.A[row + lane] = 0.0;
        uint64_t seen = 1ull << lane, frontier = seen;
        for (;;) {
            uint64_t next = 0;
            for (uint64_t f = frontier; f; f &= f - 1ull) next |= adj[__ffsll((unsigned long long)f) - 1];
            next &= ~seen & all;
            if (!next) break;
            ++d;
            if (need_dist)
                for (uint64_t m = next & ((1ull << lane) - 1ull); m; m &= m - 1ull) w.A[row + __ffsll((unsigned long long)m) - 1] = (double)d;
            t += d * __popcll(next);
            seen |= next;
            frontier = next;
        }
    }
    const int min_t = (int)wave_min_u32(in ? (uint32_t)t : 0xFFFFFFFFu), max_t = (int)wave_max_u32(in ? (uint32_t)t : 0u);
    const int diam = (int)wave_max_u32(in ? (uint32_t)d : 0u), rad = (int)wave_min_u32(in ? (uint32_t)d : 0xFFFFFFFFu);
    const int max_deg = (int)wave_max_u32(in ? (uint32_t)deg : 0u), min_deg = (int)wave_min_u32(in ? (uint32_t)deg : 0xFFFFFFFFu);
    const int sum_t = (int)dense_inv_sum_u32((uint32_t)t), m2 = (int)dense_inv_sum_u32((uint32_t)deg); // (lanes >= n hold 0)
    hook();
    const int q23 = (2 * diam) / 3;
    const int dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : q23 >= 1 ? q23 - 1 : n - 1;
    double eig_adj = 0.0, eig_dist = 0.0;
    // ---- the spectral passes: 0 = distance matrix (the BFS's rows), 1 = adjacency matrix (refilled from the bitsets)
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !need_dist : !need_adj) continue;
        if (pass == 1) {
            LDS_SYNC();
            if (in) {
                const uint64_t nb = adj[lane];
                for (int c = 0; c <= lane; ++c) w.A[row + c] = (nb >> c) & 1ull ? 1.0 : 0.0;
            }
        }
        const int k = pass == 0 ? dist_k : adj_index;
        // Householder reduction: step i clears column i below row i + 1; lane i keeps (diag_i, sub_i)
        double dg = 0.0, sb = 0.0;
#pragma unroll 1
        for (int i = 0; i + 2 < n; ++i) {
            LDS_SYNC();
            const bool act = in && lane > i;
            const double x = act ? w.A[row + i] : 0.0;
            const double tail = dense_tree_sum(lane > i + 1 ? x * x : 0.0);
            const double x1 = __shfl(x, i + 1, 64);
            if (lane == i) dg = w.A[row + i];
            // (the column is tridiagonal already -- adjacency matrices: often -- or is rounding noise of a matrix whose rank is used
            // up: c21_host.h, DENSE_INV_DEFLATE.  At every n and either row limit)
            if (tail == 0.0 || tail < DENSE_INV_DEFLATE) {
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
        // multisection for the eigenvalue of ascending index j = n - 1 - k (the `c <= j` rule and the TINY pivot guard as in the AH cost:
        // repeated eigenvalues -- K_n, stars -- depend on both)
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
        if (pass == 0) eig_dist = eig;
        else eig_adj = eig;
    }
    out.inv[0] = (double)(m2 / 2);
    out.inv[1] = (double)max_deg;
    out.inv[2] = (double)min_deg;
    out.inv[3] = (double)diam;
    out.inv[4] = (double)rad;
    out.inv[5] = (double)min_t / (double)(n - 1);
    out.inv[6] = (double)max_t / (double)(n - 1);
    out.inv[7] = (double)sum_t / (double)(n * (n - 1));
    out.inv[DENSE_INV_ADJ_EIG] = eig_adj;
    out.inv[DENSE_INV_DIST_EIG] = eig_dist;
    double c = rc->bias;
#pragma unroll
    for (int i = 0; i < DENSE_INV_COUNT; ++i) {
        const double wi = rc->weight[i];
        const double term = wi * out.inv[i];
        if (wi != 0.0) c = c + term;
    }
    out.dist_k = dist_k;
    out.computed = DENSE_INV_ALWAYS | (need_adj ? 1u << DENSE_INV_ADJ_EIG : 0u) | (need_dist ? 1u << DENSE_INV_DIST_EIG : 0u);
    out.cost = (float)c;
    out.eval = rc->eval_scale * (out.cost + rc->eval_offset);
}

// ---------------------------------------------------------------- the weighted-invariant cost as a DenseSpace's cost policy (space_dense.inc)
// A wave's block is the AH block of the same row limit (DenseAhSpaceLdsT<KW, ROWS>: at 32 rows the pool step plans 10 / 9 / 7 waves at
// key widths 2 / 4 / 10, at 64 rows what the LDS holds, as there).  4 <= n <= ROWS, so E <= 496 or 2016.
// The recipe reaches the kernels without a field of Arenas (every search kernel receives that block): it lies in device memory
// behind the per-agent cost arrays.  An agent's record between launches:
//   cur_lambda[i B + t] = I_i, i = 0 .. 9;  cur_lambda + 10 B: the engine's DenseInvRecipe (azd_engine_set_dense_inv_recipe)
//   cur_mu[t] = the distance index used, cur_mu[B + t] = the `computed` mask.  No per-node arena: node_mate is null.
// The record is written where it is computed (evaluate, root_cost: lane 0, like the new node's tree record) and read by the host
// alone: St carries nothing of the cost from call to call, so load_cost / store_cost have nothing to move -- twenty-two words a
// wave does not hold across the search loop.  A call that creates no node leaves the record of the last one that did, as the
// other costs' load / store pairs do.
__device__ __forceinline__ const DenseInvRecipe *dense_inv_recipe(const Arenas &a) {
    return reinterpret_cast<const DenseInvRecipe *>(a.cur_lambda + (size_t)DENSE_INV_COUNT * (size_t)a.B);
}
template <int ROWS>
struct DenseCostInvT {
    using ArgminRec = std::conditional_t<ROWS == DENSE_INV_MAX_N, DenseInvArgminRec, DenseInvWideArgminRec>; // (what engine.hip sizes argmin_d for)
    template <int KW_>
    using Lds = DenseAhSpaceLdsT<KW_, ROWS>;
    template <int KW_>
    struct St {
        uint64_t rem[KW_];
    };
    struct Replay {
        DenseInvCost c;
        float ev;
    };
    template <class S>
    __device__ static __forceinline__ void new_node_begin(S &, const uint32_t, const uint32_t) {}
    template <class L>
    __device__ static __forceinline__ void new_node_end(const Arenas &, const int, L &, const uint32_t) {}
    template <class S>
    __device__ static __forceinline__ void load_cost(const Arenas &, const int, S &) {}
    template <class S>
    __device__ static __forceinline__ void store_cost(const Arenas &, const int, const S &) {}
    __device__ static __forceinline__ void keep(const Arenas &a, const int t, const DenseInvCost &c) { // (one lane)
#pragma unroll
        for (int i = 0; i < DENSE_INV_COUNT; ++i) a.cur_lambda[(size_t)i * a.B + t] = c.inv[i];
        a.cur_mu[t] = c.dist_k;
        a.cur_mu[a.B + t] = (int32_t)c.computed;
    }
    template <class L, class S, class Hook>
    __device__ static __forceinline__ float evaluate(const Arenas &a, L &s, S &, const int t, Hook &&hook) {
        const unsigned long long ph0 = PH_NOW();
        DenseInvCost c;
        dense_inv_cost_wave(s.adj, s.ah, a.n, dense_inv_recipe(a), hook, c);
        if (LANE == 0) keep(a, t, c);
        CTR_ADD(22, PH_NOW() - ph0);
        return c.eval;
    }
    template <class L, class S>
    __device__ static __forceinline__ float root_cost(const Arenas &a, const int t, L &s, S &) {
        DenseInvCost c;
        dense_inv_cost_wave(s.adj, s.ah, a.n, dense_inv_recipe(a), DenseNoHook{}, c);
        if (LANE == 0) keep(a, t, c);
        return c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_cost(const Arenas &a, L &s, Replay &r) {
        dense_inv_cost_wave(s.adj, s.ah, a.n, dense_inv_recipe(a), DenseNoHook{}, r.c);
        r.ev = r.c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_write(const Arenas &a, L &s, const Replay &r, const int wt, const uint32_t win_node) {
        ArgminRec *out = reinterpret_cast<ArgminRec *>(a.argmin_d);
        if (LANE < ROWS) out->adj[LANE] = LANE < a.n ? s.adj[LANE] : 0ull;
        if (LANE < (int)(sizeof(out->permitted) / sizeof(uint64_t))) out->permitted[LANE] = s.slotmask[LANE];
        if (LANE == 0) {
#pragma unroll
            for (int i = 0; i < DENSE_INV_COUNT; ++i) out->inv[i] = r.c.inv[i];
            out->dist_k = r.c.dist_k;
            out->computed = r.c.computed;
            out->cost = r.c.cost;
            out->eval = r.c.eval;
            out->agent = wt;
            out->node = win_node;
        }
    }
};
// Named structs, not aliases: the kernels' names carry them (k_rollout<DenseSpace<2, DenseCostInv>>)
struct DenseCostInv : DenseCostInvT<DENSE_INV_MAX_N> {};
struct DenseCostInvWide : DenseCostInvT<DENSE_INV_WIDE_MAX_N> {};

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
