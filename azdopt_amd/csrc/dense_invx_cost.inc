// dense_invx_cost.inc -- the extended invariant cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_ah_cost.inc, whose LDS layout and constants it uses).
//
// BUILD-DEFINED (c21_host.h: DenseInvxRecipe; DESIGN.md "The extended invariant cost"): sixteen invariants in a fixed order --
//   0 edges  1 max_degree  2 min_degree  3 diameter  4 radius  5 proximity  6 remoteness  7 avg_distance  8 adj_eig  9 dist_eig
//   10 lap_eig  11 slap_eig  12 randic  13 zagreb1  14 zagreb2  15 triangles
// -- combined by a recipe the caller gives at RUN time: c = bias, then c = c + weight[i] * I_i for every i whose weight is not zero,
// in order, then c = c + coef_t * (I_a * I_b or I_a / I_b) for every pair term whose coefficient is not zero, in order;
// cost = (f32)c; eval = eval_scale * (cost + eval_offset).  The first ten are dense_inv_cost.inc's, and with weights 10 .. 15 zero
// and no pair term the sequence of operations is that unit's: the weighted-invariant cost, and so the Aouchiche-Hansen cost, are
// recipes of this one and come out bit for bit.
//
// Stages and lane roles are dense_inv_cost_wave's: all-sources BFS (lane u is source u; degree, eccentricity, transmission),
// Householder reduction in the packed lower triangle (lane r owns row r), Sturm-count multisection for ONE eigenvalue by index
// (lane l owns shift l), every f64 step one IEEE operation, every f64 reduction the xor-butterfly.  Householder and multisection
// are written out again here instead of being shared with dense_inv_cost.inc, so that the INV units compile to the code they
// compiled to before.
// One triangle serves up to four spectral passes, one after the other: the DISTANCE pass first, on the rows the BFS left; then the
// ADJACENCY, LAPLACIAN (D - A) and SIGNLESS-LAPLACIAN (D + A) passes, each refilling the triangle from the bitsets, which are still
// in LDS, and the lane's degree.  So the wave's LDS block is the AH block.
// The degree-based invariants run after the passes, in ONE wave-uniform loop over v = 0 .. n - 1: lane u takes v when
// v < u is its neighbour (every edge once, ascending in v), with d_v by a wave-wide shuffle and N(v) by an LDS broadcast.
// Each of the invariants 8 .. 15 is computed only when its weight is not zero or a pair term with a non-zero coefficient names it
// (wave-uniform branches: the recipe is the same for all lanes): otherwise 0.0, and its bit of `computed` is clear.
//
// The row limit ROWS is a template parameter of everything here that depends on it, as in dense_inv_cost.inc: 32 (DenseCostInvX:
// dense_invx_kernels.hip, AZD_ENGINE_DENSE_INVX) or 64 (DenseCostInvXWide: dense_invx_wide_kernels.hip, AZD_ENGINE_DENSE_INVX_WIDE
// beside the first flag: a triangle of 2080 doubles serves the four passes), and the engine's argmin record follows from it.  Order
// of operations, lane roles and reductions do not depend on it: at n <= 32 the two compute the same bits.
__device__ __forceinline__ uint32_t dense_invx_sum_u32(uint32_t v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v += (uint32_t)__shfl_xor((int)v, w, 64);
    return uni(v);
}
// adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read).  rc: the recipe in device memory, the same address in
// every lane.  hook: called once, after the BFS (the pool step's deferred post).  Wave-uniform result in `out`.
template <int ROWS, class Hook>
__device__ __forceinline__ void dense_invx_cost_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int n, const DenseInvxRecipe *rc,
                                                     Hook &&hook, DenseInvxCost &out) {
    static_assert(ROWS == DENSE_INVX_MAX_N || ROWS == DENSE_INVX_WIDE_MAX_N, "the row limits that are built");
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const uint64_t all = ROWS < 64 ? (1ull << n) - 1ull : ~0ull >> (64 - n); // (64 rows: n = 64 must not shift by 64; n >= 4)
    const uint32_t need = uni(dense_invx_needed(*rc));
    const bool need_dist = ((need >> DENSE_INV_DIST_EIG) & 1u) != 0u;
    const int dist_index = (int)uni((uint32_t)rc->dist_index);
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
    const int sum_t = (int)dense_invx_sum_u32((uint32_t)t), m2 = (int)dense_invx_sum_u32((uint32_t)deg); // (lanes >= n hold 0)
    hook();
    const int q23 = (2 * diam) / 3;
    const int dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : q23 >= 1 ? q23 - 1 : n - 1;
    double eig[4] = {0.0, 0.0, 0.0, 0.0}; // by pass
    // ---- the spectral passes: 0 = distance matrix (the BFS's rows), then refilled from the bitsets: 1 = adjacency matrix,
    // 2 = Laplacian D - A, 3 = signless Laplacian D + A
#pragma unroll 1
    for (int pass = 0; pass < 4; ++pass) {
        const int which = pass == 0 ? DENSE_INV_DIST_EIG : pass == 1 ? DENSE_INV_ADJ_EIG : pass == 2 ? DENSE_INVX_LAP_EIG : DENSE_INVX_SLAP_EIG;
        if (!((need >> which) & 1u)) continue;
        if (pass > 0) {
            LDS_SYNC();
            if (in) {
                const uint64_t nb = adj[lane];
                const double off = pass == 2 ? -1.0 : 1.0;
                for (int c = 0; c < lane; ++c) w.A[row + c] = (nb >> c) & 1ull ? off : 0.0;
                w.A[row + lane] = pass == 1 ? 0.0 : (double)deg;
            }
        }
        const int k = pass == 0   ? dist_k
                      : pass == 1 ? (int)uni((uint32_t)rc->adj_index)
                      : pass == 2 ? (int)uni((uint32_t)rc->lap_index)
                                  : (int)uni((uint32_t)rc->slap_index);
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
            // (the column is tridiagonal already -- adjacency and Laplacian matrices: often -- or is rounding noise of a matrix whose
            // rank is used up: c21_host.h, DENSE_INV_DEFLATE)
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
        const double e = (lo + hi) * 0.5;
        eig[0] = pass == 0 ? e : eig[0];
        eig[1] = pass == 1 ? e : eig[1];
        eig[2] = pass == 2 ? e : eig[2];
        eig[3] = pass == 3 ? e : eig[3];
    }
    // ---- the degree-based invariants, after the passes so that nothing of them is held across the reductions (lanes >= n hold 0
    // throughout: deg = 0, no neighbour)
    double randic = 0.0;
    int z1 = 0, z2 = 0, tri = 0;
    if (need >> DENSE_INVX_RANDIC) {
        const uint64_t nb = in ? adj[lane] & all : 0ull;
        double r = 0.0, cc = 0.0; // the lane's sum and the sum of its additions' rounding errors
        int s2 = 0, s3 = 0;
#pragma unroll 1
        for (int v = 0; v < n; ++v) { // (wave-uniform: the shuffle below has every lane active)
            const int dv = __shfl(deg, v, 64);
            const uint64_t nv = adj[v];
            if (v < lane && ((nb >> v) & 1ull)) {
                const double s = sqrt((double)(deg * dv));
                const double term = 1.0 / s;
                // TwoSum (Knuth): t + e == r + term exactly.  Uncompensated, K_27's 351 equal terms round the same way 351 times
                // and the sum leaves the n 2^-52 the invariant is held to (c21_host.h)
                const double t = r + term;
                const double bp = t - r;
                const double ap = t - bp;
                const double e = (r - ap) + (term - bp);
                cc = cc + e;
                r = t;
                s2 += deg * dv;
                s3 += __popcll(nb & nv);
            }
        }
        randic = dense_tree_sum(r + cc);
        z1 = (int)dense_invx_sum_u32((uint32_t)(deg * deg));
        z2 = (int)dense_invx_sum_u32((uint32_t)s2);
        tri = (int)dense_invx_sum_u32((uint32_t)s3);
    }
    const auto has = [need](const int i) { return ((need >> i) & 1u) != 0u; };
    out.inv[0] = (double)(m2 / 2);
    out.inv[1] = (double)max_deg;
    out.inv[2] = (double)min_deg;
    out.inv[3] = (double)diam;
    out.inv[4] = (double)rad;
    out.inv[5] = (double)min_t / (double)(n - 1);
    out.inv[6] = (double)max_t / (double)(n - 1);
    out.inv[7] = (double)sum_t / (double)(n * (n - 1));
    out.inv[DENSE_INV_ADJ_EIG] = eig[1];
    out.inv[DENSE_INV_DIST_EIG] = eig[0];
    out.inv[DENSE_INVX_LAP_EIG] = eig[2];
    out.inv[DENSE_INVX_SLAP_EIG] = eig[3];
    out.inv[DENSE_INVX_RANDIC] = has(DENSE_INVX_RANDIC) ? randic : 0.0;
    out.inv[DENSE_INVX_ZAGREB1] = has(DENSE_INVX_ZAGREB1) ? (double)z1 : 0.0;
    out.inv[DENSE_INVX_ZAGREB2] = has(DENSE_INVX_ZAGREB2) ? (double)z2 : 0.0;
    out.inv[DENSE_INVX_TRIANGLES] = has(DENSE_INVX_TRIANGLES) ? (double)(tri / 3) : 0.0;
    double c = rc->bias;
#pragma unroll
    for (int i = 0; i < DENSE_INVX_COUNT; ++i) {
        const double wi = rc->weight[i];
        const double term = wi * out.inv[i];
        if (wi != 0.0) c = c + term;
    }
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

// ---------------------------------------------------------------- the extended invariant cost as a DenseSpace's cost policy (space_dense.inc)
// A wave's block is the AH block of the same row limit (DenseAhSpaceLdsT<KW, ROWS>), so at 32 rows the pool step plans the INV tier's
// 10 / 9 / 7 waves at key widths 2 / 4 / 10, at 64 rows what the LDS holds, as the INV-wide tier.  4 <= n <= ROWS, so E <= 496 or 2016.
// The recipe lies in device memory behind the per-agent cost arrays, as the INV tier's does.  An agent's record between launches:
//   cur_lambda[i B + t] = I_i, i = 0 .. 15;  cur_lambda + 16 B: the engine's DenseInvxRecipe (azd_engine_set_dense_invx_recipe)
//   cur_mu[t] = the distance index used, cur_mu[B + t] = the `computed` mask.  No per-node arena: node_mate is null.
// The record is written where it is computed and read by the host alone: St carries nothing of the cost.
__device__ __forceinline__ const DenseInvxRecipe *dense_invx_recipe(const Arenas &a) {
    return reinterpret_cast<const DenseInvxRecipe *>(a.cur_lambda + (size_t)DENSE_INVX_COUNT * (size_t)a.B);
}
template <int ROWS>
struct DenseCostInvXT {
    using ArgminRec = std::conditional_t<ROWS == DENSE_INVX_MAX_N, DenseInvxArgminRec, DenseInvxWideArgminRec>; // (what engine.hip sizes argmin_d for)
    template <int KW_>
    using Lds = DenseAhSpaceLdsT<KW_, ROWS>;
    template <int KW_>
    struct St {
        uint64_t rem[KW_];
    };
    struct Replay {
        DenseInvxCost c;
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
    __device__ static __forceinline__ void keep(const Arenas &a, const int t, const DenseInvxCost &c) { // (one lane)
#pragma unroll
        for (int i = 0; i < DENSE_INVX_COUNT; ++i) a.cur_lambda[(size_t)i * a.B + t] = c.inv[i];
        a.cur_mu[t] = c.dist_k;
        a.cur_mu[a.B + t] = (int32_t)c.computed;
    }
    template <class L, class S, class Hook>
    __device__ static __forceinline__ float evaluate(const Arenas &a, L &s, S &, const int t, Hook &&hook) {
        const unsigned long long ph0 = PH_NOW();
        DenseInvxCost c;
        dense_invx_cost_wave(s.adj, s.ah, a.n, dense_invx_recipe(a), hook, c);
        if (LANE == 0) keep(a, t, c);
        CTR_ADD(22, PH_NOW() - ph0);
        return c.eval;
    }
    template <class L, class S>
    __device__ static __forceinline__ float root_cost(const Arenas &a, const int t, L &s, S &) {
        DenseInvxCost c;
        dense_invx_cost_wave(s.adj, s.ah, a.n, dense_invx_recipe(a), DenseNoHook{}, c);
        if (LANE == 0) keep(a, t, c);
        return c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_cost(const Arenas &a, L &s, Replay &r) {
        dense_invx_cost_wave(s.adj, s.ah, a.n, dense_invx_recipe(a), DenseNoHook{}, r.c);
        r.ev = r.c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_write(const Arenas &a, L &s, const Replay &r, const int wt, const uint32_t win_node) {
        ArgminRec *out = reinterpret_cast<ArgminRec *>(a.argmin_d);
        if (LANE < ROWS) out->adj[LANE] = LANE < a.n ? s.adj[LANE] : 0ull;
        if (LANE < (int)(sizeof(out->permitted) / sizeof(uint64_t))) out->permitted[LANE] = s.slotmask[LANE];
        if (LANE == 0) {
#pragma unroll
            for (int i = 0; i < DENSE_INVX_COUNT; ++i) out->inv[i] = r.c.inv[i];
            out->dist_k = r.c.dist_k;
            out->computed = r.c.computed;
            out->cost = r.c.cost;
            out->eval = r.c.eval;
            out->agent = wt;
            out->node = win_node;
        }
    }
};
// Named structs, not aliases: the kernels' names carry them (k_rollout<DenseSpace<2, DenseCostInvX>>)
struct DenseCostInvX : DenseCostInvXT<DENSE_INVX_MAX_N> {};
struct DenseCostInvXWide : DenseCostInvXT<DENSE_INVX_WIDE_MAX_N> {};

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
