// dense_invs_cost.inc -- the spectrum invariant cost of a connected graph on the device, one wave per graph (included inside
// namespace azd after tree_core.inc, space_dense.inc and dense_ah_cost.inc, whose LDS layout and constants it uses).
//
// BUILD-DEFINED (c21_host.h: DenseInvsRecipe; DESIGN.md "The spectrum invariant cost"): twenty-one invariants in a fixed order --
//   0 .. 15 the extended invariant cost's (dense_invx_cost.inc)
//   16 adj_energy  17 dist_energy  18 lap_energy  19 slap_energy  20 adj_spread
// -- combined by a recipe the caller gives at RUN time, by the extended cost's rule over twenty-one weights and up to four pair
// terms.  With weights 16 .. 20 zero and no term naming 16 .. 20 the sequence of operations is dense_invx_cost_wave's, and the
// first sixteen invariants, dist_k, computed, cost and eval come out bit for bit.
//
// Stages and lane roles are dense_invx_cost_wave's, written out again so that the INVX units compile to the code they compiled to
// before.  What is new is a second finisher on the tridiagonal form that every spectral pass leaves in w.diag / w.sub2:
//   multisection (as before): 64 lanes share ONE bracket, lane l owns shift l, DENSE_AH_ROUNDS rounds -- one eigenvalue by index;
//   whole spectrum: lane l < n owns eigenvalue l (ascending) and a bracket of its own, DENSE_INVS_ROUNDS rounds of plain bisection on
//   the same Sturm count (the `c <= l` rule, the TINY pivot guard) -- all eigenvalues at once.  The round count is a constant, so
//   the loop is wave-uniform; the Sturm loop's reads of w.diag[i] and w.sub2[i - 1] are at one address for the whole wave (an LDS
//   broadcast: one LDS cycle each), and its one division per row is the dependent chain that sets the finisher's time.
// An energy is the xor-butterfly over |theta_l| (adjacency, distance) or |theta_l - s| (Laplacians, s the mean degree), lanes >= n
// holding 0.0; the spread is theta_{n-1} - theta_0 by two shuffles.  Each is folded into its pass: nothing of the finisher but
// its one result is held across the next reduction.
// A matrix is reduced at most once per cost: a pass runs when its *_eig, its energy or (adjacency) the spread is needed; after the
// reduction the multisection runs only for the *_eig, the bisections only for the energy or the spread (wave-uniform branches).
// The row limit is 32: the 64-row form of this cost is not built.
__device__ __forceinline__ uint32_t dense_invs_sum_u32(uint32_t v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v += (uint32_t)__shfl_xor((int)v, w, 64);
    return uni(v);
}
// adj: the graph's neighbourhood bitsets in LDS (n <= 32 words are read).  rc: the recipe in device memory, the same address in
// every lane.  hook: called once, after the BFS (the pool step's deferred post).  Wave-uniform result in `out`.
template <class Hook>
__device__ __forceinline__ void dense_invs_cost_wave(const uint64_t *adj, DenseAhLdsT<DENSE_INVS_MAX_N> &w, const int n, const DenseInvsRecipe *rc,
                                                     Hook &&hook, DenseInvsCost &out) {
    constexpr int ROWS = DENSE_INVS_MAX_N;
    const int lane = LANE;
    const int row = lane * (lane + 1) / 2; // this lane's row of the packed triangle (lanes < n only)
    const bool in = lane < n;
    const uint64_t all = (1ull << n) - 1ull;
    const uint32_t need = uni(dense_invs_needed(*rc));
    const auto has = [need](const int i) { return ((need >> i) & 1u) != 0u; };
    const bool need_dist = has(DENSE_INV_DIST_EIG) || has(DENSE_INVS_DIST_ENERGY);
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
    const int sum_t = (int)dense_invs_sum_u32((uint32_t)t), m2 = (int)dense_invs_sum_u32((uint32_t)deg); // (lanes >= n hold 0)
    hook();
    const int q23 = (2 * diam) / 3;
    const int dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : q23 >= 1 ? q23 - 1 : n - 1;
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
        if (pass > 0) {
            LDS_SYNC();
            if (in) {
                const uint64_t nb = adj[lane];
                const double off = pass == 2 ? -1.0 : 1.0;
                for (int c = 0; c < lane; ++c) w.A[row + c] = (nb >> c) & 1ull ? off : 0.0;
                w.A[row + lane] = pass == 1 ? 0.0 : (double)deg;
            }
        }
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
            // (the column is tridiagonal already, or is rounding noise of a matrix whose rank is used up: c21_host.h, DENSE_INV_DEFLATE)
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
        const double sb_below = __shfl(sb, lane > 0 ? lane - 1 : 0, 64);
        const double g = (fabs(dg) + (lane > 0 ? fabs(sb_below) : 0.0)) + fabs(sb); // Gershgorin; >= 0: the bit patterns order like the numbers
        const double R = __longlong_as_double((long long)wave_max_u64(in ? (uint64_t)__double_as_longlong(g) : 0ull));
        if (lane < ROWS) {
            w.diag[lane] = dg;
            w.sub2[lane] = sb * sb;
        }
        LDS_SYNC();
        if (want_eig) {
            // multisection for the eigenvalue of ascending index j = n - 1 - k (the `c <= j` rule and the TINY pivot guard as in the AH
            // cost: repeated eigenvalues -- K_n, stars -- depend on both)
            const int k = pass == 0   ? dist_k
                          : pass == 1 ? (int)uni((uint32_t)rc->adj_index)
                          : pass == 2 ? (int)uni((uint32_t)rc->lap_index)
                                      : (int)uni((uint32_t)rc->slap_index);
            const int j = n - 1 - k;
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
        if (want_energy || want_spread) {
            // the whole spectrum: lane l brackets eigenvalue l by its own bisection (lanes >= n run along on index l >= n: their
            // brackets close on hi, and they contribute 0.0)
            double hi = R + 1.0, lo = -hi;
#pragma unroll 1
            for (int round = 0; round < DENSE_INVS_ROUNDS; ++round) {
                const double x = (lo + hi) * 0.5;
                double qq = w.diag[0] - x;
                if (fabs(qq) < DENSE_AH_TINY) qq = -DENSE_AH_TINY;
                int c = qq < 0.0 ? 1 : 0;
                for (int i = 1; i < n; ++i) {
                    const double r = w.sub2[i - 1] / qq;
                    qq = (w.diag[i] - x) - r;
                    if (fabs(qq) < DENSE_AH_TINY) qq = -DENSE_AH_TINY;
                    c += qq < 0.0 ? 1 : 0;
                }
                if (c <= lane) lo = x;
                else hi = x;
            }
            const double theta = (lo + hi) * 0.5;
            if (want_energy) {
                const double shift = (double)m2 / (double)n; // the mean degree: the centre of the Laplacian energies
                const double a = !in ? 0.0 : pass >= 2 ? fabs(theta - shift) : fabs(theta);
                const double e = dense_tree_sum(a);
                energy[0] = pass == 0 ? e : energy[0];
                energy[1] = pass == 1 ? e : energy[1];
                energy[2] = pass == 2 ? e : energy[2];
                energy[3] = pass == 3 ? e : energy[3];
            }
            if (want_spread) spread = __shfl(theta, n - 1, 64) - __shfl(theta, 0, 64);
        }
    }
    // ---- the degree-based invariants, after the passes so that nothing of them is held across the reductions (lanes >= n hold 0
    // throughout: deg = 0, no neighbour)
    double randic = 0.0;
    int z1 = 0, z2 = 0, tri = 0;
    if ((need >> DENSE_INVX_RANDIC) & 0xFu) {
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
                const double t = r + term; // TwoSum (Knuth), as in the extended invariant cost
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
        z1 = (int)dense_invs_sum_u32((uint32_t)(deg * deg));
        z2 = (int)dense_invs_sum_u32((uint32_t)s2);
        tri = (int)dense_invs_sum_u32((uint32_t)s3);
    }
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
    out.inv[DENSE_INVS_ADJ_ENERGY] = energy[1];
    out.inv[DENSE_INVS_DIST_ENERGY] = energy[0];
    out.inv[DENSE_INVS_LAP_ENERGY] = energy[2];
    out.inv[DENSE_INVS_SLAP_ENERGY] = energy[3];
    out.inv[DENSE_INVS_ADJ_SPREAD] = spread;
    double c = rc->bias;
#pragma unroll
    for (int i = 0; i < DENSE_INVS_COUNT; ++i) {
        const double wi = rc->weight[i];
        const double term = wi * out.inv[i];
        if (wi != 0.0) c = c + term;
    }
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

// ---------------------------------------------------------------- the spectrum invariant cost as a DenseSpace's cost policy (space_dense.inc)
// A wave's block is the 32-row AH block (DenseAhSpaceLdsT<KW, 32>).  4 <= n <= 32, so E <= 496.  (No pool searchers are built with
// this policy: dense_invs_kernels.hip.)  The recipe lies in device memory behind the per-agent cost arrays, as the INVX
// tier's does.  An agent's record between launches:
//   cur_lambda[i B + t] = I_i, i = 0 .. 20;  cur_lambda + 21 B: the engine's DenseInvsRecipe (azd_engine_set_dense_invs_recipe)
//   cur_mu[t] = the distance index used, cur_mu[B + t] = the `computed` mask.  No per-node arena: node_mate is null.
// The record is written where it is computed and read by the host alone: St carries nothing of the cost.
__device__ __forceinline__ const DenseInvsRecipe *dense_invs_recipe(const Arenas &a) {
    return reinterpret_cast<const DenseInvsRecipe *>(a.cur_lambda + (size_t)DENSE_INVS_COUNT * (size_t)a.B);
}
struct DenseCostInvS {
    static constexpr int ROWS = DENSE_INVS_MAX_N;
    using ArgminRec = DenseInvsArgminRec; // (what engine.hip sizes argmin_d for)
    template <int KW_>
    using Lds = DenseAhSpaceLdsT<KW_, ROWS>;
    template <int KW_>
    struct St {
        uint64_t rem[KW_];
    };
    struct Replay {
        DenseInvsCost c;
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
    __device__ static __forceinline__ void keep(const Arenas &a, const int t, const DenseInvsCost &c) { // (one lane)
#pragma unroll
        for (int i = 0; i < DENSE_INVS_COUNT; ++i) a.cur_lambda[(size_t)i * a.B + t] = c.inv[i];
        a.cur_mu[t] = c.dist_k;
        a.cur_mu[a.B + t] = (int32_t)c.computed;
    }
    template <class L, class S, class Hook>
    __device__ static __forceinline__ float evaluate(const Arenas &a, L &s, S &, const int t, Hook &&hook) {
        const unsigned long long ph0 = PH_NOW();
        DenseInvsCost c;
        dense_invs_cost_wave(s.adj, s.ah, a.n, dense_invs_recipe(a), hook, c);
        if (LANE == 0) keep(a, t, c);
        CTR_ADD(22, PH_NOW() - ph0);
        return c.eval;
    }
    template <class L, class S>
    __device__ static __forceinline__ float root_cost(const Arenas &a, const int t, L &s, S &) {
        DenseInvsCost c;
        dense_invs_cost_wave(s.adj, s.ah, a.n, dense_invs_recipe(a), DenseNoHook{}, c);
        if (LANE == 0) keep(a, t, c);
        return c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_cost(const Arenas &a, L &s, Replay &r) {
        dense_invs_cost_wave(s.adj, s.ah, a.n, dense_invs_recipe(a), DenseNoHook{}, r.c);
        r.ev = r.c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_write(const Arenas &a, L &s, const Replay &r, const int wt, const uint32_t win_node) {
        ArgminRec *out = reinterpret_cast<ArgminRec *>(a.argmin_d);
        if (LANE < ROWS) out->adj[LANE] = LANE < a.n ? s.adj[LANE] : 0ull;
        if (LANE < (int)(sizeof(out->permitted) / sizeof(uint64_t))) out->permitted[LANE] = s.slotmask[LANE];
        if (LANE == 0) {
#pragma unroll
            for (int i = 0; i < DENSE_INVS_COUNT; ++i) out->inv[i] = r.c.inv[i];
            out->dist_k = r.c.dist_k;
            out->computed = r.c.computed;
            out->cost = r.c.cost;
            out->eval = r.c.eval;
            out->agent = wt;
            out->node = win_node;
        }
    }
};

// The cost outside any engine (space_ops.h: launch_probe_invs_cost): one wave per graph, `reps` repetitions (timing), the result of
// the last one.  The host has checked the graphs and the recipe (engine_probes.hip): LDS is indexed by the bits of adj.
__global__ __launch_bounds__(64) void k_probe_invs_cost(const uint64_t *__restrict__ adj, const int n, const int count, const int reps,
                                                        const DenseInvsRecipe *__restrict__ recipe, DenseInvsCost *__restrict__ out) {
    __shared__ uint64_t s_adj[DENSE_INVS_MAX_N];
    __shared__ DenseAhLdsT<DENSE_INVS_MAX_N> w;
    const int g = blockIdx.x;
    if (g >= count) return;
    if (LANE < DENSE_INVS_MAX_N) s_adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    DenseInvsCost c;
    for (int r = 0; r < reps; ++r) {
        dense_invs_cost_wave(s_adj, w, n, recipe, DenseNoHook{}, c);
        LDS_SYNC();
    }
    if (LANE == 0) out[g] = c;
}
