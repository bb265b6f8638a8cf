// dense_spectral.inc -- the stages the dense-graph space's spectral costs are composed of, one wave per graph (included inside
// namespace azd after tree_core.inc and space_dense.inc, before the cost files: dense_ah_cost.inc, dense_inv_cost.inc,
// dense_invx_cost.inc, dense_invs_cost.inc).
//
//   dense_bfs_wave            all-sources BFS over the bitsets: a lane's degree, eccentricity, transmission, its row of distances
//   dense_refill_wave         the packed triangle filled again from the bitsets (adjacency, Laplacian, signless Laplacian)
//   dense_tridiag_wave        Householder reduction of the triangle to tridiagonal form in w.diag / w.sub2; the Gershgorin radius
//   dense_sturm_count         eigenvalues of that form below one shift
//   dense_multisection_wave   ONE eigenvalue by index: 64 lanes count at 64 shifts, the bracket shrinks by 65 a round
//   dense_bisect_all_wave     the WHOLE spectrum: lane l bisects for eigenvalue l
//   dense_degree_sums_wave    Randic, Zagreb 1 and 2, triangles in one loop over the vertices
// and the cost policy of the costs that a recipe defines (DenseCostRecipeT).
//
// ONE text of each: a numerical fix is made here once and reaches every tier.  What holds a tier's device code in place is not
// the machine code it compiled to before but its bits: every device cost is pinned, as bytes, to its host function
// (dense_cost_host.cpp: ah_bfs, ah_householder, ah_sturm, ah_multisection share these stages the same way) by the GPU suite, and the
// host functions to the Python references.  So every f64 step here is one IEEE operation (-ffp-contract=off; f64 division and
// sqrt are correctly rounded on gfx950) in the order the host runs it, and every reduction an xor-butterfly = a balanced binary
// tree.  Everything is __forceinline__ (tools/check_kernels.py: no device function out of line in a tree unit) and takes the
// wave's LDS block by reference.
//
// Lanes: BFS -- lane u is source u.  Householder -- lane r owns row r of the working matrix.  Multisection -- lane l owns shift l;
// whole spectrum -- lane l owns eigenvalue l; the tridiagonal entries are LDS broadcasts.  `lane`, `row` (the lane's row of the
// packed triangle) and `in` (lane < n) are the caller's, computed once.
// The working matrix is kept as its LOWER TRIANGLE, packed (row r at r (r + 1) / 2: 4.1 KB a wave where the square is 8.3 KB --
// sixteen waves' blocks of the pool step's searchers have to share a CU's 160 KB).  The host form keeps the square; the values are
// the same to the bit, because the rank-two update A_rc - (v_r q_c + q_r v_c) is symmetric in (r, c) operation by operation
// (products and the sum commute), so the square's two triangles never differ.
// The row limit ROWS is a template parameter of everything that depends on it: 32, or 64 (a triangle of 2080 doubles, 16.6 KB a
// wave).  Order of operations, lane roles and reductions do not depend on it: at n <= 32 the two compute the same bits.
__device__ __forceinline__ int dense_ah_at(const int r, const int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }
template <int ROWS>
struct DenseAhLdsT {
    static_assert(ROWS == 32 || ROWS == 64, "the lanes of one wave own the rows");
    static constexpr int TRI = ROWS * (ROWS + 1) / 2;
    double A[TRI]; // working matrix (lower triangle, packed), reduced in place
    double v[ROWS], q[ROWS]; // Householder vector and its companion, by row
    double diag[ROWS], sub2[ROWS]; // the tridiagonal form: diagonal, squared subdiagonal
};
using DenseAhLds = DenseAhLdsT<DENSE_AH_MAX_N>;
using DenseAhWideLds = DenseAhLdsT<DENSE_AH_WIDE_MAX_N>;

__device__ __forceinline__ uint32_t dense_sum_u32(uint32_t v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v += (uint32_t)__shfl_xor((int)v, w, 64);
    return uni(v);
}
template <int ROWS>
__device__ __forceinline__ uint64_t dense_vertex_mask(const int n) { // (64 rows: n = 64 must not shift by 64; n >= 4)
    return ROWS < 64 ? (1ull << n) - 1ull : ~0ull >> (64 - n);
}
// the eigenvalue index of the Aouchiche-Hansen cost: k = 2D/3 - 1, or n - 1 when 2D/3 = 0
__device__ __forceinline__ int dense_ah_index(const int diam, const int n) {
    const int q23 = (2 * diam) / 3;
    return q23 >= 1 ? q23 - 1 : n - 1;
}

// ---- BFS from every vertex at once.  adj: the graph's neighbourhood bitsets in LDS (n <= ROWS words are read); all: the mask of
// the n vertices.  Lane u < n gets its degree, its eccentricity d and its transmission t (lanes >= n: 0), and with need_dist
// (wave-uniform) its row of the distance matrix in w.A.
template <int ROWS>
__device__ __forceinline__ void dense_bfs_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int lane, const int row, const bool in,
                                               const uint64_t all, const bool need_dist, int &t, int &d, int &deg) {
    t = 0, d = 0, deg = 0;
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
}
// what the recipe costs reduce from the BFS over the wave, and the eight invariants that come of it (0 edges  1 max_degree
// 2 min_degree  3 diameter  4 radius  5 proximity  6 remoteness  7 avg_distance)
struct DenseBfsSums {
    int min_t, max_t, diam, rad, max_deg, min_deg, sum_t, m2;
};
__device__ __forceinline__ DenseBfsSums dense_bfs_sums_wave(const bool in, const int t, const int d, const int deg) {
    DenseBfsSums s;
    s.min_t = (int)wave_min_u32(in ? (uint32_t)t : 0xFFFFFFFFu), s.max_t = (int)wave_max_u32(in ? (uint32_t)t : 0u);
    s.diam = (int)wave_max_u32(in ? (uint32_t)d : 0u), s.rad = (int)wave_min_u32(in ? (uint32_t)d : 0xFFFFFFFFu);
    s.max_deg = (int)wave_max_u32(in ? (uint32_t)deg : 0u), s.min_deg = (int)wave_min_u32(in ? (uint32_t)deg : 0xFFFFFFFFu);
    s.sum_t = (int)dense_sum_u32((uint32_t)t), s.m2 = (int)dense_sum_u32((uint32_t)deg); // (lanes >= n hold 0)
    return s;
}
__device__ __forceinline__ void dense_bfs_invariants(const DenseBfsSums &s, const int n, double *inv) {
    inv[0] = (double)(s.m2 / 2);
    inv[1] = (double)s.max_deg;
    inv[2] = (double)s.min_deg;
    inv[3] = (double)s.diam;
    inv[4] = (double)s.rad;
    inv[5] = (double)s.min_t / (double)(n - 1);
    inv[6] = (double)s.max_t / (double)(n - 1);
    inv[7] = (double)s.sum_t / (double)(n * (n - 1));
}

// ---- the triangle again from the bitsets, which are still in LDS: `off` where lane and column are neighbours, 0.0 where not,
// `diagonal` on the diagonal (adjacency: 1, 0; Laplacian D - A: -1, the degree; signless Laplacian D + A: 1, the degree)
template <int ROWS>
__device__ __forceinline__ void dense_refill_wave(const uint64_t *adj, DenseAhLdsT<ROWS> &w, const int lane, const int row, const bool in,
                                                  const double off, const double diagonal) {
    LDS_SYNC();
    if (in) {
        const uint64_t nb = adj[lane];
        for (int c = 0; c < lane; ++c) w.A[row + c] = (nb >> c) & 1ull ? off : 0.0;
        w.A[row + lane] = diagonal;
    }
}

// ---- Householder reduction: step i clears column i below row i + 1; lane i keeps (diag_i, sub_i), which end in w.diag / w.sub2
// (the subdiagonal squared).  Returns the Gershgorin radius of the tridiagonal form, wave-uniform.
// A step whose column tail is zero is skipped: the column is tridiagonal already (adjacency and Laplacian matrices: often).  With
// DEFLATE one whose tail is below DENSE_INV_DEFLATE is skipped too, at every n and either row limit (dense_cost_host.h: the tail is
// rounding noise of a matrix whose rank is used up; a rank-deficient adjacency matrix otherwise runs the reduction into subnormal
// squares and NaN -- after some 20 steps on K(10,11) or a double broom with the heavier end first; from 19 vertices on).  The
// Aouchiche-Hansen cost reduces distance matrices alone and does not deflate.
template <int ROWS, bool DEFLATE>
__device__ __forceinline__ double dense_tridiag_wave(DenseAhLdsT<ROWS> &w, const int n, const int lane, const int row, const bool in) {
    double dg = 0.0, sb = 0.0;
#pragma unroll 1
    for (int i = 0; i + 2 < n; ++i) {
        LDS_SYNC();
        const bool act = in && lane > i;
        const double x = act ? w.A[row + i] : 0.0;
        const double tail = dense_tree_sum(lane > i + 1 ? x * x : 0.0);
        const double x1 = __shfl(x, i + 1, 64);
        if (lane == i) dg = w.A[row + i];
        if (tail == 0.0 || (DEFLATE && tail < DENSE_INV_DEFLATE)) {
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
    return R;
}

// ---- eigenvalues of the tridiagonal form below x = negative pivots of T - x.  Both finishers' rules for repeated eigenvalues
// (K_n, stars) depend on the TINY pivot guard.  The reads of w.diag[i] and w.sub2[i - 1] are at one address for the whole wave (an
// LDS broadcast); the one division per row is the dependent chain that sets a finisher's time.
template <int ROWS>
__device__ __forceinline__ int dense_sturm_count(const DenseAhLdsT<ROWS> &w, const int n, const double x) {
    double qq = w.diag[0] - x;
    if (fabs(qq) < DENSE_AH_TINY) qq = -DENSE_AH_TINY;
    int c = qq < 0.0 ? 1 : 0;
    for (int i = 1; i < n; ++i) {
        const double r = w.sub2[i - 1] / qq;
        qq = (w.diag[i] - x) - r;
        if (fabs(qq) < DENSE_AH_TINY) qq = -DENSE_AH_TINY;
        c += qq < 0.0 ? 1 : 0;
    }
    return c;
}
// ---- multisection for the eigenvalue of ascending index j (the `c <= j` rule), DENSE_AH_ROUNDS rounds from the radius R
template <int ROWS>
__device__ __forceinline__ double dense_multisection_wave(const DenseAhLdsT<ROWS> &w, const int n, const int lane, const int j, const double R) {
    double hi = R + 1.0, lo = -hi;
#pragma unroll 1
    for (int round = 0; round < DENSE_AH_ROUNDS; ++round) {
        const double wd = hi - lo;
        const double x = lo + (wd * (double)(lane + 1)) / 65.0;
        const int c = dense_sturm_count(w, n, x);
        const int m = __popcll(__ballot(c <= j));
        const double x_lo = __shfl(x, m > 0 ? m - 1 : 0, 64), x_hi = __shfl(x, m < 64 ? m : 63, 64);
        lo = m > 0 ? x_lo : lo;
        hi = m < 64 ? x_hi : hi;
    }
    return (lo + hi) * 0.5;
}
// ---- the whole spectrum: lane l brackets eigenvalue l (ascending) by its own bisection on the same count (the `c <= l` rule),
// DENSE_INVS_ROUNDS rounds -- a constant, so the loop is wave-uniform.  Lanes >= n run along on index l >= n: their brackets close
// on hi, and the caller takes nothing from them.
template <int ROWS>
__device__ __forceinline__ double dense_bisect_all_wave(const DenseAhLdsT<ROWS> &w, const int n, const int lane, const double R) {
    double hi = R + 1.0, lo = -hi;
#pragma unroll 1
    for (int round = 0; round < DENSE_INVS_ROUNDS; ++round) {
        const double x = (lo + hi) * 0.5;
        const int c = dense_sturm_count(w, n, x);
        if (c <= lane) lo = x;
        else hi = x;
    }
    return (lo + hi) * 0.5;
}

// ---- the degree-based invariants in ONE wave-uniform loop over v = 0 .. n - 1: lane u takes v when v < u is its neighbour (every
// edge once, ascending in v), with d_v by a wave-wide shuffle and N(v) by an LDS broadcast.  Lanes >= n hold 0 throughout
// (deg = 0, no neighbour).  tri3 counts every triangle three times.
__device__ __forceinline__ void dense_degree_sums_wave(const uint64_t *adj, const int n, const int lane, const bool in, const uint64_t all,
                                                       const int deg, double &randic, int &z1, int &z2, int &tri3) {
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
            // and the sum leaves the n 2^-52 the invariant is held to (dense_cost_host.h)
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
    z1 = (int)dense_sum_u32((uint32_t)(deg * deg));
    z2 = (int)dense_sum_u32((uint32_t)s2);
    tri3 = (int)dense_sum_u32((uint32_t)s3);
}

// ---- a recipe's linear part: c = bias, then c = c + weight[i] * I_i for every i whose weight is not zero, in order
template <int COUNT>
__device__ __forceinline__ double dense_weighted_sum(const double bias, const double *weight, const double *inv) {
    double c = bias;
#pragma unroll
    for (int i = 0; i < COUNT; ++i) {
        const double wi = weight[i];
        const double term = wi * inv[i];
        if (wi != 0.0) c = c + term;
    }
    return c;
}
// entry `pass` of a per-pass array takes e (selects, so that the array stays in registers under a run-time pass)
__device__ __forceinline__ void dense_set_by_pass(double (&a)[4], const int pass, const double e) {
    a[0] = pass == 0 ? e : a[0];
    a[1] = pass == 1 ? e : a[1];
    a[2] = pass == 2 ? e : a[2];
    a[3] = pass == 3 ? e : a[3];
}

// ---------------------------------------------------------------- what the costs' policies share (space_dense.inc: a DenseSpace's cost policy)
// A wave's block: DenseLds without the matching, with the spectral working set.  4 <= n <= ROWS, so E <= 496 or 2016.  Every
// spectral cost uses this block at its row limit: at 32 rows the pool step plans 10 / 9 / 7 waves at key widths 2 / 4 / 10, at 64
// rows what the LDS holds.
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

// The policy of a cost that a recipe given at RUN time defines (INV, INVX, INVS at their row limits).  Rec: the cost's record
// (inv[COUNT], dist_k, computed, cost, eval); Recipe: what the caller gives; Argmin: the engine's argmin record (what engine.hip
// sizes argmin_d for); Fn::run: the cost function.
// The recipe reaches the kernels without a field of Arenas (every search kernel receives that block): it lies in device memory
// behind the per-agent cost arrays.  An agent's record between launches:
//   cur_lambda[i B + t] = I_i, i = 0 .. COUNT - 1;  cur_lambda + COUNT B: the engine's recipe (azd_engine_set_dense_*_recipe)
//   cur_mu[t] = the distance index used, cur_mu[B + t] = the `computed` mask.  No per-node arena: node_mate is null.
// The record is written where it is computed (evaluate, root_cost: lane 0, like the new node's tree record) and read by the host
// alone: St carries nothing of the cost from call to call, so load_cost / store_cost have nothing to move -- 2 COUNT + 2 words a
// wave does not hold across the search loop.  A call that creates no node leaves the record of the last one that did, as the
// other costs' load / store pairs do.
template <class Rec, class Recipe, int COUNT, int ROWS, class Argmin, class Fn>
struct DenseCostRecipeT {
    using ArgminRec = Argmin;
    template <int KW_>
    using Lds = DenseAhSpaceLdsT<KW_, ROWS>;
    template <int KW_>
    struct St {
        uint64_t rem[KW_];
    };
    struct Replay {
        Rec c;
        float ev;
    };
    __device__ static __forceinline__ const Recipe *recipe(const Arenas &a) {
        return reinterpret_cast<const Recipe *>(a.cur_lambda + (size_t)COUNT * (size_t)a.B);
    }
    template <class S>
    __device__ static __forceinline__ void new_node_begin(S &, const uint32_t, const uint32_t) {}
    template <class L>
    __device__ static __forceinline__ void new_node_end(const Arenas &, const int, L &, const uint32_t) {}
    template <class S>
    __device__ static __forceinline__ void load_cost(const Arenas &, const int, S &) {}
    template <class S>
    __device__ static __forceinline__ void store_cost(const Arenas &, const int, const S &) {}
    __device__ static __forceinline__ void keep(const Arenas &a, const int t, const Rec &c) { // (one lane)
#pragma unroll
        for (int i = 0; i < COUNT; ++i) a.cur_lambda[(size_t)i * a.B + t] = c.inv[i];
        a.cur_mu[t] = c.dist_k;
        a.cur_mu[a.B + t] = (int32_t)c.computed;
    }
    template <class L, class S, class Hook>
    __device__ static __forceinline__ float evaluate(const Arenas &a, L &s, S &, const int t, Hook &&hook) {
        const unsigned long long ph0 = PH_NOW();
        Rec c;
        Fn::run(s.adj, s.ah, a.n, recipe(a), hook, c);
        if (LANE == 0) keep(a, t, c);
        CTR_ADD(22, PH_NOW() - ph0);
        return c.eval;
    }
    template <class L, class S>
    __device__ static __forceinline__ float root_cost(const Arenas &a, const int t, L &s, S &) {
        Rec c;
        Fn::run(s.adj, s.ah, a.n, recipe(a), DenseNoHook{}, c);
        if (LANE == 0) keep(a, t, c);
        return c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_cost(const Arenas &a, L &s, Replay &r) {
        Fn::run(s.adj, s.ah, a.n, recipe(a), DenseNoHook{}, r.c);
        r.ev = r.c.eval;
    }
    template <class L>
    __device__ static __forceinline__ void argmin_write(const Arenas &a, L &s, const Replay &r, const int wt, const uint32_t win_node) {
        ArgminRec *out = reinterpret_cast<ArgminRec *>(a.argmin_d);
        if (LANE < ROWS) out->adj[LANE] = LANE < a.n ? s.adj[LANE] : 0ull;
        if (LANE < (int)(sizeof(out->permitted) / sizeof(uint64_t))) out->permitted[LANE] = s.slotmask[LANE];
        if (LANE == 0) {
#pragma unroll
            for (int i = 0; i < COUNT; ++i) out->inv[i] = r.c.inv[i];
            out->dist_k = r.c.dist_k;
            out->computed = r.c.computed;
            out->cost = r.c.cost;
            out->eval = r.c.eval;
            out->agent = wt;
            out->node = win_node;
        }
    }
};
