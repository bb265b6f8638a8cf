// c21_host.cpp -- host side of the c21 space seam: dimensions and the seeded root generator
// that stands in for the driver's `init_states` closure (graph-state/examples/04-c21-tree.rs:108-112,
// graph-state/src/rooted_tree/mod.rs:14-20, modify_parent_once.rs:14-25; the reference draws from
// thread_rng, this build from a counter-based generator so that runs are reproducible and
// shard-invariant -- the stream of an agent depends only on (seed, epoch, global agent id)).
#include "c21_host.h"

#include <cmath>
#include <vector>

namespace azd {

uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
uint64_t stream_key(uint64_t seed, uint64_t domain, uint64_t agent, uint64_t draw) {
    return splitmix64(splitmix64(splitmix64(splitmix64(seed) ^ domain) ^ agent) ^ draw);
}
uint32_t draw_below(uint64_t r, uint32_t n) { return (uint32_t)(((r >> 32) * (uint64_t)n) >> 32); }

int c21_state_dim(int n) { return (n - 1) * (n - 2) - 2; }
int c21_action_dim(int n) { return (n - 1) * (n - 2) / 2 - 1; }
int c21_key_words(int n) { return (c21_action_dim(n) + 63) / 64; }

float c21_eval_slope(int n) { // 04-c21-tree.rs:58-74
    int r = 0;
    while ((r + 1) * (r + 1) <= n - 1) ++r;
    int sq = (r * r == n - 1) ? r : r + 1;
    int upper = sq + (n + 1) / 2;
    return 1.0f / (float)(upper - 2);
}

// initial bracket of the lambda_1 multisection: path (smallest lambda_1 among trees on n vertices, 2 cos(pi / (n + 1)))
// and star (largest, sqrt(n - 1)), rounded to f32 and widened by 2^-20 -- the same doubles as the oracle's
void c21_lambda_bracket(int n, double *lo, double *hi) {
    *lo = (double)(float)(2.0 * std::cos(3.14159265358979323846 / (double)(n + 1))) - 0x1p-20;
    *hi = (double)(float)std::sqrt((double)(n - 1)) + 0x1p-20;
}

void c21_shuffle_permitted(uint64_t seed, uint64_t domain, uint64_t agent, int n, int k, uint64_t *permitted) {
    const int A = c21_action_dim(n), KW = c21_key_words(n);
    std::vector<uint32_t> perm((size_t)A);
    for (int i = 0; i < A; ++i) perm[(size_t)i] = (uint32_t)i;
    for (int w = 0; w < KW; ++w) permitted[w] = 0;
    for (int j = 0; j < k; ++j) {
        uint32_t r = (uint32_t)j + draw_below(stream_key(seed, domain, agent, 64 + (uint64_t)j), (uint32_t)(A - j));
        uint32_t tmp = perm[(size_t)j];
        perm[(size_t)j] = perm[r];
        perm[r] = tmp;
        permitted[perm[(size_t)j] >> 6] |= 1ull << (perm[(size_t)j] & 63);
    }
}

void c21_fresh_root(uint64_t seed, uint64_t domain, uint64_t agent, int n, int k, uint8_t *parents,
                    uint64_t *permitted) {
    for (int v = 0; v < n; ++v) parents[v] = 0;
    for (int v = 2; v <= n - 2; ++v) parents[v] = (uint8_t)draw_below(stream_key(seed, domain, agent, (uint64_t)v), (uint32_t)v);
    c21_shuffle_permitted(seed, domain, agent, n, k, permitted);
}

void c21_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin, int kmax,
                        uint8_t *parents, uint64_t *permitted) {
    const int KW = c21_key_words(n);
    const uint64_t domain = DOMAIN_ROOT ^ (epoch << 32);
    for (int i = 0; i < count; ++i) {
        uint64_t agent = first_agent + (uint64_t)i;
        int k = kmin + (int)draw_below(stream_key(seed, domain, agent, 0), (uint32_t)(kmax - kmin + 1));
        c21_fresh_root(seed, domain, agent, n, k, parents + (size_t)i * n, permitted + (size_t)i * KW);
    }
}

// ---- Ramsey space: seeded stand-in for the drivers' init_state closure (01-r333.rs:84-90,
// 02-r44.rs:84-90: ColoredCompleteBitsetGraph::generate with uniform colour weights +
// RamseyCountsNoRecolor::generate).  colour[e] = below(draw 1024 + e, C), or with colour weights (05-r45.rs:84-90) the
// number of thresholds the draw's high word reaches (c21_host.h); permitted edges = first k of the Fisher-Yates shuffle
// of 0..E-1 (draws 64 + j).
int ramsey_edges(int n) { return n * (n - 1) / 2; }
int ramsey_state_dim(int n, int c) { return ramsey_edges(n) * (2 * c + 1); }
int ramsey_action_dim(int n, int c) { return ramsey_edges(n) * c; }
int ramsey_key_words(int n, int c) { return (ramsey_action_dim(n, c) + 63) / 64; }

void shuffle_mask(uint64_t seed, uint64_t domain, uint64_t agent, int universe, int words, int k, uint64_t *mask) {
    std::vector<uint32_t> perm((size_t)universe);
    for (int i = 0; i < universe; ++i) perm[(size_t)i] = (uint32_t)i;
    for (int w = 0; w < words; ++w) mask[w] = 0;
    for (int j = 0; j < k; ++j) {
        uint32_t r = (uint32_t)j + draw_below(stream_key(seed, domain, agent, 64 + (uint64_t)j), (uint32_t)(universe - j));
        uint32_t tmp = perm[(size_t)j];
        perm[(size_t)j] = perm[r];
        perm[r] = tmp;
        mask[perm[(size_t)j] >> 6] |= 1ull << (perm[(size_t)j] & 63);
    }
}
const char *ramsey_check_color_weights(const double *w, int c) {
    if (!w) return "color_weights: null";
    for (int i = 0; i < c; ++i)
        if (!std::isfinite(w[i]) || !(w[i] > 0.0)) return "color_weights: every weight must be finite and positive";
    return nullptr;
}
void ramsey_color_thresholds(const double *w, int c, uint64_t *thr) {
    double cum[4] = {0.0, 0.0, 0.0, 0.0}, run = 0.0;
    for (int i = 0; i < c; ++i) {
        run = run + w[i];
        cum[i] = run;
    }
    const double W = cum[c - 1];
    for (int i = 0; i < RAMSEY_COLOR_THRESHOLDS; ++i) {
        thr[i] = 1ull << 32;
        if (i < c - 1) {
            const double t = std::ceil((cum[i] / W) * 4294967296.0);
            thr[i] = t >= 4294967296.0 ? (1ull << 32) : (uint64_t)t;
        }
    }
}
uint32_t ramsey_weighted_color(uint64_t r, int c, const uint64_t *thr) {
    const uint64_t hi = r >> 32;
    uint32_t col = 0;
    for (int i = 0; i < c - 1; ++i) col += hi >= thr[i] ? 1u : 0u;
    return col;
}
// thr: the colour thresholds (ramsey_color_thresholds), or nullptr for uniform colours
static void ramsey_fresh_root_thr(uint64_t seed, uint64_t domain, uint64_t agent, int n, int c, int k, const uint64_t *thr,
                                  uint8_t *colors, uint64_t *permitted) {
    const int E = ramsey_edges(n);
    for (int e = 0; e < E; ++e) {
        const uint64_t r = stream_key(seed, domain, agent, 1024 + (uint64_t)e);
        colors[e] = (uint8_t)(thr ? ramsey_weighted_color(r, c, thr) : draw_below(r, (uint32_t)c));
    }
    shuffle_mask(seed, domain, agent, E, ramsey_key_words(n, c), k, permitted);
}
void ramsey_fresh_root(uint64_t seed, uint64_t domain, uint64_t agent, int n, int c, int k, uint8_t *colors,
                       uint64_t *permitted) {
    ramsey_fresh_root_thr(seed, domain, agent, n, c, k, nullptr, colors, permitted);
}
void ramsey_generate_roots_weighted(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int c, int kmin,
                                    int kmax, const uint64_t *thr, uint8_t *colors, uint64_t *permitted) {
    const int E = ramsey_edges(n), KW = ramsey_key_words(n, c);
    const uint64_t domain = DOMAIN_ROOT ^ (epoch << 32);
    for (int i = 0; i < count; ++i) {
        uint64_t agent = first_agent + (uint64_t)i;
        int k = kmin + (int)draw_below(stream_key(seed, domain, agent, 0), (uint32_t)(kmax - kmin + 1));
        ramsey_fresh_root_thr(seed, domain, agent, n, c, k, thr, colors + (size_t)i * E, permitted + (size_t)i * KW);
    }
}
void ramsey_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int c, int kmin,
                           int kmax, uint8_t *colors, uint64_t *permitted) {
    ramsey_generate_roots_weighted(seed, epoch, first_agent, count, n, c, kmin, kmax, nullptr, colors, permitted);
}

// ---- dense-graph space: seeded stand-in for ConnectedBitsetGraph::generate(p) (connected_bitset_graph/mod.rs:84-97:
// redraw G(n, p) until it is connected) + a modifiable-slot set in the image of modify_parent_once.rs:14-25.
//   attempt t = 0, 1, ...: the edge at slot e is present iff (draw(4096 + t E + e) >> 40) < p24 (p24 = p 2^24);
//   modifiable slots = first k of the Fisher-Yates shuffle of 0..E-1 (draws 64 + j)
int dense_edges(int n) { return n * (n - 1) / 2; }
int dense_state_dim(int n) { return 3 * dense_edges(n) + 1; }
int dense_action_dim(int n) { return 2 * dense_edges(n); }
int dense_key_words(int n) { return (dense_action_dim(n) + 63) / 64; }
bool dense_connected(const uint64_t *adj, int n) {
    uint64_t seen = 1ull, frontier = 1ull;
    const uint64_t all = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    while (frontier) {
        uint64_t next = 0;
        while (frontier) {
            const int w = __builtin_ctzll(frontier);
            frontier &= frontier - 1;
            next |= adj[w];
        }
        frontier = next & ~seen;
        seen |= next;
    }
    return (seen & all) == all;
}
void dense_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin, int kmax,
                          uint32_t p24, uint64_t *adj_out, uint64_t *slots) {
    const int E = dense_edges(n), KW = dense_key_words(n);
    const uint64_t domain = DOMAIN_ROOT ^ (epoch << 32);
    for (int i = 0; i < count; ++i) {
        const uint64_t agent = first_agent + (uint64_t)i;
        const int k = kmin + (int)draw_below(stream_key(seed, domain, agent, 0), (uint32_t)(kmax - kmin + 1));
        uint64_t *adj = adj_out + (size_t)i * n;
        for (uint64_t t = 0;; ++t) {
            for (int v = 0; v < n; ++v) adj[v] = 0;
            int e = 0;
            for (int v = 1; v < n; ++v)
                for (int u = 0; u < v; ++u, ++e)
                    if ((uint32_t)(stream_key(seed, domain, agent, 4096ull + t * (uint64_t)E + (uint64_t)e) >> 40) < p24) {
                        adj[v] |= 1ull << u;
                        adj[u] |= 1ull << v;
                    }
            if (dense_connected(adj, n)) break;
        }
        uint64_t *so = slots + (size_t)i * KW;
        for (int w = 0; w < KW; ++w) so[w] = 0;
        shuffle_mask(seed, domain, agent, E, (E + 63) / 64, k, so);
    }
}

// ---- Aouchiche-Hansen cost (the dense space's second objective).  connected_bitset_graph/mod.rs:156-198 restated: BFS from every
// vertex over the bitsets (distance matrix, transmissions, diameter), proximity = min transmission / (n - 1), k = 2D/3 - 1 (n - 1
// when 2D/3 = 0), cost = (f32)(proximity + entry k of the distance matrix's eigenvalues sorted descending).  The eigenvalue comes
// from a Householder reduction to tridiagonal form and a Sturm-count multisection, written as the 64-lane wave of
// dense_ah_cost.inc runs it: `lane` loops stand for the lanes, tree64 for the xor-butterfly.  One IEEE operation at a time
// (this file is built with -ffp-contract=off); tests/dense_ah_ref.py is the same sequence in Python.
float dense_ah_eval_slope(int n) { return 1.0f / (float)(2 * n + 2); }
static const char *ah_check_graph(const uint64_t *adj, int n, int max_n, const char *bad_n) {
    if (!adj) return "adj: null";
    if (n < 4 || n > max_n) return bad_n;
    const uint64_t all = ~0ull >> (64 - n); // (no shift by 64 at n = 64)
    for (int v = 0; v < n; ++v) {
        if (adj[v] & ~all) return "adj: a neighbour beyond n";
        if ((adj[v] >> v) & 1ull) return "adj: a loop";
        for (int u = 0; u < n; ++u)
            if (((adj[v] >> u) & 1ull) != ((adj[u] >> v) & 1ull)) return "adj: not symmetric";
    }
    if (!dense_connected(adj, n)) return "adj: the graph is not connected";
    return nullptr;
}
const char *dense_ah_check_graph(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_AH_MAX_N, "n: the Aouchiche-Hansen cost needs 4 <= n <= 32 (AZD_DENSE_AH_MAX_N)");
}
const char *dense_ah_check_graph_wide(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_AH_WIDE_MAX_N, "n: the wide Aouchiche-Hansen cost needs 4 <= n <= 64 (AZD_DENSE_AH_WIDE_MAX_N)");
}
static double ah_tree64(const double *v) { // balanced binary tree over 64 slots, adjacent pairs first
    double t[64];
    for (int i = 0; i < 64; ++i) t[i] = v[i];
    for (int w = 64; w > 1; w >>= 1)
        for (int i = 0; i < w / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    return t[0];
}
static int ah_sturm(const double *diag, const double *sub2, int n, double x) {
    double q = diag[0] - x;
    if (std::fabs(q) < DENSE_AH_TINY) q = -DENSE_AH_TINY;
    int c = q < 0.0 ? 1 : 0;
    for (int i = 1; i < n; ++i) {
        const double r = sub2[i - 1] / q;
        q = (diag[i] - x) - r;
        if (std::fabs(q) < DENSE_AH_TINY) q = -DENSE_AH_TINY;
        c += q < 0.0 ? 1 : 0;
    }
    return c;
}
// The three stages of the procedure, shared by the Aouchiche-Hansen cost and the weighted-invariant cost below.
// BFS from every vertex: row u of A (pitch DENSE_AH_STRIDE) receives d(u, .), trans[u] the transmission, ecc[u] the eccentricity
static void ah_bfs(const uint64_t *adj, int n, double *A, int *trans, int *ecc) {
    constexpr int P = DENSE_AH_STRIDE;
    for (int u = 0; u < n; ++u) {
        uint64_t seen = 1ull << u, frontier = seen;
        int d = 0, t = 0;
        for (;;) {
            uint64_t next = 0;
            for (uint64_t f = frontier; f; f &= f - 1ull) next |= adj[__builtin_ctzll(f)];
            next &= ~seen;
            if (!next) break;
            ++d;
            if (A)
                for (uint64_t m = next; m; m &= m - 1ull) A[u * P + __builtin_ctzll(m)] = (double)d;
            t += d * __builtin_popcountll(next);
            seen |= next;
            frontier = next;
        }
        trans[u] = t;
        ecc[u] = d;
    }
}
// Householder reduction of the symmetric matrix A (pitch DENSE_AH_STRIDE, reduced in place): step i clears column i below row i + 1.
// deflate: a column whose tail is below it is left as it is, like one whose tail is zero (0.0: none -- the Aouchiche-Hansen cost,
// which reduces distance matrices only; the invariant costs pass DENSE_INV_DEFLATE at every n: c21_host.h)
static void ah_householder(double *A, int n, double *diag, double *sub, double deflate = 0.0) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    double v[64], p[64], q[64], tmp[64];
    for (int i = 0; i < MAX_N; ++i) diag[i] = sub[i] = 0.0;
    for (int i = 0; i + 2 < n; ++i) {
        for (int lane = 0; lane < 64; ++lane) {
            v[lane] = lane > i && lane < n ? A[lane * P + i] : 0.0;
            tmp[lane] = lane > i + 1 ? v[lane] * v[lane] : 0.0;
        }
        const double tail = ah_tree64(tmp), x1 = v[i + 1];
        diag[i] = A[i * P + i];
        if (tail == 0.0 || tail < deflate) {
            sub[i] = x1;
            continue;
        }
        const double sigma = tail + x1 * x1;
        const double s = std::sqrt(sigma);
        const double alpha = x1 >= 0.0 ? -s : s;
        const double v1 = x1 - alpha;
        v[i + 1] = v1;
        const double beta = 2.0 / (tail + v1 * v1);
        for (int lane = 0; lane < 64; ++lane) {
            double acc = 0.0;
            if (lane > i && lane < n)
                for (int c = i + 1; c < n; ++c) acc = acc + A[lane * P + c] * v[c];
            p[lane] = lane > i && lane < n ? beta * acc : 0.0;
            tmp[lane] = v[lane] * p[lane];
        }
        const double vp = ah_tree64(tmp);
        const double K = (0.5 * beta) * vp;
        for (int lane = 0; lane < 64; ++lane) q[lane] = lane > i && lane < n ? p[lane] - K * v[lane] : 0.0;
        for (int lane = i + 1; lane < n; ++lane)
            for (int c = i + 1; c < n; ++c) A[lane * P + c] = A[lane * P + c] - (v[lane] * q[c] + q[lane] * v[c]);
        sub[i] = alpha;
    }
    diag[n - 2] = A[(n - 2) * P + (n - 2)];
    sub[n - 2] = A[(n - 1) * P + (n - 2)];
    diag[n - 1] = A[(n - 1) * P + (n - 1)];
}
// multisection for entry k of the tridiagonal matrix's eigenvalues sorted descending = ascending index j = n - 1 - k
static double ah_multisection(const double *diag, const double *sub, int n, int k) {
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    const int j = n - 1 - k;
    double sub2[MAX_N], R = 0.0;
    for (int i = 0; i < n; ++i) {
        sub2[i] = sub[i] * sub[i];
        const double g = (std::fabs(diag[i]) + (i > 0 ? std::fabs(sub[i - 1]) : 0.0)) + std::fabs(sub[i]);
        if (g > R) R = g;
    }
    double hi = R + 1.0, lo = -hi;
    for (int round = 0; round < DENSE_AH_ROUNDS; ++round) {
        const double w = hi - lo;
        double xs[64];
        int m = 0;
        for (int lane = 0; lane < 64; ++lane) {
            xs[lane] = lo + (w * (double)(lane + 1)) / 65.0;
            m += ah_sturm(diag, sub2, n, xs[lane]) <= j ? 1 : 0;
        }
        const double nlo = m > 0 ? xs[m - 1] : lo, nhi = m < 64 ? xs[m] : hi;
        lo = nlo;
        hi = nhi;
    }
    return (lo + hi) * 0.5;
}
void dense_ah_cost_host(const uint64_t *adj, int n, DenseAhCost *out) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N; // (the values do not depend on the pitch or on the rows beyond n)
    std::vector<double> Am((size_t)MAX_N * P, 0.0);
    int trans[MAX_N], ecc[MAX_N];
    ah_bfs(adj, n, Am.data(), trans, ecc);
    int min_t = 0x7FFFFFFF, diam = 0;
    for (int u = 0; u < n; ++u) {
        if (trans[u] < min_t) min_t = trans[u];
        if (ecc[u] > diam) diam = ecc[u];
    }
    const double prox = (double)min_t / (double)(n - 1);
    const int q23 = (2 * diam) / 3, k = q23 >= 1 ? q23 - 1 : n - 1;
    double diag[MAX_N], sub[MAX_N];
    ah_householder(Am.data(), n, diag, sub);
    const double eig = ah_multisection(diag, sub, n, k);
    out->proximity = prox;
    out->eigenvalue = eig;
    out->diameter = diam;
    out->k = k;
    out->cost = (float)(prox + eig);
    out->eval = dense_ah_eval_slope(n) * (out->cost + 2.0f);
}

// ---- weighted-invariant cost (c21_host.h: DenseInvRecipe; the dense space's third objective): the host form of
// dense_inv_cost_wave (dense_inv_cost.inc), the same IEEE operations in the same order, over the three stages above.
const char *dense_inv_check_graph(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_INV_MAX_N, "n: the weighted-invariant cost needs 4 <= n <= 32 (AZD_DENSE_INV_MAX_N)");
}
const char *dense_inv_check_graph_wide(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_INV_WIDE_MAX_N, "n: the wide weighted-invariant cost needs 4 <= n <= 64 (AZD_DENSE_INV_WIDE_MAX_N)");
}
const char *dense_inv_check_recipe(const DenseInvRecipe *r, int n) {
    if (!r) return "recipe: null";
    bool any = false;
    for (int i = 0; i < DENSE_INV_COUNT; ++i) {
        if (!std::isfinite(r->weight[i])) return "weight: every weight must be finite";
        any = any || r->weight[i] != 0.0;
    }
    if (!any) return "weight: all ten weights are zero";
    if (!std::isfinite(r->bias)) return "bias: must be finite";
    if (!std::isfinite(r->eval_offset)) return "eval_offset: must be finite";
    if (!std::isfinite(r->eval_scale) || r->eval_scale == 0.0f) return "eval_scale: must be finite and not zero";
    if (r->adj_index < 0 || r->adj_index > n - 1) return "adj_index: must be in 0 .. n - 1 (descending index into the adjacency spectrum)";
    if (r->dist_index != DENSE_INV_INDEX_AH && (r->dist_index < 0 || r->dist_index > n - 1))
        return "dist_index: must be in 0 .. n - 1 (descending index into the distance spectrum) or AZD_DENSE_INV_INDEX_AH";
    return nullptr;
}
void dense_inv_cost_host(const uint64_t *adj, int n, const DenseInvRecipe &r, DenseInvCost *out) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    const bool need_adj = r.weight[DENSE_INV_ADJ_EIG] != 0.0, need_dist = r.weight[DENSE_INV_DIST_EIG] != 0.0;
    std::vector<double> Am((size_t)MAX_N * P, 0.0);
    double *A = Am.data();
    int trans[MAX_N], ecc[MAX_N];
    ah_bfs(adj, n, need_dist ? A : nullptr, trans, ecc);
    int m2 = 0, max_deg = 0, min_deg = 0x7FFFFFFF, diam = 0, rad = 0x7FFFFFFF, min_t = 0x7FFFFFFF, max_t = 0, sum_t = 0;
    for (int u = 0; u < n; ++u) {
        const int deg = __builtin_popcountll(adj[u]);
        m2 += deg;
        max_deg = deg > max_deg ? deg : max_deg;
        min_deg = deg < min_deg ? deg : min_deg;
        diam = ecc[u] > diam ? ecc[u] : diam;
        rad = ecc[u] < rad ? ecc[u] : rad;
        min_t = trans[u] < min_t ? trans[u] : min_t;
        max_t = trans[u] > max_t ? trans[u] : max_t;
        sum_t += trans[u];
    }
    const int q23 = (2 * diam) / 3;
    const int dist_k = r.dist_index != DENSE_INV_INDEX_AH ? r.dist_index : q23 >= 1 ? q23 - 1 : n - 1;
    double I[DENSE_INV_COUNT];
    I[0] = (double)(m2 / 2);
    I[1] = (double)max_deg;
    I[2] = (double)min_deg;
    I[3] = (double)diam;
    I[4] = (double)rad;
    I[5] = (double)min_t / (double)(n - 1);
    I[6] = (double)max_t / (double)(n - 1);
    I[7] = (double)sum_t / (double)(n * (n - 1));
    I[8] = I[9] = 0.0;
    double diag[MAX_N], sub[MAX_N];
    // the distance pass runs first, on the rows the BFS left; the adjacency pass refills the matrix from the bitsets
    if (need_dist) {
        ah_householder(A, n, diag, sub, DENSE_INV_DEFLATE);
        I[DENSE_INV_DIST_EIG] = ah_multisection(diag, sub, n, dist_k);
    }
    if (need_adj) {
        for (int u = 0; u < n; ++u)
            for (int v = 0; v < n; ++v) A[u * P + v] = (adj[u] >> v) & 1ull ? 1.0 : 0.0;
        ah_householder(A, n, diag, sub, DENSE_INV_DEFLATE);
        I[DENSE_INV_ADJ_EIG] = ah_multisection(diag, sub, n, r.adj_index);
    }
    double c = r.bias;
    for (int i = 0; i < DENSE_INV_COUNT; ++i) {
        out->inv[i] = I[i];
        if (r.weight[i] != 0.0) {
            const double term = r.weight[i] * I[i];
            c = c + term;
        }
    }
    out->dist_k = dist_k;
    out->computed = DENSE_INV_ALWAYS | (need_adj ? 1u << DENSE_INV_ADJ_EIG : 0u) | (need_dist ? 1u << DENSE_INV_DIST_EIG : 0u);
    out->cost = (float)c;
    out->eval = r.eval_scale * (out->cost + r.eval_offset);
}

// ---- extended invariant cost (c21_host.h: DenseInvxRecipe; AZD_ENGINE_DENSE_INVX): the host form of dense_invx_cost_wave
// (dense_invx_cost.inc), the same IEEE operations in the same order, over the stages above.
const char *dense_invx_check_graph(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_INVX_MAX_N, "n: the extended invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVX_MAX_N)");
}
const char *dense_invx_check_graph_wide(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_INVX_WIDE_MAX_N, "n: the wide extended invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVX_WIDE_MAX_N)");
}
const char *dense_invx_check_recipe(const DenseInvxRecipe *r, int n) {
    if (!r) return "recipe: null";
    bool any = false;
    for (int i = 0; i < DENSE_INVX_COUNT; ++i) {
        if (!std::isfinite(r->weight[i])) return "weight: every weight must be finite";
        any = any || r->weight[i] != 0.0;
    }
    if (r->n_terms < 0 || r->n_terms > DENSE_INVX_MAX_TERMS) return "n_terms: must be in 0 .. 4 (AZD_DENSE_INVX_MAX_TERMS)";
    for (int t = 0; t < r->n_terms; ++t) {
        const DenseInvxTerm &p = r->term[t];
        if (!std::isfinite(p.coef)) return "term.coef: every coefficient must be finite";
        if (p.a < 0 || p.a >= DENSE_INVX_COUNT) return "term.a: must be in 0 .. 15 (an invariant's index)";
        if (p.b < 0 || p.b >= DENSE_INVX_COUNT) return "term.b: must be in 0 .. 15 (an invariant's index)";
        if (p.op != DENSE_INVX_MUL && p.op != DENSE_INVX_DIV) return "term.op: must be AZD_DENSE_INVX_MUL or AZD_DENSE_INVX_DIV";
        if (p.op == DENSE_INVX_DIV && !((DENSE_INVX_DIVISORS >> p.b) & 1u))
            return "term.b: a divisor must be positive on every connected graph: indices 0 .. 7, 12 (randic), 13 (zagreb1), 14 (zagreb2)";
        any = any || p.coef != 0.0;
    }
    if (!any) return "weight: all sixteen weights and all coefficients are zero";
    if (!std::isfinite(r->bias)) return "bias: must be finite";
    if (!std::isfinite(r->eval_offset)) return "eval_offset: must be finite";
    if (!std::isfinite(r->eval_scale) || r->eval_scale == 0.0f) return "eval_scale: must be finite and not zero";
    if (r->adj_index < 0 || r->adj_index > n - 1) return "adj_index: must be in 0 .. n - 1 (descending index into the adjacency spectrum)";
    if (r->dist_index != DENSE_INV_INDEX_AH && (r->dist_index < 0 || r->dist_index > n - 1))
        return "dist_index: must be in 0 .. n - 1 (descending index into the distance spectrum) or AZD_DENSE_INV_INDEX_AH";
    if (r->lap_index < 0 || r->lap_index > n - 1) return "lap_index: must be in 0 .. n - 1 (descending index into the Laplacian spectrum)";
    if (r->slap_index < 0 || r->slap_index > n - 1) return "slap_index: must be in 0 .. n - 1 (descending index into the signless-Laplacian spectrum)";
    return nullptr;
}
void dense_invx_cost_host(const uint64_t *adj, int n, const DenseInvxRecipe &r, DenseInvxCost *out) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    const uint32_t need = dense_invx_needed(r);
    const auto needs = [need](int i) { return ((need >> i) & 1u) != 0u; };
    const bool need_dist = needs(DENSE_INV_DIST_EIG);
    std::vector<double> Am((size_t)MAX_N * P, 0.0);
    double *A = Am.data();
    int trans[MAX_N], ecc[MAX_N], deg[MAX_N];
    ah_bfs(adj, n, need_dist ? A : nullptr, trans, ecc);
    int m2 = 0, max_deg = 0, min_deg = 0x7FFFFFFF, diam = 0, rad = 0x7FFFFFFF, min_t = 0x7FFFFFFF, max_t = 0, sum_t = 0;
    for (int u = 0; u < n; ++u) {
        deg[u] = __builtin_popcountll(adj[u]);
        m2 += deg[u];
        max_deg = deg[u] > max_deg ? deg[u] : max_deg;
        min_deg = deg[u] < min_deg ? deg[u] : min_deg;
        diam = ecc[u] > diam ? ecc[u] : diam;
        rad = ecc[u] < rad ? ecc[u] : rad;
        min_t = trans[u] < min_t ? trans[u] : min_t;
        max_t = trans[u] > max_t ? trans[u] : max_t;
        sum_t += trans[u];
    }
    const int q23 = (2 * diam) / 3;
    const int dist_k = r.dist_index != DENSE_INV_INDEX_AH ? r.dist_index : q23 >= 1 ? q23 - 1 : n - 1;
    double I[DENSE_INVX_COUNT];
    I[0] = (double)(m2 / 2);
    I[1] = (double)max_deg;
    I[2] = (double)min_deg;
    I[3] = (double)diam;
    I[4] = (double)rad;
    I[5] = (double)min_t / (double)(n - 1);
    I[6] = (double)max_t / (double)(n - 1);
    I[7] = (double)sum_t / (double)(n * (n - 1));
    for (int i = DENSE_INV_ADJ_EIG; i < DENSE_INVX_COUNT; ++i) I[i] = 0.0;
    // the degree-based invariants: vertex u over its neighbours v < u, ascending (every edge once)
    if (need >> DENSE_INVX_RANDIC) {
        double part[64];
        int z1 = 0, z2 = 0, tri = 0;
        for (int u = 0; u < 64; ++u) part[u] = 0.0;
        for (int u = 0; u < n; ++u) {
            z1 += deg[u] * deg[u];
            double rr = 0.0, cc = 0.0;
            for (int v = 0; v < u; ++v)
                if ((adj[u] >> v) & 1ull) {
                    const double s = std::sqrt((double)(deg[u] * deg[v]));
                    const double term = 1.0 / s;
                    // TwoSum (Knuth): t + e == rr + term exactly; the rounding errors are summed beside the sum
                    const double t = rr + term;
                    const double bp = t - rr;
                    const double ap = t - bp;
                    const double e = (rr - ap) + (term - bp);
                    cc = cc + e;
                    rr = t;
                    z2 += deg[u] * deg[v];
                    tri += __builtin_popcountll(adj[u] & adj[v]);
                }
            part[u] = rr + cc;
        }
        if (needs(DENSE_INVX_RANDIC)) I[DENSE_INVX_RANDIC] = ah_tree64(part);
        if (needs(DENSE_INVX_ZAGREB1)) I[DENSE_INVX_ZAGREB1] = (double)z1;
        if (needs(DENSE_INVX_ZAGREB2)) I[DENSE_INVX_ZAGREB2] = (double)z2;
        if (needs(DENSE_INVX_TRIANGLES)) I[DENSE_INVX_TRIANGLES] = (double)(tri / 3);
    }
    double diag[MAX_N], sub[MAX_N];
    // one matrix, up to four passes: the distance pass on the rows the BFS left, then the adjacency, Laplacian and signless-Laplacian
    // refills from the bitsets and the degrees
    if (need_dist) {
        ah_householder(A, n, diag, sub, DENSE_INV_DEFLATE);
        I[DENSE_INV_DIST_EIG] = ah_multisection(diag, sub, n, dist_k);
    }
    for (int pass = 1; pass < 4; ++pass) {
        const int which = pass == 1 ? DENSE_INV_ADJ_EIG : pass == 2 ? DENSE_INVX_LAP_EIG : DENSE_INVX_SLAP_EIG;
        if (!needs(which)) continue;
        const double off = pass == 2 ? -1.0 : 1.0;
        for (int u = 0; u < n; ++u)
            for (int v = 0; v < n; ++v) A[u * P + v] = pass > 1 && u == v ? (double)deg[u] : (adj[u] >> v) & 1ull ? off : 0.0;
        ah_householder(A, n, diag, sub, DENSE_INV_DEFLATE);
        I[which] = ah_multisection(diag, sub, n, pass == 1 ? r.adj_index : pass == 2 ? r.lap_index : r.slap_index);
    }
    double c = r.bias;
    for (int i = 0; i < DENSE_INVX_COUNT; ++i) {
        out->inv[i] = I[i];
        if (r.weight[i] != 0.0) {
            const double term = r.weight[i] * I[i];
            c = c + term;
        }
    }
    for (int t = 0; t < r.n_terms; ++t) {
        const DenseInvxTerm &p = r.term[t];
        if (p.coef == 0.0) continue;
        const double v = p.op == DENSE_INVX_DIV ? I[p.a] / I[p.b] : I[p.a] * I[p.b];
        const double term = p.coef * v;
        c = c + term;
    }
    out->dist_k = dist_k;
    out->computed = DENSE_INV_ALWAYS | need;
    out->cost = (float)c;
    out->eval = r.eval_scale * (out->cost + r.eval_offset);
}

// ---- spectrum invariant cost (c21_host.h: DenseInvsRecipe; AZD_ENGINE_DENSE_INVS): the host form of dense_invs_cost_wave
// (dense_invs_cost.inc), the same IEEE operations in the same order, over the stages above and the whole-spectrum finisher.
const char *dense_invs_check_graph(const uint64_t *adj, int n) {
    return ah_check_graph(adj, n, DENSE_INVS_MAX_N, "n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)");
}
const char *dense_invs_check_graph_wide(const uint64_t *adj, int n) {
    static_assert(DENSE_INVS_WIDE_MAX_N <= DENSE_AH_WIDE_MAX_N, "the host stages below are sized by DENSE_AH_WIDE_MAX_N");
    return ah_check_graph(adj, n, DENSE_INVS_WIDE_MAX_N, "n: the wide spectrum invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVS_WIDE_MAX_N)");
}
const char *dense_invs_check_recipe(const DenseInvsRecipe *r, int n) {
    if (!r) return "recipe: null";
    bool any = false;
    for (int i = 0; i < DENSE_INVS_COUNT; ++i) {
        if (!std::isfinite(r->weight[i])) return "weight: every weight must be finite";
        any = any || r->weight[i] != 0.0;
    }
    if (r->n_terms < 0 || r->n_terms > DENSE_INVX_MAX_TERMS) return "n_terms: must be in 0 .. 4 (AZD_DENSE_INVX_MAX_TERMS)";
    for (int t = 0; t < r->n_terms; ++t) {
        const DenseInvxTerm &p = r->term[t];
        if (!std::isfinite(p.coef)) return "term.coef: every coefficient must be finite";
        if (p.a < 0 || p.a >= DENSE_INVS_COUNT) return "term.a: must be in 0 .. 20 (an invariant's index)";
        if (p.b < 0 || p.b >= DENSE_INVS_COUNT) return "term.b: must be in 0 .. 20 (an invariant's index)";
        if (p.op != DENSE_INVX_MUL && p.op != DENSE_INVX_DIV) return "term.op: must be AZD_DENSE_INVX_MUL or AZD_DENSE_INVX_DIV";
        if (p.op == DENSE_INVX_DIV && !((DENSE_INVS_DIVISORS >> p.b) & 1u))
            return "term.b: a divisor must be positive on every connected graph: indices 0 .. 7, 12 (randic), 13 (zagreb1), 14 (zagreb2), 16 .. 20 (the energies and the spread)";
        any = any || p.coef != 0.0;
    }
    if (!any) return "weight: all twenty-one weights and all coefficients are zero";
    if (!std::isfinite(r->bias)) return "bias: must be finite";
    if (!std::isfinite(r->eval_offset)) return "eval_offset: must be finite";
    if (!std::isfinite(r->eval_scale) || r->eval_scale == 0.0f) return "eval_scale: must be finite and not zero";
    if (r->adj_index < 0 || r->adj_index > n - 1) return "adj_index: must be in 0 .. n - 1 (descending index into the adjacency spectrum)";
    if (r->dist_index != DENSE_INV_INDEX_AH && (r->dist_index < 0 || r->dist_index > n - 1))
        return "dist_index: must be in 0 .. n - 1 (descending index into the distance spectrum) or AZD_DENSE_INV_INDEX_AH";
    if (r->lap_index < 0 || r->lap_index > n - 1) return "lap_index: must be in 0 .. n - 1 (descending index into the Laplacian spectrum)";
    if (r->slap_index < 0 || r->slap_index > n - 1) return "slap_index: must be in 0 .. n - 1 (descending index into the signless-Laplacian spectrum)";
    return nullptr;
}
// the whole-spectrum finisher: slot l < n brackets eigenvalue l (ascending) of the tridiagonal matrix by a bisection of its own
static void invs_whole_spectrum(const double *diag, const double *sub, int n, double *theta) {
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    double sub2[MAX_N], R = 0.0;
    for (int i = 0; i < n; ++i) {
        sub2[i] = sub[i] * sub[i];
        const double g = (std::fabs(diag[i]) + (i > 0 ? std::fabs(sub[i - 1]) : 0.0)) + std::fabs(sub[i]);
        if (g > R) R = g;
    }
    for (int l = 0; l < n; ++l) {
        double hi = R + 1.0, lo = -hi;
        for (int round = 0; round < DENSE_INVS_ROUNDS; ++round) {
            const double x = (lo + hi) * 0.5;
            if (ah_sturm(diag, sub2, n, x) <= l) lo = x;
            else hi = x;
        }
        theta[l] = (lo + hi) * 0.5;
    }
}
// matrix `which` of the graph (DENSE_INVS_MATRIX_*) in A; the distance matrix is what ah_bfs left there
static void invs_fill(const uint64_t *adj, int n, const int *deg, int which, double *A) {
    constexpr int P = DENSE_AH_STRIDE;
    const double off = which == DENSE_INVS_MATRIX_LAP ? -1.0 : 1.0;
    for (int u = 0; u < n; ++u)
        for (int v = 0; v < n; ++v)
            A[u * P + v] = which != DENSE_INVS_MATRIX_ADJ && u == v ? (double)deg[u] : (adj[u] >> v) & 1ull ? off : 0.0;
}
void dense_invs_spectrum_host(const uint64_t *adj, int n, int which, double *out) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    std::vector<double> Am((size_t)MAX_N * P, 0.0);
    int trans[MAX_N], ecc[MAX_N], deg[MAX_N];
    for (int u = 0; u < n; ++u) deg[u] = __builtin_popcountll(adj[u]);
    if (which == DENSE_INVS_MATRIX_DIST) ah_bfs(adj, n, Am.data(), trans, ecc);
    else invs_fill(adj, n, deg, which, Am.data());
    double diag[MAX_N], sub[MAX_N];
    ah_householder(Am.data(), n, diag, sub, DENSE_INV_DEFLATE);
    invs_whole_spectrum(diag, sub, n, out);
}
void dense_invs_cost_host(const uint64_t *adj, int n, const DenseInvsRecipe &r, DenseInvsCost *out) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    const uint32_t need = dense_invs_needed(r);
    const auto needs = [need](int i) { return ((need >> i) & 1u) != 0u; };
    const bool need_dist = needs(DENSE_INV_DIST_EIG) || needs(DENSE_INVS_DIST_ENERGY);
    std::vector<double> Am((size_t)MAX_N * P, 0.0);
    double *A = Am.data();
    int trans[MAX_N], ecc[MAX_N], deg[MAX_N];
    ah_bfs(adj, n, need_dist ? A : nullptr, trans, ecc);
    int m2 = 0, max_deg = 0, min_deg = 0x7FFFFFFF, diam = 0, rad = 0x7FFFFFFF, min_t = 0x7FFFFFFF, max_t = 0, sum_t = 0;
    for (int u = 0; u < n; ++u) {
        deg[u] = __builtin_popcountll(adj[u]);
        m2 += deg[u];
        max_deg = deg[u] > max_deg ? deg[u] : max_deg;
        min_deg = deg[u] < min_deg ? deg[u] : min_deg;
        diam = ecc[u] > diam ? ecc[u] : diam;
        rad = ecc[u] < rad ? ecc[u] : rad;
        min_t = trans[u] < min_t ? trans[u] : min_t;
        max_t = trans[u] > max_t ? trans[u] : max_t;
        sum_t += trans[u];
    }
    const int q23 = (2 * diam) / 3;
    const int dist_k = r.dist_index != DENSE_INV_INDEX_AH ? r.dist_index : q23 >= 1 ? q23 - 1 : n - 1;
    double I[DENSE_INVS_COUNT];
    I[0] = (double)(m2 / 2);
    I[1] = (double)max_deg;
    I[2] = (double)min_deg;
    I[3] = (double)diam;
    I[4] = (double)rad;
    I[5] = (double)min_t / (double)(n - 1);
    I[6] = (double)max_t / (double)(n - 1);
    I[7] = (double)sum_t / (double)(n * (n - 1));
    for (int i = DENSE_INV_ADJ_EIG; i < DENSE_INVS_COUNT; ++i) I[i] = 0.0;
    // the degree-based invariants: vertex u over its neighbours v < u, ascending (every edge once)
    if ((need >> DENSE_INVX_RANDIC) & 0xFu) {
        double part[64];
        int z1 = 0, z2 = 0, tri = 0;
        for (int u = 0; u < 64; ++u) part[u] = 0.0;
        for (int u = 0; u < n; ++u) {
            z1 += deg[u] * deg[u];
            double rr = 0.0, cc = 0.0;
            for (int v = 0; v < u; ++v)
                if ((adj[u] >> v) & 1ull) {
                    const double s = std::sqrt((double)(deg[u] * deg[v]));
                    const double term = 1.0 / s;
                    const double t = rr + term; // TwoSum, as in the extended invariant cost
                    const double bp = t - rr;
                    const double ap = t - bp;
                    const double e = (rr - ap) + (term - bp);
                    cc = cc + e;
                    rr = t;
                    z2 += deg[u] * deg[v];
                    tri += __builtin_popcountll(adj[u] & adj[v]);
                }
            part[u] = rr + cc;
        }
        if (needs(DENSE_INVX_RANDIC)) I[DENSE_INVX_RANDIC] = ah_tree64(part);
        if (needs(DENSE_INVX_ZAGREB1)) I[DENSE_INVX_ZAGREB1] = (double)z1;
        if (needs(DENSE_INVX_ZAGREB2)) I[DENSE_INVX_ZAGREB2] = (double)z2;
        if (needs(DENSE_INVX_TRIANGLES)) I[DENSE_INVX_TRIANGLES] = (double)(tri / 3);
    }
    const double shift = (double)m2 / (double)n; // the mean degree: the centre of the Laplacian energies
    double diag[MAX_N], sub[MAX_N], theta[64], part[64];
    // one matrix, up to four passes, each reduced once: the distance pass on the rows the BFS left, then the adjacency, Laplacian and
    // signless-Laplacian refills; after a reduction the multisection for the *_eig and the bisections for the energy, each if needed
    for (int pass = 0; pass < 4; ++pass) {
        const int eig_i = pass == 0 ? DENSE_INV_DIST_EIG : pass == 1 ? DENSE_INV_ADJ_EIG : pass == 2 ? DENSE_INVX_LAP_EIG : DENSE_INVX_SLAP_EIG;
        const int energy_i = pass == 0 ? DENSE_INVS_DIST_ENERGY : pass == 1 ? DENSE_INVS_ADJ_ENERGY : pass == 2 ? DENSE_INVS_LAP_ENERGY : DENSE_INVS_SLAP_ENERGY;
        const bool whole = needs(energy_i) || (pass == 1 && needs(DENSE_INVS_ADJ_SPREAD));
        if (!needs(eig_i) && !whole) continue;
        if (pass > 0) invs_fill(adj, n, deg, pass == 1 ? DENSE_INVS_MATRIX_ADJ : pass == 2 ? DENSE_INVS_MATRIX_LAP : DENSE_INVS_MATRIX_SLAP, A);
        ah_householder(A, n, diag, sub, DENSE_INV_DEFLATE);
        if (needs(eig_i))
            I[eig_i] = ah_multisection(diag, sub, n, pass == 0 ? dist_k : pass == 1 ? r.adj_index : pass == 2 ? r.lap_index : r.slap_index);
        if (!whole) continue;
        invs_whole_spectrum(diag, sub, n, theta);
        if (needs(energy_i)) {
            for (int l = 0; l < 64; ++l) part[l] = l >= n ? 0.0 : pass >= 2 ? std::fabs(theta[l] - shift) : std::fabs(theta[l]);
            I[energy_i] = ah_tree64(part);
        }
        if (pass == 1 && needs(DENSE_INVS_ADJ_SPREAD)) I[DENSE_INVS_ADJ_SPREAD] = theta[n - 1] - theta[0];
    }
    double c = r.bias;
    for (int i = 0; i < DENSE_INVS_COUNT; ++i) {
        out->inv[i] = I[i];
        if (r.weight[i] != 0.0) {
            const double term = r.weight[i] * I[i];
            c = c + term;
        }
    }
    for (int t = 0; t < r.n_terms; ++t) {
        const DenseInvxTerm &p = r.term[t];
        if (p.coef == 0.0) continue;
        const double v = p.op == DENSE_INVX_DIV ? I[p.a] / I[p.b] : I[p.a] * I[p.b];
        const double term = p.coef * v;
        c = c + term;
    }
    out->dist_k = dist_k;
    out->computed = DENSE_INV_ALWAYS | need;
    out->cost = (float)c;
    out->eval = r.eval_scale * (out->cost + r.eval_offset);
}

} // namespace azd
