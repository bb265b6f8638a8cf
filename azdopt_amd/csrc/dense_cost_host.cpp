// dense_cost_host.cpp -- the dense-graph space's spectral costs on the host: the stages (BFS, Householder reduction, Sturm-count
// multisection and bisection) as the 64-lane wave of dense_spectral.inc runs them, the Aouchiche-Hansen cost over them, the one host
// cost of the three recipe costs, and the checks of a graph and of a recipe.  One IEEE operation at a time: this file is built with
// -ffp-contract=off, like the kernel units whose results it must equal bit for bit.
#include "dense_cost_host.h"

#include <cmath>
#include <vector>

#include "c21_host.h"

namespace azd {

// ---- Aouchiche-Hansen cost (the dense space's second objective).  connected_bitset_graph/mod.rs:156-198 restated: BFS from every
// vertex over the bitsets (distance matrix, transmissions, diameter), proximity = min transmission / (n - 1), k = 2D/3 - 1 (n - 1
// when 2D/3 = 0), cost = (f32)(proximity + entry k of the distance matrix's eigenvalues sorted descending).  The eigenvalue comes
// from a Householder reduction to tridiagonal form and a Sturm-count multisection, written as the 64-lane wave of
// dense_ah_cost.inc runs it: `lane` loops stand for the lanes, tree64 for the xor-butterfly.  tests/dense_ah_ref.py is the same
// sequence in Python.
float dense_ah_eval_slope(int n) { return 1.0f / (float)(2 * n + 2); }
const char *dense_check_graph(const uint64_t *adj, int n, int max_n, const char *bad_n) {
    static_assert(DENSE_INVS_WIDE_MAX_N <= DENSE_AH_WIDE_MAX_N && DENSE_INVX_WIDE_MAX_N <= DENSE_AH_WIDE_MAX_N && DENSE_INV_WIDE_MAX_N <= DENSE_AH_WIDE_MAX_N,
                  "the host stages below are sized by DENSE_AH_WIDE_MAX_N");
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
    return dense_check_graph(adj, n, DENSE_AH_MAX_N, "n: the Aouchiche-Hansen cost needs 4 <= n <= 32 (AZD_DENSE_AH_MAX_N)");
}
const char *dense_ah_check_graph_wide(const uint64_t *adj, int n) {
    return dense_check_graph(adj, n, DENSE_AH_WIDE_MAX_N, "n: the wide Aouchiche-Hansen cost needs 4 <= n <= 64 (AZD_DENSE_AH_WIDE_MAX_N)");
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
// The three stages of the procedure, shared by the Aouchiche-Hansen cost and the recipe costs below.
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
// which reduces distance matrices only; the recipe costs pass DENSE_INV_DEFLATE at every n: dense_cost_host.h)
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

// ---- the three recipe costs (dense_cost_host.h: DenseInvRecipe, DenseInvxRecipe, DenseInvsRecipe): what differs between them ...
const DenseFamilyDesc &dense_family(DenseFamily f) {
    static const DenseFamilyDesc families[DENSE_FAMILY_COUNT] = {
        {DENSE_INV_COUNT, false, 0u, "weight: all ten weights are zero", nullptr, nullptr, nullptr,
         {DENSE_INV_MAX_N, DENSE_INV_WIDE_MAX_N},
         {"n: the weighted-invariant cost needs 4 <= n <= 32 (AZD_DENSE_INV_MAX_N)",
          "n: the wide weighted-invariant cost needs 4 <= n <= 64 (AZD_DENSE_INV_WIDE_MAX_N)"},
         {"AZD_ENGINE_DENSE_INV", "AZD_ENGINE_DENSE_INV_WIDE"}, {"azd_engine_dense_inv_argmin_data", "azd_engine_dense_inv_wide_argmin_data"},
         "azd_engine_set_dense_inv_recipe", "azd_engine_dense_inv_agent_cost"},
        {DENSE_INVX_COUNT, true, DENSE_INVX_DIVISORS, "weight: all sixteen weights and all coefficients are zero",
         "term.a: must be in 0 .. 15 (an invariant's index)", "term.b: must be in 0 .. 15 (an invariant's index)",
         "term.b: a divisor must be positive on every connected graph: indices 0 .. 7, 12 (randic), 13 (zagreb1), 14 (zagreb2)",
         {DENSE_INVX_MAX_N, DENSE_INVX_WIDE_MAX_N},
         {"n: the extended invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVX_MAX_N)",
          "n: the wide extended invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVX_WIDE_MAX_N)"},
         {"AZD_ENGINE_DENSE_INVX", "AZD_ENGINE_DENSE_INVX_WIDE"}, {"azd_engine_dense_invx_argmin_data", "azd_engine_dense_invx_wide_argmin_data"},
         "azd_engine_set_dense_invx_recipe", "azd_engine_dense_invx_agent_cost"},
        {DENSE_INVS_COUNT, true, DENSE_INVS_DIVISORS, "weight: all twenty-one weights and all coefficients are zero",
         "term.a: must be in 0 .. 20 (an invariant's index)", "term.b: must be in 0 .. 20 (an invariant's index)",
         "term.b: a divisor must be positive on every connected graph: indices 0 .. 7, 12 (randic), 13 (zagreb1), 14 (zagreb2), 16 .. 20 (the energies and the spread)",
         {DENSE_INVS_MAX_N, DENSE_INVS_WIDE_MAX_N},
         {"n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)",
          "n: the wide spectrum invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVS_WIDE_MAX_N)"},
         {"AZD_ENGINE_DENSE_INVS", "AZD_ENGINE_DENSE_INVS_WIDE"}, {"azd_engine_dense_invs_argmin_data", "azd_engine_dense_invs_wide_argmin_data"},
         "azd_engine_set_dense_invs_recipe", "azd_engine_dense_invs_agent_cost"},
    };
    return families[f];
}
// ... and how a smaller recipe becomes the largest, and the largest cost's record a smaller one's
template <class Recipe>
static DenseInvsRecipe widen_common(const Recipe &r) {
    DenseInvsRecipe w{}; // the weights r lacks are zero, lap_index = slap_index = 0, no term
    for (size_t i = 0; i < sizeof(r.weight) / sizeof(r.weight[0]); ++i) w.weight[i] = r.weight[i];
    w.bias = r.bias;
    w.adj_index = r.adj_index;
    w.dist_index = r.dist_index;
    w.eval_offset = r.eval_offset;
    w.eval_scale = r.eval_scale;
    return w;
}
DenseInvsRecipe dense_widen_recipe(const DenseInvRecipe &r) { return widen_common(r); }
DenseInvsRecipe dense_widen_recipe(const DenseInvxRecipe &r) {
    DenseInvsRecipe w = widen_common(r);
    w.lap_index = r.lap_index;
    w.slap_index = r.slap_index;
    for (int t = 0; t < DENSE_INVX_MAX_TERMS; ++t) w.term[t] = r.term[t];
    w.n_terms = r.n_terms;
    return w;
}
template <class Cost>
static void narrow_cost(const DenseInvsCost &w, Cost *out) {
    for (size_t i = 0; i < sizeof(out->inv) / sizeof(out->inv[0]); ++i) out->inv[i] = w.inv[i];
    out->dist_k = w.dist_k;
    out->computed = w.computed;
    out->cost = w.cost;
    out->eval = w.eval;
}
const char *dense_check_recipe_wide(const DenseInvsRecipe &r, int n, const DenseFamilyDesc &f) {
    bool any = false;
    for (int i = 0; i < f.count; ++i) {
        if (!std::isfinite(r.weight[i])) return "weight: every weight must be finite";
        any = any || r.weight[i] != 0.0;
    }
    if (r.n_terms < 0 || r.n_terms > DENSE_INVX_MAX_TERMS) return "n_terms: must be in 0 .. 4 (AZD_DENSE_INVX_MAX_TERMS)";
    for (int t = 0; t < r.n_terms; ++t) {
        const DenseInvxTerm &p = r.term[t];
        if (!std::isfinite(p.coef)) return "term.coef: every coefficient must be finite";
        if (p.a < 0 || p.a >= f.count) return f.term_a;
        if (p.b < 0 || p.b >= f.count) return f.term_b;
        if (p.op != DENSE_INVX_MUL && p.op != DENSE_INVX_DIV) return "term.op: must be AZD_DENSE_INVX_MUL or AZD_DENSE_INVX_DIV";
        if (p.op == DENSE_INVX_DIV && !((f.divisors >> p.b) & 1u)) return f.divisor;
        any = any || p.coef != 0.0;
    }
    if (!any) return f.all_zero;
    if (!std::isfinite(r.bias)) return "bias: must be finite";
    if (!std::isfinite(r.eval_offset)) return "eval_offset: must be finite";
    if (!std::isfinite(r.eval_scale) || r.eval_scale == 0.0f) return "eval_scale: must be finite and not zero";
    if (r.adj_index < 0 || r.adj_index > n - 1) return "adj_index: must be in 0 .. n - 1 (descending index into the adjacency spectrum)";
    if (r.dist_index != DENSE_INV_INDEX_AH && (r.dist_index < 0 || r.dist_index > n - 1))
        return "dist_index: must be in 0 .. n - 1 (descending index into the distance spectrum) or AZD_DENSE_INV_INDEX_AH";
    if (!f.extended) return nullptr;
    if (r.lap_index < 0 || r.lap_index > n - 1) return "lap_index: must be in 0 .. n - 1 (descending index into the Laplacian spectrum)";
    if (r.slap_index < 0 || r.slap_index > n - 1) return "slap_index: must be in 0 .. n - 1 (descending index into the signless-Laplacian spectrum)";
    return nullptr;
}

// ---- the host form of the recipe costs' wave (dense_spectral.inc: DenseCostRecipeT; dense_inv_cost.inc, dense_invx_cost.inc,
// dense_invs_cost.inc), the same IEEE operations in the same order, in named steps over the stages above.
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
// the integer reductions over deg / ecc / trans: invariants 0 .. 7, the degrees, the degree sum, and the distance index the recipe
// resolves to on this graph
static int invs_integer_invariants(const uint64_t *adj, int n, const int *trans, const int *ecc, int dist_index, int *deg, double *I, int *dist_k) {
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
    *dist_k = dist_index != DENSE_INV_INDEX_AH ? dist_index : q23 >= 1 ? q23 - 1 : n - 1;
    I[0] = (double)(m2 / 2);
    I[1] = (double)max_deg;
    I[2] = (double)min_deg;
    I[3] = (double)diam;
    I[4] = (double)rad;
    I[5] = (double)min_t / (double)(n - 1);
    I[6] = (double)max_t / (double)(n - 1);
    I[7] = (double)sum_t / (double)(n * (n - 1));
    return m2;
}
// the degree-based invariants 12 .. 15, those of them `need` names: vertex u over its neighbours v < u, ascending (every edge once)
static void invs_degree_invariants(const uint64_t *adj, int n, const int *deg, uint32_t need, double *I) {
    const auto needs = [need](int i) { return ((need >> i) & 1u) != 0u; };
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
void dense_recipe_combine(const DenseInvsRecipe &r, const double *inv, int count, float *cost, float *eval) {
    double c = r.bias;
    for (int i = 0; i < count; ++i)
        if (r.weight[i] != 0.0) {
            const double term = r.weight[i] * inv[i];
            c = c + term;
        }
    for (int t = 0; t < r.n_terms; ++t) {
        const DenseInvxTerm &p = r.term[t];
        if (p.coef == 0.0) continue;
        const double v = p.op == DENSE_INVX_DIV ? inv[p.a] / inv[p.b] : inv[p.a] * inv[p.b];
        const double term = p.coef * v;
        c = c + term;
    }
    *cost = (float)c;
    *eval = r.eval_scale * (*cost + r.eval_offset);
}
void dense_invs_cost_host(const uint64_t *adj, int n, const DenseInvsRecipe &r, DenseInvsCost *out) {
    constexpr int P = DENSE_AH_STRIDE;
    constexpr int MAX_N = DENSE_AH_WIDE_MAX_N;
    const uint32_t need = dense_invs_needed(r);
    const auto needs = [need](int i) { return ((need >> i) & 1u) != 0u; };
    const bool need_dist = needs(DENSE_INV_DIST_EIG) || needs(DENSE_INVS_DIST_ENERGY);
    std::vector<double> Am((size_t)MAX_N * P, 0.0);
    double *A = Am.data(), *I = out->inv;
    int trans[MAX_N], ecc[MAX_N], deg[MAX_N];
    ah_bfs(adj, n, need_dist ? A : nullptr, trans, ecc);
    const int m2 = invs_integer_invariants(adj, n, trans, ecc, r.dist_index, deg, I, &out->dist_k);
    for (int i = DENSE_INV_ADJ_EIG; i < DENSE_INVS_COUNT; ++i) I[i] = 0.0;
    if ((need >> DENSE_INVX_RANDIC) & 0xFu) invs_degree_invariants(adj, n, deg, need, I);
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
            I[eig_i] = ah_multisection(diag, sub, n, pass == 0 ? out->dist_k : pass == 1 ? r.adj_index : pass == 2 ? r.lap_index : r.slap_index);
        if (!whole) continue;
        invs_whole_spectrum(diag, sub, n, theta);
        if (needs(energy_i)) {
            for (int l = 0; l < 64; ++l) part[l] = l >= n ? 0.0 : pass >= 2 ? std::fabs(theta[l] - shift) : std::fabs(theta[l]);
            I[energy_i] = ah_tree64(part);
        }
        if (pass == 1 && needs(DENSE_INVS_ADJ_SPREAD)) I[DENSE_INVS_ADJ_SPREAD] = theta[n - 1] - theta[0];
    }
    out->computed = DENSE_INV_ALWAYS | need;
    dense_recipe_combine(r, I, DENSE_INVS_COUNT, &out->cost, &out->eval);
}
// The two smaller recipes: with the weights beyond theirs zero and no term naming an invariant beyond theirs, `need` has no bit above
// their count, so the degree step, the passes and the finishers they lack drop out and the sequence of operations is the one their
// own wave runs (dense_inv_cost.inc, dense_invx_cost.inc)
void dense_inv_cost_host(const uint64_t *adj, int n, const DenseInvRecipe &r, DenseInvCost *out) {
    DenseInvsCost w;
    dense_invs_cost_host(adj, n, dense_widen_recipe(r), &w);
    narrow_cost(w, out);
}
void dense_invx_cost_host(const uint64_t *adj, int n, const DenseInvxRecipe &r, DenseInvxCost *out) {
    DenseInvsCost w;
    dense_invs_cost_host(adj, n, dense_widen_recipe(r), &w);
    narrow_cost(w, out);
}

} // namespace azd
