// dense_cost_host.h -- the dense-graph space's spectral costs on the host (see dense_cost_host.cpp): the Aouchiche-Hansen cost and the
// three recipe costs (weighted-invariant, extended, spectrum), their constants and ABI mirrors -- which the kernel units read too -- and
// the checks of a graph and of a recipe.  c21_host.h includes this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace azd {

// Aouchiche-Hansen cost of a connected graph on 4 <= n <= DENSE_AH_MAX_N vertices (connected_bitset_graph/mod.rs:156-198,
// restated; DESIGN.md "The AH cost"): the host form of dense_ah_cost_wave (dense_ah_cost.inc), the same IEEE f64 operations in
// the same order.  The constants below are shared by both.
constexpr int DENSE_AH_MAX_N = 32;
constexpr int DENSE_AH_WIDE_MAX_N = 64;    // AZD_ENGINE_DENSE_AH_WIDE engines, azd_dense_ah_cost_wide: the same procedure with 64 rows
constexpr int DENSE_AH_STRIDE = 65;        // row pitch of the host's working matrix in doubles (either limit)
constexpr int DENSE_AH_ROUNDS = 11;        // multisection rounds of 64 shifts: the bracket shrinks by 65 a round
constexpr double DENSE_AH_TINY = 0x1p-512; // a Sturm pivot smaller than this in magnitude becomes -DENSE_AH_TINY
struct DenseAhCost {
    double proximity, eigenvalue; // pi = min transmission / (n - 1); entry k of the distance spectrum, descending
    int diameter, k;
    float cost, eval;             // (f32)(pi + eigenvalue); slope (cost + 2) with slope = 1 / (2 n + 2) (build-defined)
};
float dense_ah_eval_slope(int n);
// nullptr when the graph is acceptable, else what is wrong with it (an argument name leads the text): 4 <= n <= max_n, else bad_n
const char *dense_check_graph(const uint64_t *adj, int n, int max_n, const char *bad_n);
const char *dense_ah_check_graph(const uint64_t *adj, int n);      // 4 <= n <= DENSE_AH_MAX_N
const char *dense_ah_check_graph_wide(const uint64_t *adj, int n); // 4 <= n <= DENSE_AH_WIDE_MAX_N
// n <= DENSE_AH_WIDE_MAX_N (one function behind azd_dense_ah_cost and azd_dense_ah_cost_wide: the limit is the callers' check)
void dense_ah_cost_host(const uint64_t *adj, int n, DenseAhCost *out);

// Weighted-invariant cost of a connected graph on 4 <= n <= DENSE_INV_MAX_N vertices (BUILD-DEFINED; DESIGN.md "The invariant
// cost"): ten invariants in a fixed order -- index and name are ABI -- combined with weights the caller gives at run time:
//   0 edges m   1 max_degree   2 min_degree   3 diameter   4 radius   5 proximity = min_u t(u) / (n - 1)
//   6 remoteness = max_u t(u) / (n - 1)   7 avg_distance = sum_u t(u) / (n (n - 1))
//   8 adj_eig = eigenvalue of the adjacency matrix at descending index adj_index
//   9 dist_eig = eigenvalue of the distance matrix at descending index dist_index, or (DENSE_INV_INDEX_AH) k = 2D/3 - 1, n - 1 when 2D/3 = 0
//   c = bias; for i = 0 .. 9 in order, if weight[i] != 0: c = c + weight[i] * I_i (two IEEE f64 operations, never fused)
//   cost = (float)c;  eval = eval_scale * (cost + eval_offset)  (f32, this order)
// A spectral invariant whose weight is zero is not computed: its value is 0.0 and its bit of `computed` is clear.  The matching
// number is not in the list: it needs the default cost's per-node matching arena and repair (space_dense.inc), and lambda_1 + mu
// stays that tier's objective.  The spectral procedure and its constants are the Aouchiche-Hansen cost's (DENSE_AH_ROUNDS,
// DENSE_AH_TINY); with weight[5] = weight[9] = 1, dist_index = DENSE_INV_INDEX_AH, offset 2 and scale 1.0f / (2 n + 2) the cost
// and eval are that cost's, bit for bit.
constexpr int DENSE_INV_MAX_N = 32;
constexpr int DENSE_INV_WIDE_MAX_N = 64; // AZD_ENGINE_DENSE_INV_WIDE engines, azd_dense_inv_cost_wide: the same procedure with 64 rows
// At every n, in the invariant costs (INV at either row limit and INVX; the AH cost reduces distance matrices only, which do not
// starve, and keeps its bits): a Householder step whose column tail -- the sum of squares below the subdiagonal -- is below this is
// skipped like one whose tail is exactly zero.  A rank-deficient matrix (the adjacency matrix of a double broom: rank 20 at n = 50;
// of a complete bipartite graph: rank 2) leaves a trailing block of rounding noise that shrinks by about 2^-53 every other step;
// once its squares are subnormal, beta = 2 / (tail + v1 v1) overflows and the reduction ends in NaN, which the multisection turns
// into a finite, wrong eigenvalue.  That takes some 36 steps on the brooms of 50 and 56 vertices that were met first, but 20 on
// K(10,11) relabelled (n = 21) and on double_broom(23, 19, 2), the heavier end first: the narrow tiers starve from 19 vertices on
// (DESIGN.md "The invariant cost up to 64 vertices" has the counts).  All four matrices have integer entries, so ||M||_F >= 1: the
// entries dropped are below 2^-100 each, far inside the cost's own backward error 64 n 2^-53 ||M||_F, and every tail that is
// reduced keeps beta <= 2^201.
constexpr double DENSE_INV_DEFLATE = 0x1p-200;
constexpr int DENSE_INV_COUNT = 10;
constexpr int DENSE_INV_ADJ_EIG = 8, DENSE_INV_DIST_EIG = 9;
constexpr int DENSE_INV_INDEX_AH = -1;
constexpr uint32_t DENSE_INV_ALWAYS = 0xFFu; // bits of `computed` that are always set: the eight integer invariants
struct DenseInvRecipe {
    double weight[DENSE_INV_COUNT];
    double bias;
    int adj_index, dist_index;
    float eval_offset, eval_scale;
};
struct DenseInvCost {
    double inv[DENSE_INV_COUNT];
    int dist_k;        // the distance index the recipe resolves to on this graph (reported whether or not dist_eig is computed)
    uint32_t computed; // bit i: inv[i] was computed
    float cost, eval;
};
// n <= DENSE_INV_WIDE_MAX_N (one function behind azd_dense_inv_cost and azd_dense_inv_cost_wide: the limit is the callers' check)
void dense_inv_cost_host(const uint64_t *adj, int n, const DenseInvRecipe &r, DenseInvCost *out);

// Extended invariant cost of a connected graph on 4 <= n <= DENSE_INVX_MAX_N vertices, or DENSE_INVX_WIDE_MAX_N in the 64-row form
// (BUILD-DEFINED; DESIGN.md "The extended invariant cost"; AZD_ENGINE_DENSE_INVX, AZD_ENGINE_DENSE_INVX_WIDE): sixteen invariants -- index and name are ABI.  0 .. 9 are the weighted-invariant cost's;
//   10 lap_eig = eigenvalue of L = D - A at descending index lap_index   11 slap_eig = eigenvalue of Q = D + A at slap_index
//   12 randic = sum_{uv in E} 1 / sqrt(d_u d_v): per vertex u, over its neighbours v < u ascending, x = 1.0 / sqrt((double)(d_u d_v)),
//      (r, e) = TwoSum(r, x), c = c + e, one IEEE operation at a time (a compensated sum: the vertex's part r + c is right to an ulp;
//      plain r = r + x is off by four ulps of the sum on K_27, whose 351 equal terms round the same way, and misses the
//      n 2^-52 of math.fsum that the invariant is held to); then the balanced tree over the 64 lanes' parts (vertices >= n hold 0)
//   13 zagreb1 = sum_u d_u^2   14 zagreb2 = sum_{uv in E} d_u d_v   15 triangles = (sum_{uv in E} popcount(N(u) & N(v))) / 3   (integers)
//   c = bias; the sixteen weights as above; then for t = 0 .. n_terms - 1 in order, if coef_t != 0: v = I_a * I_b or I_a / I_b,
//   c = c + coef_t * v (three IEEE f64 operations); cost = (float)c; eval = eval_scale * (cost + eval_offset)
// 0 .. 7 are always computed; each of 8 .. 15 only when its weight is not zero or a pair term with a non-zero coefficient names it
// (else 0.0, bit clear).  A divisor is one of DENSE_INVX_DIVISORS: positive on every connected graph with n >= 4, so the cost is
// finite.  With weights 10 .. 15 zero and no term the sequence of operations is dense_inv_cost_host's.
constexpr int DENSE_INVX_MAX_N = 32;
constexpr int DENSE_INVX_WIDE_MAX_N = 64; // AZD_ENGINE_DENSE_INVX_WIDE engines, azd_dense_invx_cost_wide: the same procedure with 64 rows
constexpr int DENSE_INVX_COUNT = 16;
constexpr int DENSE_INVX_LAP_EIG = 10, DENSE_INVX_SLAP_EIG = 11, DENSE_INVX_RANDIC = 12, DENSE_INVX_ZAGREB1 = 13, DENSE_INVX_ZAGREB2 = 14,
              DENSE_INVX_TRIANGLES = 15;
constexpr int DENSE_INVX_MAX_TERMS = 4;
constexpr int DENSE_INVX_MUL = 0, DENSE_INVX_DIV = 1;
constexpr uint32_t DENSE_INVX_DIVISORS = 0xFFu | 1u << DENSE_INVX_RANDIC | 1u << DENSE_INVX_ZAGREB1 | 1u << DENSE_INVX_ZAGREB2;
struct DenseInvxTerm {
    double coef;
    int a, b, op;
};
struct DenseInvxRecipe {
    double weight[DENSE_INVX_COUNT];
    double bias;
    int adj_index, dist_index, lap_index, slap_index;
    float eval_offset, eval_scale;
    DenseInvxTerm term[DENSE_INVX_MAX_TERMS];
    int n_terms;
};
struct DenseInvxCost {
    double inv[DENSE_INVX_COUNT];
    int dist_k;
    uint32_t computed;
    float cost, eval;
};
// bits 8 .. 15 of `computed` under a checked recipe: the invariants its weights and its pair terms ask for (constexpr: the device
// code calls it too)
constexpr uint32_t dense_invx_needed(const DenseInvxRecipe &r) {
    uint32_t m = 0;
    for (int i = DENSE_INV_ADJ_EIG; i < DENSE_INVX_COUNT; ++i) m |= r.weight[i] != 0.0 ? 1u << i : 0u;
    for (int t = 0; t < r.n_terms; ++t)
        if (r.term[t].coef != 0.0) m |= (1u << r.term[t].a | 1u << r.term[t].b) & ~DENSE_INV_ALWAYS;
    return m;
}
// n <= DENSE_INVX_WIDE_MAX_N (one function behind azd_dense_invx_cost and azd_dense_invx_cost_wide: the limit is the callers' check)
void dense_invx_cost_host(const uint64_t *adj, int n, const DenseInvxRecipe &r, DenseInvxCost *out);

// Spectrum invariant cost of a connected graph on 4 <= n <= DENSE_INVS_MAX_N vertices, or DENSE_INVS_WIDE_MAX_N in the 64-row form
// (BUILD-DEFINED; DESIGN.md "The spectrum invariant cost"; AZD_ENGINE_DENSE_INVS, AZD_ENGINE_DENSE_INVS_WIDE): twenty-one invariants -- index and name are ABI.  0 .. 15 are the extended invariant cost's;
//   16 adj_energy = sum_l |theta_l(A)|   17 dist_energy = sum_l |theta_l(D)|
//   18 lap_energy = sum_l |theta_l(L) - s|   19 slap_energy = sum_l |theta_l(Q) - s|,  s = (double)(sum of degrees) / (double)n
//   20 adj_spread = theta_{n-1}(A) - theta_0(A)
// theta_0 <= .. <= theta_{n-1}: ALL eigenvalues of the tridiagonal form the matrix's one reduction leaves (the same Householder
// steps, the same DENSE_INV_DEFLATE rule), each by a bisection of its own on the Sturm count: hi = R + 1, lo = -hi (R the
// Gershgorin bound, as the multisection's), DENSE_INVS_ROUNDS rounds of x = (lo + hi) * 0.5, c = count(x), c <= l ? lo = x : hi = x,
// then theta_l = (lo + hi) * 0.5.  The final bracket 2 (R + 1) 2^-67 is no wider than the multisection's 2 (R + 1) 65^-11.  An energy
// is the balanced tree over 64 slots of |theta_l| or |theta_l - s| (slots >= n hold 0.0); every step one IEEE operation.
// A matrix is reduced at most once per cost; after it the multisection runs only when the matrix's *_eig is needed, the bisections
// only when its energy (or, for A, the spread) is.  Needed as in the extended cost: a non-zero weight, or a pair term with a
// non-zero coefficient that names it; else 0.0 and the bit of `computed` clear.  All five are positive on every connected graph
// with n >= 4 (A, D, L - sI and Q - sI are not zero and have trace zero), so all five may divide.  With weights 16 .. 20 zero and no
// term naming 16 .. 20 the sequence of operations is the extended invariant cost's: this recipe is the form the host works in, and
// the two smaller recipes are widened to it (dense_widen_recipe).
constexpr int DENSE_INVS_MAX_N = 32;
constexpr int DENSE_INVS_WIDE_MAX_N = 64; // AZD_ENGINE_DENSE_INVS_WIDE engines, azd_dense_invs_cost_wide: the same procedure with 64 rows
constexpr int DENSE_INVS_COUNT = 21;
constexpr int DENSE_INVS_ADJ_ENERGY = 16, DENSE_INVS_DIST_ENERGY = 17, DENSE_INVS_LAP_ENERGY = 18, DENSE_INVS_SLAP_ENERGY = 19, DENSE_INVS_ADJ_SPREAD = 20;
constexpr int DENSE_INVS_ROUNDS = 67; // bisection rounds of the whole-spectrum finisher: the same for every lane
constexpr uint32_t DENSE_INVS_DIVISORS = DENSE_INVX_DIVISORS | 0x1Fu << DENSE_INVS_ADJ_ENERGY;
struct DenseInvsRecipe {
    double weight[DENSE_INVS_COUNT];
    double bias;
    int adj_index, dist_index, lap_index, slap_index;
    float eval_offset, eval_scale;
    DenseInvxTerm term[DENSE_INVX_MAX_TERMS];
    int n_terms;
};
struct DenseInvsCost {
    double inv[DENSE_INVS_COUNT];
    int dist_k;
    uint32_t computed;
    float cost, eval;
};
// bits 8 .. 20 of `computed` under a checked recipe (constexpr: the device code calls it too)
constexpr uint32_t dense_invs_needed(const DenseInvsRecipe &r) {
    uint32_t m = 0;
    for (int i = DENSE_INV_ADJ_EIG; i < DENSE_INVS_COUNT; ++i) m |= r.weight[i] != 0.0 ? 1u << i : 0u;
    for (int t = 0; t < r.n_terms; ++t)
        if (r.term[t].coef != 0.0) m |= (1u << r.term[t].a | 1u << r.term[t].b) & ~DENSE_INV_ALWAYS;
    return m;
}
// the four matrices, as azd_dense_invs_spectrum names them
constexpr int DENSE_INVS_MATRIX_ADJ = 0, DENSE_INVS_MATRIX_DIST = 1, DENSE_INVS_MATRIX_LAP = 2, DENSE_INVS_MATRIX_SLAP = 3;
// n <= DENSE_INVS_WIDE_MAX_N (one function behind azd_dense_invs_cost and azd_dense_invs_cost_wide, and one behind the two
// spectrum calls: the limit is the callers' check).  The host cost of all three recipes: the two smaller ones widen, call it, narrow.
void dense_invs_cost_host(const uint64_t *adj, int n, const DenseInvsRecipe &r, DenseInvsCost *out);
// theta_0 .. theta_{n-1} of matrix `which` (DENSE_INVS_MATRIX_*), ascending: what the energies and the spread are summed from
void dense_invs_spectrum_host(const uint64_t *adj, int n, int which, double *out);

// ---- the three recipe costs as one family.  Every recipe is a prefix of DenseInvsRecipe: a smaller one widens to it with the
// weights it lacks zero, lap_index = slap_index = 0 and no term where it has none, everything else verbatim (checked or not).
DenseInvsRecipe dense_widen_recipe(const DenseInvRecipe &r);
DenseInvsRecipe dense_widen_recipe(const DenseInvxRecipe &r);
inline const DenseInvsRecipe &dense_widen_recipe(const DenseInvsRecipe &r) { return r; }
// bias, the first `count` weights and the pair terms over the invariants, then (float)c and the eval: the one statement on the host
// of the sequence the device runs (dense_spectral.inc), one IEEE operation at a time
void dense_recipe_combine(const DenseInvsRecipe &r, const double *inv, int count, float *cost, float *eval);
enum DenseFamily { DENSE_FAMILY_INV, DENSE_FAMILY_INVX, DENSE_FAMILY_INVS, DENSE_FAMILY_COUNT };
// What differs between the three, beyond the types: the limits, and the texts as the checks and the engine's entries spell them
struct DenseFamilyDesc {
    int count;         // invariants, and doubles per agent in front of the engine's copy of the recipe
    bool extended;     // the recipe has lap_index, slap_index and pair terms
    uint32_t divisors; // invariants a pair term may divide by
    const char *all_zero, *term_a, *term_b, *divisor;                       // check_recipe's texts that differ
    int max_n[2];                                                           // [wide]: the row limits ...
    const char *bad_n[2];                                                   // ... and check_graph's text beyond them
    const char *flag[2], *argmin_reader[2];                                 // [wide]: the engine flag and the tier's argmin entry
    const char *setter, *agent_cost;                                        // the family's recipe setter and per-agent reader
};
const DenseFamilyDesc &dense_family(DenseFamily f);
// nullptr when the widened recipe is acceptable to family f for graphs on n vertices, else what is wrong with it (a field name leads
// the text).  One order of checks serves all three: a recipe without terms passes the term checks.
const char *dense_check_recipe_wide(const DenseInvsRecipe &r, int n, const DenseFamilyDesc &f);
template <DenseFamily F> struct DenseFamilyOf;
template <> struct DenseFamilyOf<DENSE_FAMILY_INV> {
    using Recipe = DenseInvRecipe;
    using Cost = DenseInvCost;
    static constexpr auto cost_host = dense_inv_cost_host;
};
template <> struct DenseFamilyOf<DENSE_FAMILY_INVX> {
    using Recipe = DenseInvxRecipe;
    using Cost = DenseInvxCost;
    static constexpr auto cost_host = dense_invx_cost_host;
};
template <> struct DenseFamilyOf<DENSE_FAMILY_INVS> {
    using Recipe = DenseInvsRecipe;
    using Cost = DenseInvsCost;
    static constexpr auto cost_host = dense_invs_cost_host;
};
template <DenseFamily F>
const char *dense_check_recipe(const typename DenseFamilyOf<F>::Recipe *r, int n) {
    return r ? dense_check_recipe_wide(dense_widen_recipe(*r), n, dense_family(F)) : "recipe: null";
}

} // namespace azd
