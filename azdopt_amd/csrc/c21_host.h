// c21_host.h -- host-side helpers of the c21 space seam (see c21_host.cpp)
#pragma once
#include <stdint.h>

namespace azd {

constexpr uint64_t DOMAIN_ROOT = 0x726f6f74ull;  // "root"
constexpr uint64_t DOMAIN_PRED = 0x70726564ull;  // "pred"
constexpr uint64_t DOMAIN_RESET = 0x72657365ull; // "rese"

uint64_t splitmix64(uint64_t x);
uint64_t stream_key(uint64_t seed, uint64_t domain, uint64_t agent, uint64_t draw);
uint32_t draw_below(uint64_t r, uint32_t n);

int c21_state_dim(int n);
int c21_action_dim(int n);
int c21_key_words(int n);
float c21_eval_slope(int n);
void c21_lambda_bracket(int n, double *lo, double *hi);

void c21_shuffle_permitted(uint64_t seed, uint64_t domain, uint64_t agent, int n, int k, uint64_t *permitted);
void c21_fresh_root(uint64_t seed, uint64_t domain, uint64_t agent, int n, int k, uint8_t *parents,
                    uint64_t *permitted);
void c21_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin, int kmax,
                        uint8_t *parents, uint64_t *permitted);

// Ramsey space (ramsey_counts/space.rs:40-42): E = N(N-1)/2, ACTION = E*C, STATE = E*(2C+1)
int ramsey_edges(int n);
int ramsey_state_dim(int n, int c);
int ramsey_action_dim(int n, int c);
int ramsey_key_words(int n, int c);
void shuffle_mask(uint64_t seed, uint64_t domain, uint64_t agent, int universe, int words, int k, uint64_t *mask);
void ramsey_fresh_root(uint64_t seed, uint64_t domain, uint64_t agent, int n, int c, int k, uint8_t *colors,
                       uint64_t *permitted);
void ramsey_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int c, int kmin,
                           int kmax, uint8_t *colors, uint64_t *permitted);
// Weighted edge colours (05-r45.rs:84-90: WeightedIndex over the colour probabilities), integer-only once the thresholds exist:
//   cum_c = cum_{c-1} + w_c (f64, in colour order), W = cum_{C-1}, T_c = min(2^32, ceil((cum_c / W) * 2^32)) for c < C - 1;
//   colour of a draw r = #{ c < C - 1 : (r >> 32) >= T_c }.  Equal weights give draw_below(r, C) for C = 2, 3, 4.
// nullptr when the weights are acceptable (finite and positive), else what is wrong with them.
constexpr int RAMSEY_COLOR_THRESHOLDS = 3; // C - 1 at most
const char *ramsey_check_color_weights(const double *w, int c);
void ramsey_color_thresholds(const double *w, int c, uint64_t *thr /* [RAMSEY_COLOR_THRESHOLDS], 2^32 beyond C - 1 */);
uint32_t ramsey_weighted_color(uint64_t r, int c, const uint64_t *thr);
// thr = nullptr: ramsey_generate_roots
void ramsey_generate_roots_weighted(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int c, int kmin,
                                    int kmax, const uint64_t *thr, uint8_t *colors, uint64_t *permitted);

// dense-graph space (space_dense.inc; oracle/dense_graph.inc): E = N(N-1)/2 slots, ACTION = 2E (AddOrDeleteEdge,
// bitset_graph/space/action.rs:10-27), STATE = 3E + 1 (= E + ACTION + 1, 05-ah.rs:39-40)
int dense_edges(int n);
int dense_state_dim(int n);
int dense_action_dim(int n);
int dense_key_words(int n); // u64 words of an action-id set (host-visible keys, root slot masks)
bool dense_connected(const uint64_t *adj, int n);
void dense_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin, int kmax,
                          uint32_t p24, uint64_t *adj, uint64_t *slots);

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
// nullptr when the graph is acceptable, else what is wrong with it (an argument name leads the text)
const char *dense_ah_check_graph(const uint64_t *adj, int n);
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
// nullptr when the recipe is acceptable for graphs on n vertices, else what is wrong with it (a field name leads the text)
const char *dense_inv_check_recipe(const DenseInvRecipe *r, int n);
const char *dense_inv_check_graph(const uint64_t *adj, int n); // as dense_ah_check_graph, in this cost's words
const char *dense_inv_check_graph_wide(const uint64_t *adj, int n); // 4 <= n <= DENSE_INV_WIDE_MAX_N
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
// nullptr when the recipe is acceptable for graphs on n vertices, else what is wrong with it (a field name leads the text)
const char *dense_invx_check_recipe(const DenseInvxRecipe *r, int n);
const char *dense_invx_check_graph(const uint64_t *adj, int n); // 4 <= n <= DENSE_INVX_MAX_N, in this cost's words
const char *dense_invx_check_graph_wide(const uint64_t *adj, int n); // 4 <= n <= DENSE_INVX_WIDE_MAX_N
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
// term naming 16 .. 20 the sequence of operations is dense_invx_cost_host's.
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
const char *dense_invs_check_recipe(const DenseInvsRecipe *r, int n);
const char *dense_invs_check_graph(const uint64_t *adj, int n); // 4 <= n <= DENSE_INVS_MAX_N, in this cost's words
const char *dense_invs_check_graph_wide(const uint64_t *adj, int n); // 4 <= n <= DENSE_INVS_WIDE_MAX_N
// n <= DENSE_INVS_WIDE_MAX_N (one function behind azd_dense_invs_cost and azd_dense_invs_cost_wide, and one behind the two
// spectrum calls: the limit is the callers' check)
void dense_invs_cost_host(const uint64_t *adj, int n, const DenseInvsRecipe &r, DenseInvsCost *out);
// theta_0 .. theta_{n-1} of matrix `which` (DENSE_INVS_MATRIX_*), ascending: what the energies and the spread are summed from
void dense_invs_spectrum_host(const uint64_t *adj, int n, int which, double *out);

} // namespace azd
