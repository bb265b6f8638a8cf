/* dense_graph.inc -- CPU ORACLE pieces of the dense-graph space (test infrastructure; included by azd_oracle.cpp
 * inside its anonymous namespace).
 *
 * BASELINE.json configs[4] names an "N = 50 dense-graph StateActionSpace".  The reference holds the MATERIAL for one --
 * ConnectedBitsetGraph with is_cut_edge / action_kinds / maximum_matching / conjecture_2_1_cost
 * (graph-state/src/simple_graph/connected_bitset_graph/mod.rs:45-71,139-158,226-338), AddOrDeleteEdge action indexing
 * (bitset_graph/space/action.rs:4-27), the STATE = E + ACTION + 1 hint (examples/05-ah.rs:39-40) -- but NO live
 * NablaStateActionSpace over general graphs (05-ah.rs is a todo!() stub).  The space below is therefore BUILD-DEFINED
 * from those pieces, in the image of the c21 space ROTModifyParentsOnce (rooted_tree/space.rs:14-125):
 *
 *   state     a connected graph on N <= 64 vertices (neighbourhood bitsets) + the set of edge SLOTS (colex positions)
 *             that may still be modified; every slot at most once ("modify each edge once"): ActionsNeverRepeat, and
 *             the graph reached does not depend on the order: ActionOrderIndependent -- so ActionSet keys are licensed
 *   action    a < E: Add(edge at colex position a);  a >= E: Delete(edge at a - E)            (action.rs:10-27)
 *   legal     for a remaining slot: Add if the edge is absent; Delete if it is present and NOT a cut edge, so that the
 *             graph stays connected (action_kinds, mod.rs:139-158); ascending action id
 *   cost      Conjecture2Dot1Cost { lambda_1, matching } (mod.rs:319-344); evaluate = squish(mu + lambda_1) with the
 *             bounds of 04-c21-tree.rs:58-74; g = c_s - h, h_sa = c* as in that driver (:103-104)
 *   vector    [0, E) edge bools (edge_bools, mod.rs:127-137); [E, 2E) slot still modifiable and edge absent;
 *             [2E, 3E) slot still modifiable and edge present; [3E] = |remaining slots| / E
 *
 * Third-party arithmetic the reference delegates (faer eigenvalues, mod.rs:325-331) and its exponential matching search
 * (:235-317, kept below literally for validation on small graphs) are replaced by procedures the GPU can run per node;
 * oracle and GPU run the SAME procedures, so they agree bit for bit:
 *   lambda_1  power iteration on B = A + I from the all-ones vector: every y_v = (B x)_v is a sequential f64 sum in ascending
 *             neighbour order; at every fourth step (three plain steps x <- B x between) the Collatz-Wielandt ratios y_v / x_v
 *             (their min / max bracket the Perron root of a non-negative irreducible matrix; exact min / max) decide
 *             whether to stop -- bracket <= 1e-4, or 2000 steps -- and x is scaled back to maximum 1.  The VALUE is the
 *             Rayleigh quotient of the last pair, (x . y) / (x . x) - 1, whose error is of the order of the bracket
 *             SQUARED over the spectral gap (B is symmetric): half the steps of waiting for the bracket itself to close
 *             to 1e-7 -- where the bracket closed: a run that the 2000-step cap ends has no such bound (3.2e-5 measured on a
 *             64-vertex near-tree with a gap of 3.6e-3: DESIGN.md "The dense cost at the step cap").  The two dot products are balanced binary trees over the 64 vertex slots (0 beyond n) -- the order
 *             a wave's xor-butterfly adds in -- so oracle and GPU agree bit for bit
 *   mu        the matching number, EXACTLY (as the reference's maximum_matching().len(), mod.rs:235-317, whose search is
 *             exponential): Edmonds' blossom algorithm here; the GPU keeps a maximum matching per tree node and repairs it
 *             after the one edge an action toggles (at most one augmenting-path search: a toggle moves the matching number
 *             by at most one), so both sides hold the same NUMBER whatever matchings they hold.  (Rounds 1-2 used the rank
 *             of a Tutte matrix over GF(2^31 - 1): exact only up to a probability of N / 2^31 per evaluation, and 94 us of
 *             a 178 us expansion on the GPU.  Kept below as a cross-check.) */

constexpr int DMAXN = 64;
constexpr uint32_t TUTTE_P = 2147483647u; /* 2^31 - 1 */
constexpr uint64_t DOMAIN_TUTTE = 0x7475747465ull; /* "tutte" */

inline uint32_t tutte_mul(uint32_t a, uint32_t b) {
    uint64_t x = (uint64_t)a * (uint64_t)b;
    uint64_t t = (x & TUTTE_P) + (x >> 31);
    t = (t & TUTTE_P) + (t >> 31);
    return (uint32_t)(t >= TUTTE_P ? t - TUTTE_P : t);
}
inline uint32_t tutte_sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + TUTTE_P - b; }
inline uint32_t tutte_neg(uint32_t a) { return a ? TUTTE_P - a : 0u; }
inline uint32_t tutte_inv(uint32_t a) { /* a^(P - 2) */
    uint32_t r = 1, b = a;
    uint32_t e = TUTTE_P - 2u;
    for (int i = 0; i < 31; ++i) {
        if ((e >> i) & 1u) r = tutte_mul(r, b);
        b = tutte_mul(b, b);
    }
    return r;
}
inline uint32_t tutte_entry(int e) { return 1u + (uint32_t)(key4(DOMAIN_TUTTE, (uint64_t)e, 0, 0) % (uint64_t)(TUTTE_P - 1u)); }

inline bool dense_has_edge(const uint64_t *adj, int v, int u) { return (adj[v] >> u) & 1ull; }

/* matching number = rank(Tutte) / 2, skew-symmetric elimination on the upper triangle T(a, b), a < b, stored at the
 * colex position of the edge {a, b}; M(a, b) = T(a, b) for a < b, -T(b, a) for a > b.  Eliminating the pivot pair (i, j),
 * p = M(i, j):  M'(a, b) = M(a, b) + (M(a, i) M(j, b) - M(a, j) M(i, b)) / p. */
int dense_matching_tutte(const uint64_t *adj, int n) {
    const int E = n * (n - 1) / 2;
    std::vector<uint32_t> T((size_t)E, 0u);
    for (int v = 1; v < n; ++v)
        for (int u = 0; u < v; ++u)
            if (dense_has_edge(adj, v, u)) T[(size_t)colex_position(v, u)] = tutte_entry(colex_position(v, u));
    auto M = [&](int a, int b) -> uint32_t { /* a != b */
        return a < b ? T[(size_t)colex_position(b, a)] : tutte_neg(T[(size_t)colex_position(a, b)]);
    };
    uint64_t alive = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    int pairs = 0;
    while (alive) {
        const int i = __builtin_ctzll(alive);
        int j = -1;
        for (int c = 0; c < n; ++c)
            if (c != i && ((alive >> c) & 1ull) && M(i, c) != 0u) {
                j = c;
                break;
            }
        if (j < 0) {
            alive &= ~(1ull << i);
            continue;
        }
        const uint32_t inv = tutte_inv(M(i, j));
        const uint64_t rest = alive & ~(1ull << i) & ~(1ull << j);
        for (int b = 1; b < n; ++b) {
            if (!((rest >> b) & 1ull)) continue;
            for (int a = 0; a < b; ++a) {
                if (!((rest >> a) & 1ull)) continue;
                const uint32_t t = tutte_sub(tutte_mul(M(a, i), M(j, b)), tutte_mul(M(a, j), M(i, b)));
                uint32_t &dst = T[(size_t)colex_position(b, a)];
                const uint32_t add = tutte_mul(t, inv);
                uint32_t s = dst + add; /* < 2^32 */
                dst = s >= TUTTE_P ? s - TUTTE_P : s;
            }
        }
        alive = rest;
        pairs += 1;
    }
    return pairs;
}

/* matching number, exactly: Edmonds' blossom algorithm (one augmenting-path search per free vertex over the greedy start;
 * a vertex whose search fails stays free for good -- Berge) */
int dense_matching_exact(const uint64_t *adj, int n) {
    int mate[DMAXN], p[DMAXN], base[DMAXN];
    for (int v = 0; v < n; ++v) mate[v] = -1;
    for (int v = 0; v < n; ++v) /* greedy start */
        if (mate[v] < 0)
            for (uint64_t nb = adj[v]; nb; nb &= nb - 1) {
                const int u = __builtin_ctzll(nb);
                if (mate[u] < 0) {
                    mate[v] = u;
                    mate[u] = v;
                    break;
                }
            }
    auto lca = [&](int a, int b) {
        uint64_t mark = 0;
        for (;;) {
            a = base[a];
            mark |= 1ull << a;
            if (mate[a] < 0) break;
            a = p[mate[a]];
        }
        for (;;) {
            b = base[b];
            if ((mark >> b) & 1ull) return b;
            b = p[mate[b]];
        }
    };
    for (int root = 0; root < n; ++root) {
        if (mate[root] >= 0) continue;
        for (int v = 0; v < n; ++v) {
            p[v] = -1;
            base[v] = v;
        }
        uint64_t used = 1ull << root;
        std::vector<int> q{root};
        int found = -1;
        for (size_t qh = 0; qh < q.size() && found < 0; ++qh) {
            const int v = q[qh];
            for (uint64_t nb = adj[v]; nb && found < 0; nb &= nb - 1) {
                const int to = __builtin_ctzll(nb);
                if (base[v] == base[to] || mate[v] == to) continue;
                if (to == root || (mate[to] >= 0 && p[mate[to]] >= 0)) { /* an even vertex: a blossom */
                    const int cur = lca(v, to);
                    uint64_t blossom = 0;
                    auto mark_path = [&](int x, int child) {
                        while (base[x] != cur) {
                            blossom |= 1ull << base[x];
                            blossom |= 1ull << base[mate[x]];
                            p[x] = child;
                            child = mate[x];
                            x = p[mate[x]];
                        }
                    };
                    mark_path(v, to);
                    mark_path(to, v);
                    for (int i = 0; i < n; ++i)
                        if ((blossom >> base[i]) & 1ull) {
                            base[i] = cur;
                            if (!((used >> i) & 1ull)) {
                                used |= 1ull << i;
                                q.push_back(i);
                            }
                        }
                } else if (p[to] < 0) {
                    p[to] = v;
                    if (mate[to] < 0) found = to;
                    else {
                        used |= 1ull << mate[to];
                        q.push_back(mate[to]);
                    }
                }
            }
        }
        for (int x = found; x >= 0;) { /* flip the path */
            const int pv = p[x], ppv = mate[pv];
            mate[x] = pv;
            mate[pv] = x;
            x = ppv;
        }
    }
    int m = 0;
    for (int v = 0; v < n; ++v) m += mate[v] >= 0 ? 1 : 0;
    return m / 2;
}

/* connected_bitset_graph/mod.rs:235-317 maximum_matching, literally (DFS branch and bound over a stack of partial
 * matchings; exponential: validation on small graphs and the reference's own test vectors only) */
int dense_matching_reference(const uint64_t *adj, int n, std::vector<std::pair<int, int>> *out = nullptr) {
    struct Search {
        std::vector<std::pair<int, int>> edges;
        uint64_t unvisited;
    };
    if (n == 0) return 0;
    std::vector<Search> queue;
    queue.push_back({{}, n >= 64 ? ~0ull : ((1ull << n) - 1ull)});
    size_t matching_number = 0;
    std::vector<std::pair<int, int>> best;
    while (!queue.empty()) {
        Search m = std::move(queue.back());
        queue.pop_back();
        uint64_t unvisited = m.unvisited;
        int max_future = __builtin_popcountll(unvisited) / 2;
        if (m.edges.size() + (size_t)max_future <= matching_number) continue;
        const int next_v = 63 - __builtin_clzll(unvisited); /* max_unchecked */
        unvisited &= ~(1ull << next_v);
        max_future = __builtin_popcountll(unvisited) / 2;
        if (m.edges.size() + (size_t)max_future > matching_number) queue.push_back({m.edges, unvisited});
        uint64_t nb = unvisited & adj[next_v];
        while (nb) { /* iter(): ascending */
            const int next_u = __builtin_ctzll(nb);
            nb &= nb - 1;
            std::vector<std::pair<int, int>> ne = m.edges;
            ne.push_back({next_v, next_u});
            const uint64_t nun = unvisited & ~(1ull << next_u);
            if (ne.size() > matching_number) {
                matching_number = ne.size();
                best = ne;
            }
            if (ne.size() + (size_t)(__builtin_popcountll(nun) / 2) > matching_number) queue.push_back({std::move(ne), nun});
        }
    }
    if (out) *out = best;
    return (int)matching_number;
}

/* connected_bitset_graph/mod.rs:47-71 is_cut_edge, literally */
bool dense_is_cut_edge(const uint64_t *adj, int v, int u) {
    uint64_t new_vertices = adj[v] ^ (1ull << u); /* add_or_remove_unchecked(u): the edge is present, so this removes u */
    uint64_t explored = 1ull << v;
    while (new_vertices) {
        if ((new_vertices >> u) & 1ull) return false;
        explored |= new_vertices;
        uint64_t recent = new_vertices;
        new_vertices = 0;
        while (recent) {
            const int w = __builtin_ctzll(recent);
            recent &= recent - 1;
            new_vertices |= adj[w];
        }
        new_vertices &= ~explored;
    }
    return true;
}
bool dense_is_connected(const uint64_t *adj, int n) {
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

/* lambda_1: see the header of this file.  Every operation one IEEE f64 operation (-ffp-contract=off). */
constexpr int DENSE_LAMBDA_ITERS = 2000;
constexpr double DENSE_LAMBDA_BRACKET = 1e-4;
inline double dense_tree_sum64(const double *v) { /* balanced binary tree over 64 slots: ((v0 + v1) + (v2 + v3)) + ... */
    double t[64];
    for (int i = 0; i < 64; ++i) t[i] = v[i];
    for (int w = 1; w < 64; w <<= 1)
        for (int i = 0; i < 64; i += 2 * w) t[i] = t[i] + t[i + w];
    return t[0];
}
/* steps: where given, the number of steps x <- B x the iteration took (a multiple of 4; DENSE_LAMBDA_ITERS: the cap ended it) */
double dense_lambda1(const uint64_t *adj, int n, int *steps = nullptr) {
    double x[DMAXN], y[DMAXN];
    for (int v = 0; v < n; ++v) x[v] = 1.0;
    auto step = [&]() { /* y = (A + I) x, neighbours in ascending order */
        for (int v = 0; v < n; ++v) {
            double s = x[v];
            uint64_t nb = adj[v];
            while (nb) {
                const int u = __builtin_ctzll(nb);
                nb &= nb - 1;
                s = s + x[u];
            }
            y[v] = s;
        }
    };
    /* three plain steps, then one with the Collatz-Wielandt ratios, the exit test and the scaling back to maximum 1 */
    for (int it = 0;; it += 4) {
        for (int k = 0; k < 3; ++k) {
            step();
            for (int v = 0; v < n; ++v) x[v] = y[v];
        }
        step();
        double mn = 0.0, mx = 0.0, ymax = 0.0;
        for (int v = 0; v < n; ++v) {
            const double r = y[v] / x[v];
            if (v == 0 || r < mn) mn = r;
            if (v == 0 || r > mx) mx = r;
            if (v == 0 || y[v] > ymax) ymax = y[v];
        }
        if (mx - mn <= DENSE_LAMBDA_BRACKET || it + 4 >= DENSE_LAMBDA_ITERS) {
            if (steps) *steps = it + 4;
            break;
        }
        for (int v = 0; v < n; ++v) x[v] = y[v] / ymax;
    }
    double xy[64], xx[64];
    for (int v = 0; v < 64; ++v) {
        xy[v] = v < n ? x[v] * y[v] : 0.0;
        xx[v] = v < n ? x[v] * x[v] : 0.0;
    }
    const double q = dense_tree_sum64(xy) / dense_tree_sum64(xx);
    return q - 1.0;
}
