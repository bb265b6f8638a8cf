// space_dense.inc -- the dense-graph space on the device (included inside namespace azd after tree_core.inc).
//
// BASELINE.json configs[4] names an "N = 50 dense-graph StateActionSpace".  The reference holds the material for one
// (ConnectedBitsetGraph: is_cut_edge / action_kinds / maximum_matching / conjecture_2_1_cost,
// graph-state/src/simple_graph/connected_bitset_graph/mod.rs:45-71,139-158,226-338; AddOrDeleteEdge indexing,
// bitset_graph/space/action.rs:4-27; STATE = E + ACTION + 1, examples/05-ah.rs:39-40) but NO live NablaStateActionSpace
// over general graphs.  The space is BUILD-DEFINED from those pieces in the image of the c21 space; its definition and
// the procedures that stand in for faer's eigenvalues and the exponential matching search are spelled out in
// oracle/dense_graph.inc, which this file mirrors operation for operation (integer work exactly; the f64 power iteration
// one IEEE operation at a time, -ffp-contract=off).  The COST is a policy of the space (DenseCostC21 below: lambda_1 + matching
// number, the default and what every comment up to the policy speaks of; DenseCostAH, dense_ah_cost.inc: the objective 05-ah.rs
// searches with).
//
// State of one agent:
//   adj[v]   u64   neighbourhood bitsets of the connected graph, N <= 64                         static LDS
//   aid[r]   u16   action id of the root's r-th modifiable slot, ascending action id, r < 64 KW   static LDS
//   rem      KW words  ranks whose slot has not been modified yet                                 registers
// A node holds at most 64 KW legal actions (the root's modifiable slots; KW = 2, 4, 10 or 16 chosen by the engine from
// azd_engine_config::max_slots: up to E / 2 = 612 slots at N = 50 need KW = 10).  With KW = 2 the two-chunk selection code of
// tree_core.inc runs unchanged, beyond that its chunk-by-chunk form (select_big).  Transposition keys are the 64 KW-bit set of
// MODIFIED RANKS (= the ActionSet of the path, re-indexed: ranks ascend with the action ids, so the keys order as the
// action-id sets do), which is why SP::key_bit / SP::bit_action exist.  The host converts keys back to action-id sets on export.

constexpr int DENSE_MAX_N = 64;

template <int KW_>
struct DenseLds {
    uint64_t adj[DENSE_MAX_N];
    double x[DENSE_MAX_N];           // power-iteration vector
    uint64_t slotmask[32];           // write_vec / argmin_out: remaining slots as a bitmap over colex positions (E <= 2016)
    uint16_t aid[64 * KW_];          // rank -> action id
    uint8_t mate[DENSE_MAX_N];       // a maximum matching of the graph in `adj` when a node's cost is computed (0xFF: unmatched)
    unsigned long long ctr[NUM_COUNTERS];
    uint16_t seq[4];                 // unused (Layered<L, _> is not built for this space); tree_core.inc names it
    uint32_t stack[PATH_STACK];     // nodes of the current path, root first (tree_core.inc: cascade)
};

__device__ __forceinline__ void dense_from_colex(const int pos, int &mx, int &mn) { // edge.rs:55-65
    int v = (int)((sqrtf(8.0f * (float)pos + 1.0f) + 1.0f) * 0.5f);
    while (v * (v - 1) / 2 > pos) --v;
    while (v * (v + 1) / 2 <= pos) ++v;
    mx = v;
    mn = pos - v * (v - 1) / 2;
}
__device__ __forceinline__ int dense_colex(const int mx, const int mn) { return mx * (mx - 1) / 2 + mn; }

// connected_bitset_graph/mod.rs:47-71 is_cut_edge for the present edge {v, u}; one lane, the graph in LDS
template <class L>
__device__ __forceinline__ bool dense_is_cut_edge(const L &s, const int v, const int u) {
    uint64_t nw = s.adj[v] ^ (1ull << u);
    uint64_t explored = 1ull << v;
    while (nw) {
        if ((nw >> u) & 1ull) return false;
        explored |= nw;
        uint64_t recent = nw;
        nw = 0;
        while (recent) {
            const int w = __ffsll((unsigned long long)recent) - 1;
            recent &= recent - 1;
            nw |= s.adj[w];
        }
        nw &= ~explored;
    }
    return true;
}

// lambda_1: power iteration on B = A + I (oracle/dense_graph.inc dense_lambda1, the same operations in the same order).  Three
// plain steps x <- B x, then one whose Collatz-Wielandt ratios (B x)_v / x_v bracket lambda_1 + 1 and decide whether to stop
// (bracket <= 1e-4, or the step cap), x scaled back to maximum 1 otherwise.  The value is the Rayleigh quotient of the last
// pair, (x . y) / (x . x) - 1: its error is of the order of the bracket squared over the spectral gap, so the iteration stops
// after half the steps the bracket itself would need to reach 1e-7.  That figure holds only where the bracket closed: a run the
// step cap ends (near-trees at N = 64 whose two largest eigenvalues are within a few 1e-3) has no such bound -- 3.2e-5 measured
// (DESIGN.md "The dense cost at the step cap"; tests/test_dense_cost_cases.py).  The dot products are xor-butterflies over the wave = the
// oracle's balanced binary tree over 64 slots, operand order included (a + b == b + a bit for bit).
constexpr int DENSE_LAMBDA_ITERS = 2000;
constexpr double DENSE_LAMBDA_BRACKET = 1e-4;
__device__ __forceinline__ double dense_tree_sum(double v) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) v = v + __shfl_xor(v, w, 64);
    return v;
}
struct DenseNoHook {
    __device__ __forceinline__ void operator()() const {}
};
// hook: called once, after DENSE_LAMBDA_HOOK_AT steps or when the iteration ends, whichever comes first (the pool step's deferred
// post: tree_core.inc, new node)
constexpr int DENSE_LAMBDA_HOOK_AT = 8;
template <class L, class Hook>
__device__ __forceinline__ double dense_lambda1_wave(L &s, const int n, Hook &&hook) {
    const int v = LANE;
    const bool in = v < n;
    if (in) s.x[v] = 1.0;
    const uint64_t nb0 = in ? s.adj[v] : 0ull;
    auto step = [&]() __attribute__((always_inline)) -> double { // (B x)_v from the x in LDS
        // The sum runs over the neighbours in ascending order, one dependent f64 add each; the LDS reads behind the adds are
        // requested four neighbours at a time, so that their latencies overlap (a slot without a neighbour adds 0.0, which
        // leaves a positive sum as it is, bit for bit).
        double sum = 1.0;
        if (in) {
            sum = s.x[v];
            uint64_t nb = nb0;
            while (nb) {
                int u[4];
                bool has[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    has[q] = nb != 0ull;
                    u[q] = has[q] ? __ffsll((unsigned long long)nb) - 1 : v;
                    nb &= nb - 1ull; // (0 stays 0)
                }
                double xq[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) xq[q] = s.x[u[q]];
#pragma unroll
                for (int q = 0; q < 4; ++q) sum = sum + (has[q] ? xq[q] : 0.0);
            }
        }
        return sum;
    };
    double xv = 1.0, y = 1.0;
    bool hooked = false;
    for (int it = 0;; it += 4) {
#pragma unroll 1
        for (int k = 0; k < 3; ++k) {
            LDS_SYNC();
            const double yk = step();
            LDS_SYNC();
            if (in) s.x[v] = yk;
        }
        LDS_SYNC();
        xv = in ? s.x[v] : 1.0;
        y = step();
        const double r = in ? y / xv : 1.0;
        // all values are positive: the bit patterns order like the numbers
        const uint64_t rb = (uint64_t)__double_as_longlong(r), yb = (uint64_t)__double_as_longlong(y);
        const double lo = __longlong_as_double((long long)wave_min_u64(in ? rb : ~0ull));
        const double hi = __longlong_as_double((long long)wave_max_u64(in ? rb : 0ull));
        if (hi - lo <= DENSE_LAMBDA_BRACKET || it + 4 >= DENSE_LAMBDA_ITERS) break;
        if (it + 4 == DENSE_LAMBDA_HOOK_AT) {
            hook();
            hooked = true;
        }
        const double ymax = __longlong_as_double((long long)wave_max_u64(in ? yb : 0ull));
        LDS_SYNC();
        if (in) s.x[v] = y / ymax;
    }
    if (!hooked) hook();
    LDS_SYNC();
    const double xy = dense_tree_sum(in ? xv * y : 0.0), xx = dense_tree_sum(in ? xv * xv : 0.0);
    const double q = xy / xx;
    return q - 1.0;
}

// ---------------------------------------------------------------- matching number, exactly (Edmonds' blossom algorithm)
// The cost needs the matching NUMBER (connected_bitset_graph/mod.rs:235-317 maximum_matching().len()); the oracle computes it
// from scratch per node (dense_matching_exact).  Here every tree node keeps a maximum matching of its graph (Arenas::node_mate,
// 64 bytes), and a new node repairs its parent's after the one edge its action toggles:
//   Add(u, v)     both unmatched: match them; else an augmenting path must pass the new edge -- one search from u if u is
//                 unmatched (or v), else from every unmatched vertex until one succeeds (none with fewer than two of them)
//   Delete(u, v)  not in the matching: nothing; else unmatch u and v, search from u, then from v
// One single-root search (the classical BFS with blossom contraction; see the oracle for the plain form): lane i holds
// mate[i], p[i], base[i] in registers, the vertex sets (used, queue, blossom) are 64-bit scalars, a vertex is read with
// v_readlane.  All unvisited neighbours of the scanned vertex are taken in one step (their assignments are independent:
// each brings its own mate); only even neighbours (blossoms) are handled one at a time.
constexpr uint32_t DM_NONE = 0xFFu;
#define DM_RL(V, I) ((uint32_t)__builtin_amdgcn_readlane((int)(V), (int)(I)))
template <class L>
__device__ bool dense_augment_from(const L &s, const int n, const int r, uint32_t &mate_i) {
    const int i = LANE;
    uint32_t p_i = DM_NONE, base_i = (uint32_t)i;
    uint64_t used = 1ull << r, Q = 1ull << r;
    while (Q) {
        const int v = __ffsll((unsigned long long)Q) - 1;
        Q &= Q - 1ull;
        const uint32_t base_v = DM_RL(base_i, v), mate_v = DM_RL(mate_i, v);
        const uint64_t nbv = s.adj[v];
        const bool diff = i < n && ((nbv >> i) & 1ull) && base_i != base_v && (uint32_t)i != mate_v;
        // `to` is even (outer) iff it is the root or its mate has a parent
        const uint32_t p_of_mate = (uint32_t)__shfl((int)p_i, (int)(mate_i & 63u), 64);
        const bool even_to = i == r || (mate_i != DM_NONE && p_of_mate != DM_NONE);
        const bool fresh = diff && !even_to && p_i == DM_NONE;
        const uint64_t fresh_m = __ballot(fresh);
        if (fresh) p_i = (uint32_t)v;
        const uint64_t free_m = __ballot(fresh && mate_i == DM_NONE);
        if (free_m) { // an unmatched vertex: flip the path that ends there
            uint32_t x = (uint32_t)(__ffsll((unsigned long long)free_m) - 1);
            while (x != DM_NONE) {
                const uint32_t pv = DM_RL(p_i, x), ppv = DM_RL(mate_i, pv);
                if ((uint32_t)i == x) mate_i = pv;
                if ((uint32_t)i == pv) mate_i = x;
                x = ppv;
            }
            return true;
        }
        {   // the mates of the fresh vertices become even
            const uint64_t nw = __ballot(mate_i != DM_NONE && ((fresh_m >> (mate_i & 63u)) & 1ull)) & ~used;
            used |= nw;
            Q |= nw;
        }
        uint64_t ev_m = __ballot(diff && even_to);
        while (ev_m) { // an even neighbour with another base: a blossom
            const int to = __ffsll((unsigned long long)ev_m) - 1;
            ev_m &= ev_m - 1ull;
            if (DM_RL(base_i, v) == DM_RL(base_i, to)) continue; // contracted together meanwhile
            uint64_t mark = 0;
            uint32_t a = (uint32_t)v;
            for (;;) { // lowest common ancestor of the two bases
                a = DM_RL(base_i, a);
                mark |= 1ull << a;
                const uint32_t ma = DM_RL(mate_i, a);
                if (ma == DM_NONE) break;
                a = DM_RL(p_i, ma);
            }
            uint32_t b = (uint32_t)to;
            for (;;) {
                b = DM_RL(base_i, b);
                if ((mark >> b) & 1ull) break;
                b = DM_RL(p_i, DM_RL(mate_i, b));
            }
            const uint32_t cur = b;
            uint64_t blossom = 0;
#pragma unroll 1
            for (int side = 0; side < 2; ++side) { // mark_path(v, cur, to); mark_path(to, cur, v)
                uint32_t x = side ? (uint32_t)to : (uint32_t)v, child = side ? (uint32_t)v : (uint32_t)to;
                while (DM_RL(base_i, x) != cur) {
                    const uint32_t mx_ = DM_RL(mate_i, x);
                    blossom |= 1ull << DM_RL(base_i, x);
                    blossom |= 1ull << DM_RL(base_i, mx_);
                    if ((uint32_t)i == x) p_i = child;
                    child = mx_;
                    x = DM_RL(p_i, mx_);
                }
            }
            const bool inb = i < n && ((blossom >> (base_i & 63u)) & 1ull);
            if (inb) base_i = cur;
            const uint64_t nw = __ballot(inb) & ~used;
            used |= nw;
            Q |= nw;
        }
    }
    return false;
}
// a maximum matching of s.adj from nothing (roots, the argmin's replay): greedy, then one search per vertex still unmatched
// (a vertex whose search fails stays unmatched for good); returns the matching number, the matching in s.mate
template <class L>
__device__ int dense_matching_scratch(L &s, const int n) {
    const int i = LANE;
    uint32_t mate_i = DM_NONE;
    uint64_t free_m = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    for (int v = 0; v < n; ++v) { // the oracle's greedy start (any maximal start gives the same NUMBER)
        if (!((free_m >> v) & 1ull)) continue;
        const uint64_t cand = s.adj[v] & free_m;
        if (!cand) continue;
        const int u = __ffsll((unsigned long long)cand) - 1;
        if (i == v) mate_i = (uint32_t)u;
        if (i == u) mate_i = (uint32_t)v;
        free_m &= ~((1ull << v) | (1ull << u));
    }
    for (uint64_t todo = free_m; todo; todo &= todo - 1ull) {
        const int r = __ffsll((unsigned long long)todo) - 1;
        if (DM_RL(mate_i, r) != DM_NONE) continue; // matched as the far end of an earlier path
        dense_augment_from(s, n, r, mate_i);
    }
    s.mate[i] = (uint8_t)mate_i;
    return __popcll(__ballot(i < n && mate_i != DM_NONE)) >> 1;
}
// ... and after the action that toggled the edge {mx, mn} of the graph whose maximum matching is in s.mate (s.adj holds the
// graph AFTER the toggle)
template <class L>
__device__ __forceinline__ int dense_matching_update(L &s, const int n, const int mx, const int mn) {
    const int i = LANE;
    uint32_t mate_i = s.mate[i];
    const bool present = (s.adj[mx] >> mn) & 1ull; // added
    const uint32_t m_mx = DM_RL(mate_i, mx), m_mn = DM_RL(mate_i, mn);
    if (present) {
        if (m_mx == DM_NONE && m_mn == DM_NONE) {
            if (i == mx) mate_i = (uint32_t)mn;
            if (i == mn) mate_i = (uint32_t)mx;
        } else if (m_mx == DM_NONE) dense_augment_from(s, n, mx, mate_i);
        else if (m_mn == DM_NONE) dense_augment_from(s, n, mn, mate_i);
        else {
            const uint64_t free_m = __ballot(i < n && mate_i == DM_NONE);
            if (__popcll(free_m) >= 2)
                for (uint64_t todo = free_m; todo; todo &= todo - 1ull)
                    if (dense_augment_from(s, n, __ffsll((unsigned long long)todo) - 1, mate_i)) break;
        }
    } else if (m_mx == (uint32_t)mn) { // the deleted edge was in the matching
        if (i == mx || i == mn) mate_i = DM_NONE;
        if (!dense_augment_from(s, n, mx, mate_i)) dense_augment_from(s, n, mn, mate_i);
    }
    s.mate[i] = (uint8_t)mate_i;
    return __popcll(__ballot(i < n && mate_i != DM_NONE)) >> 1;
}

__device__ __forceinline__ float c21_eval_dense(float slope, double lambda1, int mu) {
    const float c = (float)mu + (float)lambda1;
    const float x = c - 2.0f;
    return slope * x;
}
// ---------------------------------------------------------------- the cost of a DenseSpace: a policy
// What a dense engine minimises enters the space as a class: its part of the wave's LDS block and of the register state, what a
// new node computes (and keeps per node), what an agent keeps between launches, and the argmin record.  DenseCostC21 is
// conjecture_2_1_cost (mod.rs:319-338: lambda_1 + matching number) through the procedures above, the default; DenseCostAH
// (dense_ah_cost.inc, built in dense_ah_kernels.hip) is the Aouchiche-Hansen cost.
struct DenseCostC21 {
    template <int KW_>
    using Lds = DenseLds<KW_>;
    template <int KW_>
    struct St {
        uint64_t rem[KW_];
        double lambda;
        int mu;
        uint32_t last_aid; // the action that leads to the node being created (new_node_begin): its edge is what the matching repairs
        uint32_t mate_of;  // ... and the node whose matching is repaired (the parent)
    };
    struct Replay { // the argmin's recomputed cost
        double lam;
        int mu;
        float ev;
    };
    // tree_core.inc, new node: the parent's maximum matching (one 64-byte row of an arena of gigabytes) is requested by
    // evaluate() -- after the state row has left (a load ahead of the row's stores would be waited for with them: the counter is
    // in order) -- and stays in flight while lambda_1 iterates; the new node's goes out once the node has its index.
    template <class S>
    __device__ static __forceinline__ void new_node_begin(S &st, const uint32_t parent, const uint32_t aid) {
        st.last_aid = aid;
        st.mate_of = parent;
    }
    template <class L>
    __device__ static __forceinline__ void new_node_end(const Arenas &a, const int t, L &s, const uint32_t node) {
        a.node_mate[((size_t)t * a.node_cap + node) * DENSE_MAX_N + LANE] = s.mate[LANE];
    }
    template <class S>
    __device__ static __forceinline__ void load_cost(const Arenas &a, const int t, S &st) {
        st.lambda = a.cur_lambda[t];
        st.mu = a.cur_mu[t];
    }
    template <class S>
    __device__ static __forceinline__ void store_cost(const Arenas &a, const int t, const S &st) { // (one lane)
        a.cur_lambda[t] = st.lambda;
        a.cur_mu[t] = st.mu;
    }
    template <class L, class S, class Hook>
    __device__ static __forceinline__ float evaluate(const Arenas &a, L &s, S &st, const int t, Hook &&hook) {
        const unsigned long long ph_l0 = PH_NOW();
        const uint8_t parent_mate = a.node_mate[((size_t)t * a.node_cap + st.mate_of) * DENSE_MAX_N + LANE];
        st.lambda = dense_lambda1_wave(s, a.n, hook);
        const unsigned long long ph_l1 = PH_NOW();
        {   // the parent's matching (new_node_begin) after the toggle of this action's edge
            int mx, mn;
            dense_from_colex((int)(st.last_aid % (uint32_t)a.E), mx, mn);
            s.mate[LANE] = parent_mate;
            LDS_SYNC();
            st.mu = dense_matching_update(s, a.n, mx, mn);
        }
        CTR_ADD(22, ph_l1 - ph_l0);
        CTR_ADD(23, PH_NOW() - ph_l1);
        return c21_eval_dense(a.eval_slope, st.lambda, st.mu);
    }
    // the cost of a root from nothing (the graph is in s.adj): the agent's record, the root node's matching
    template <class L, class S>
    __device__ static __forceinline__ float root_cost(const Arenas &a, const int t, L &s, S &st) {
        const int n = a.n;
        st.lambda = dense_lambda1_wave(s, n, DenseNoHook{});
        st.mu = dense_matching_scratch(s, n);
        st.last_aid = 0;
        a.node_mate[((size_t)t * a.node_cap) * DENSE_MAX_N + LANE] = s.mate[LANE]; // the root node's matching
        if (LANE == 0) {
            a.cur_lambda[t] = st.lambda;
            a.cur_mu[t] = st.mu;
        }
        return c21_eval_dense(a.eval_slope, st.lambda, st.mu);
    }
    template <class L>
    __device__ static __forceinline__ void argmin_cost(const Arenas &a, L &s, Replay &r) {
        r.lam = dense_lambda1_wave(s, a.n, DenseNoHook{});
        r.mu = dense_matching_scratch(s, a.n);
        r.ev = c21_eval_dense(a.eval_slope, r.lam, r.mu);
    }
    // ArgminData { state, cost, eval } (log.rs:1-11); s.slotmask holds the open slots
    template <class L>
    __device__ static __forceinline__ void argmin_write(const Arenas &a, L &s, const Replay &r, const int wt, const uint32_t win_node) {
        DenseArgminRec *out = a.argmin_d;
        out->adj[LANE] = LANE < a.n ? s.adj[LANE] : 0ull;
        if (LANE < 40) out->permitted[LANE] = LANE < 32 ? s.slotmask[LANE] : 0ull;
        if (LANE == 0) {
            out->lambda_1 = r.lam;
            out->matching_size = r.mu;
            out->eval = r.ev;
            out->agent = wt;
            out->node = win_node;
        }
    }
};

// (the contract: tree_core.inc, SpaceDefaults.  No tables to prepare, no LDS copy of the root -- it is as large as the live state --
// and the observation map h_sa = c_as*, 04-c21-tree.rs:104: the defaults)
template <int KW_, class Cost = DenseCostC21>
struct DenseSpace : SpaceDefaults {
    static constexpr int KW = KW_; // words of a rank set: the root's modifiable slots, at most 64 KW
    static constexpr int CH = KW_; // chunks of 64 predictions a node may hold
    static constexpr int MAX_SLOTS = 64 * KW_;
    using Lds = typename Cost::template Lds<KW_>;
    using St = typename Cost::template St<KW_>;
    static size_t dyn_bytes(const Arenas &) {
        const size_t t = (size_t)512 * KW_; // select_big's two lists of 64 KW words
        return t > CORE_DYN_BYTES ? t : CORE_DYN_BYTES;
    }
    // tree_core.inc, new node: what the cost keeps per node (DenseCostC21: the parent's maximum matching)
    __device__ static __forceinline__ void new_node_begin(const Arenas &, const int, Lds &, St &st, const uint32_t parent, const uint32_t aid) {
        Cost::new_node_begin(st, parent, aid);
    }
    __device__ static __forceinline__ void new_node_end(const Arenas &a, const int t, Lds &s, const St &, const uint32_t node) {
        Cost::new_node_end(a, t, s, node);
    }
    __device__ static __forceinline__ float *row_stage(const Arenas &, const uint32_t) { return nullptr; } // pool step: not built for this space
    __device__ static __forceinline__ void load_tables(const Arenas &a, const int t, Lds &s) {
#pragma unroll
        for (int w = 0; w < KW; ++w) s.aid[64 * w + LANE] = a.root_aid[(size_t)t * MAX_SLOTS + 64 * w + LANE];
    }
    __device__ static __forceinline__ void load_cur(const Arenas &a, const int t, Lds &s, const uint32_t, St &st) {
        s.adj[LANE] = a.cur_adj[(size_t)t * DENSE_MAX_N + LANE];
        load_tables(a, t, s);
#pragma unroll
        for (int w = 0; w < KW; ++w) st.rem[w] = a.cur_perm[(size_t)t * KW + w];
        Cost::load_cost(a, t, st);
    }
    __device__ static __forceinline__ void load_root(const Arenas &a, const int t, Lds &s, const uint32_t, St &st) {
        s.adj[LANE] = a.root_adj[(size_t)t * DENSE_MAX_N + LANE];
        load_tables(a, t, s);
#pragma unroll
        for (int w = 0; w < KW; ++w) st.rem[w] = a.root_perm[(size_t)t * KW + w];
    }
    __device__ static __forceinline__ void load_root_cached(const Arenas &a, const int t, Lds &s, const uint32_t dyn, St &st) { load_root(a, t, s, dyn, st); }
    __device__ static __forceinline__ void store_cur(const Arenas &a, const int t, Lds &s, const uint32_t, const St &st) {
        a.cur_adj[(size_t)t * DENSE_MAX_N + LANE] = s.adj[LANE];
        if (LANE == 0) {
#pragma unroll
            for (int w = 0; w < KW; ++w) a.cur_perm[(size_t)t * KW + w] = st.rem[w];
            Cost::store_cost(a, t, st);
        }
    }
    // the ActionSet key of a path is kept over the RANKS of the root's modifiable slots
    __device__ static __forceinline__ uint32_t key_bit(const Lds &s, const uint32_t aid) {
        uint32_t r = 0;
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const uint64_t m = __ballot(s.aid[64 * w + LANE] == (uint16_t)aid);
            if (m) r = 64u * (uint32_t)w + (uint32_t)first_lane(m);
        }
        return r;
    }
    __device__ static __forceinline__ uint32_t bit_action(const Lds &s, const uint32_t bit) { return s.aid[bit]; }
    // AddOrDeleteEdge::from_action_index (action.rs:20-27) + add_or_remove_edge_unchecked; the slot is used up
    __device__ static __forceinline__ void act(const Arenas &a, Lds &s, const uint32_t, St &st, const uint32_t aid) {
        const uint32_t r = key_bit(s, aid);
        int mx, mn;
        dense_from_colex((int)(aid % (uint32_t)a.E), mx, mn);
        if (LANE == 0) {
            s.adj[mx] ^= 1ull << mn;
            s.adj[mn] ^= 1ull << mx;
        }
#pragma unroll
        for (int w = 0; w < KW; ++w)
            if ((int)(r >> 6) == w) st.rem[w] &= ~(1ull << (r & 63u));
        WAVE_SYNC();
    }
    // the policy's cost of the state just acted into, squished (DenseCostC21: conjecture_2_1_cost, mod.rs:319-338, and the squish of
    // 04-c21-tree.rs:58-74 with N's bounds)
    static constexpr bool EVALUATE_TAKES_HOOK = true; // hook() = the row's drain and the request's post
    __device__ static __forceinline__ float evaluate(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const int t) {
        return evaluate_hooked(a, s, dyn, st, t, DenseNoHook{});
    }
    template <class Hook>
    __device__ static __forceinline__ float evaluate_hooked(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const int t, Hook &&hook) {
        return Cost::evaluate(a, s, st, t, hook);
    }
    // action_kinds (mod.rs:139-158) over the remaining ranks: bit r of legal[r >> 6]
    __device__ static __forceinline__ void legal_ranks(const Arenas &a, const Lds &s, const St &st, uint64_t (&legal)[KW]) {
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            bool ok = false;
            if ((st.rem[w] >> LANE) & 1ull) {
                const uint32_t aid = s.aid[w * 64 + LANE];
                if (aid < (uint32_t)a.E) ok = true; // Add: the slot is unmodified, so the edge is still absent
                else {
                    int mx, mn;
                    dense_from_colex((int)(aid - (uint32_t)a.E), mx, mn);
                    ok = !dense_is_cut_edge(s, mx, mn); // Delete keeps the graph connected
                }
            }
            legal[w] = __ballot(ok);
        }
    }
    __device__ static __forceinline__ bool terminal(const Arenas &a, Lds &s, const uint32_t, const St &st) {
        uint64_t legal[KW];
        legal_ranks(a, s, st, legal);
        return mask_empty<KW>(legal);
    }
    // remaining slots as a bitmap over colex positions -> s.slotmask
    __device__ static __forceinline__ void open_slots(const Arenas &a, Lds &s, const St &st) {
        if (LANE < 32) s.slotmask[LANE] = 0;
        LDS_SYNC();
#pragma unroll
        for (int w = 0; w < KW; ++w)
            if ((st.rem[w] >> LANE) & 1ull) {
                const uint32_t slot = (uint32_t)s.aid[w * 64 + LANE] % (uint32_t)a.E;
                atomicOr((unsigned long long *)&s.slotmask[slot >> 6], 1ull << (slot & 63u));
            }
        LDS_SYNC();
    }
    // oracle/dense_graph.inc: [0, E) edge bools, [E, 2E) modifiable and absent, [2E, 3E) modifiable and present, [3E] remaining / E
    __device__ static void write_vec(const Arenas &a, Lds &s, const uint32_t, const St &st, float *row) {
        const int E = a.E;
        open_slots(a, s, st);
        for (int e = LANE; e < E; e += 64) {
            int mx, mn;
            dense_from_colex(e, mx, mn);
            const bool present = (s.adj[mx] >> mn) & 1ull;
            const bool open = (s.slotmask[e >> 6] >> (e & 63)) & 1ull;
            row[e] = present ? 1.0f : 0.0f;
            row[E + e] = (open && !present) ? 1.0f : 0.0f;
            row[2 * E + e] = (open && present) ? 1.0f : 0.0f;
        }
        if (LANE == 0) row[3 * E] = (float)mask_count<KW>(st.rem) / (float)E;
    }
    // the same row as bf16 (what the bf16 evaluator rounds it to on its way in): 0 / 1 are exact, the last entry RNE.  Call
    // right after write_vec: s.slotmask still holds the open slots
    __device__ static void write_vec16(const Arenas &a, Lds &s, const uint32_t, const St &st, uint16_t *row) {
        const int E = a.E;
        for (int e = LANE; e < E; e += 64) {
            int mx, mn;
            dense_from_colex(e, mx, mn);
            const bool present = (s.adj[mx] >> mn) & 1ull;
            const bool open = (s.slotmask[e >> 6] >> (e & 63)) & 1ull;
            row[e] = present ? (uint16_t)0x3F80u : (uint16_t)0;
            row[E + e] = (open && !present) ? (uint16_t)0x3F80u : (uint16_t)0;
            row[2 * E + e] = (open && present) ? (uint16_t)0x3F80u : (uint16_t)0;
        }
        if (LANE == 0) row[3 * E] = (uint16_t)bf16_bits((float)mask_count<KW>(st.rem) / (float)E);
    }
    // Pool step: the same two rows, eight entries per lane and step, as whole 16-byte write-through stores (the batched GEMM that
    // reads them runs in another kernel, on other XCDs).  S = 3E + 1 need not be a multiple of 8: the last piece runs into the
    // row's padding (the f32 row's pitch is S: its last entry is stored alone), which stays zero.
    static constexpr bool ROWS_DIRECT = true;
    __device__ static void write_rows_direct(const Arenas &a, Lds &s, const uint32_t, const St &st, float *row, uint16_t *row16) {
        const int E = a.E, S = 3 * E + 1;
        // (LDS-scope syncs only in here: a workgroup-scope release would wait for the row's own write-through stores -- the caller
        // drains them when it posts the request: tree_core.inc, new node)
        open_slots(a, s, st); // s.slotmask: the open slots as a bitmap over colex positions
        // the present edges as the same kind of bitmap: vertex v's neighbours below v sit at colex positions v (v - 1) / 2 .. + v - 1,
        // i.e. the low v bits of its adjacency word, in place (s.x is scratch outside the power iteration)
        unsigned long long *P = reinterpret_cast<unsigned long long *>(s.x);
        if (LANE < 32) P[LANE] = 0ull;
        LDS_SYNC();
        if (LANE >= 1 && LANE < a.n) {
            const unsigned long long bits = s.adj[LANE] & ((1ull << LANE) - 1ull);
            const int base = LANE * (LANE - 1) / 2, w = base >> 6, sh = base & 63;
            if (bits) {
                atomicOr(&P[w], bits << sh);
                if (sh && (bits >> (64 - sh))) atomicOr(&P[w + 1], bits >> (64 - sh));
            }
        }
        LDS_SYNC();
        const float last = (float)mask_count<KW>(st.rem) / (float)E;
        // Round 4: the searchers of this space keep their SIMDs busy (22.2 M expansions/s with 16 waves per CU, 21.9 with 14, 20.7
        // with 12: instructions, not latencies, set a call's time), and this loop was ~13 % of a new node's instructions: two LDS
        // reads and a dozen operations per ENTRY.  Now a piece's eight entries are one byte -- a funnel-shifted read of each bitmap,
        // the section's rule applied to the eight bits at once (a piece that runs over the end of its section continues with the
        // next section's first bits) -- and the byte is spread into four bf16 pairs by two multiplications each.
        // eight consecutive bits of a bitmap from position e on (words past the map's last are read as they lie -- s.x and
        // s.slotmask are followed by other members of the block -- and never used)
        auto bits8 = [](const unsigned long long *map, const int e) __attribute__((always_inline)) -> uint32_t {
            const int w = e >> 6, sh = e & 63;
            const unsigned long long lo = map[w], hi = map[w + 1];
            return (uint32_t)((sh ? (lo >> sh) | (hi << (64 - sh)) : lo) & 0xFFull);
        };
        auto rule = [](const int sec, const uint32_t pb, const uint32_t ob) __attribute__((always_inline)) -> uint32_t {
            return sec == 0 ? pb : sec == 1 ? (ob & ~pb) : (ob & pb); // present | open and absent | open and present
        };
        const unsigned long long *O = reinterpret_cast<const unsigned long long *>(s.slotmask);
        const uint32_t p_first = (uint32_t)(P[0] & 0xFFull), o_first = (uint32_t)(O[0] & 0xFFull);
        for (int i0 = 8 * LANE; i0 < S; i0 += 8 * 64) {
            const int sec0 = i0 >= 2 * E ? 2 : i0 >= E ? 1 : 0, e0 = i0 - sec0 * E; // (i0 = 3 E: sec 2, e0 = E, n_in = 0)
            const int n_in = E - e0 < 8 ? E - e0 : 8;                                // entries of this piece inside section sec0
            const int n_bits = 3 * E - i0 < 8 ? 3 * E - i0 : 8;                      // ... that are bits at all (the row's last entry is a number)
            uint32_t b = rule(sec0, bits8(P, e0), bits8(O, e0));
            if (n_in < 8) b = (b & ((1u << n_in) - 1u)) | (rule(sec0 + 1, p_first, o_first) << n_in);
            b &= (1u << n_bits) - 1u;
            // f32 row (pitch S; S = 3 E + 1 is rarely a multiple of 4: dword stores)
            if ((S & 3) == 0) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if (i0 + 4 * h < S) {
                        azd_f32x4 w;
#pragma unroll
                        for (int q = 0; q < 4; ++q) w[q] = i0 + 4 * h + q == 3 * E ? last : ((b >> (4 * h + q)) & 1u) ? 1.0f : 0.0f;
                        st_sc1_x4(row + i0 + 4 * h, w);
                    }
            } else if (i0 + 8 <= 3 * E) {
#pragma unroll
                for (int q = 0; q < 8; ++q) st_sc1_f32(row + i0 + q, __uint_as_float(((b >> q) & 1u) * 0x3F800000u));
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (i0 + q < S) st_sc1_f32(row + i0 + q, i0 + q == 3 * E ? last : ((b >> q) & 1u) ? 1.0f : 0.0f);
            }
            if (row16) { // pitch S16: a multiple of 64, so every piece is a whole aligned 16 bytes
                azd_f32x4 w;
                uint32_t h[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) h[q] = ((((b >> (2 * q)) & 3u) * 0x8001u) & 0x10001u) * 0x3F80u; // bit 2q -> low half, bit 2q + 1 -> high half
                if (i0 <= 3 * E && 3 * E < i0 + 8) { // the piece holding the row's last entry
                    const int q = 3 * E - i0;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
                        if (qq == (q >> 1)) h[qq] |= bf16_bits(last) << (16 * (q & 1));
                }
                __builtin_memcpy(&w, h, 16);
                st_sc1_x4(reinterpret_cast<float *>(row16 + i0), w);
            }
        }
        LDS_SYNC();
    }

    // graph_operations.rs:32-56 with the legal actions above and g = c_s - h (04-c21-tree.rs:103)
    template <bool SC1 = false>
    __device__ static __forceinline__ void add_actions(const Arenas &a, Lds &s, const int t, const RolloutOut *hint, RolloutOut * /*pick: pool step only*/) {
        St st;
        s.adj[LANE] = a.cur_adj[(size_t)t * DENSE_MAX_N + LANE];
        load_tables(a, t, s);
#pragma unroll
        for (int w = 0; w < KW; ++w) st.rem[w] = a.cur_perm[(size_t)t * KW + w];
        WAVE_SYNC();
        uint64_t legal[KW];
        legal_ranks(a, s, st, legal);
        const uint32_t cnt = (uint32_t)mask_count<KW>(legal);
        const uint32_t begin = hint ? hint->n_preds : a.n_preds[t];
        if (!add_actions_fits(a, t, begin, cnt, (uint32_t)MAX_SLOTS)) return;
        const uint32_t node = hint ? hint->pos : a.state_pos[t];
        PredRec *preds = a.preds + (size_t)t * a.pred_cap;
        const float c = hint ? hint->c : a.nodes[(size_t)t * a.node_cap + node].c;
        const uint2 link = node_link(a, t, node);
        const float *h = a.h_theta + (size_t)t * a.A;
        // (the row's entries of every chunk requested before any of them is used: chunk by chunk, request then store, a node of the driver's
        // slot range -- ten chunks -- was ten round trips; round 5)
        uint32_t aidv[KW];
        float hv[KW];
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            aidv[w] = s.aid[w * 64 + LANE];
            hv[w] = 0.f;
            if ((legal[w] >> LANE) & 1ull) hv[w] = SC1 ? ld_sc1_f32(h + aidv[w]) : h[aidv[w]];
        }
        uint32_t before = 0;
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            if ((legal[w] >> LANE) & 1ull) {
                const uint32_t rank = before + (uint32_t)__popcll(legal[w] & ((1ull << LANE) - 1ull));
                preds[begin + rank] = pred_new(aidv[w], c, c - hv[w]);
            }
            before += (uint32_t)__popcll(legal[w]);
        }
        add_actions_commit(a, t, node, begin, cnt, hint ? s.ctr : nullptr, link);
    }

    // The rank table of a root: its modifiable slots by ascending ACTION id -- Add(e) = e for the absent edges, then
    // Delete(e) = E + e for the present ones, each group by ascending slot -- and the mask of its k ranks.  The graph is in
    // s.adj, the slots in `slots` ((E + 63) / 64 words, global or LDS).  Returns k (> MAX_SLOTS: the table is cut off there).
    __device__ static int rank_table(const Arenas &a, Lds &s, const uint64_t *slots, uint64_t (&mask)[KW]) {
        const int E = a.E;
        for (int r = LANE; r < MAX_SLOTS; r += 64) s.aid[r] = 0xFFFFu;
        WAVE_SYNC();
        int k = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int base = 0; base < E; base += 64) {
                const int e = base + LANE;
                bool take = false;
                if (e < E && ((slots[e >> 6] >> (e & 63)) & 1ull)) {
                    int mx, mn;
                    dense_from_colex(e, mx, mn);
                    const bool present = (s.adj[mx] >> mn) & 1ull;
                    take = present == (pass == 1);
                }
                const uint64_t m = __ballot(take);
                if (take) {
                    const int r = k + __popcll(m & ((1ull << LANE) - 1ull));
                    if (r < MAX_SLOTS) s.aid[r] = (uint16_t)(pass == 0 ? e : E + e);
                }
                k += __popcll(m);
            }
        WAVE_SYNC();
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const int hi = k - 64 * w;
            mask[w] = hi <= 0 ? 0ull : (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull));
        }
        return k;
    }

    // packed root (engine.hip upload_dense_roots / the device root policy): neighbourhoods u64[n]; per agent 17 KW words =
    // [initial rank mask: KW][rank -> action id table: 64 KW x u16]
    static constexpr int PACKED_WORDS = 17 * KW_;
    __device__ static float init_root(const Arenas &a, const int t, Lds &s, const uint32_t dyn, const uint8_t *__restrict__ root_bytes,
                                      const uint64_t *__restrict__ packed, St &st) {
        const int n = a.n;
        const uint64_t *adj = reinterpret_cast<const uint64_t *>(root_bytes) + (size_t)t * n;
        const uint64_t row = LANE < n ? adj[LANE] : 0ull;
        s.adj[LANE] = row;
        a.root_adj[(size_t)t * DENSE_MAX_N + LANE] = row;
        a.cur_adj[(size_t)t * DENSE_MAX_N + LANE] = row;
        const uint64_t *pk = packed + (size_t)t * PACKED_WORDS;
        const uint16_t *tab = reinterpret_cast<const uint16_t *>(pk + KW);
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const uint16_t v = tab[64 * w + LANE];
            a.root_aid[(size_t)t * MAX_SLOTS + 64 * w + LANE] = v;
            s.aid[64 * w + LANE] = v;
        }
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            st.rem[w] = pk[w];
            if (LANE == 0) {
                a.root_perm[(size_t)t * KW + w] = st.rem[w];
                a.cur_perm[(size_t)t * KW + w] = st.rem[w];
            }
        }
        WAVE_SYNC();
        return Cost::root_cost(a, t, s, st);
    }

    // ---- hooks of the device root policy (root_policy.inc): the drivers' modify_root (04-c21-tree.rs:172-206) over this space --
    // node chosen by the same rule, its path replayed onto the root's graph, k' of the E edge slots re-drawn as modifiable
    static constexpr int UNIVERSE_MAX = DENSE_MAX_N * (DENSE_MAX_N - 1) / 2, SLOT_WORDS_MAX = 32;
    static constexpr bool SEQ_POLICY = false; // sequence-keyed paths: not built for this space's policy (the engine refuses)
    __device__ static __forceinline__ int slot_words(const Arenas &a) { return (a.E + 63) / 64; }
    __device__ static __forceinline__ int policy_universe(const Arenas &a) { return a.E; }
    __device__ static __forceinline__ int root_bytes(const Arenas &a) { return 8 * a.n; }
    __device__ static __forceinline__ int permitted_count(const St &st) { return mask_count<KW>(st.rem); }
    // oracle gen_dense_root: G(n, p) redrawn until connected (ConnectedBitsetGraph::generate, mod.rs:84-97), seeded: at attempt
    // t the edge at slot e is present iff (key(seed, domain, agent, 4096 + t E + e) >> 40) < p24
    __device__ static void fresh_root(const Arenas &a, Lds &s, uint64_t seed, uint64_t domain, uint64_t agent, uint8_t *po) {
        const int n = a.n, E = a.E;
        for (uint64_t att = 0;; ++att) {
            s.adj[LANE] = 0ull;
            WAVE_SYNC();
            for (int e = LANE; e < E; e += 64)
                if ((uint32_t)(stream_key_dev(seed, domain, agent, 4096ull + att * (uint64_t)E + (uint64_t)e) >> 40) < a.dense_p24) {
                    int mx, mn;
                    dense_from_colex(e, mx, mn);
                    atomicOr((unsigned long long *)&s.adj[mx], 1ull << mn);
                    atomicOr((unsigned long long *)&s.adj[mn], 1ull << mx);
                }
            WAVE_SYNC();
            // connected?  (wave-uniform BFS over the bitsets)
            const uint64_t all = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
            uint64_t seen = 1ull, frontier = 1ull;
            while (frontier) {
                uint64_t next = 0;
                for (uint64_t f = frontier; f; f &= f - 1ull) next |= s.adj[__ffsll((unsigned long long)f) - 1];
                frontier = next & ~seen;
                seen |= next;
            }
            if ((seen & all) == all) break;
            WAVE_SYNC();
        }
        pack_root(a, s, po);
    }
    __device__ static __forceinline__ void pack_root(const Arenas &a, Lds &s, uint8_t *po) {
        if (LANE < a.n) reinterpret_cast<uint64_t *>(po)[LANE] = s.adj[LANE];
    }
    // the new root's packed rank table, as k_init_roots takes it (the graph is in s.adj; `slots` = the mask just drawn)
    __device__ static void finish_root(const Arenas &a, Lds &s, const int t, const uint8_t *, const uint64_t *slots, uint64_t *out_packed) {
        uint64_t mask[KW];
        rank_table(a, s, slots, mask); // (k <= kmax <= MAX_SLOTS: checked by the host)
        uint64_t *pk = out_packed + (size_t)t * PACKED_WORDS;
        uint16_t *tab = reinterpret_cast<uint16_t *>(pk + KW);
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            tab[64 * w + LANE] = s.aid[64 * w + LANE];
            if (LANE == 0) pk[w] = mask[w];
        }
    }

    // ArgminData { state, cost, eval } (log.rs:1-11)
    __device__ static void argmin_out(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const int wt, const uint32_t win_node) {
        typename Cost::Replay r;
        Cost::argmin_cost(a, s, r);
        open_slots(a, s, st);
        Cost::argmin_write(a, s, r, wt, win_node);
        // a.argmin->eval is what k_argmin / k_argmin_log1 compare against
        if (LANE == 0) a.argmin->eval = r.ev;
    }
};

// host side: the key width (words of a rank set) follows the engine's max_slots: 2, 4, 10 or 16 (engine.hip)
// (DenseSpace<KW> = DenseSpace<KW, DenseCostC21>)
#define DISPATCH_DKW(A, FN, ...)                                  \
    switch ((A).KW) {                                             \
    case 2: FN<DenseSpace<2>>(__VA_ARGS__); break;                \
    case 4: FN<DenseSpace<4>>(__VA_ARGS__); break;                \
    case 10: FN<DenseSpace<10>>(__VA_ARGS__); break;              \
    default: FN<DenseSpace<16>>(__VA_ARGS__); break;              \
    }
// ... and of an engine with another cost policy (key widths 2 / 4 / 10: dense_ah_kernels.hip, dense_ah_wide_kernels.hip)
#define DISPATCH_DKW_COST(COST, A, FN, ...)                       \
    switch ((A).KW) {                                             \
    case 2: FN<DenseSpace<2, COST>>(__VA_ARGS__); break;          \
    case 4: FN<DenseSpace<4, COST>>(__VA_ARGS__); break;          \
    default: FN<DenseSpace<10, COST>>(__VA_ARGS__); break;        \
    }

// The default cost outside any engine (space_ops.h: launch_probe_dense_cost; a template, so that only the unit that launches it
// holds it): one wave per graph.  Step 0 is a root's cost -- lambda_1 and a maximum matching from nothing -- and step j = 1 ..
// n_toggles a new node's: the edge at colex slot toggles[g][j - 1] flipped, the previous step's matching repaired, lambda_1 with
// a hook that counts its calls (evaluate() above, without the arenas).  Outputs are [count][n_toggles + 1], mate [..][64] bytes.
// The host has checked the graphs and the slots (engine_probes.hip): LDS is indexed by the bits of adj.
template <int KW_>
__global__ __launch_bounds__(64) void k_probe_dense_cost(const uint64_t *__restrict__ adj, const int n, const int count,
                                                         const uint16_t *__restrict__ toggles, const int n_toggles, double *__restrict__ lambda_1,
                                                         int *__restrict__ matching_size, uint8_t *__restrict__ mate, int *__restrict__ hook_calls) {
    __shared__ DenseLds<KW_> s;
    const int g = blockIdx.x;
    if (g >= count) return;
    s.adj[LANE] = LANE < n ? adj[(size_t)g * n + LANE] : 0ull;
    LDS_SYNC();
    const size_t row = (size_t)g * (size_t)(n_toggles + 1);
    for (int j = 0; j <= n_toggles; ++j) {
        int mu, calls = 0;
        if (j == 0) mu = dense_matching_scratch(s, n);
        else {
            int mx, mn;
            dense_from_colex((int)toggles[(size_t)g * n_toggles + j - 1], mx, mn);
            if (LANE == 0) {
                s.adj[mx] ^= 1ull << mn;
                s.adj[mn] ^= 1ull << mx;
            }
            LDS_SYNC();
            mu = dense_matching_update(s, n, mx, mn);
        }
        const double lam = dense_lambda1_wave(s, n, [&]() { calls += 1; });
        mate[(row + j) * DENSE_MAX_N + LANE] = s.mate[LANE];
        if (LANE == 0) {
            lambda_1[row + j] = lam;
            matching_size[row + j] = mu;
            hook_calls[row + j] = calls;
        }
        LDS_SYNC();
    }
}
