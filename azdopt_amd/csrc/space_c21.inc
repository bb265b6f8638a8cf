// space_c21.inc -- the c21 state/action space on the device (included inside namespace azd after
// tree_core.inc): ROTModifyParentsOnce<N, Conjecture2Dot1Cost> (graph-state/src/rooted_tree/space.rs:14-125)
// with the driver's closures (graph-state/examples/04-c21-tree.rs:96-105).
// ---------------------------------------------------------------- per-wave LDS
// The selection scratch (kids / tmp_arc), the cascade frontier and the lambda_1 columns are never
// live together, so they share the dynamic LDS region (8 KiB per agent at N = 19).
struct WaveLds {
    uint8_t par[PARENTS_STRIDE];     // parents of the agent's current state
    uint8_t act_parent[256];         // action id -> (parent, child), ordered_edge.rs:40-42
    uint8_t act_child[256];
    unsigned long long ctr[NUM_COUNTERS]; // per-call counters (wave-uniform; kept out of the register file)
    uint16_t seq[MAX_NODE_ACTIONS];       // actions of the current path in the order taken (Layered<L, _> only)
    uint32_t stack[PATH_STACK];     // nodes of the current path, root first (tree_core.inc: cascade)
    uint64_t root_perm[4];          // the agent's root (cache_root): a call goes back to it once per transposition or terminal
    uint8_t root_par[PARENTS_STRIDE];
};
__device__ __forceinline__ double *lds_pq(uint32_t dyn) { return (double *)lds_base(dyn); } // [n-2][32][2] lambda_1 (P, Q) pairs
static size_t dyn_lds_bytes(int n) {
    size_t pq = (size_t)2 * (n > 2 ? n - 2 : 1) * 32 * sizeof(double);
    return CORE_DYN_BYTES > pq ? CORE_DYN_BYTES : pq;
}

// action id -> (parent, child): index(parent, child) = child(child-1)/2 + parent - 1
// (edge.rs:48-65 colex position minus the skipped edge 0-1, ordered_edge.rs:35-42)
__device__ __forceinline__ void build_action_table(WaveLds &s, int A) {
    for (int i = LANE; i < A; i += 64) {
        int c = 2;
        while (c * (c + 1) / 2 - 1 <= i) ++c;
        s.act_child[i] = (uint8_t)c;
        s.act_parent[i] = (uint8_t)(i - (c * (c - 1) / 2 - 1));
    }
}

// bit a set <=> action a is a current parent edge (rooted_tree/mod.rs:60-72)
template <int KW>
__device__ __forceinline__ void current_edges(const WaveLds &s, int A, uint64_t (&out)[KW]) {
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        int i = w * 64 + LANE;
        bool e = (i < A) && (s.par[s.act_child[i]] == s.act_parent[i]);
        out[w] = __ballot(e);
    }
}

// space.rs:56-73 `act`: parents[child] = parent; drop every permitted (u, child), u < child --
// those ids are the contiguous range [child(child-1)/2 - 1, +child)
template <int KW>
__device__ __forceinline__ void do_act(WaveLds &s, uint64_t (&perm)[KW], uint32_t a) {
    int p = s.act_parent[a], c = s.act_child[a];
    if (LANE == 0) s.par[c] = (uint8_t)p;
    clear_bit_range<KW>(perm, c * (c - 1) / 2 - 1, c);
    LDS_SYNC(); // (an LDS hand-off: does not wait for the wave's global stores)
}


// lambda_1 cost contract (DESIGN.md "lambda_1"; stands in for faer at ordered_edge.rs:72-82):
// phi_v = characteristic polynomial of the subtree below v is positive for every v  <=>  x > lambda_1.
// Division-free fold of each vertex into its parent's running pair (P, Q), initially (1, 0):
//     phi = x P[v] - Q[v];   Q[p] = Q[p] phi + P[p] P[v];   P[p] = P[p] phi        (v = N-1 .. 1)
// at 32 trial points per round (33-section of the bracket; lanes l and l+32 duplicate each other),
// at most 12 rounds.  FULL = false (node costs): stop once both bracket ends round to the same f32,
// which is all `lambda_1 as f32` (04-c21-tree.rs:100) can see.
// Shape of the loop: the kernel waits for its slowest agent, so single-wave latency is what counts,
// and on this machine that means NO BRANCHES in the vertex loop (a taken scalar branch costs more
// than the six f64 operations of a fold).  Every vertex runs the same straight-line body; the
// wave-uniform tree only enters through LDS addresses: per-lane (P, Q) live in LDS columns
// [slot][lane], slot(v) = v for v = 0..n-3 (vertices n-1 and n-2 are leaves by construction and are
// peeled), and parents are packed 5 bits each into two scalars, so the loop issues no LDS read for
// the tree itself.  Four ds_read_b64 go out together per vertex, then six DP ops, then two writes.
// parents[] as two wave-uniform scalars, 5 bits per vertex (12 vertices per word)
struct PackedTree {
    uint64_t par0, par1;
};
__device__ __forceinline__ PackedTree pack_tree(const WaveLds &s, int n) {
    uint64_t w0 = 0, w1 = 0;
    if (LANE >= 1 && LANE < n) {
        uint64_t pv = s.par[LANE];
        if (LANE < 12) w0 = pv << (5 * LANE);
        else w1 = pv << (5 * (LANE - 12));
    }
    PackedTree t;
    t.par0 = uni64(wave_or_u64(w0));
    t.par1 = uni64(wave_or_u64(w1));
    return t;
}

// |maximum matching| of the tree.  The reference strips leaves round by round
// (ordered_edge.rs:94-124; restated literally in matching_wave below, which k_argmin uses to report
// the edges); that procedure only ever matches a leaf of the remaining forest with its parent,
// which is always safe, so its size is the matching number -- here computed by the one-pass
// children-before-parents greedy on the scalar unit (tests compare both against the oracle).
__device__ __forceinline__ int matching_size_wave(const PackedTree &t, int n) {
    uint32_t matched = 0;
    int m = 0;
    for (int v = n - 1; v >= 1; --v) {
        const uint32_t p = (uint32_t)((v < 12 ? (t.par0 >> (5 * v)) : (t.par1 >> (5 * (v - 12)))) & 31ull);
        const uint32_t free_both = ~(matched >> v) & ~(matched >> p) & 1u;
        matched |= (free_both << v) | (free_both << p);
        m += (int)free_both;
    }
    return m;
}

// NS > 0: the vertex count as a compile-time constant (the vertex loop unrolls: no loop branch,
// constant LDS offsets and field shifts); NS = 0: runtime n.
template <bool FULL, int NS>
__device__ double lambda1_impl(const PackedTree &t, int n_rt, uint32_t dyn, const double lo0, const double hi0) {
    const int n = NS ? NS : n_rt;
    uint64_t par0 = t.par0, par1 = t.par1;
    const int nslot = n > 2 ? n - 2 : 1;
    const int l = LANE & 31;
    // (P, Q) of a vertex side by side: one 16-byte LDS access per pair instead of two of 8 (the column of
    // lane l is 16 bytes wide; both half-waves compute the same 32 points)
    double2 *PQ = reinterpret_cast<double2 *>(lds_pq(dyn)) + l;
    const int p_last = (int)(((n - 1) < 12 ? (par0 >> ((5 * (n - 1)) & 63)) : (par1 >> ((5 * (n - 13)) & 63))) & 31ull);
    const int p_prev = (int)(((n - 2) < 12 ? (par0 >> ((5 * (n - 2)) & 63)) : (par1 >> ((5 * (n - 14)) & 63))) & 31ull);
    double lo = lo0, hi = hi0; // path ... star (c21_host.cpp:c21_lambda_bracket)
    // Round 4: once both ends of the bracket carry a value of the tree's characteristic polynomial phi_0 with the signs of a
    // simple crossing (phi_0(lo) < 0 < phi_0(hi)), the round's 32 trial points go into a WINDOW around the secant's estimate
    // of the root -- half-width 8 (span / 2)^2 (the secant's error for |phi'' / phi'| up to ~8), at least span / 1024 -- clipped to
    // the bracket, instead of across the whole bracket.  The bracket stays a bracket whatever the window catches (the ends are
    // replaced by trial points only), so the value is unchanged where both procedures converge; 5.25 -> 3.6 rounds per node cost.
    // Round 5: a window may miss the root (all 32 points on one side of it).  A near miss is harmless, but with lambda_2 close to
    // lambda_1 (the double brooms) every window misses and the bracket creeps instead of shrinking: the THIRD miss of a solve
    // switches the window off for the rest of it (plain 33-section from there).  Every round that is no miss shrinks the bracket
    // 33-fold at least, so 15 rounds give what 12 plain rounds give (33^12 > 2^60).
    // The same operations, one IEEE f64 operation each, in oracle/azd_oracle.cpp:lambda1_sturm and oracle/py_oracle.py:lambda1.
    double flo = 0.0, fhi = 0.0;
    bool have_lo = false, have_hi = false;
    int misses = 0;
    for (int round = 0; round < 15; ++round) {
        if (!FULL && (float)lo == (float)hi) break;
        double wlo = lo, whi = hi;
        bool in_window = false;
        if (misses < 3 && have_lo && have_hi && flo < 0.0 && fhi > 0.0) {
            const double span = hi - lo;
            const double den = flo - fhi;
            const double tt = flo / den;
            const double st = span * tt;
            const double c = lo + st;
            const double half = span * 0.5;
            const double hh = half * half;
            double d = 8.0 * hh;
            const double dmin = span * 0.0009765625;
            if (d < dmin) d = dmin;
            if (d < half) {
                const double wa = c - d, wb = c + d;
                if (wa > lo) wlo = wa;
                if (wb < hi) whi = wb;
                in_window = true;
            }
        }
        const double ws = whi - wlo;
        const double w = ws / 33.0;
        const double step = w * (double)(l + 1);
        const double x = wlo + step;
        bool ok = false;
        double phi0 = 0.0;
        if (LANE < 32) { // (the upper half-wave would compute the same 32 points over again)
        for (int v = 0; v < nslot; ++v) PQ[v * 32] = make_double2(1.0, 0.0);
        ok = x > 0.0;
        // peeled leaves n-1 and n-2 (n >= 4): phi = x*1 - 0 = x, psi = 1
        {
            const double2 pq = PQ[p_last * 32];
            const double pp = pq.x, qp = pq.y;
            const double qphi = qp * x, ppsi = pp * 1.0;
            PQ[p_last * 32] = make_double2(pp * x, qphi + ppsi);
        }
        {
            const double2 pq = PQ[p_prev * 32];
            const double pp = pq.x, qp = pq.y;
            const double qphi = qp * x, ppsi = pp * 1.0;
            PQ[p_prev * 32] = make_double2(pp * x, qphi + ppsi);
        }
        for (int v = n - 3; v >= 1; --v) {
            const int p = (int)((v < 12 ? (par0 >> (5 * v)) : (par1 >> (5 * (v - 12)))) & 31ull);
            const double2 own = PQ[v * 32];
            const double2 par = PQ[p * 32];
            const double pv = own.x, qv = own.y;
            const double pp = par.x, qp = par.y;
            const double xp = x * pv;
            const double phi = xp - qv;
            ok = ok && (phi > 0.0);
            const double qphi = qp * phi;
            const double ppsi = pp * pv;
            PQ[p * 32] = make_double2(pp * phi, qphi + ppsi);
        }
        const double2 root = PQ[0];
        const double xp0 = x * root.x;
        phi0 = xp0 - root.y;
        ok = ok && (phi0 > 0.0);
        }
        const uint32_t m = (uint32_t)__ballot(ok);
        const int first = m ? (__ffs((int)m) - 1) : 32;
        if (first > 0) {
            lo = rdlane_f64(x, first - 1);
            flo = rdlane_f64(phi0, first - 1);
            have_lo = true;
        }
        if (first < 32) {
            hi = rdlane_f64(x, first);
            fhi = rdlane_f64(phi0, first);
            have_hi = true;
        }
        if (in_window && (first == 0 || first == 32)) ++misses;
    }
    return hi;
}

template <bool FULL>
__device__ __forceinline__ double lambda1_wave(const PackedTree &t, int n, uint32_t dyn, const double lo0, const double hi0) {
    // lambda1_impl<FULL, 19> (vertex loop unrolled at compile time for the drivers' N = 19) is 1.8x faster in
    // isolation (tools/probe_cost.py).  Its register pressure costs the search loop around it some spills:
    // in the asynchronous step the trade is a win (new node 22.7 -> 15.6 us, select 1.77 -> 1.87 us, +3.5 % end
    // to end), in the barrier step and as an out-of-line call it measured slower, so only that unit uses it.
#ifdef AZD_TU_ASYNC
    if (n == 19) return lambda1_impl<FULL, 19>(t, 19, dyn, lo0, hi0);
#endif
    return lambda1_impl<FULL, 0>(t, n, dyn, lo0, hi0);
}

// ordered_edge.rs:94-124 maximum_matching (leaf stripping), on bit masks.  Returns |matching|;
// optionally writes the (parent, child) pairs.
__device__ int matching_wave(const WaveLds &s, int n, int32_t *pairs_out) {
    uint32_t avail = (n >= 32) ? 0xFFFFFFFFu : ((1u << n) - 1u);
    int m = 0;
    for (int guard = 0; guard < 64; ++guard) {
        uint32_t leaf = avail;
        for (int i = 1; i < n; ++i)
            if ((avail >> i) & 1u) leaf &= ~(1u << s.par[i]);
        for (int i = 1; i < n; ++i) {
            if ((leaf >> i) & 1u) {
                avail &= ~(1u << i);
                int p = s.par[i];
                if ((avail >> p) & 1u) {
                    avail &= ~(1u << p);
                    if (pairs_out && LANE == 0) {
                        pairs_out[2 * m] = p;
                        pairs_out[2 * m + 1] = i;
                    }
                    ++m;
                }
            }
        }
        if (__popc(avail) < 2) break;
    }
    return m;
}

// 04-c21-tree.rs:98-102: squish(matching.len() as f32 + lambda_1 as f32)
__device__ __forceinline__ float c21_eval(float slope, double lambda1, int mu) {
    float c = (float)mu + (float)lambda1;
    float x = c - 2.0f;
    return slope * x;
}

// space.rs:91-101 write_vec: [0, A) one-hot of current parent edges, [A, 2A) permitted mask
template <int KW>
__device__ __forceinline__ void write_state_vec(const WaveLds &s, const uint64_t (&perm)[KW], int A, float *row) {
    uint64_t cur[KW];
    current_edges<KW>(s, A, cur);
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        int i = w * 64 + LANE;
        if (i < A) {
            row[i] = (float)((cur[w] >> LANE) & 1ull);
            row[A + i] = (float)((perm[w] >> LANE) & 1ull);
        }
    }
}

// ---------------------------------------------------------------- the policy tree_core.inc drives (the contract: tree_core.inc, SpaceDefaults)
// Its ActionSet key is the bit mask of the action ids themselves, and its observation map h_sa = c_as* (04-c21-tree.rs:104): the defaults.
template <int KW_>
struct C21Space : SpaceDefaults {
    static constexpr int KW = KW_;
    using Lds = WaveLds;
    struct St {
        uint64_t perm[KW_]; // permitted action ids (modify_parent_once.rs:8-12)
        double lambda;      // Conjecture2Dot1Cost of the last node created (optimizer costs[i])
        int mu;
    };
    static size_t dyn_bytes(const Arenas &a) { return dyn_lds_bytes(a.n); }
    // pool step: the state-vector row is built over the wave's search scratch, which is dead by then
    static size_t pool_dyn_bytes(const Arenas &a) { return dyn_lds_bytes(a.n) > (size_t)a.S * 4 ? dyn_lds_bytes(a.n) : (size_t)a.S * 4; }
    static constexpr bool POOL_EVAL_GROUPS = true; // k_pool is built with evaluator groups too (launchers.inc: l_pool)
    __device__ static __forceinline__ float *row_stage(const Arenas &, const uint32_t dyn) { return reinterpret_cast<float *>(lds_base(dyn)); }

    __device__ static __forceinline__ void prepare(const Arenas &a, Lds &s) { build_action_table(s, a.A); }
    __device__ static __forceinline__ void load_cur(const Arenas &a, const int t, Lds &s, const uint32_t, St &st) {
        if (LANE < PARENTS_STRIDE) s.par[LANE] = a.cur_parents[(size_t)t * PARENTS_STRIDE + LANE];
#pragma unroll
        for (int w = 0; w < KW; ++w) st.perm[w] = a.cur_perm[(size_t)t * KW + w];
        st.lambda = a.cur_lambda[t];
        st.mu = a.cur_mu[t];
    }
    // Two-phase load of an agent's state (rollout_agent, round 5): every request first -- unconditionally, by every lane: a lane-masked
    // block is a scheduling barrier, and each one of them was a round trip of its own at the head of every call -- then the values where they go.
    static constexpr bool TWO_PHASE_LOAD = true;
    struct Raw {
        uint64_t perm[KW], root_perm;
        double lambda;
        int32_t mu;
        uint8_t par, root_par;
    };
    __device__ static __forceinline__ void load_issue(const Arenas &a, const int t, Raw &r) {
        r.par = a.cur_parents[(size_t)t * PARENTS_STRIDE + (LANE & (PARENTS_STRIDE - 1))];
        r.root_par = a.root_parents[(size_t)t * PARENTS_STRIDE + (LANE & (PARENTS_STRIDE - 1))];
#pragma unroll
        for (int w = 0; w < KW; ++w) r.perm[w] = a.cur_perm[(size_t)t * KW + w];
        r.root_perm = a.root_perm[(size_t)t * KW + (LANE < KW ? LANE : 0)];
        r.lambda = a.cur_lambda[t];
        r.mu = a.cur_mu[t];
    }
    __device__ static __forceinline__ void load_finish(Lds &s, St &st, const Raw &r) { // = load_cur + cache_root
        if (LANE < PARENTS_STRIDE) {
            s.par[LANE] = r.par;
            s.root_par[LANE] = r.root_par;
        }
        if (LANE < KW) s.root_perm[LANE] = r.root_perm;
#pragma unroll
        for (int w = 0; w < KW; ++w) st.perm[w] = r.perm[w];
        st.lambda = r.lambda;
        st.mu = r.mu;
    }
    __device__ static __forceinline__ void load_root(const Arenas &a, const int t, Lds &s, const uint32_t, St &st) {
        if (LANE < PARENTS_STRIDE) s.par[LANE] = a.root_parents[(size_t)t * PARENTS_STRIDE + LANE];
#pragma unroll
        for (int w = 0; w < KW; ++w) st.perm[w] = a.root_perm[(size_t)t * KW + w];
    }
    // roll_out_episodes: the root is fetched with the rest of the agent's state when the call starts and kept in LDS; every
    // return to it inside the call (tree/mod.rs:172-179, :220-229) is then a copy instead of a round trip to memory
    __device__ static __forceinline__ void cache_root(const Arenas &a, const int t, Lds &s) {
        if (LANE < PARENTS_STRIDE) s.root_par[LANE] = a.root_parents[(size_t)t * PARENTS_STRIDE + LANE];
        if (LANE < KW) s.root_perm[LANE] = a.root_perm[(size_t)t * KW + LANE];
    }
    __device__ static __forceinline__ void load_root_cached(const Arenas &, const int, Lds &s, const uint32_t, St &st) {
        if (LANE < PARENTS_STRIDE) s.par[LANE] = s.root_par[LANE];
#pragma unroll
        for (int w = 0; w < KW; ++w) st.perm[w] = s.root_perm[w];
    }
    __device__ static __forceinline__ void store_cur(const Arenas &a, const int t, Lds &s, const uint32_t, const St &st) {
        if (LANE < PARENTS_STRIDE) a.cur_parents[(size_t)t * PARENTS_STRIDE + LANE] = s.par[LANE];
        if (LANE == 0) {
#pragma unroll
            for (int w = 0; w < KW; ++w) a.cur_perm[(size_t)t * KW + w] = st.perm[w];
            a.cur_lambda[t] = st.lambda;
            a.cur_mu[t] = st.mu;
        }
    }
    __device__ static __forceinline__ void act(const Arenas &, Lds &s, const uint32_t, St &st, const uint32_t aid) {
        do_act<KW>(s, st.perm, aid);
    }
    // Round 5: the steps of a descent through nodes that exist need no state -- next_action reads predictions only -- so rollout_agent
    // applies a path's actions when a state is called for (a new node: its row, its cost, its legal actions), all at once: the actions of
    // this space commute and never repeat (ActionOrderIndependent + ActionsNeverRepeat, rooted_tree/space.rs:124-125; space/axioms.rs:16-19), so
    // root + {the path's ActionSet} is the state the reference reaches step by step (tree/mod.rs:139-151).  A lane per action id: the ids in
    // `todo` set parents[child] = parent (every child at most once on a path: acting on it removes all its other actions), and every id
    // whose child was acted on leaves the permitted set (space.rs:63-70).
    static constexpr bool DEFER_ACT = true;
    __device__ static __forceinline__ void act_set(const Arenas &a, Lds &s, const uint32_t, St &st, const uint64_t (&todo)[KW]) {
        uint32_t mine = 0u;
        int child[KW];
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const int id = 64 * w + LANE;
            child[w] = id < a.A ? (int)s.act_child[id] : 0;
            if ((todo[w] >> LANE) & 1ull) {
                s.par[child[w]] = (uint8_t)s.act_parent[id];
                mine |= 1u << child[w];
            }
        }
        const uint32_t acted = uni(wave_or_u32(mine));
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const int id = 64 * w + LANE;
            st.perm[w] &= ~(uint64_t)__ballot(id < a.A && ((acted >> child[w]) & 1u) != 0u);
        }
        LDS_SYNC();
    }
    // node cost (f32-exact early stop of the lambda_1 bracket), 04-c21-tree.rs:98-102
    __device__ static __forceinline__ float evaluate(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const int) {
        const unsigned long long ph_l0 = PH_NOW();
        const PackedTree pt = pack_tree(s, a.n);
        st.lambda = lambda1_wave<false>(pt, a.n, dyn, a.lam_lo, a.lam_hi);
        const unsigned long long ph_l1 = PH_NOW();
        st.mu = matching_size_wave(pt, a.n);
        CTR_ADD(22, ph_l1 - ph_l0);
        CTR_ADD(23, PH_NOW() - ph_l1);
        return c21_eval(a.eval_slope, st.lambda, st.mu);
    }
    __device__ static __forceinline__ bool terminal(const Arenas &a, Lds &s, const uint32_t, const St &st) {
        uint64_t cur[KW], legal[KW];
        current_edges<KW>(s, a.A, cur);
#pragma unroll
        for (int w = 0; w < KW; ++w) legal[w] = st.perm[w] & ~cur[w];
        return mask_empty<KW>(legal);
    }
    __device__ static __forceinline__ void write_vec(const Arenas &a, Lds &s, const uint32_t, const St &st, float *row) {
        write_state_vec<KW>(s, st.perm, a.A, row);
    }

    // graph_operations.rs:32-56 with space.rs:75-89 action_data and g = c_s - h (04-c21-tree.rs:103)
    template <bool SC1 = false>
    __device__ static __forceinline__ void add_actions(const Arenas &a, Lds &s, const int t, const RolloutOut *hint, RolloutOut *pick) {
        const int A = a.A;
        uint64_t perm[KW];
#pragma unroll
        for (int w = 0; w < KW; ++w) perm[w] = a.cur_perm[(size_t)t * KW + w];
        // every request of the call first, by every lane (a lane-masked block that holds a request AND its use is a round trip of its
        // own: round 5): the parents' row, the prediction row -- it travels with the state, not behind it -- and, where the caller knows the
        // node, the node's link
        const uint8_t pv = a.cur_parents[(size_t)t * PARENTS_STRIDE + (LANE & (PARENTS_STRIDE - 1))];
        const float *h = a.h_theta + (size_t)t * A;
        float hv[KW];
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            const int i = w * 64 + LANE, ic = i < A ? i : A - 1;
            const float x = SC1 ? ld_sc1_f32(h + ic) : h[ic];
            hv[w] = i < A ? x : 0.0f;
        }
        uint2 link_early = make_uint2(NONE, 0u);
        if (hint) link_early = node_link(a, t, hint->pos);
        if (LANE < PARENTS_STRIDE) s.par[LANE] = pv;
        WAVE_SYNC();
        uint64_t cur[KW], legal[KW];
        current_edges<KW>(s, A, cur);
#pragma unroll
        for (int w = 0; w < KW; ++w) legal[w] = perm[w] & ~cur[w];
        const uint32_t cnt = (uint32_t)mask_count<KW>(legal);
        const uint32_t begin = hint ? hint->n_preds : a.n_preds[t];
        if (!add_actions_fits(a, t, begin, cnt)) return;
        const uint32_t node = hint ? hint->pos : a.state_pos[t];
        PredRec *preds = a.preds + (size_t)t * a.pred_cap;
        const float c = hint ? hint->c : a.nodes[(size_t)t * a.node_cap + node].c;
        const uint2 link = hint ? link_early : node_link(a, t, node);
        uint32_t before = 0;
        FirstPick fp;
        fp.key = 0ull;
        fp.aid = 0u;
        fp.g = 0.f;
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            int i = w * 64 + LANE;
            if ((legal[w] >> LANE) & 1ull) {
                uint32_t rank = before + (uint32_t)__popcll(legal[w] & ((1ull << LANE) - 1ull));
                const float g = c - hv[w];
                const PredRec p = pred_new((uint32_t)i, c, g);
                preds[begin + rank] = p;
                pick_note(fp, __uint_as_float(p.w0), g, rank, (uint32_t)i);
            }
            before += (uint32_t)__popcll(legal[w]);
        }
        add_actions_commit(a, t, node, begin, cnt, hint ? s.ctr : nullptr, link);
        if (pick) pick_finish(fp, begin, cnt, pick);
    }

    // packed root = parents[n] + permitted action mask
    __device__ static float init_root(const Arenas &a, const int t, Lds &s, const uint32_t dyn, const uint8_t *__restrict__ parents,
                                      const uint64_t *__restrict__ permitted, St &st) {
        const int n = a.n;
        if (LANE < PARENTS_STRIDE) {
            uint8_t p = LANE < n ? parents[(size_t)t * n + LANE] : 0;
            s.par[LANE] = p;
            a.root_parents[(size_t)t * PARENTS_STRIDE + LANE] = p;
            a.cur_parents[(size_t)t * PARENTS_STRIDE + LANE] = p;
        }
#pragma unroll
        for (int w = 0; w < KW; ++w) {
            st.perm[w] = permitted[(size_t)t * KW + w];
            if (LANE == 0) {
                a.root_perm[(size_t)t * KW + w] = st.perm[w];
                a.cur_perm[(size_t)t * KW + w] = st.perm[w];
            }
        }
        WAVE_SYNC();
        const PackedTree pt = pack_tree(s, n);
        st.lambda = lambda1_wave<false>(pt, n, dyn, a.lam_lo, a.lam_hi);
        st.mu = matching_size_wave(pt, n);
        if (LANE == 0) {
            a.cur_lambda[t] = st.lambda;
            a.cur_mu[t] = st.mu;
        }
        return c21_eval(a.eval_slope, st.lambda, st.mu);
    }

    // ---- hooks of the device root policy (root_policy.inc)
    static constexpr int UNIVERSE_MAX = 256, SLOT_WORDS_MAX = 4;
    static constexpr bool SEQ_POLICY = true;
    __device__ static __forceinline__ int policy_universe(const Arenas &a) { return a.A; }
    __device__ static __forceinline__ int root_bytes(const Arenas &a) { return a.n; }
    __device__ static __forceinline__ int permitted_count(const St &st) { return mask_count<KW>(st.perm); }
    // ROTWithActionPermissions::generate's tree (rooted_tree/mod.rs:14-20), seeded: parents[v] = below(draw v, v)
    __device__ static __forceinline__ void fresh_root(const Arenas &a, Lds &, uint64_t seed, uint64_t domain, uint64_t agent, uint8_t *po) {
        const int n = a.n;
        if (LANE < n) {
            uint8_t p = 0;
            if (LANE >= 2 && LANE <= n - 2) p = (uint8_t)below_dev(stream_key_dev(seed, domain, agent, (uint64_t)LANE), (uint32_t)LANE);
            po[LANE] = p;
        }
    }
    __device__ static __forceinline__ void pack_root(const Arenas &a, Lds &s, uint8_t *po) {
        if (LANE < a.n) po[LANE] = s.par[LANE];
    }

    // ArgminData { state, cost, eval } (log.rs:1-11), cost at the full f64 bracket
    __device__ static void argmin_out(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const int wt, const uint32_t win_node) {
        const int n = a.n;
        ArgminRec *out = a.argmin;
        double lam = lambda1_wave<true>(pack_tree(s, n), n, dyn, a.lam_lo, a.lam_hi);
        int mu = matching_wave(s, n, out->matching);
        float ev = c21_eval(a.eval_slope, lam, mu);
        if (LANE < 32) out->parents[LANE] = LANE < n ? s.par[LANE] : 0;
        if (LANE == 0) {
#pragma unroll
            for (int w = 0; w < 4; ++w) out->permitted[w] = 0;
#pragma unroll
            for (int w = 0; w < KW; ++w) out->permitted[w] = st.perm[w];
            out->lambda_1 = lam;
            out->matching_size = mu;
            out->eval = ev;
            out->agent = wt;
            out->node = win_node;
        }
    }
};

// host side: the instantiation an engine's key width selects
// BIG is a spare specialisation flag (n > 19); the kernels no longer depend on it
#define DISPATCH_KW(A, FN, ...)                                   \
    switch ((A).KW) {                                             \
    case 1: FN<C21Space<1>>(__VA_ARGS__); break;                  \
    case 2: FN<C21Space<2>>(__VA_ARGS__); break;                  \
    case 3: FN<C21Space<3>>(__VA_ARGS__); break;                  \
    default: FN<C21Space<4>>(__VA_ARGS__); break;                 \
    }
