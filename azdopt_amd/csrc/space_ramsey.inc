// space_ramsey.inc -- the Ramsey colour-reassignment space on the device (included inside namespace
// azd after tree_core.inc): RamseySpaceNoEdgeRecolor<B32, N, E, C> (graph-state/src/ramsey_counts/
// space.rs:10-176) over RamseyCountsNoRecolor (no_recolor.rs:9-13) / RamseyCounts (mod.rs:12-17).
//
// State of one agent:
//   nbr[c][v]     u32   neighbourhood of v in colour class c (BitsetGraph<N, B32>)        static LDS
//   counts[c][e]  i32   #(sizes[c]-2)-cliques of colour c inside the common c-neighbourhood
//                       of the endpoints of edge position e (every pair, adjacent or not)  dynamic LDS
//   tot[c]        i32   #monochromatic sizes[c]-cliques (TotalCounts)                      registers
//   perm          bits  permitted edge positions                                           registers
// An action id a = e + new_colour * E recolours edge e (space.rs:48-54) and retires it.  Lanes
// parallelise over the third vertex w of the affected cliques (32 lanes per endpoint) and over the
// second vertex of the affected vertex pairs; all touched counts are distinct edges, so the updates
// need no atomics.  Integer work throughout; the only f32 arithmetic is evaluate / g / h_sa.

constexpr int RAMSEY_MAX_E = 256;
constexpr int RAMSEY_WIDE_MAX_E = 496; // N = 32 (wide engines: azd_engine_config::max_slots > 0)
constexpr int RAMSEY_U64_MAX_E = 1128; // N = 48 (the 64-bit tier: AZD_ENGINE_RAMSEY_U64; E*C <= 2304 bounds E at two colours)
constexpr int RAMSEY_MAX_C = 4;

// W: the neighbourhood word (BitsetGraph<N, B32> / <N, B64>): uint32_t rows of 32 vertices, or uint64_t rows of 64 for the 64-bit tier
template <int ME, class W = uint32_t>
struct RamseyLdsT {
    using Word = W;
    static constexpr int NV = (int)sizeof(W) * 8; // vertices a row can hold
    W nbr[RAMSEY_MAX_C][NV];
    uint8_t ev[ME]; // edge position -> larger endpoint (edge.rs:55-65)
    uint8_t eu[ME]; //               -> smaller endpoint
    unsigned long long ctr[NUM_COUNTERS];
    uint16_t seq[MAX_NODE_ACTIONS]; // actions of the current path in the order taken (Layered<L, _> only)
    uint32_t stack[PATH_STACK];     // nodes of the current path, root first (tree_core.inc: cascade)
};
using RamseyLds = RamseyLdsT<RAMSEY_MAX_E>;
using RamseyWideLds = RamseyLdsT<RAMSEY_WIDE_MAX_E>;
using RamseyU64Lds = RamseyLdsT<RAMSEY_U64_MAX_E, uint64_t>;

__device__ __forceinline__ int nb_popc(uint32_t x) { return __popc(x); }
__device__ __forceinline__ int nb_popc(uint64_t x) { return __popcll(x); }
__device__ __forceinline__ int nb_ffs(uint32_t x) { return __ffs((int)x); }
__device__ __forceinline__ int nb_ffs(uint64_t x) { return __ffsll((unsigned long long)x); }

__device__ __forceinline__ uint32_t u32_add(uint32_t a, uint32_t b) { return a + b; }
// wave-wide sum: the same DPP ladder as wave_min_u32 is an inclusive scan, lane 63 holds the total
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    AZD_DPP_STEP(u32_add, 0u, v, 0x111, 0xf, 0xf);
    AZD_DPP_STEP(u32_add, 0u, v, 0x112, 0xf, 0xf);
    AZD_DPP_STEP(u32_add, 0u, v, 0x114, 0xf, 0xe);
    AZD_DPP_STEP(u32_add, 0u, v, 0x118, 0xf, 0xc);
    AZD_DPP_STEP(u32_add, 0u, v, 0x142, 0xa, 0xf);
    AZD_DPP_STEP(u32_add, 0u, v, 0x143, 0xc, 0xf);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// edge.rs:48-53 colex_position for mx > mn
__device__ __forceinline__ int colex_pos(int mx, int mn) { return mx * (mx - 1) / 2 + mn; }

// bitset_graph/mod.rs:164-185 count_cliques_inside at a fixed depth K: a compile-time recursion that is inlined whole (no stack: the K
// sets of a lane are registers).  Each level takes the largest vertex u of the clique and goes on in the part of the set below u.  The
// reference's `1 + |T| >= size` filter only skips terms that are zero: from K = 4 a set with fewer than K - 1 vertices is left at once.
template <int K, class W>
__device__ __forceinline__ int cliques_nest(const W *nb, const W S) {
    if constexpr (K == 0) return 1;
    else if constexpr (K == 1) return nb_popc(S);
    else {
        int sum = 0;
        for (W r = S; r; r &= r - (W)1) {
            const int u = nb_ffs(r) - 1;
            const W T = S & nb[u] & (((W)1 << u) - (W)1);
            if constexpr (K >= 4) {
                if (nb_popc(T) < K - 1) continue;
            }
            sum += cliques_nest<K - 1>(nb, T);
        }
        return sum;
    }
}
// count_cliques_inside for k <= DEPTH, the deepest count a space asks for: 3 (clique sizes up to 5; RamseySpaceBase's default) as
// written-out loops, 6 (RamseyU64BigSpace: sizes up to AZD_RAMSEY_BIG_CLIQUE_MAX) as the nest the run-time depth picks in one
// wave-uniform switch.
template <int DEPTH, class W>
__device__ __forceinline__ int cliques_inside(const W *nb, W S, int k) {
    static_assert(DEPTH == 3 || DEPTH == 6, "written out for depths 0..3 and 0..6");
    if constexpr (DEPTH == 3) {
        if (k == 0) return 1;
        if (k == 1) return nb_popc(S);
        int sum = 0;
        for (W r = S; r; r &= r - (W)1) {
            const int u = nb_ffs(r) - 1;
            const W T = S & nb[u] & (((W)1 << u) - (W)1);
            if (k == 2) sum += nb_popc(T);
            else
                for (W q = T; q; q &= q - (W)1) {
                    const int x = nb_ffs(q) - 1;
                    sum += nb_popc(T & nb[x] & (((W)1 << x) - (W)1));
                }
        }
        return sum;
    } else {
        switch (k) {
        case 0: return 1;
        case 1: return cliques_nest<1>(nb, S);
        case 2: return cliques_nest<2>(nb, S);
        case 3: return cliques_nest<3>(nb, S);
        case 4: return cliques_nest<4>(nb, S);
        case 5: return cliques_nest<5>(nb, S);
        default: return cliques_nest<6>(nb, S);
        }
    }
}

// (atomicOr has no uint64_t overload: the 64-bit rows go through unsigned long long)
__device__ __forceinline__ uint32_t *nbr_atomic(uint32_t *p) { return p; }
__device__ __forceinline__ unsigned long long *nbr_atomic(uint64_t *p) { return reinterpret_cast<unsigned long long *>(p); }
__device__ __forceinline__ uint32_t nbr_atomic_bit(int b, uint32_t) { return 1u << b; }
__device__ __forceinline__ unsigned long long nbr_atomic_bit(int b, uint64_t) { return 1ull << b; }

// ramsey_counts/mod.rs:101-164 reassign_color_count_adjustment (edge uv absent from `color`'s graph)
template <int DEPTH, class LDS>
__device__ __forceinline__ void ramsey_adjust(LDS &s, int32_t *counts, const int E, const bool subtract, const int u,
                                              const int v, const int color, const int size) {
    if (size <= 2) return;
    using W = typename LDS::Word;
    const W *nb = s.nbr[color];
    int32_t *cnt = counts + color * E;
    const W n_u = nb[u], n_v = nb[v], n_uv = n_u & n_v;
    if constexpr (sizeof(W) == 8) {
        // 64 vertices: one endpoint per pass, lanes over w.  Pass 0: edge {v, w} for w in n_u; pass 1: edge {u, w} for w in n_v.
        // Within a pass the edges are distinct; the passes run one after the other.
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            const int w = LANE;
            const W mem = pass ? n_v : n_u;
            const int other = pass ? u : v;
            if ((mem >> w) & (W)1) {
                const int change = cliques_inside<DEPTH>(nb, n_uv & nb[w], size - 3);
                if (change != 0) {
                    const int pos = other > w ? colex_pos(other, w) : colex_pos(w, other);
                    cnt[pos] += subtract ? -change : change;
                }
            }
        }
    } else {
        // lanes 0..31: edge {v, w} for w in n_u; lanes 32..63: edge {u, w} for w in n_v
        const int w = LANE & 31;
        const bool hi = LANE >= 32;
        const W mem = hi ? n_v : n_u;
        const int other = hi ? u : v;
        if ((mem >> w) & (W)1) {
            const int change = cliques_inside<DEPTH>(nb, n_uv & nb[w], size - 3);
            if (change != 0) {
                const int pos = other > w ? colex_pos(other, w) : colex_pos(w, other);
                cnt[pos] += subtract ? -change : change;
            }
        }
    }
    if (size == 3) return;
    // edge {w, x} for w < x both in n_uv (tuple_combinations): scalar over w, lanes over x
    for (W r = n_uv; r; r &= r - (W)1) {
        const int w = nb_ffs(r) - 1;
        const W n_uvw = n_uv & nb[w];
        const int x = LANE;
        if (x < LDS::NV && x > w && ((n_uv >> x) & (W)1)) {
            const int change = cliques_inside<DEPTH>(nb, n_uvw & nb[x], size - 4);
            if (change != 0) cnt[colex_pos(x, w)] += subtract ? -change : change;
        }
    }
}

// The space over an edge capacity ME, ARG the argmin record it writes and CH_ chunks of 64 predictions per node.  RamseySpace<KW>
// (below) is today's space: ME = 256, two chunks (MAX_NODE_ACTIONS).  RamseyWideSpace<KW> takes N <= 32 (ME = 496) and nodes of
// up to 64 KW actions (select_big); the engine picks it when azd_engine_config::max_slots > 0.  The clique counts sit in the dynamic
// LDS behind the search scratch, which is CORE_DYN_BYTES or select_big's two lists of 64 CH words, whichever is larger.
// (The contract: tree_core.inc, SpaceDefaults.  The ActionSet key is the bit mask of the action ids themselves, and there is no LDS
// copy of the root -- it is as large as the live state: the defaults.)
template <int KW_, int ME, class ARG, int CH_, class W_ = uint32_t, int DEPTH = 3>
struct RamseySpaceBase : SpaceDefaults {
    using W = W_;                                    // neighbourhood word
    static constexpr int NV = (int)sizeof(W_) * 8;   // vertices per row: nbr is [RAMSEY_MAX_C][NV] words
    static constexpr int NBL = RAMSEY_MAX_C * NV / 64; // words of nbr per lane: 2 or 4
    static_assert(NBL == 2 || NBL == 4, "uint32_t or uint64_t neighbourhood words");
    static constexpr int KW = KW_;
    static constexpr int CH = CH_; // chunks of 64 predictions a node may hold
    static constexpr int PW = (KW_ + 1) / 2; // permitted-edge words: E = A / C <= A / 2
    static constexpr bool FRONTIER_SPILL = true; // cascade levels wider than the LDS frontier go to memory (tree_core.inc: cascade)
    static constexpr size_t SCRATCH = (size_t)512 * CH_ > CORE_DYN_BYTES ? (size_t)512 * CH_ : CORE_DYN_BYTES;
    static constexpr int APW = sizeof(ARG::permitted) / 8; // permitted words of the argmin record
    using Lds = RamseyLdsT<ME, W_>;
    struct St {
        uint64_t perm[PW];
        int32_t tot[RAMSEY_MAX_C];
    };
    __device__ static __forceinline__ int32_t *lds_counts(uint32_t dyn) { return (int32_t *)(lds_base(dyn) + SCRATCH); }
    static size_t dyn_bytes(const Arenas &a) { return SCRATCH + (size_t)a.C * a.E * sizeof(int32_t); }
    // pool step: write_vec reads the live clique counts (behind the search scratch), the scratch itself is dead by then:
    // the state-vector row is built over the scratch if it fits there, else behind the counts
    static size_t pool_dyn_bytes(const Arenas &a) {
        const size_t base = (dyn_bytes(a) + 15) & ~(size_t)15;
        return (size_t)a.S * 4 <= SCRATCH ? base : base + (size_t)a.S * 4;
    }
    __device__ static __forceinline__ float *row_stage(const Arenas &a, const uint32_t dyn) {
        if ((size_t)a.S * 4 <= SCRATCH) return reinterpret_cast<float *>(lds_base(dyn));
        return reinterpret_cast<float *>(lds_base(dyn) + ((SCRATCH + (size_t)a.C * a.E * sizeof(int32_t) + 15) & ~(size_t)15));
    }

    __device__ static __forceinline__ void prepare(const Arenas &a, Lds &s) {
        for (int e = LANE; e < a.E; e += 64) {
            int v = 1;
            while (v * (v + 1) / 2 <= e) ++v;
            s.ev[e] = (uint8_t)v;
            s.eu[e] = (uint8_t)(v - (v * (v + 1) / 2 - e));
        }
    }
    __device__ static __forceinline__ void load_from(const Arenas &a, const int t, Lds &s, const uint32_t dyn, St &st,
                                                     const uint32_t *nbr, const int32_t *counts, const int32_t *tot,
                                                     const uint64_t *perm) {
        // every request first, by every lane, then the values where they go (round 5: the counts' loop -- a request and its LDS store per
        // trip, a runtime trip count -- was a round trip per 64 counts, at the head of every call AND at every return to the root; C E <= 64 KW)
        W *dst = &s.nbr[0][0];
        const W *src = reinterpret_cast<const W *>(nbr) + (size_t)t * (RAMSEY_MAX_C * NV);
        // (two named words per lane for the 32-bit rows, four for the 64-bit ones: as an array the two cost the narrow kernels registers)
        const W n0 = src[LANE], n1 = src[LANE + 64];
        W n2 = 0, n3 = 0;
        if constexpr (NBL == 4) {
            n2 = src[LANE + 128];
            n3 = src[LANE + 192];
        }
        const int CE = a.C * a.E;
        int32_t *lc = lds_counts(dyn);
        const int32_t *gc = counts + (size_t)t * CE;
        int32_t cv[KW];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int i = 64 * k + LANE;
            cv[k] = gc[i < CE ? i : 0];
        }
#pragma unroll
        for (int w = 0; w < PW; ++w) st.perm[w] = perm[(size_t)t * KW + w];
#pragma unroll
        for (int c = 0; c < RAMSEY_MAX_C; ++c) st.tot[c] = tot[(size_t)t * RAMSEY_MAX_C + c];
        __builtin_amdgcn_sched_barrier(0);
        dst[LANE] = n0;
        dst[LANE + 64] = n1;
        if constexpr (NBL == 4) {
            dst[LANE + 128] = n2;
            dst[LANE + 192] = n3;
        }
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int i = 64 * k + LANE;
            if (i < CE) lc[i] = cv[k];
        }
    }
    __device__ static __forceinline__ void load_cur(const Arenas &a, const int t, Lds &s, const uint32_t dyn, St &st) {
        load_from(a, t, s, dyn, st, a.cur_nbr, a.cur_counts, a.cur_tot, a.cur_perm);
    }
    __device__ static __forceinline__ void load_root(const Arenas &a, const int t, Lds &s, const uint32_t dyn, St &st) {
        load_from(a, t, s, dyn, st, a.root_nbr, a.root_counts, a.root_tot, a.root_perm);
    }
    __device__ static __forceinline__ void load_root_cached(const Arenas &a, const int t, Lds &s, const uint32_t dyn, St &st) { load_root(a, t, s, dyn, st); }
    __device__ static __forceinline__ void store_to(const Arenas &a, const int t, Lds &s, const uint32_t dyn, const St &st,
                                                    uint32_t *nbr, int32_t *counts, int32_t *tot, uint64_t *perm) {
        const W *src = &s.nbr[0][0];
        W *dst = reinterpret_cast<W *>(nbr) + (size_t)t * (RAMSEY_MAX_C * NV);
        dst[LANE] = src[LANE];
        dst[LANE + 64] = src[LANE + 64];
        if constexpr (NBL == 4) {
            dst[LANE + 128] = src[LANE + 128];
            dst[LANE + 192] = src[LANE + 192];
        }
        const int CE = a.C * a.E;
        const int32_t *lc = lds_counts(dyn);
        int32_t *gc = counts + (size_t)t * CE;
        for (int i = LANE; i < CE; i += 64) gc[i] = lc[i];
        if (LANE == 0) {
#pragma unroll
            for (int w = 0; w < KW; ++w) perm[(size_t)t * KW + w] = w < PW ? st.perm[w < PW ? w : 0] : 0ull;
#pragma unroll
            for (int c = 0; c < RAMSEY_MAX_C; ++c) tot[(size_t)t * RAMSEY_MAX_C + c] = st.tot[c];
        }
    }
    __device__ static __forceinline__ void store_cur(const Arenas &a, const int t, Lds &s, const uint32_t dyn, const St &st) {
        store_to(a, t, s, dyn, st, a.cur_nbr, a.cur_counts, a.cur_tot, a.cur_perm);
    }

    // space.rs:71-86 act = reassign_color (mod.rs:78-99) + permitted_edges.remove
    __device__ static void act(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const uint32_t aid) { act_body(a, s, dyn, st, aid); }
    __device__ static __forceinline__ void act_body(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const uint32_t aid) {
        const int E = a.E, C = a.C;
        const int e = (int)(aid % (uint32_t)E), nc = (int)(aid / (uint32_t)E);
        const int v = s.ev[e], u = s.eu[e];
        int oc = 0;
        for (int c = 0; c < C; ++c)
            if ((s.nbr[c][u] >> v) & (W)1) oc = c; // ColoredCompleteBitsetGraph::color
        oc = (int)uni((uint32_t)oc);
        int32_t *counts = lds_counts(dyn);
        WAVE_SYNC();
        if (LANE == 0) {
            s.nbr[oc][v] ^= (W)1 << u;
            s.nbr[oc][u] ^= (W)1 << v;
        }
        WAVE_SYNC();
        ramsey_adjust<DEPTH>(s, counts, E, true, u, v, oc, a.sizes[oc]);
        ramsey_adjust<DEPTH>(s, counts, E, false, u, v, nc, a.sizes[nc]);
        WAVE_SYNC();
        if (LANE == 0) {
            s.nbr[nc][v] ^= (W)1 << u;
            s.nbr[nc][u] ^= (W)1 << v;
        }
        const int32_t d_old = counts[oc * E + e], d_new = counts[nc * E + e];
#pragma unroll
        for (int c = 0; c < RAMSEY_MAX_C; ++c) {
            if (c == oc) st.tot[c] -= d_old;
            if (c == nc) st.tot[c] += d_new;
        }
#pragma unroll
        for (int w = 0; w < PW; ++w)
            if ((e >> 6) == w) st.perm[w] &= ~(1ull << (e & 63));
        WAVE_SYNC();
    }
    // space.rs:155-165: sum_c total[c] as f32 * weights[c], in colour order from 0
    __device__ static __forceinline__ float evaluate(const Arenas &a, Lds &, const uint32_t, St &st, const int) {
        float sum = 0.0f;
#pragma unroll
        for (int c = 0; c < RAMSEY_MAX_C; ++c)
            if (c < a.C) sum = sum + (float)st.tot[c] * a.cweights[c];
        return sum;
    }
    __device__ static __forceinline__ bool terminal(const Arenas &, Lds &, const uint32_t, const St &st) {
        return mask_empty<PW>(st.perm);
    }
    // space.rs:122-153 write_vec: [counts C x E][edge bools C x E][permitted E]
    __device__ static void write_vec(const Arenas &a, Lds &s, const uint32_t dyn, const St &st, float *row) {
        const int E = a.E, C = a.C;
        const int32_t *counts = lds_counts(dyn);
#pragma unroll
        for (int w = 0; w < PW; ++w) {
            const int e = w * 64 + LANE;
            if (e < E) {
                const int v = s.ev[e], u = s.eu[e];
                for (int c = 0; c < C; ++c) {
                    row[c * E + e] = (float)counts[c * E + e];
                    row[C * E + c * E + e] = (float)((s.nbr[c][v] >> u) & (W)1);
                }
                row[2 * C * E + e] = (float)((st.perm[w] >> LANE) & 1ull);
            }
        }
    }
    // space.rs:174-177 h_sa = 1 - c_as* / c_as (f32 division through f64: exactly rounded)
    __device__ static __forceinline__ float h_sa(float, float c_as, float c_as_star) {
        const float q = (float)((double)c_as_star / (double)c_as);
        return 1.0f - q;
    }

    // the C - 1 actions of permitted edge e (larger endpoint v) from its colour classes nbv, counts cnv and prediction entries hv in
    // every colour: predictions begin + rank (C - 1) + k
    __device__ static __forceinline__ void edge_actions(const Arenas &a, const int e, const int v, const W (&nbv)[RAMSEY_MAX_C],
                                                        const int32_t (&cnv)[RAMSEY_MAX_C], const float (&hv)[RAMSEY_MAX_C], const float c_s,
                                                        PredRec *preds, const uint32_t begin, const uint32_t rank, FirstPick &fp) {
        const int E = a.E, C = a.C;
        int oc = 0;
#pragma unroll
        for (int c = 0; c < RAMSEY_MAX_C; ++c)
            if (c < C && ((nbv[c] >> v) & (W)1)) oc = c;
        int32_t cnt_oc = cnv[0];
#pragma unroll
        for (int c = 1; c < RAMSEY_MAX_C; ++c) cnt_oc = oc == c ? cnv[c] : cnt_oc;
        float cw_oc = a.cweights[0];
#pragma unroll
        for (int c = 1; c < RAMSEY_MAX_C; ++c) cw_oc = oc == c ? a.cweights[c] : cw_oc; // (a select over the four weights, not a per-lane load)
        const float r_old = (float)cnt_oc * cw_oc;
        uint32_t k = 0;
#pragma unroll
        for (int nc = 0; nc < RAMSEY_MAX_C; ++nc) {
            if (nc >= C || nc == oc) continue;
            const float r_sa = r_old - (float)cnv[nc] * a.cweights[nc];
            const uint32_t a_id = (uint32_t)(e + nc * E);
            const float hh = hv[nc];
            const float g = c_s * hh + r_sa * (1.0f - hh);
            const PredRec p = pred_new(a_id, c_s, g);
            preds[begin + rank * (uint32_t)(C - 1) + k] = p;
            pick_note(fp, __uint_as_float(p.w0), g, rank * (uint32_t)(C - 1) + k, a_id);
            ++k;
        }
    }
    // graph_operations.rs:32-56 with space.rs:88-120 action_data (edges ascending, new colours
    // ascending, a_id = e + new_colour * E) and g = c_s h + r (1 - h), r = old_count w[old] -
    // new_count w[new] (:167-172).  Reads the state from HBM: in the persistent step the dynamic LDS
    // region has been reused by the evaluator by the time this runs.
    template <bool SC1 = false>
    __device__ static __forceinline__ void add_actions(const Arenas &a, Lds &s, const int t, const RolloutOut *hint, RolloutOut *pick) {
        const int E = a.E, C = a.C;
        uint64_t perm[PW];
#pragma unroll
        for (int w = 0; w < PW; ++w) perm[w] = a.cur_perm[(size_t)t * KW + w];
        const uint32_t cnt = (uint32_t)mask_count<PW>(perm) * (uint32_t)(C - 1);
        const uint32_t begin = hint ? hint->n_preds : a.n_preds[t];
        if (!add_actions_fits(a, t, begin, cnt, 64u * CH)) return;
        const uint32_t node = hint ? hint->pos : a.state_pos[t];
        PredRec *preds = a.preds + (size_t)t * a.pred_cap;
        const float c_s = hint ? hint->c : a.nodes[(size_t)t * a.node_cap + node].c;
        const uint2 link = node_link(a, t, node);
        const float *h = a.h_theta + (size_t)t * a.A;
        const W *nbr = reinterpret_cast<const W *>(a.cur_nbr) + (size_t)t * (RAMSEY_MAX_C * NV);
        const int32_t *counts = a.cur_counts + (size_t)t * C * E;
        uint32_t before = 0;
        FirstPick fp;
        fp.key = 0ull;
        fp.aid = 0u;
        fp.g = 0.f;
        if constexpr (CH > PRED_CHUNKS) {
            // wide: a word of 64 edges at a time (every word's requests at once -- 8 words x 4 colours x 3 values -- do not fit the
            // CU-resident forms' 128 registers)
#pragma unroll 1
            for (int w = 0; w < PW; ++w) {
                const uint64_t pw = a.cur_perm[(size_t)t * KW + w];
                const int e = w * 64 + LANE, ec = ((pw >> LANE) & 1ull) ? e : 0;
                const int ev1 = s.ev[ec], eu1 = s.eu[ec];
                W nbv[RAMSEY_MAX_C];
                int32_t cnv[RAMSEY_MAX_C];
                float hv[RAMSEY_MAX_C];
#pragma unroll
                for (int c = 0; c < RAMSEY_MAX_C; ++c) {
                    nbv[c] = 0u;
                    cnv[c] = 0;
                    hv[c] = 0.f;
                    if (c < C) {
                        nbv[c] = nbr[c * NV + eu1];
                        cnv[c] = counts[c * E + ec];
                        hv[c] = SC1 ? ld_sc1_f32(h + (ec + c * E)) : h[ec + c * E];
                    }
                }
                if ((pw >> LANE) & 1ull) {
                    const uint32_t rank = before + (uint32_t)__popcll(pw & ((1ull << LANE) - 1ull));
                    edge_actions(a, e, ev1, nbv, cnv, hv, c_s, preds, begin, rank, fp);
                }
                before += (uint32_t)__popcll(pw);
            }
        } else {
        // Every request first (round 5): an edge's colour classes, its counts and its prediction-row entries in EVERY colour do not depend on
        // which colour it has -- requested edge by edge and colour by colour behind that question they were three dependent round trips per
        // 64 edges, nine at the head of every call of R(4,4).  A lane without a permitted edge in a chunk reads edge 0's (unused).
        W nbv[PW][RAMSEY_MAX_C];
        int32_t cnv[PW][RAMSEY_MAX_C];
        float hv[PW][RAMSEY_MAX_C];
        int ev_[PW], eu_[PW];
#pragma unroll
        for (int w = 0; w < PW; ++w) {
            const int e = w * 64 + LANE, ec = ((perm[w] >> LANE) & 1ull) ? e : 0;
            ev_[w] = s.ev[ec];
            eu_[w] = s.eu[ec];
#pragma unroll
            for (int c = 0; c < RAMSEY_MAX_C; ++c) {
                nbv[w][c] = 0u;
                cnv[w][c] = 0;
                hv[w][c] = 0.f;
                if (c < C) {
                    nbv[w][c] = nbr[c * NV + eu_[w]];
                    cnv[w][c] = counts[c * E + ec];
                    hv[w][c] = SC1 ? ld_sc1_f32(h + (ec + c * E)) : h[ec + c * E];
                }
            }
        }
#pragma unroll
        for (int w = 0; w < PW; ++w) {
            const int e = w * 64 + LANE;
            if ((perm[w] >> LANE) & 1ull) {
                const uint32_t rank = before + (uint32_t)__popcll(perm[w] & ((1ull << LANE) - 1ull));
                const int v = ev_[w];
                int oc = 0;
#pragma unroll
                for (int c = 0; c < RAMSEY_MAX_C; ++c)
                    if (c < C && ((nbv[w][c] >> v) & (W)1)) oc = c;
                int32_t cnt_oc = cnv[w][0];
#pragma unroll
                for (int c = 1; c < RAMSEY_MAX_C; ++c) cnt_oc = oc == c ? cnv[w][c] : cnt_oc;
                float cw_oc = a.cweights[0];
#pragma unroll
                for (int c = 1; c < RAMSEY_MAX_C; ++c) cw_oc = oc == c ? a.cweights[c] : cw_oc; // (a select over the four weights, not a per-lane load)
                const float r_old = (float)cnt_oc * cw_oc;
                uint32_t k = 0;
#pragma unroll
                for (int nc = 0; nc < RAMSEY_MAX_C; ++nc) {
                    if (nc >= C || nc == oc) continue;
                    const float r_sa = r_old - (float)cnv[w][nc] * a.cweights[nc];
                    const uint32_t a_id = (uint32_t)(e + nc * E);
                    const float hh = hv[w][nc];
                    const float g = c_s * hh + r_sa * (1.0f - hh);
                    const PredRec p = pred_new(a_id, c_s, g);
                    preds[begin + rank * (uint32_t)(C - 1) + k] = p;
                    pick_note(fp, __uint_as_float(p.w0), g, rank * (uint32_t)(C - 1) + k, a_id);
                    ++k;
                }
            }
            before += (uint32_t)__popcll(perm[w]);
        }
        }
        add_actions_commit(a, t, node, begin, cnt, hint ? s.ctr : nullptr, link);
        if (pick) pick_finish(fp, begin, cnt, pick);
    }

    // packed root = colour of every edge in colex order (E bytes) + permitted edge mask;
    // RamseyCounts::new (mod.rs:20-68)
    __device__ static float init_root(const Arenas &a, const int t, Lds &s, const uint32_t dyn, const uint8_t *__restrict__ colors,
                                      const uint64_t *__restrict__ permitted, St &st) {
        const int E = a.E, C = a.C;
        W *nb = &s.nbr[0][0];
        nb[LANE] = 0u;
        nb[LANE + 64] = 0u;
        if constexpr (NBL == 4) {
            nb[LANE + 128] = 0u;
            nb[LANE + 192] = 0u;
        }
        WAVE_SYNC();
        for (int e = LANE; e < E; e += 64) {
            const int c = colors[(size_t)t * E + e];
            const int v = s.ev[e], u = s.eu[e];
            atomicOr(nbr_atomic(&s.nbr[c][v]), nbr_atomic_bit(u, (W)0));
            atomicOr(nbr_atomic(&s.nbr[c][u]), nbr_atomic_bit(v, (W)0));
        }
        WAVE_SYNC();
        int32_t *counts = lds_counts(dyn);
        uint32_t part[RAMSEY_MAX_C] = {0u, 0u, 0u, 0u};
        for (int e = LANE; e < E; e += 64) {
            const int v = s.ev[e], u = s.eu[e];
#pragma unroll
            for (int c = 0; c < RAMSEY_MAX_C; ++c) {
                if (c < C) {
                    const W common = s.nbr[c][v] & s.nbr[c][u];
                    const int cnt = cliques_inside<DEPTH>(s.nbr[c], common, a.sizes[c] - 2);
                    counts[c * E + e] = cnt;
                    if ((s.nbr[c][v] >> u) & (W)1) part[c] += (uint32_t)cnt;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < RAMSEY_MAX_C; ++c) {
            st.tot[c] = 0;
            if (c < C) st.tot[c] = (int32_t)(wave_sum_u32(part[c]) / (uint32_t)(a.sizes[c] * (a.sizes[c] - 1) / 2));
        }
#pragma unroll
        for (int w = 0; w < PW; ++w) st.perm[w] = permitted[(size_t)t * KW + w];
        WAVE_SYNC();
        store_to(a, t, s, dyn, st, a.root_nbr, a.root_counts, a.root_tot, a.root_perm);
        store_to(a, t, s, dyn, st, a.cur_nbr, a.cur_counts, a.cur_tot, a.cur_perm);
        return evaluate(a, s, dyn, st, 0);
    }

    // ---- hooks of the device root policy (root_policy.inc)
    static constexpr int UNIVERSE_MAX = ME, SLOT_WORDS_MAX = KW_ > MAX_KW ? KW_ : MAX_KW;
    static constexpr bool SEQ_POLICY = ME == RAMSEY_MAX_E; // (wide engines take ActionSet keys only: the engine refuses the others)
    __device__ static __forceinline__ int policy_universe(const Arenas &a) { return a.E; }
    __device__ static __forceinline__ int root_bytes(const Arenas &a) { return a.E; }
    __device__ static __forceinline__ int permitted_count(const St &st) { return mask_count<PW>(st.perm); }
    // ColoredCompleteBitsetGraph::generate, seeded: colour[e] = below(draw 1024 + e, C) with uniform weights; with colour weights
    // (05-r45.rs:84-90; azd_root_policy::color_weights) the number of thresholds the draw's high word reaches (c21_host.h)
    static constexpr bool WEIGHTED_ROOTS = true; // (fresh_root takes the policy)
    __device__ static __forceinline__ void fresh_root(const Arenas &a, Lds &, uint64_t seed, uint64_t domain, uint64_t agent, uint8_t *po,
                                                      const RootPolicyArgs &rp) {
        for (int e = LANE; e < a.E; e += 64) {
            const uint64_t r = stream_key_dev(seed, domain, agent, 1024 + (uint64_t)e);
            uint32_t col = below_dev(r, (uint32_t)a.C);
            if (rp.weighted) {
                const uint64_t hi = r >> 32;
                col = 0;
#pragma unroll
                for (int c = 0; c < RAMSEY_MAX_C - 1; ++c) col += (c < a.C - 1 && hi >= rp.color_thr[c]) ? 1u : 0u;
            }
            po[e] = (uint8_t)col;
        }
    }
    __device__ static __forceinline__ void pack_root(const Arenas &a, Lds &s, uint8_t *po) {
        for (int e = LANE; e < a.E; e += 64) {
            const int v = s.ev[e], u = s.eu[e];
            int col = 0;
            for (int c = 0; c < a.C; ++c)
                if ((s.nbr[c][v] >> u) & (W)1) col = c;
            po[e] = (uint8_t)col;
        }
    }

    // ArgminData { state, cost: TotalCounts, eval } (log.rs:1-11)
    __device__ static void argmin_out(const Arenas &a, Lds &s, const uint32_t dyn, St &st, const int wt, const uint32_t win_node) {
        const int E = a.E, C = a.C;
        ARG *out = reinterpret_cast<ARG *>(a.argmin_r); // (a wide engine's record is the wide one: engine.hip sizes it)
        for (int e = LANE; e < E; e += 64) {
            const int v = s.ev[e], u = s.eu[e];
            int col = 0;
            for (int c = 0; c < C; ++c)
                if ((s.nbr[c][v] >> u) & (W)1) col = c;
            out->colors[e] = (uint8_t)col;
        }
        const float ev = evaluate(a, s, dyn, st, 0);
        if (LANE == 0) {
#pragma unroll
            for (int w = 0; w < APW; ++w) out->permitted[w] = 0;
#pragma unroll
            for (int w = 0; w < PW; ++w) out->permitted[w] = st.perm[w];
#pragma unroll
            for (int c = 0; c < RAMSEY_MAX_C; ++c) out->totals[c] = st.tot[c];
            out->eval = ev;
            out->agent = wt;
            out->node = win_node;
            a.argmin->eval = ev; // the strict-improvement bound every argmin pass reads
            a.argmin->agent = wt;
            a.argmin->node = win_node;
        }
    }
};

template <int KW_>
struct RamseySpace : RamseySpaceBase<KW_, RAMSEY_MAX_E, RamseyArgminRec, PRED_CHUNKS> {};
template <int KW_>
struct RamseyWideSpace : RamseySpaceBase<KW_, RAMSEY_WIDE_MAX_E, RamseyWideArgminRec, KW_> {
    using Base = RamseySpaceBase<KW_, RAMSEY_WIDE_MAX_E, RamseyWideArgminRec, KW_>;
    static constexpr bool REPLAY_BY_WORD = true; // (tree_core.inc: argmin_replay)
    // Pool step: the state-vector row goes straight to memory (tree_core.inc: ROWS_DIRECT) instead of through an LDS stage behind
    // the counts -- 5.5 KB per searcher wave at r45, 9.9 KB at N = 32, C = 2: sixteen of them are what kept the searcher side of the
    // pool plan beyond 160 KB.  The entries are write_vec's, as 4-byte write-through stores (the request is posted after a drain).
    static constexpr bool ROWS_DIRECT = true;
    static size_t pool_dyn_bytes(const Arenas &a) { return (Base::dyn_bytes(a) + 15) & ~(size_t)15; }
    __device__ static void write_rows_direct(const Arenas &a, typename Base::Lds &s, const uint32_t dyn, const typename Base::St &st, float *row,
                                             uint16_t *) {
        const int E = a.E, C = a.C, CE = a.C * a.E;
        const int32_t *counts = Base::lds_counts(dyn);
        for (int i = LANE; i < CE; i += 64) st_sc1_f32(row + i, (float)counts[i]);
        for (int e = LANE; e < E; e += 64) {
            const int v = s.ev[e], u = s.eu[e];
            for (int c = 0; c < C; ++c) st_sc1_f32(row + CE + c * E + e, (float)((s.nbr[c][v] >> u) & 1u));
        }
#pragma unroll
        for (int w = 0; w < Base::PW; ++w) {
            const int e = w * 64 + LANE;
            if (e < E) st_sc1_f32(row + 2 * CE + e, (float)((st.perm[w] >> LANE) & 1ull));
        }
    }
    // (forced inline: left to its heuristics hipcc outlines it from the widest step kernels -- tools/check_kernels.py)
    __device__ static __forceinline__ void act(const Arenas &a, typename Base::Lds &s, const uint32_t dyn, typename Base::St &st, const uint32_t aid) {
        Base::act_body(a, s, dyn, st, aid);
    }
};

// The 64-bit tier (AZD_ENGINE_RAMSEY_U64): N <= 64 over uint64_t rows, E <= 1128, keys of RAMSEY_U64_KW words (E*C <= 2304) whatever
// the shape.  A node holds up to 64 RAMSEY_U64_CH actions -- NOT tied to the key width as RamseyWideSpace does: at 36 words
// select_big's two lists would be 18 KB per wave.
// (RAMSEY_U64_KW, RAMSEY_U64_CH: engine_types.h)
template <int DEPTH>
struct RamseyU64SpaceT : RamseySpaceBase<RAMSEY_U64_KW, RAMSEY_U64_MAX_E, RamseyU64ArgminRec, RAMSEY_U64_CH, uint64_t, DEPTH> {
    using Base = RamseySpaceBase<RAMSEY_U64_KW, RAMSEY_U64_MAX_E, RamseyU64ArgminRec, RAMSEY_U64_CH, uint64_t, DEPTH>;
    static constexpr bool REPLAY_BY_WORD = true;
    // (write_vec goes straight to the row in memory -- 20 KB at N = 34, four colours -- there is no LDS stage to avoid: the pool step,
    // whose SP::row_stage ROWS_DIRECT replaces, is not built for this tier)
    __device__ static __forceinline__ void act(const Arenas &a, typename Base::Lds &s, const uint32_t dyn, typename Base::St &st, const uint32_t aid) {
        Base::act_body(a, s, dyn, st, aid);
    }
    // space.rs:122-153 write_vec, by entry rather than by permitted word (18 words unrolled over four colours are more code than hipcc
    // inlines: tools/check_kernels.py)
    __device__ static __forceinline__ void write_vec(const Arenas &a, typename Base::Lds &s, const uint32_t dyn, const typename Base::St &st, float *row) {
        const int E = a.E, C = a.C, CE = a.C * a.E;
        const int32_t *counts = Base::lds_counts(dyn);
        for (int i = LANE; i < CE; i += 64) row[i] = (float)counts[i];
        for (int e = LANE; e < E; e += 64) {
            const int v = s.ev[e], u = s.eu[e];
            for (int c = 0; c < C; ++c) row[CE + c * E + e] = (float)((s.nbr[c][v] >> u) & 1ull);
        }
#pragma unroll
        for (int w = 0; w < Base::PW; ++w) {
            const int e = w * 64 + LANE;
            if (e < E) row[2 * CE + e] = (float)((st.perm[w] >> LANE) & 1ull);
        }
    }
};
// Named structs, not aliases: the kernels' names carry them (k_rollout<RamseyU64Space>).  Forbidden cliques up to K5, and up to
// AZD_RAMSEY_BIG_CLIQUE_MAX (AZD_ENGINE_RAMSEY_BIG_CLIQUES: ramsey64_big_kernels.hip, ramsey64_big_ext_kernels.hip).
struct RamseyU64Space : RamseyU64SpaceT<3> {};
struct RamseyU64BigSpace : RamseyU64SpaceT<6> {};

// host side: what the instantiation an engine's key width selects needs of the LDS (the CU-resident forms' plans).  A wide engine's
// keys are padded to 10 or 16 words (engine.hip), a width no narrow engine has (1..6): the key width names the engine's mode.
// (The 64-bit tier's 36 words never come here: its table refuses the CU-resident forms, ramsey64_kernels.hip.)
static inline bool ramsey_wide(const Arenas &a) { return a.KW > MAX_KW; }
static inline size_t ramsey_dyn_bytes(const Arenas &a) {
    return a.KW == 16 ? RamseyWideSpace<16>::dyn_bytes(a) : a.KW == 10 ? RamseyWideSpace<10>::dyn_bytes(a) : RamseySpace<1>::dyn_bytes(a);
}
static inline size_t ramsey_pool_dyn_bytes(const Arenas &a) {
    return a.KW == 16 ? RamseyWideSpace<16>::pool_dyn_bytes(a) : a.KW == 10 ? RamseyWideSpace<10>::pool_dyn_bytes(a) : RamseySpace<1>::pool_dyn_bytes(a);
}
static inline size_t ramsey_lds_bytes(const Arenas &a) { return ramsey_wide(a) ? sizeof(RamseyWideLds) : sizeof(RamseyLds); }

// narrow engines: key widths 1..6; wide engines (max_slots > 0): 10 or 16.  The 64-bit tier's 36 never reach this switch: its engines
// have a table of their own (ramsey64_kernels.hip)
#define DISPATCH_RKW(A, FN, ...)                                  \
    switch ((A).KW) {                                             \
    case 1: FN<RamseySpace<1>>(__VA_ARGS__); break;               \
    case 2: FN<RamseySpace<2>>(__VA_ARGS__); break;               \
    case 3: FN<RamseySpace<3>>(__VA_ARGS__); break;               \
    case 4: FN<RamseySpace<4>>(__VA_ARGS__); break;               \
    case 5: FN<RamseySpace<5>>(__VA_ARGS__); break;               \
    case 10: FN<RamseyWideSpace<10>>(__VA_ARGS__); break;         \
    case 16: FN<RamseyWideSpace<16>>(__VA_ARGS__); break;         \
    default: FN<RamseySpace<6>>(__VA_ARGS__); break;              \
    }
