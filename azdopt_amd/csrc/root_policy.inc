// root_policy.inc -- included after tree_core.inc and a space policy (inside namespace azd).
//
// The drivers' `modify_root` closure (graph-state/examples/04-c21-tree.rs:172-206; the Ramsey
// drivers' 02-r44.rs:196-228 is the same policy over edges) on the device, one wavefront per
// tree, so that the epoch boundary needs no host round trip:
//   n = tree.node_data()  (BTreeMap order: ActionSet keys compared lexicographically over their
//                          ascending elements, a proper prefix first; n[0] is the root)
//   c_root == c_root*:  k == kmax ? fresh random root
//                                 : keep nodes with c == c_root, pick one uniformly, replay its
//                                   path onto the root, k' in k..=kmax
//   else:               keep nodes with c <= (c_root + 3 c_root*)/4, pick one uniformly, replay,
//                       k' in kmin..=kmax
//                       (RootPolicyArgs::rule = ROOT_RULE_BEST: keep nodes with c == c_root* instead -- 05-r45.rs:201,
//                       03-r3333.rs:191; c_root* is the cost of some node, carried up by a cascade, so the kept set is never empty)
//   then re-randomise the permitted set (k' of ACTION_DIM for c21, k' of the E edges for Ramsey).
// "Pick uniformly" = index r = below(draw 0, #kept) into the kept nodes IN KEY ORDER (that is what
// `n.choose` sees); the r-th key in that order is found by an MSB-first radix select over the
// keys' element sequences (digit j = j-th smallest element + 1, 0 = end of sequence), with LDS
// histograms -- no sort.  Seeded draws: DESIGN.md "Seeded generator".


// bits 0..e of a KW-word mask
template <int KW>
__device__ __forceinline__ void mask_le(int e, uint64_t (&m)[KW]) {
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        int hi = e - 64 * w; // highest bit index within this word that is included
        m[w] = hi < 0 ? 0ull : (hi >= 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull));
    }
}

// first k of a Fisher-Yates shuffle of 0..A-1 as a bit mask of `ow` words (modify_parent_once.rs:14-25 stand-in);
// step j swaps j with j + below(draw 64 + j, A - j).  perm_arr [A], draws [k], bm [ow]: LDS scratch.
__device__ void shuffle_permitted(uint64_t seed, uint64_t domain, uint64_t agent, int A, int k, uint32_t *perm_arr,
                                  uint32_t *draws, uint64_t *bm, const int ow, uint64_t *out /* [ow] */) {
    for (int i = LANE; i < A; i += 64) perm_arr[i] = (uint32_t)i;
    for (int j = LANE; j < k; j += 64) draws[j] = (uint32_t)j + below_dev(stream_key_dev(seed, domain, agent, 64 + (uint64_t)j), (uint32_t)(A - j));
    for (int w = LANE; w < ow; w += 64) bm[w] = 0ull;
    WAVE_SYNC();
    if (LANE == 0) {
        for (int j = 0; j < k; ++j) {
            const uint32_t r = draws[j];
            const uint32_t tmp = perm_arr[j];
            perm_arr[j] = perm_arr[r];
            perm_arr[r] = tmp;
            const uint32_t v = perm_arr[j];
            bm[v >> 6] |= 1ull << (v & 63u);
        }
    }
    WAVE_SYNC();
    for (int w = LANE; w < ow; w += 64) out[w] = bm[w];
    WAVE_SYNC();
}

// Sequence-keyed trees (ActionSequence / OrderedActionSet): the search graph is a tree, node v > 0
// was created by arc v - 1, and the BTreeMap order of the keys (lexicographic over the actions in the
// order taken, a prefix first) is the preorder walk that visits siblings by ascending action id.
// The r-th kept node in that order is found by descending with per-subtree counts of kept nodes.
constexpr int POLICY_SEQ_MAX_NODES = 4096;

// What the policy needs from a space is the root-policy set of the space contract (tree_core.inc, SpaceDefaults): SP::UNIVERSE_MAX
// items the permitted set is drawn from, SP::SLOT_WORDS_MAX words of that set's bit mask; SP::slot_words(a) of them are written per
// root to `out_slots` ([B][slot_words]: the host's `permitted` argument of par_new / par_reset_trees).  `out_perm` is what
// k_init_roots takes as its `permitted` argument: the same mask for c21 / Ramsey (out_slots == out_perm), the packed rank table for
// the dense-graph space (SP::finish_root builds it from the new root's graph and slots).
// A space whose fresh roots depend on the policy (SP::WEIGHTED_ROOTS: the Ramsey colour weights) takes it as a last argument.

// what the policy did with tree t (azd_engine_root_policy_report): three words, plain stores of the wave's first lane
__device__ __forceinline__ void policy_report(const RootPolicyArgs &rp, const int t, const uint32_t branch, const uint32_t node,
                                              const uint32_t kept) {
    if (LANE == 0) {
        uint32_t *o = rp.report + (size_t)t * 3;
        o[0] = branch;
        o[1] = node;
        o[2] = kept;
    }
}

template <class SP>
__global__ __launch_bounds__(64) void k_modify_roots(Arenas a, uint64_t seed, uint64_t epoch, uint64_t first_agent, int kmin,
                                                     int kmax, uint8_t *__restrict__ out_parents,
                                                     uint64_t *__restrict__ out_perm, uint64_t *__restrict__ out_slots,
                                                     const RootPolicyArgs rp) {
    constexpr int KW = SP::KW;
    constexpr int CH = SP::CH;
    constexpr int HQ = KW + 1;       // histogram buckets per lane: digits 0 .. 64 KW
    constexpr int HD = 64 * HQ;
    __shared__ typename SP::Lds s;
    __shared__ uint32_t hist[HD];
    __shared__ uint32_t perm_arr[SP::UNIVERSE_MAX];
    __shared__ uint32_t draws[64 * CH];
    __shared__ uint64_t bm[SP::SLOT_WORDS_MAX];
    __shared__ uint32_t sub[SP::SEQ_POLICY ? POLICY_SEQ_MAX_NODES : 1]; // sequence keys: kept nodes per subtree
    const uint32_t dyn = 0;
    const int t = blockIdx.x;
    const int U = SP::policy_universe(a); // what the permitted set is drawn from
    const uint64_t agent = first_agent + (uint64_t)t;
    const uint64_t domain = DOMAIN_RESET_DEV ^ (epoch << 32);
    const NodeRec *nodes = a.nodes + (size_t)t * a.node_cap;
    const uint64_t *keys = a.keys + (size_t)t * a.node_cap * KW;
    const uint32_t nn = a.n_nodes[t];
    uint8_t *po = out_parents + (size_t)t * SP::root_bytes(a);
    const int ow = SP::slot_words(a);
    uint64_t *mo = out_slots + (size_t)t * ow;
    SP::prepare(a, s);
    WAVE_SYNC();
    typename SP::St st;
    SP::load_root(a, t, s, dyn, st);
    WAVE_SYNC();
    const float c_root = nodes[0].c, c_root_star = nodes[0].c_star;
    const uint64_t r0 = stream_key_dev(seed, domain, agent, 0), r1 = stream_key_dev(seed, domain, agent, 1);
    const bool same = c_root == c_root_star;
    const int kcur = SP::permitted_count(st);
    if (same && kcur == kmax) { // *state = a freshly generated root with k permitted
        const int k = kmin + (int)below_dev(r1, (uint32_t)(kmax - kmin + 1));
        if constexpr (SP::WEIGHTED_ROOTS) SP::fresh_root(a, s, seed, domain, agent, po, rp);
        else SP::fresh_root(a, s, seed, domain, agent, po);
        shuffle_permitted(seed, domain, agent, U, k, perm_arr, draws, bm, ow, mo);
        SP::finish_root(a, s, t, po, mo, out_perm);
        policy_report(rp, t, ROOT_BRANCH_FRESH, NONE, 0u);
        return;
    }
    const float three_cs = 3.0f * c_root_star;
    const float thr = (c_root + three_cs) / 4.0f;
    // the nodes the tree keeps: stagnant c == c_root; improved c <= thr, or under ROOT_RULE_BEST c == c_root*
    const bool exact = same || rp.rule == ROOT_RULE_BEST;
    const float c_keep = same ? c_root : c_root_star;
    auto kept = [&](const float c) { return exact ? (c == c_keep) : (c <= thr); };
    const int k_new = same ? kcur + (int)below_dev(r1, (uint32_t)(kmax - kcur + 1)) : kmin + (int)below_dev(r1, (uint32_t)(kmax - kmin + 1));
    // ---- count the kept nodes
    uint32_t m_local = 0;
    for (uint32_t v = LANE; v < nn; v += 64) {
        const float c = nodes[v].c;
        m_local += kept(c) ? 1u : 0u;
    }
    uint32_t m = m_local;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m += __shfl_xor(m, off, 64);
    // (m == 0 is the reference's unwrap() on None.  It cannot happen -- the root itself has c == c_root, some node c == c_root* --
    // but no index is drawn from an empty set: the agent is flagged, the root stays where it is, the host call reports it.)
    if (m == 0 && LANE == 0) {
        a.flags[t] |= FLAG_UNREACHABLE;
        atomicAdd(&a.status->failed, 1ull);
    }
    uint32_t r = m ? below_dev(r0, m) : 0u;
    uint32_t chosen = 0; // node id of the chosen key
    // ---- radix select of the r-th kept key in BTreeMap order
    uint64_t prefix[KW], le[KW];
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        prefix[w] = 0;
        le[w] = 0; // elements <= last chosen element (none yet)
    }
    if (m == 0) { // nothing to choose from: the key stays the root's
    } else if (SP::SEQ_POLICY && a.path_kind == PATH_SEQUENCE) {
        const ArcRec *arcs = a.arcs + (size_t)t * a.arc_cap;
        const PredRec *preds = a.preds + (size_t)t * a.pred_cap;
        for (uint32_t v = LANE; v < nn; v += 64) {
            const float c = nodes[v].c;
            sub[v] = kept(c) ? 1u : 0u;
        }
        WAVE_SYNC();
        // children have larger indices than their parents: one backward pass accumulates the subtrees
        for (int base = (int)((nn - 1) & ~63u); base >= 0; base -= 64) {
            const uint32_t v = (uint32_t)base + (uint32_t)LANE;
            uint32_t par = 0;
            if (v >= 1 && v < nn) par = arcs[v - 1].src;
            for (int i = 63; i >= 0; --i) {
                const uint32_t vi = (uint32_t)(base + i);
                if (vi >= 1 && vi < nn) {
                    const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)par, i);
                    if (LANE == 0) sub[p] += sub[vi];
                }
            }
        }
        WAVE_SYNC();
        uint32_t u = 0, rr = r;
        for (uint32_t guard = 0; guard <= nn; ++guard) {
            const NodeRec ru = nodes[u];
            if (kept(ru.c)) {
                if (rr == 0) break; // u is the chosen node
                rr -= 1;
            }
            const uint32_t nact = ru.act_end - ru.act_begin;
            PredRec p0, p1;
            p0.w0 = 0; p0.w1 = 0; p0.w2 = NONE; p0.w3 = 0;
            p1 = p0;
            if ((uint32_t)LANE < nact) p0 = preds[ru.act_begin + (uint32_t)LANE];
            if ((uint32_t)LANE + 64u < nact) p1 = preds[ru.act_begin + 64u + (uint32_t)LANE];
            uint32_t last = 0; // action ids + 1 already passed
            uint32_t next_u = NONE;
            for (uint32_t it = 0; it < nact && next_u == NONE; ++it) {
                uint32_t k0 = (pred_expanded(p0) && pred_aid(p0) + 1u > last) ? pred_aid(p0) + 1u : 0xFFFFFFFFu;
                uint32_t k1 = (pred_expanded(p1) && pred_aid(p1) + 1u > last) ? pred_aid(p1) + 1u : 0xFFFFFFFFu;
                const uint32_t km = wave_min_u32(k0 < k1 ? k0 : k1);
                if (km == 0xFFFFFFFFu) break;
                const bool mine0 = k0 == km, mine1 = k1 == km;
                const int src = first_lane(__ballot(mine0 || mine1));
                const uint32_t ch = rdlane(mine0 ? pred_child(p0) : pred_child(p1), src);
                const uint32_t cnt = sub[ch];
                if (rr < cnt) next_u = ch;
                else rr -= cnt;
                last = km;
            }
            if (next_u == NONE) break; // cannot happen: rr < kept nodes below u
            u = next_u;
        }
#pragma unroll
        for (int w = 0; w < KW; ++w) prefix[w] = keys[(size_t)u * KW + w];
        chosen = u;
    } else {
    for (int j = 0; j <= 64 * CH + 1; ++j) { // a key holds at most one action per permitted item
        for (int i = LANE; i < HD; i += 64) hist[i] = 0;
        WAVE_SYNC();
        for (uint32_t base = 0; base < nn; base += 64) {
            const uint32_t v = base + (uint32_t)LANE;
            if (v < nn) {
                const float c = nodes[v].c;
                bool cand = kept(c);
                uint64_t k[KW];
                int d = 0;
                bool found = false;
#pragma unroll
                for (int w = 0; w < KW; ++w) {
                    k[w] = keys[(size_t)v * KW + w];
                    cand = cand && ((k[w] & le[w]) == prefix[w]);
                    const uint64_t rest = k[w] & ~le[w];
                    if (!found && rest) {
                        d = 64 * w + (__ffsll((unsigned long long)rest) - 1) + 1;
                        found = true;
                    }
                }
                if (cand) atomicAdd(&hist[d], 1u);
            }
        }
        WAVE_SYNC();
        // smallest digit whose cumulative count exceeds r (digits 0 .. 64 KW; HQ per lane)
        uint32_t h4[HQ], sum4 = 0;
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            h4[q] = hist[LANE * HQ + q];
            sum4 += h4[q];
        }
        uint32_t incl = sum4; // inclusive scan over lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t o = __shfl_up(incl, off, 64);
            if (LANE >= off) incl += o;
        }
        const uint32_t excl = incl - sum4;
        const bool mine = (r >= excl) && (r < incl);
        const int src = first_lane(__ballot(mine));
        // r relative to lane `src`'s four buckets, then walk them
        uint32_t rr = (uint32_t)__shfl((int)(r - excl), src, 64);
        int dsel = 0;
        bool done = false;
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const uint32_t hq = (uint32_t)__shfl((int)h4[q], src, 64);
            if (!done) {
                if (rr < hq) {
                    dsel = src * HQ + q;
                    done = true;
                } else rr -= hq;
            }
        }
        r = rr;
        WAVE_SYNC();
        if (dsel == 0) break; // end of sequence: the chosen key is exactly `prefix`
        const int e = dsel - 1;
        prefix[e >> 6] |= 1ull << (e & 63);
        mask_le<KW>(e, le);
    }
    // the node that holds the chosen key (keys are unique within a tree), for the report
    uint32_t found = NONE;
    for (uint32_t base = 0; base < nn; base += 64) {
        const uint32_t v = base + (uint32_t)LANE;
        bool eq = v < nn;
        if (eq) {
#pragma unroll
            for (int w = 0; w < KW; ++w) eq = eq && keys[(size_t)v * KW + w] == prefix[w];
        }
        if (eq && v < found) found = v;
    }
    chosen = wave_min_u32(found);
    }
    // ---- p.actions_taken().for_each(|a| space.act(state, &a))   (ascending)
#pragma unroll
    for (int w = 0; w < KW; ++w) {
        uint64_t bits = prefix[w];
        while (bits) {
            const int b = __ffsll((unsigned long long)bits) - 1;
            bits &= bits - 1;
            SP::act(a, s, dyn, st, SP::bit_action(s, (uint32_t)(w * 64 + b)));
        }
    }
    SP::pack_root(a, s, po);
    shuffle_permitted(seed, domain, agent, U, k_new, perm_arr, draws, bm, ow, mo); // randomize_permitted_actions / _edges
    SP::finish_root(a, s, t, po, mo, out_perm);
    policy_report(rp, t, same ? ROOT_BRANCH_STAGNANT : ROOT_BRANCH_IMPROVED, chosen, m);
}
