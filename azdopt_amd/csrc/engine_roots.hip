// engine_roots.hip -- the root policy: the device policy's entry points, the policy's description, and the c21 policy on the host.
#include "engine_impl.h"

extern "C" {

// the report of the policy launch the stream has completed: an empty kept set (k_modify_roots left that tree's root where it was)
static int root_report_check(azd_engine *e) {
    e->root_report_valid = true;
    for (int t = 0; t < e->a.B; ++t)
        if (e->root_report[(size_t)t * 3] != (uint32_t)azd::ROOT_BRANCH_FRESH && e->root_report[(size_t)t * 3 + 2] == 0) {
            char buf[128];
            snprintf(buf, sizeof(buf), "root policy: tree %d keeps no node (the reference's unwrap() on None)", t);
            azd::g_last_error = buf;
            return AZD_ERR_UNREACHABLE;
        }
    return AZD_OK;
}

// par_reset_trees with the c21 driver's modify_root policy (04-c21-tree.rs:172-206) evaluated on the
// device: no host round trip at the epoch boundary.
static int c21_policy_args_ok(azd_engine *e, int kmin, int kmax) {
    if (!e || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (e->a.space == azd::SPACE_DENSE) {
        if (e->a.path_kind == azd::PATH_SEQUENCE) {
            azd::g_last_error = "the device root policy of the dense-graph space handles ActionSet keys only";
            return AZD_ERR_UNSUPPORTED;
        }
        if (kmin < 1 || kmax < kmin || kmax > e->a.E || kmax > e->dense_slots) {
            azd::g_last_error = "dense root policy: need 1 <= kmin <= kmax <= min(E, 64 * key words) (azd_engine_config::max_slots)";
            return AZD_ERR_INVALID_ARGUMENT;
        }
        return AZD_OK;
    }
    if (e->a.path_kind == azd::PATH_SEQUENCE && e->a.node_cap > 4096) {
        azd::g_last_error = "the device root policy handles sequence-keyed trees of at most 4096 nodes";
        return AZD_ERR_UNSUPPORTED;
    }
    if (e->a.space == azd::SPACE_RAMSEY) { // the node cap: max_slots edges on a wide engine, MAX_NODE_ACTIONS / (C - 1) otherwise
        if (kmin < 1 || kmax < kmin || kmax > e->a.E || kmax > e->ramsey_slots) {
            if (e->tier->cap_from_slots) azd::g_last_error = "Ramsey root policy: need 1 <= kmin <= kmax <= max_slots (azd_engine_config::max_slots)";
            return AZD_ERR_INVALID_ARGUMENT;
        }
        return AZD_OK;
    }
    if (kmin < 1 || kmax < kmin || kmax > e->a.A || kmax > azd::MAX_NODE_ACTIONS) return AZD_ERR_INVALID_ARGUMENT;
    return AZD_OK;
}
int azd_engine_par_reset_trees_c21(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax) {
    AZD_ST(c21_policy_args_ok(e, kmin, kmax));
    if (!e->ev) return AZD_ERR_NO_EVALUATOR;
    AZD_ENTER(e);
    const azd::Arenas &a = e->a;
    e->root_report_valid = false;
    e->ops->modify_roots(a, seed, epoch, e->cfg.first_agent, kmin, kmax, e->d_stage_parents, e->d_stage_perm, e->d_stage_slots, e->root_args,
                         e->stream);
    AZD_HIP(hipMemsetAsync(&a.status->failed, 0, sizeof(unsigned long long), e->stream));
    e->ops->init_roots(a, e->d_stage_parents, e->d_stage_perm, e->stream);
    AZD_HIP(hipMemsetAsync(a.h_theta, 0, (size_t)a.B * a.A * 4, e->stream));
    AZD_HIP(hipGetLastError());
    AZD_ST(run_evaluator(e));
    e->ops->add_actions(e->a, 1, e->stream); // reset_finish, with the policy's report read back under the same synchronisation
    AZD_HIP(hipMemcpyAsync(e->root_report, e->d_root_report, (size_t)e->a.B * 3 * 4, hipMemcpyDeviceToHost, e->stream));
    AZD_ST(sync_status(e));
    return root_report_check(e);
}
int azd_c21_modify_roots_dev(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax, uint8_t *parents_out,
                             uint64_t *permitted_out) {
    AZD_ST(c21_policy_args_ok(e, kmin, kmax));
    if (!parents_out || !permitted_out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    const azd::Arenas &a = e->a;
    e->root_report_valid = false;
    e->ops->modify_roots(a, seed, epoch, e->cfg.first_agent, kmin, kmax, e->d_stage_parents, e->d_stage_perm, e->d_stage_slots, e->root_args,
                         e->stream);
    AZD_HIP(hipMemcpyAsync(e->root_report, e->d_root_report, (size_t)e->a.B * 3 * 4, hipMemcpyDeviceToHost, e->stream));
    if (a.space == azd::SPACE_DENSE) { // roots_out: neighbourhoods (8 n bytes per root); permitted_out: slot masks in kw_host words per root
        const int ow = (a.E + 63) / 64;
        std::vector<uint64_t> sl((size_t)a.B * ow);
        AZD_HIP(hipMemcpyAsync(parents_out, e->d_stage_parents, (size_t)a.B * a.n * 8, hipMemcpyDeviceToHost, e->stream));
        AZD_HIP(hipMemcpyAsync(sl.data(), e->d_stage_slots, sl.size() * 8, hipMemcpyDeviceToHost, e->stream));
        AZD_HIP(hipStreamSynchronize(e->stream));
        AZD_HIP(hipGetLastError());
        memset(permitted_out, 0, (size_t)a.B * e->kw_host * 8);
        for (int i = 0; i < a.B; ++i) memcpy(permitted_out + (size_t)i * e->kw_host, &sl[(size_t)i * ow], (size_t)ow * 8);
        return root_report_check(e);
    }
    AZD_HIP(hipMemcpyAsync(parents_out, e->d_stage_parents, (size_t)a.B * (a.space == azd::SPACE_RAMSEY ? a.E : a.n), hipMemcpyDeviceToHost, e->stream));
    if (e->tier->padded_keys) { // device masks are a.KW words, the caller's kw_host
        std::vector<uint64_t> pm((size_t)a.B * a.KW);
        AZD_HIP(hipMemcpyAsync(pm.data(), e->d_stage_perm, pm.size() * 8, hipMemcpyDeviceToHost, e->stream));
        AZD_HIP(hipStreamSynchronize(e->stream));
        for (int i = 0; i < a.B; ++i) memcpy(permitted_out + (size_t)i * e->kw_host, &pm[(size_t)i * a.KW], (size_t)e->kw_host * 8);
    } else AZD_HIP(hipMemcpyAsync(permitted_out, e->d_stage_perm, (size_t)a.B * a.KW * 8, hipMemcpyDeviceToHost, e->stream));
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipGetLastError());
    return root_report_check(e);
}

// ---- the policy's description (include/azdopt_amd.h: azd_root_policy)
int azd_root_policy_check(int space_id, int n_colors, const azd_root_policy *p) {
    if (!p) return AZD_OK; // the defaults
    if (p->rule != AZD_ROOT_RULE_THRESHOLD && p->rule != AZD_ROOT_RULE_BEST) {
        azd::g_last_error = "rule: AZD_ROOT_RULE_THRESHOLD or AZD_ROOT_RULE_BEST";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (p->n_color_weights == 0) return AZD_OK;
    if (space_id != AZD_SPACE_RAMSEY) {
        azd::g_last_error = "color_weights: only an AZD_SPACE_RAMSEY engine colours its fresh roots";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (p->n_color_weights != n_colors) {
        azd::g_last_error = "n_color_weights: 0 or the engine's n_colors";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (const char *why = azd::ramsey_check_color_weights(p->color_weights, n_colors)) {
        azd::g_last_error = why;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    return AZD_OK;
}
int azd_engine_set_root_policy(azd_engine *e, const azd_root_policy *p) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ST(azd_root_policy_check(e->a.space, e->a.C, p));
    const azd_root_policy defaults{AZD_ROOT_RULE_THRESHOLD, 0, {0.0, 0.0, 0.0, 0.0}};
    e->root_policy = p ? *p : defaults;
    for (int c = e->root_policy.n_color_weights; c < 4; ++c) e->root_policy.color_weights[c] = 0.0;
    e->root_args.rule = e->root_policy.rule;
    e->root_args.weighted = e->root_policy.n_color_weights != 0;
    for (int c = 0; c < azd::RAMSEY_COLOR_THRESHOLDS; ++c) e->root_args.color_thr[c] = 1ull << 32;
    if (e->root_args.weighted) azd::ramsey_color_thresholds(e->root_policy.color_weights, e->a.C, e->root_args.color_thr);
    return AZD_OK;
}
int azd_engine_get_root_policy(const azd_engine *e, azd_root_policy *p) {
    if (!p) return AZD_ERR_INVALID_ARGUMENT;
    const azd_root_policy defaults{AZD_ROOT_RULE_THRESHOLD, 0, {0.0, 0.0, 0.0, 0.0}};
    *p = e ? e->root_policy : defaults;
    return AZD_OK;
}
int azd_engine_root_policy_report(azd_engine *e, uint8_t *branch, uint32_t *node, uint32_t *kept) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (!e->root_report_valid) {
        azd::g_last_error = "root policy report: no policy call has completed on this engine";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    for (int t = 0; t < e->a.B; ++t) {
        if (branch) branch[t] = (uint8_t)e->root_report[(size_t)t * 3];
        if (node) node[t] = e->root_report[(size_t)t * 3 + 1];
        if (kept) kept[t] = e->root_report[(size_t)t * 3 + 2];
    }
    return AZD_OK;
}

// space-neutral names of the two entry points above (the policy is the same for both spaces)
int azd_engine_par_reset_trees_policy(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax) {
    return azd_engine_par_reset_trees_c21(e, seed, epoch, kmin, kmax);
}
int azd_engine_modify_roots_dev(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax, uint8_t *roots_out,
                                uint64_t *permitted_out) {
    return azd_c21_modify_roots_dev(e, seed, epoch, kmin, kmax, roots_out, permitted_out);
}

// ------------------------------------------------------------------ c21 root policy (host)
// 04-c21-tree.rs:172-206 applied to node_data() (tree/mod.rs:302-307: BTreeMap order, i.e. keys
// compared lexicographically over their ascending elements; n[0] is the root).
static bool key_less(const uint64_t *x, const uint64_t *y, int KW) {
    // d = lowest differing action id; the set holding d is smaller iff the other has an element > d
    for (int w = 0; w < KW; ++w) {
        uint64_t diff = x[w] ^ y[w];
        if (!diff) continue;
        int b = __builtin_ctzll(diff);
        bool x_has = (x[w] >> b) & 1ull;
        const uint64_t *other = x_has ? y : x;
        bool other_has_more = (b < 63 ? (other[w] >> (b + 1)) != 0 : false);
        for (int w2 = w + 1; w2 < KW && !other_has_more; ++w2) other_has_more = other[w2] != 0;
        // x_has: x < y iff y continues; else y has d: x < y iff x does NOT continue (x is a proper prefix)
        return x_has ? other_has_more : !other_has_more;
    }
    return false;
}

int azd_c21_modify_roots(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax, uint8_t *parents_out,
                         uint64_t *permitted_out) {
    if (!e || !parents_out || !permitted_out || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (e->a.space != azd::SPACE_C21 || e->a.path_kind != azd::PATH_SET) return AZD_ERR_UNSUPPORTED;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    const azd::Arenas &a = e->a;
    const int B = a.B, KW = a.KW, n = a.n;
    std::vector<uint32_t> n_nodes((size_t)B);
    AZD_HIP(hipMemcpy(n_nodes.data(), a.n_nodes, (size_t)B * 4, hipMemcpyDeviceToHost));
    std::vector<uint8_t> rp((size_t)B * azd::PARENTS_STRIDE);
    std::vector<uint64_t> rm((size_t)B * KW);
    AZD_HIP(hipMemcpy(rp.data(), a.root_parents, rp.size(), hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(rm.data(), a.root_perm, rm.size() * 8, hipMemcpyDeviceToHost));
    uint32_t max_nodes = 0;
    for (uint32_t v : n_nodes) max_nodes = std::max(max_nodes, v);
    std::vector<azd::NodeRec> nodes((size_t)max_nodes);
    std::vector<uint64_t> keys((size_t)max_nodes * KW);
    const uint64_t domain = azd::DOMAIN_RESET ^ (epoch << 32);
    // (parent, child) of an action id
    auto act = [&](uint8_t *par, uint64_t *perm, int aid) {
        int c = 2;
        while (c * (c + 1) / 2 - 1 <= aid) ++c;
        int p = aid - (c * (c - 1) / 2 - 1);
        par[c] = (uint8_t)p;
        for (int u = 0; u < c; ++u) {
            int id = c * (c - 1) / 2 + u - 1;
            perm[id >> 6] &= ~(1ull << (id & 63));
        }
    };
    std::vector<uint32_t> keep;
    for (int i = 0; i < B; ++i) {
        const uint64_t agent = e->cfg.first_agent + (uint64_t)i;
        const uint32_t nn = n_nodes[(size_t)i];
        AZD_HIP(hipMemcpy(nodes.data(), a.nodes + (size_t)i * a.node_cap, (size_t)nn * sizeof(azd::NodeRec), hipMemcpyDeviceToHost));
        AZD_HIP(hipMemcpy(keys.data(), a.keys + (size_t)i * a.node_cap * KW, (size_t)nn * KW * 8, hipMemcpyDeviceToHost));
        uint8_t par[azd::PARENTS_STRIDE];
        uint64_t perm[azd::MAX_KW] = {0, 0, 0, 0};
        memcpy(par, &rp[(size_t)i * azd::PARENTS_STRIDE], azd::PARENTS_STRIDE);
        for (int w = 0; w < KW; ++w) perm[w] = rm[(size_t)i * KW + w];
        uint8_t *po = parents_out + (size_t)i * n;
        uint64_t *mo = permitted_out + (size_t)i * KW;
        const float c_root = nodes[0].c, c_root_star = nodes[0].c_star;
        const uint64_t r0 = azd::stream_key(seed, domain, agent, 0), r1 = azd::stream_key(seed, domain, agent, 1);
        int k_new;
        keep.clear();
        if (c_root == c_root_star) {
            int kcur = 0;
            for (int w = 0; w < KW; ++w) kcur += __builtin_popcountll(perm[w]);
            if (kcur == kmax) {
                int k = kmin + (int)azd::draw_below(r1, (uint32_t)(kmax - kmin + 1));
                azd::c21_fresh_root(seed, domain, agent, n, k, po, mo);
                continue;
            }
            for (uint32_t v = 0; v < nn; ++v)
                if (nodes[v].c == c_root) keep.push_back(v);
            k_new = kcur + (int)azd::draw_below(r1, (uint32_t)(kmax - kcur + 1));
        } else {
            const float thr = (c_root + 3.0f * c_root_star) / 4.0f;
            for (uint32_t v = 0; v < nn; ++v)
                if (nodes[v].c <= thr) keep.push_back(v);
            k_new = kmin + (int)azd::draw_below(r1, (uint32_t)(kmax - kmin + 1));
        }
        const uint32_t r = azd::draw_below(r0, (uint32_t)keep.size());
        std::nth_element(keep.begin(), keep.begin() + r, keep.end(), [&](uint32_t x, uint32_t y) {
            return key_less(&keys[(size_t)x * KW], &keys[(size_t)y * KW], KW);
        });
        const uint64_t *key = &keys[(size_t)keep[r] * KW];
        for (int w = 0; w < KW; ++w) {
            uint64_t bits = key[w];
            while (bits) {
                int b = __builtin_ctzll(bits);
                bits &= bits - 1;
                act(par, perm, w * 64 + b);
            }
        }
        memcpy(po, par, (size_t)n);
        azd::c21_shuffle_permitted(seed, domain, agent, n, k_new, mo);
    }
    return AZD_OK;
}
} // extern "C"
