// engine_readback.hip -- the read-back entries: argmin records, agent state, exported trees, counters, timing, what the last launch did.
#include "engine_impl.h"

// One of the Ramsey argmin records (the ABI's structs included) from another, field for field: the colours and masks the smaller of
// the two holds, zeros beyond them
template <typename Dst, typename Src>
static void ramsey_rec_copy(Dst *d, const Src &s) {
    memset(d, 0, sizeof(*d));
    memcpy(d->colors, s.colors, std::min(sizeof(d->colors), sizeof(s.colors)));
    memcpy(d->permitted, s.permitted, std::min(sizeof(d->permitted), sizeof(s.permitted)));
    memcpy(d->totals, s.totals, sizeof(d->totals));
    d->eval = s.eval;
    d->agent = s.agent;
    d->node = s.node;
}
template <typename Rec>
static int ramsey_rec_fetch(const void *src, azd::RamseyU64ArgminRec *out) {
    Rec r;
    AZD_HIP(hipMemcpy(&r, src, sizeof(r), hipMemcpyDeviceToHost));
    ramsey_rec_copy(out, r);
    return AZD_OK;
}
// the engine's Ramsey argmin record, whichever of the three the tier's kernels write, as the largest one
static int ramsey_argmin_fetch(azd_engine *e, azd::RamseyU64ArgminRec *out) {
    AZD_HIP(hipSetDevice(e->cfg.device));
    bool side = false; // inside a run-ahead window: the record as of the calls handed out so far
    AZD_ST(window_argmin_side(e, &side));
    AZD_HIP(hipStreamSynchronize(e->stream));
    const void *src = side ? (const void *)e->d_argmin_r_side : (const void *)e->a.argmin_r;
    switch (e->tier->id) {
    case TIER_RAMSEY_U64:
    case TIER_RAMSEY_U64_BIG: return ramsey_rec_fetch<azd::RamseyU64ArgminRec>(src, out);
    case TIER_RAMSEY_WIDE: return ramsey_rec_fetch<azd::RamseyWideArgminRec>(src, out);
    default: return ramsey_rec_fetch<azd::RamseyArgminRec>(src, out);
    }
}
// the two typed entries: any Ramsey engine whose edges fit the struct's colours
template <typename Abi>
static int ramsey_argmin_typed(azd_engine *e, Abi *out, const char *too_many_edges) {
    if (!e || !out || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (e->a.space != azd::SPACE_RAMSEY) return AZD_ERR_UNSUPPORTED;
    if (e->a.E > (int)sizeof(out->colors)) {
        azd::g_last_error = too_many_edges;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::RamseyU64ArgminRec r;
    AZD_ST(ramsey_argmin_fetch(e, &r));
    ramsey_rec_copy(out, r);
    return AZD_OK;
}

// What an entry says to the engine of a recipe tier (TierDesc::family) it does not serve: "<entry>: an <flag> engine's <thing> is
// <done> with <with>", the flag and `with` the names of the engine's own family (dense_cost_host.h: DenseFamilyDesc)
static std::string other_family(const char *entry, const char *flag, const char *thing_is_done, const char *with) {
    return std::string(entry) + ": an " + flag + " engine's " + thing_is_done + " with " + with;
}
// The dense argmin entries: `reads` is the tier whose record the entry copies out, `refusal` its text for an engine of another
// tier -- said to an engine with the Aouchiche-Hansen cost (an engine without it is refused without a text), by the wide entry and
// the recipe tiers' to all.  The engine of a recipe tier is told its own tier's reader by every entry; the two Aouchiche-Hansen
// tiers name each other's.
static int dense_argmin_read(azd_engine *e, void *out, Tier reads, size_t bytes, const char *refusal) {
    if (!e || !out || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (e->tier->id != reads) {
        if (const azd::DenseFamilyDesc *f = e->tier->family)
            azd::g_last_error = other_family("dense argmin read", f->flag[e->tier->wide], "record is read", f->argmin_reader[e->tier->wide]);
        else if (e->tier->ah || (reads != TIER_DENSE && reads != TIER_DENSE_AH)) azd::g_last_error = refusal;
        return AZD_ERR_UNSUPPORTED;
    }
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipMemcpy(out, e->a.argmin_d, bytes, hipMemcpyDeviceToHost));
    return AZD_OK;
}
// The entries of the three recipe costs (dense_cost_host.h: DenseFamily), at either row limit: the indices are checked at the engine's n.
// The recipe: checked, then copied -- the caller's bytes -- behind the per-agent doubles of cur_lambda, where the tier's kernels read it
// (dense_spectral.inc: DenseCostRecipeT::recipe); the engine keeps it widened
template <azd::DenseFamily F>
static int set_recipe(azd_engine *e, const typename azd::DenseFamilyOf<F>::Recipe *r) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    const azd::DenseFamilyDesc &f = azd::dense_family(F), *const theirs = e->tier->family;
    if (theirs != &f) {
        azd::g_last_error = theirs ? other_family(f.setter, theirs->flag[0], "recipe is set", theirs->setter) : std::string(f.setter) + ": not an " + f.flag[0] + " engine";
        return AZD_ERR_UNSUPPORTED;
    }
    if (e->inv_recipe_locked) {
        azd::g_last_error = std::string(f.setter) + ": par_new has run: the trees' evals were computed with the recipe in force, which stays";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    if (const char *why = azd::dense_check_recipe<F>(r, e->a.n)) {
        azd::g_last_error = std::string(f.setter) + ": " + why;
        return AZD_ERR_INVALID_ARGUMENT;
    }
    AZD_HIP(hipSetDevice(e->cfg.device));
    AZD_HIP(hipMemcpy(e->a.cur_lambda + (size_t)f.count * e->a.B, r, sizeof(*r), hipMemcpyHostToDevice));
    e->inv_recipe = azd::dense_widen_recipe(*r);
    e->inv_recipe_set = true;
    return AZD_OK;
}
// An agent's record: the kept invariants, and cost and eval from them by the device's combination, operation for operation
// (dense_recipe_combine)
template <azd::DenseFamily F>
static int agent_cost(azd_engine *e, int agent, typename azd::DenseFamilyOf<F>::Cost *out) {
    if (!e || !out || agent < 0 || agent >= e->a.B) return AZD_ERR_INVALID_ARGUMENT;
    const azd::DenseFamilyDesc &f = azd::dense_family(F), *const theirs = e->tier->family;
    if (theirs != &f) {
        azd::g_last_error =
            theirs ? other_family(f.agent_cost, theirs->flag[0], "record is read", theirs->agent_cost) : std::string(f.agent_cost) + ": not an " + f.flag[0] + " engine";
        return AZD_ERR_UNSUPPORTED;
    }
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    const azd::Arenas &a = e->a;
    for (int i = 0; i < f.count; ++i) AZD_HIP(hipMemcpy(&out->inv[i], a.cur_lambda + (size_t)i * a.B + agent, 8, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&out->dist_k, a.cur_mu + agent, 4, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&out->computed, a.cur_mu + a.B + agent, 4, hipMemcpyDeviceToHost));
    azd::dense_recipe_combine(e->inv_recipe, out->inv, f.count, &out->cost, &out->eval);
    return AZD_OK;
}

extern "C" {

static_assert(sizeof(azd_ramsey_argmin) == sizeof(azd::RamseyArgminRec) && sizeof(azd_ramsey_wide_argmin) == sizeof(azd::RamseyWideArgminRec),
              "ABI struct mismatch");
static_assert(sizeof(azd_ramsey_argmin::colors) == 256 && sizeof(azd_ramsey_wide_argmin::colors) == 496, "the edge counts the refusals name");
int azd_engine_ramsey_argmin_data(azd_engine *e, azd_ramsey_argmin *out) {
    return ramsey_argmin_typed(e, out, "E > 256 edges do not fit azd_ramsey_argmin: use azd_engine_ramsey_wide_argmin_data");
}
int azd_engine_ramsey_wide_argmin_data(azd_engine *e, azd_ramsey_wide_argmin *out) {
    return ramsey_argmin_typed(e, out, "E > 496 edges do not fit azd_ramsey_wide_argmin: use azd_engine_ramsey_argmin_any");
}
int azd_engine_ramsey_argmin_any(azd_engine *e, uint8_t *colors, int colors_cap, uint64_t *permitted, int permitted_words_cap,
                                 int32_t *totals, float *eval, int32_t *agent, uint32_t *node) {
    if (!e || !e->initialised || colors_cap < 0 || permitted_words_cap < 0) return AZD_ERR_INVALID_ARGUMENT;
    if (e->a.space != azd::SPACE_RAMSEY) return AZD_ERR_UNSUPPORTED;
    const int PWH = (e->a.E + 63) / 64;
    if ((colors && colors_cap < e->a.E) || (permitted && permitted_words_cap < PWH)) {
        azd::g_last_error = "azd_engine_ramsey_argmin_any: need colors_cap >= E bytes and permitted_words_cap >= (E + 63) / 64 words";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    azd::RamseyU64ArgminRec r;
    AZD_ST(ramsey_argmin_fetch(e, &r));
    if (colors) {
        memset(colors, 0, (size_t)colors_cap);
        memcpy(colors, r.colors, (size_t)e->a.E);
    }
    if (permitted) {
        memset(permitted, 0, (size_t)permitted_words_cap * 8);
        memcpy(permitted, r.permitted, (size_t)PWH * 8);
    }
    if (totals) memcpy(totals, r.totals, sizeof(r.totals));
    if (eval) *eval = r.eval;
    if (agent) *agent = r.agent;
    if (node) *node = r.node;
    return AZD_OK;
}
static_assert(sizeof(azd_dense_argmin) == sizeof(azd::DenseArgminRec) && sizeof(azd_dense_ah_argmin) == sizeof(azd::DenseAhArgminRec) &&
                  sizeof(azd_dense_ah_wide_argmin) == sizeof(azd::DenseAhWideArgminRec) &&
                  offsetof(azd_dense_ah_wide_argmin, node) == offsetof(azd::DenseAhWideArgminRec, node) &&
                  sizeof(azd_dense_inv_argmin) == sizeof(azd::DenseInvArgminRec) && offsetof(azd_dense_inv_argmin, node) == offsetof(azd::DenseInvArgminRec, node) &&
                  offsetof(azd_dense_inv_argmin, inv) == offsetof(azd::DenseInvArgminRec, inv) &&
                  sizeof(azd_dense_inv_wide_argmin) == sizeof(azd::DenseInvWideArgminRec) &&
                  offsetof(azd_dense_inv_wide_argmin, node) == offsetof(azd::DenseInvWideArgminRec, node) &&
                  offsetof(azd_dense_inv_wide_argmin, inv) == offsetof(azd::DenseInvWideArgminRec, inv) &&
                  sizeof(azd_dense_invx_argmin) == sizeof(azd::DenseInvxArgminRec) && offsetof(azd_dense_invx_argmin, node) == offsetof(azd::DenseInvxArgminRec, node) &&
                  offsetof(azd_dense_invx_argmin, inv) == offsetof(azd::DenseInvxArgminRec, inv) &&
                  sizeof(azd_dense_invx_wide_argmin) == sizeof(azd::DenseInvxWideArgminRec) &&
                  offsetof(azd_dense_invx_wide_argmin, node) == offsetof(azd::DenseInvxWideArgminRec, node) &&
                  offsetof(azd_dense_invx_wide_argmin, inv) == offsetof(azd::DenseInvxWideArgminRec, inv) &&
                  sizeof(azd_dense_invx_recipe) == sizeof(azd::DenseInvxRecipe) && offsetof(azd_dense_invx_recipe, n_terms) == offsetof(azd::DenseInvxRecipe, n_terms) &&
                  offsetof(azd_dense_invx_recipe, term) == offsetof(azd::DenseInvxRecipe, term) && sizeof(azd_dense_invx_term) == sizeof(azd::DenseInvxTerm) &&
                  offsetof(azd_dense_invx_term, op) == offsetof(azd::DenseInvxTerm, op) &&
                  sizeof(azd_dense_invx_cost_t) == sizeof(azd::DenseInvxCost) && offsetof(azd_dense_invx_cost_t, eval) == offsetof(azd::DenseInvxCost, eval) &&
                  sizeof(azd_dense_invs_argmin) == sizeof(azd::DenseInvsArgminRec) && offsetof(azd_dense_invs_argmin, node) == offsetof(azd::DenseInvsArgminRec, node) &&
                  offsetof(azd_dense_invs_argmin, inv) == offsetof(azd::DenseInvsArgminRec, inv) &&
                  sizeof(azd_dense_invs_wide_argmin) == sizeof(azd::DenseInvsWideArgminRec) &&
                  offsetof(azd_dense_invs_wide_argmin, node) == offsetof(azd::DenseInvsWideArgminRec, node) &&
                  offsetof(azd_dense_invs_wide_argmin, inv) == offsetof(azd::DenseInvsWideArgminRec, inv) &&
                  sizeof(azd_dense_invs_recipe) == sizeof(azd::DenseInvsRecipe) && offsetof(azd_dense_invs_recipe, n_terms) == offsetof(azd::DenseInvsRecipe, n_terms) &&
                  offsetof(azd_dense_invs_recipe, term) == offsetof(azd::DenseInvsRecipe, term) &&
                  sizeof(azd_dense_invs_cost_t) == sizeof(azd::DenseInvsCost) && offsetof(azd_dense_invs_cost_t, eval) == offsetof(azd::DenseInvsCost, eval) &&
                  sizeof(azd_dense_inv_recipe) == sizeof(azd::DenseInvRecipe) && offsetof(azd_dense_inv_recipe, eval_scale) == offsetof(azd::DenseInvRecipe, eval_scale) &&
                  sizeof(azd_dense_inv_cost_t) == sizeof(azd::DenseInvCost) && offsetof(azd_dense_inv_cost_t, eval) == offsetof(azd::DenseInvCost, eval),
              "ABI struct mismatch");
int azd_engine_dense_argmin_data(azd_engine *e, azd_dense_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE, sizeof(*out),
                             "azd_engine_dense_argmin_data: an AZD_ENGINE_DENSE_AH engine's record is read with azd_engine_dense_ah_argmin_data");
}
int azd_engine_dense_ah_argmin_data(azd_engine *e, azd_dense_ah_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_AH, sizeof(*out),
                             "azd_engine_dense_ah_argmin_data: an AZD_ENGINE_DENSE_AH_WIDE engine's record is read with azd_engine_dense_ah_wide_argmin_data");
}
int azd_engine_dense_ah_wide_argmin_data(azd_engine *e, azd_dense_ah_wide_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_AH_WIDE, sizeof(*out), "azd_engine_dense_ah_wide_argmin_data: not an AZD_ENGINE_DENSE_AH_WIDE engine");
}
int azd_engine_dense_inv_argmin_data(azd_engine *e, azd_dense_inv_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_INV, sizeof(*out), "azd_engine_dense_inv_argmin_data: not an AZD_ENGINE_DENSE_INV engine");
}
int azd_engine_dense_inv_wide_argmin_data(azd_engine *e, azd_dense_inv_wide_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_INV_WIDE, sizeof(*out), "azd_engine_dense_inv_wide_argmin_data: not an AZD_ENGINE_DENSE_INV_WIDE engine");
}
int azd_engine_set_dense_inv_recipe(azd_engine *e, const azd_dense_inv_recipe *recipe) {
    return set_recipe<azd::DENSE_FAMILY_INV>(e, reinterpret_cast<const azd::DenseInvRecipe *>(recipe));
}
int azd_engine_dense_inv_agent_cost(azd_engine *e, int agent, azd_dense_inv_cost_t *out) {
    return agent_cost<azd::DENSE_FAMILY_INV>(e, agent, reinterpret_cast<azd::DenseInvCost *>(out));
}
int azd_engine_dense_invx_argmin_data(azd_engine *e, azd_dense_invx_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_INVX, sizeof(*out), "azd_engine_dense_invx_argmin_data: not an AZD_ENGINE_DENSE_INVX engine");
}
int azd_engine_dense_invx_wide_argmin_data(azd_engine *e, azd_dense_invx_wide_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_INVX_WIDE, sizeof(*out), "azd_engine_dense_invx_wide_argmin_data: not an AZD_ENGINE_DENSE_INVX_WIDE engine");
}
int azd_engine_set_dense_invx_recipe(azd_engine *e, const azd_dense_invx_recipe *recipe) {
    return set_recipe<azd::DENSE_FAMILY_INVX>(e, reinterpret_cast<const azd::DenseInvxRecipe *>(recipe));
}
int azd_engine_dense_invx_agent_cost(azd_engine *e, int agent, azd_dense_invx_cost_t *out) {
    return agent_cost<azd::DENSE_FAMILY_INVX>(e, agent, reinterpret_cast<azd::DenseInvxCost *>(out));
}
int azd_engine_dense_invs_argmin_data(azd_engine *e, azd_dense_invs_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_INVS, sizeof(*out), "azd_engine_dense_invs_argmin_data: not an AZD_ENGINE_DENSE_INVS engine");
}
int azd_engine_dense_invs_wide_argmin_data(azd_engine *e, azd_dense_invs_wide_argmin *out) {
    return dense_argmin_read(e, out, TIER_DENSE_INVS_WIDE, sizeof(*out), "azd_engine_dense_invs_wide_argmin_data: not an AZD_ENGINE_DENSE_INVS_WIDE engine");
}
int azd_engine_set_dense_invs_recipe(azd_engine *e, const azd_dense_invs_recipe *recipe) {
    return set_recipe<azd::DENSE_FAMILY_INVS>(e, reinterpret_cast<const azd::DenseInvsRecipe *>(recipe));
}
int azd_engine_dense_invs_agent_cost(azd_engine *e, int agent, azd_dense_invs_cost_t *out) {
    return agent_cost<azd::DENSE_FAMILY_INVS>(e, agent, reinterpret_cast<azd::DenseInvsCost *>(out));
}
int azd_engine_dense_ah_agent_cost(azd_engine *e, int agent, azd_dense_ah_cost_t *out) {
    if (!e || !out || agent < 0 || agent >= e->a.B) return AZD_ERR_INVALID_ARGUMENT;
    if (const azd::DenseFamilyDesc *f = e->tier->family) azd::g_last_error = other_family("azd_engine_dense_ah_agent_cost", f->flag[0], "record is read", f->agent_cost);
    if (!e->tier->ah) return AZD_ERR_UNSUPPORTED;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    const azd::Arenas &a = e->a;
    AZD_HIP(hipMemcpy(&out->proximity, a.cur_lambda + agent, 8, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&out->eigenvalue, a.cur_lambda + a.B + agent, 8, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&out->diameter, a.cur_mu + agent, 4, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&out->k, a.cur_mu + a.B + agent, 4, hipMemcpyDeviceToHost));
    out->cost = (float)(out->proximity + out->eigenvalue);
    out->eval = a.eval_slope * (out->cost + 2.0f);
    return AZD_OK;
}
int azd_engine_ramsey_agent_counts(azd_engine *e, int agent, int32_t *counts, int32_t *totals) {
    if (!e || agent < 0 || agent >= e->a.B) return AZD_ERR_INVALID_ARGUMENT;
    if (e->a.space != azd::SPACE_RAMSEY) return AZD_ERR_UNSUPPORTED;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    const azd::Arenas &a = e->a;
    if (counts) AZD_HIP(hipMemcpy(counts, a.cur_counts + (size_t)agent * a.C * a.E, (size_t)a.C * a.E * 4, hipMemcpyDeviceToHost));
    if (totals) AZD_HIP(hipMemcpy(totals, a.cur_tot + (size_t)agent * 4, 16, hipMemcpyDeviceToHost));
    return AZD_OK;
}

int azd_engine_argmin_data(azd_engine *e, azd_argmin *out) {
    if (!e || !out || !e->initialised) return AZD_ERR_INVALID_ARGUMENT;
    if (e->a.space != azd::SPACE_C21) return AZD_ERR_UNSUPPORTED;
    AZD_HIP(hipSetDevice(e->cfg.device));
    bool side = false; // inside a run-ahead window: the record as of the calls handed out so far
    AZD_ST(window_argmin_side(e, &side));
    static_assert(sizeof(azd_argmin) == sizeof(azd::ArgminRec), "ABI struct mismatch");
    AZD_HIP(hipMemcpyAsync(e->h_argmin, side ? e->d_argmin_side : e->a.argmin, sizeof(azd::ArgminRec), hipMemcpyDeviceToHost, e->stream));
    AZD_HIP(hipStreamSynchronize(e->stream));
    memcpy(out, e->h_argmin, sizeof(azd_argmin));
    return AZD_OK;
}

int azd_engine_read_state_vecs(azd_engine *e, float *out) {
    if (!e || !out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipMemcpy(out, e->a.state_vecs, (size_t)e->a.B * e->a.S * 4, hipMemcpyDeviceToHost));
    return AZD_OK;
}
int azd_engine_read_predictions(azd_engine *e, float *out) {
    if (!e || !out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipMemcpy(out, e->a.h_theta, (size_t)e->a.B * e->a.A * 4, hipMemcpyDeviceToHost));
    return AZD_OK;
}

int azd_engine_tree_sizes(azd_engine *e, int agent, int *n_nodes, int *n_arcs, int *n_preds) {
    if (!e || agent < 0 || agent >= e->a.B) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    uint32_t v[3];
    AZD_HIP(hipMemcpy(&v[0], e->a.n_nodes + agent, 4, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&v[1], e->a.n_arcs + agent, 4, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(&v[2], e->a.n_preds + agent, 4, hipMemcpyDeviceToHost));
    if (n_nodes) *n_nodes = (int)v[0];
    if (n_arcs) *n_arcs = (int)v[1];
    if (n_preds) *n_preds = (int)v[2];
    return AZD_OK;
}

int azd_engine_export_tree(azd_engine *e, int agent, float *c, float *c_star, uint32_t *n_t, uint32_t *exhausted,
                           uint32_t *act_begin, uint32_t *act_end, uint64_t *keys, uint32_t *arc_src,
                           uint32_t *arc_dst, uint32_t *arc_pp, uint32_t *pred_a_id, float *pred_g,
                           int32_t *pred_arc) {
    int nn, na, np;
    AZD_ST(azd_engine_tree_sizes(e, agent, &nn, &na, &np));
    const azd::Arenas &a = e->a;
    std::vector<azd::NodeRec> nodes((size_t)nn);
    std::vector<azd::ArcRec> arcs((size_t)na);
    std::vector<azd::PredRec> preds((size_t)np);
    AZD_HIP(hipMemcpy(nodes.data(), a.nodes + (size_t)agent * a.node_cap, nodes.size() * sizeof(azd::NodeRec), hipMemcpyDeviceToHost));
    if (na) AZD_HIP(hipMemcpy(arcs.data(), a.arcs + (size_t)agent * a.arc_cap, arcs.size() * sizeof(azd::ArcRec), hipMemcpyDeviceToHost));
    if (np) AZD_HIP(hipMemcpy(preds.data(), a.preds + (size_t)agent * a.pred_cap, preds.size() * sizeof(azd::PredRec), hipMemcpyDeviceToHost));
    std::vector<float> g_exp((size_t)np); // g of the expanded predictions (the record holds the child's summary in its place)
    if (np) AZD_HIP(hipMemcpy(g_exp.data(), a.pred_g + (size_t)agent * a.pred_cap, g_exp.size() * 4, hipMemcpyDeviceToHost));
    if (keys && a.space == azd::SPACE_DENSE) { // device keys are sets of RANKS: back to action-id sets (kw_host words per node)
        const int KW = a.KW, MAXS = e->dense_slots;
        std::vector<uint64_t> rk((size_t)nn * KW);
        std::vector<uint16_t> tab((size_t)MAXS);
        AZD_HIP(hipMemcpy(rk.data(), a.keys + (size_t)agent * a.node_cap * KW, rk.size() * 8, hipMemcpyDeviceToHost));
        AZD_HIP(hipMemcpy(tab.data(), a.root_aid + (size_t)agent * MAXS, tab.size() * 2, hipMemcpyDeviceToHost));
        memset(keys, 0, (size_t)nn * e->kw_host * 8);
        for (int i = 0; i < nn; ++i)
            for (int r = 0; r < MAXS; ++r)
                if ((rk[(size_t)i * KW + (r >> 6)] >> (r & 63)) & 1ull) keys[(size_t)i * e->kw_host + (tab[(size_t)r] >> 6)] |= 1ull << (tab[(size_t)r] & 63);
    } else if (keys && e->tier->padded_keys) { // zero-padded device keys: the first kw_host words of each
        std::vector<uint64_t> rk((size_t)nn * a.KW);
        AZD_HIP(hipMemcpy(rk.data(), a.keys + (size_t)agent * a.node_cap * a.KW, rk.size() * 8, hipMemcpyDeviceToHost));
        for (int i = 0; i < nn; ++i) memcpy(keys + (size_t)i * e->kw_host, &rk[(size_t)i * a.KW], (size_t)e->kw_host * 8);
    } else if (keys) AZD_HIP(hipMemcpy(keys, a.keys + (size_t)agent * a.node_cap * a.KW, (size_t)nn * a.KW * 8, hipMemcpyDeviceToHost));
    for (int i = 0; i < nn; ++i) {
        if (c) c[i] = nodes[(size_t)i].c;
        if (c_star) c_star[i] = nodes[(size_t)i].c_star;
        if (n_t) n_t[i] = azd::node_nt(nodes[(size_t)i]);
        if (exhausted) exhausted[i] = azd::node_exhausted(nodes[(size_t)i]);
        if (act_begin) act_begin[i] = nodes[(size_t)i].act_begin;
        if (act_end) act_end[i] = nodes[(size_t)i].act_end;
    }
    for (int i = 0; i < na; ++i) {
        if (arc_src) arc_src[i] = arcs[(size_t)i].src;
        if (arc_dst) arc_dst[i] = arcs[(size_t)i].dst;
        if (arc_pp) arc_pp[i] = arcs[(size_t)i].pp;
    }
    for (int i = 0; i < np; ++i) {
        const azd::PredRec &pr = preds[(size_t)i];
        const bool ex = azd::pred_expanded(pr);
        if (pred_a_id) pred_a_id[i] = azd::pred_aid(pr);
        if (pred_g) {
            const uint32_t gb = pr.w1;
            float gv;
            memcpy(&gv, &gb, 4);
            pred_g[i] = ex ? g_exp[(size_t)i] : gv;
        }
        if (pred_arc) pred_arc[i] = ex ? (int32_t)azd::pred_arc(pr) : -1;
    }
    return AZD_OK;
}

int azd_engine_agent_state(azd_engine *e, int agent, uint8_t *parents, uint64_t *permitted, uint64_t *path,
                           uint32_t *state_pos, double *lambda_1, int *matching_size) {
    if (!e || agent < 0 || agent >= e->a.B) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    const azd::Arenas &a = e->a;
    if (a.space == azd::SPACE_DENSE) { // `parents` receives the neighbourhoods (8 n bytes); masks are kw_host words
        if (e->tier->family && (lambda_1 || matching_size)) {
            const azd::DenseFamilyDesc &f = *e->tier->family;
            azd::g_last_error = std::string("azd_engine_agent_state: lambda_1 / matching_size: an ") + f.flag[0] + " engine keeps neither (" + f.agent_cost + ")";
            return AZD_ERR_UNSUPPORTED;
        }
        if (e->tier->ah && (lambda_1 || matching_size)) {
            azd::g_last_error = "azd_engine_agent_state: lambda_1 / matching_size: an AZD_ENGINE_DENSE_AH engine keeps neither (azd_engine_dense_ah_agent_cost)";
            return AZD_ERR_UNSUPPORTED;
        }
        const int KW = a.KW, MAXS = e->dense_slots;
        std::vector<uint16_t> tab((size_t)MAXS);
        uint64_t rem[16], pth[16];
        AZD_HIP(hipMemcpy(tab.data(), a.root_aid + (size_t)agent * MAXS, tab.size() * 2, hipMemcpyDeviceToHost));
        AZD_HIP(hipMemcpy(rem, a.cur_perm + (size_t)agent * KW, (size_t)KW * 8, hipMemcpyDeviceToHost));
        AZD_HIP(hipMemcpy(pth, a.cur_path + (size_t)agent * KW, (size_t)KW * 8, hipMemcpyDeviceToHost));
        if (parents) AZD_HIP(hipMemcpy(parents, a.cur_adj + (size_t)agent * 64, (size_t)a.n * 8, hipMemcpyDeviceToHost));
        if (permitted) memset(permitted, 0, (size_t)e->kw_host * 8);
        if (path) memset(path, 0, (size_t)e->kw_host * 8);
        for (int r = 0; r < MAXS; ++r) {
            if (permitted && ((rem[r >> 6] >> (r & 63)) & 1ull)) { // open SLOTS, as in the packed root
                const int slot = tab[(size_t)r] % a.E;
                permitted[slot >> 6] |= 1ull << (slot & 63);
            }
            if (path && ((pth[r >> 6] >> (r & 63)) & 1ull)) path[tab[(size_t)r] >> 6] |= 1ull << (tab[(size_t)r] & 63);
        }
        if (state_pos) AZD_HIP(hipMemcpy(state_pos, a.state_pos + agent, 4, hipMemcpyDeviceToHost));
        if (lambda_1) AZD_HIP(hipMemcpy(lambda_1, a.cur_lambda + agent, 8, hipMemcpyDeviceToHost));
        if (matching_size) AZD_HIP(hipMemcpy(matching_size, a.cur_mu + agent, 4, hipMemcpyDeviceToHost));
        return AZD_OK;
    }
    if (a.space == azd::SPACE_RAMSEY) { // `parents` receives the colour of every edge (E bytes)
        uint32_t nbr[512]; // [4][32] uint32_t rows, or the 64-bit tier's [4][64] uint64_t rows
        const bool u64 = e->tier->id == TIER_RAMSEY_U64 || e->tier->id == TIER_RAMSEY_U64_BIG;
        AZD_HIP(hipMemcpy(nbr, a.cur_nbr + (size_t)agent * e->tier->nbr_words, e->tier->nbr_words * 4, hipMemcpyDeviceToHost));
        if (parents) {
            int pos = 0;
            for (int v = 0; v < a.n; ++v)
                for (int u = 0; u < v; ++u, ++pos) {
                    parents[pos] = 0;
                    for (int c = 0; c < a.C; ++c)
                        if (u64 ? (nbr[2 * (c * 64 + v) + (u >> 5)] >> (u & 31)) & 1u : (nbr[c * 32 + v] >> u) & 1u) parents[pos] = (uint8_t)c;
                }
        }
        // (kw_host words: a wide engine's device masks are zero-padded beyond them)
        if (permitted) AZD_HIP(hipMemcpy(permitted, a.cur_perm + (size_t)agent * a.KW, (size_t)e->kw_host * 8, hipMemcpyDeviceToHost));
        if (path) AZD_HIP(hipMemcpy(path, a.cur_path + (size_t)agent * a.KW, (size_t)e->kw_host * 8, hipMemcpyDeviceToHost));
        if (state_pos) AZD_HIP(hipMemcpy(state_pos, a.state_pos + agent, 4, hipMemcpyDeviceToHost));
        if (lambda_1) *lambda_1 = 0.0;
        if (matching_size) *matching_size = 0;
        return AZD_OK;
    }
    uint8_t par[azd::PARENTS_STRIDE];
    AZD_HIP(hipMemcpy(par, a.cur_parents + (size_t)agent * azd::PARENTS_STRIDE, azd::PARENTS_STRIDE, hipMemcpyDeviceToHost));
    if (parents) memcpy(parents, par, (size_t)a.n);
    if (permitted) AZD_HIP(hipMemcpy(permitted, a.cur_perm + (size_t)agent * a.KW, (size_t)a.KW * 8, hipMemcpyDeviceToHost));
    if (path) AZD_HIP(hipMemcpy(path, a.cur_path + (size_t)agent * a.KW, (size_t)a.KW * 8, hipMemcpyDeviceToHost));
    if (state_pos) AZD_HIP(hipMemcpy(state_pos, a.state_pos + agent, 4, hipMemcpyDeviceToHost));
    if (lambda_1) AZD_HIP(hipMemcpy(lambda_1, a.cur_lambda + agent, 8, hipMemcpyDeviceToHost));
    if (matching_size) AZD_HIP(hipMemcpy(matching_size, a.cur_mu + agent, 4, hipMemcpyDeviceToHost));
    return AZD_OK;
}

int azd_engine_counters(azd_engine *e, uint64_t *out) {
    if (!e || !out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    const azd::Arenas &a = e->a;
    std::vector<unsigned long long> h((size_t)a.B * azd::NUM_COUNTERS);
    std::vector<uint32_t> fl((size_t)a.B);
    AZD_HIP(hipMemcpy(h.data(), a.counters, h.size() * 8, hipMemcpyDeviceToHost));
    AZD_HIP(hipMemcpy(fl.data(), a.flags, fl.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < AZD_CTR_COUNT; ++k) out[k] = 0;
    for (int i = 0; i < a.B; ++i) {
        for (int k = 0; k < azd::NUM_COUNTERS; ++k) {
            unsigned long long v = h[(size_t)i * azd::NUM_COUNTERS + k];
            if (k >= AZD_CTR_COUNT) continue;
            if (k == AZD_CTR_MAX_FRONTIER || k == AZD_CTR_MAX_DEPTH || k == AZD_CTR_TICKS_MAX_CALL) out[k] = std::max<uint64_t>(out[k], v);
            else out[k] += v;
        }
    }
    uint64_t failed = 0;
    for (uint32_t f : fl) failed += f != 0;
    out[AZD_CTR_FAILED_AGENTS] = failed;
    return AZD_OK;
}

int azd_engine_agent_counters(azd_engine *e, uint64_t *out) {
    if (!e || !out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipMemcpy(out, e->a.counters, (size_t)e->a.B * azd::NUM_COUNTERS * 8, hipMemcpyDeviceToHost));
    return AZD_OK;
}
int azd_engine_agent_counters_per_agent(azd_engine *e) { return e ? (e->counters_by_wave ? 0 : 1) : AZD_ERR_INVALID_ARGUMENT; }

int azd_engine_set_timing(azd_engine *e, int enabled) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    e->timing = enabled != 0;
    e->rollout_ms = e->evaluator_ms = 0;
    e->rollout_launches = 0;
    return AZD_OK;
}
int azd_engine_timing(azd_engine *e, double *tree_ms, double *evaluator_ms, uint64_t *tree_launches) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (tree_ms) *tree_ms = e->rollout_ms;
    if (evaluator_ms) *evaluator_ms = e->evaluator_ms;
    if (tree_launches) *tree_launches = e->rollout_launches;
    return AZD_OK;
}
void *azd_engine_stream(azd_engine *e) { return e ? (void *)e->stream : nullptr; }
int azd_engine_pool_utilisation(azd_engine *e, double *eval_busy, double *search_busy) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (eval_busy) *eval_busy = e->pool_util_eval;
    if (search_busy) *search_busy = e->pool_util_search;
    return AZD_OK;
}
int azd_engine_pool_groups(azd_engine *e, int *members, int *groups, int *waves_per_slot) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (members) *members = e->pool_grp_g;
    if (groups) *groups = e->pool_grp_groups;
    if (waves_per_slot) *waves_per_slot = e->pool_grp_w;
    return AZD_OK;
}
int azd_engine_pool_agent_finish(azd_engine *e, uint64_t *ticks_out) {
    if (!e || !ticks_out) return AZD_ERR_INVALID_ARGUMENT;
    AZD_ENTER(e);
    if (!e->pool.stamp) {
        azd::g_last_error = "pool_agent_finish: this engine has run no pool step";
        return AZD_ERR_INVALID_ARGUMENT;
    }
    AZD_HIP(hipStreamSynchronize(e->stream));
    AZD_HIP(hipMemcpy(ticks_out, e->pool.stamp, (size_t)e->a.B * 8, hipMemcpyDeviceToHost));
    return AZD_OK;
}
int azd_engine_pool_split(azd_engine *e, int *eval_wgs, int *search_wgs) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (eval_wgs) *eval_wgs = e->pool_eval_wgs;
    if (search_wgs) *search_wgs = e->pool_search_wgs;
    return AZD_OK;
}
int azd_engine_step_form(azd_engine *e, int *form, const char **reason) {
    if (!e) return AZD_ERR_INVALID_ARGUMENT;
    if (form) *form = e->step_form;
    if (reason) *reason = e->step_reason.c_str();
    return AZD_OK;
}
} // extern "C"
