"""Every read-back entry of the C ABI on one engine of every tier, at the smallest shapes: which entry serves which tier, which
refuses it with which status and text, and that the typed Ramsey records and the exported keys have the layout the header gives.
The tiers: c21; Ramsey narrow, wide (max_slots > 0) and 64-bit (AZD_ENGINE_RAMSEY_U64); the dense-graph space with its default cost,
with the Aouchiche-Hansen cost (AZD_ENGINE_DENSE_AH) and with that cost's 64-row form (AZD_ENGINE_DENSE_AH_WIDE).  The six tiers
of the dense-graph space that take a recipe (AZD_ENGINE_DENSE_INV, _INVX, _INVS, each with its _WIDE form) have a test of their
own below: every setter, reader and argmin entry on an engine of every one of them, with the whole text of each refusal."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, 1, 8  # AZD_OK, AZD_ERR_INVALID_ARGUMENT, AZD_ERR_UNSUPPORTED
TOL = ([200, 50, 50], 25)
B = 16
TIERS = ("c21", "ramsey", "ramsey_wide", "ramsey_u64", "dense", "dense_ah", "dense_ah_wide")
RAMSEY = ("ramsey", "ramsey_wide", "ramsey_u64")

T_DENSE = "azd_engine_dense_argmin_data: an AZD_ENGINE_DENSE_AH engine's record is read with azd_engine_dense_ah_argmin_data"
T_AH = "azd_engine_dense_ah_argmin_data: an AZD_ENGINE_DENSE_AH_WIDE engine's record is read with azd_engine_dense_ah_wide_argmin_data"
T_AH_WIDE = "azd_engine_dense_ah_wide_argmin_data: not an AZD_ENGINE_DENSE_AH_WIDE engine"
T_STATE = "azd_engine_agent_state: lambda_1 / matching_size: an AZD_ENGINE_DENSE_AH engine keeps neither (azd_engine_dense_ah_agent_cost)"
T_NARROW = "E > 256 edges do not fit azd_ramsey_argmin: use azd_engine_ramsey_wide_argmin_data"
T_WIDE = "E > 496 edges do not fit azd_ramsey_wide_argmin: use azd_engine_ramsey_argmin_any"

U, UD, UA, UW, US = UNSUPPORTED, (UNSUPPORTED, T_DENSE), (UNSUPPORTED, T_AH), (UNSUPPORTED, T_AH_WIDE), (UNSUPPORTED, T_STATE)
# entry -> what it returns on an engine of each tier, in TIERS' order: a status, or (status, azd_last_error) where it refuses with a text
MATRIX = {
    #                            c21  ramsey  wide  u64  dense  ah   ah_wide
    "argmin_data":              (OK,  U,      U,    U,   U,     U,   U),
    "ramsey_argmin_data":       (U,   OK,     OK,   OK,  U,     U,   U),
    "ramsey_wide_argmin_data":  (U,   OK,     OK,   OK,  U,     U,   U),
    "ramsey_argmin_any":        (U,   OK,     OK,   OK,  U,     U,   U),
    "dense_argmin_data":        (U,   U,      U,    U,   OK,    UD,  UD),
    "dense_ah_argmin_data":     (U,   U,      U,    U,   U,     OK,  UA),
    "dense_ah_wide_argmin_data": (UW, UW,     UW,   UW,  UW,    UW,  OK),
    "agent_state":              (OK,  OK,     OK,   OK,  OK,    OK,  OK),
    "agent_state_cost":         (OK,  OK,     OK,   OK,  OK,    US,  US),
    "ramsey_agent_counts":      (U,   OK,     OK,   OK,  U,     U,   U),
    "dense_ah_agent_cost":      (U,   U,      U,    U,   U,     OK,  OK),
    "export_tree":              (OK,  OK,     OK,   OK,  OK,    OK,  OK),
}


def make_space(az, tier):
    if tier == "c21":
        return az.ROTModifyParentsOnce(5)
    if tier in RAMSEY:
        return az.RamseySpaceNoEdgeRecolor(6, [3, 3], max_slots=0 if tier == "ramsey" else 15, u64=tier == "ramsey_u64")
    return az.DenseGraphSpace(8, cost="c21" if tier == "dense" else "ah", ah_wide=tier == "dense_ah_wide")


@pytest.fixture(scope="module")
def engines():
    import azdopt_amd as az
    if az.device_count() < 1:
        pytest.fail("no gfx950 device: the GPU tests need the HIP path")
    out = {}
    for tier in TIERS:
        space = make_space(az, tier)
        model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, 1)
        opt = az.NablaOptimizer.par_new(space, space.generate_roots(1, B), model, B, node_capacity=256)
        for _ in range(2):
            opt.par_roll_out_episodes(TOL, n_calls=1)
        assert opt.counters()["FAILED"] == 0
        out[tier] = opt
    assert [out[t].space.tier for t in RAMSEY] == ["narrow", "wide", "u64"]
    return out


def export_keys(opt):
    """azd_engine_export_tree of agent 0 with the keys alone: (status, keys [nodes, KEY_WORDS], the guard words behind them)"""
    from azdopt_amd import _lib
    nn, kw = opt.tree_sizes(0)[0], opt.space.KEY_WORDS
    buf = np.full(nn * kw + 8, ~np.uint64(0), np.uint64)
    args = [None] * 13
    args[6] = _lib.ptr(buf)
    st = opt._L.azd_engine_export_tree(opt._h, 0, *args)
    return st, buf[:nn * kw].reshape(nn, kw), buf[nn * kw:]


def call(opt, entry):
    """one read-back entry on one engine: (status, what it wrote)"""
    from azdopt_amd import _lib
    L, h, sp = opt._L, opt._h, opt.space
    rec_of = {"argmin_data": _lib.Argmin, "ramsey_argmin_data": _lib.RamseyArgmin, "ramsey_wide_argmin_data": _lib.RamseyWideArgmin,
              "dense_argmin_data": _lib.DenseArgmin, "dense_ah_argmin_data": _lib.DenseAhArgmin,
              "dense_ah_wide_argmin_data": _lib.DenseAhWideArgmin}
    if entry in rec_of:
        rec = rec_of[entry]()
        return getattr(L, "azd_engine_" + entry)(h, C.byref(rec)), rec
    if entry == "ramsey_argmin_any":
        colors, permitted, totals = np.zeros(2016, np.uint8), np.zeros(32, np.uint64), np.zeros(4, np.int32)
        ev, agent, node = C.c_float(), C.c_int32(), C.c_uint32()
        st = L.azd_engine_ramsey_argmin_any(h, _lib.ptr(colors), len(colors), _lib.ptr(permitted), len(permitted), _lib.ptr(totals),
                                            C.byref(ev), C.byref(agent), C.byref(node))
        return st, dict(colors=colors, permitted=permitted, totals=totals, eval=ev.value, agent=agent.value, node=node.value)
    if entry in ("agent_state", "agent_state_cost"):
        parents, permitted, path = np.zeros(sp.ROOT_BYTES, np.uint8), np.zeros(sp.KEY_WORDS, np.uint64), np.zeros(sp.KEY_WORDS, np.uint64)
        pos, lam, mu = C.c_uint32(), C.c_double(), C.c_int32()
        cost = entry == "agent_state_cost"
        st = L.azd_engine_agent_state(h, 0, _lib.ptr(parents), _lib.ptr(permitted), _lib.ptr(path), C.byref(pos),
                                      C.byref(lam) if cost else None, C.byref(mu) if cost else None)
        return st, None
    if entry == "ramsey_agent_counts":
        counts, totals = np.zeros(4 * 2016, np.int32), np.zeros(4, np.int32)
        return L.azd_engine_ramsey_agent_counts(h, 0, _lib.ptr(counts), _lib.ptr(totals)), None
    if entry == "dense_ah_agent_cost":
        c = _lib.DenseAhCost()
        return L.azd_engine_dense_ah_agent_cost(h, 0, C.byref(c)), c
    assert entry == "export_tree"
    return export_keys(opt)[0], None


def test_every_read_back_entry_on_every_tier_gives_its_status_and_text(engines):
    for entry, row in MATRIX.items():
        for tier, want in zip(TIERS, row):
            st, _ = call(engines[tier], entry)
            status, text = want if isinstance(want, tuple) else (want, None)
            assert st == status, (entry, tier, st, status)
            if text is not None:
                assert engines[tier]._L.azd_last_error().decode() == text, (entry, tier)


@pytest.mark.parametrize("tier", RAMSEY)
def test_typed_ramsey_records_equal_the_any_entry_field_for_field(engines, tier):
    opt = engines[tier]
    E, pw = opt.space.E, (opt.space.E + 63) // 64
    st, a = call(opt, "ramsey_argmin_any")
    assert st == OK and not a["colors"][E:].any() and not a["permitted"][pw:].any()
    assert a["totals"][:2].sum() > 0  # (six vertices, two colours: some triangle is monochromatic)
    for entry in ("ramsey_argmin_data", "ramsey_wide_argmin_data"):
        st, rec = call(opt, entry)
        assert st == OK
        colors, permitted = np.frombuffer(bytes(rec.colors), np.uint8), np.array(list(rec.permitted), np.uint64)
        assert np.array_equal(colors[:E], a["colors"][:E]) and not colors[E:].any(), (tier, entry)
        assert np.array_equal(permitted[:pw], a["permitted"][:pw]) and not permitted[pw:].any(), (tier, entry)
        assert list(rec.totals) == a["totals"].tolist(), (tier, entry)
        assert np.float32(rec.eval).tobytes() == np.float32(a["eval"]).tobytes(), (tier, entry)
        assert (rec.agent, rec.node) == (a["agent"], a["node"]), (tier, entry)


@pytest.mark.parametrize("tier", TIERS)
def test_exported_keys_are_host_key_words_of_action_ids(engines, tier):
    opt = engines[tier]
    st, keys, guard = export_keys(opt)
    assert st == OK and (guard == ~np.uint64(0)).all(), tier  # nodes x KEY_WORDS words written, not one more
    assert len(keys) > 1, tier
    A = opt.space.ACTION_DIM
    for row in keys:
        bits = [64 * w + b for w, x in enumerate(row) for b in range(64) if (int(x) >> b) & 1]
        assert all(b < A for b in bits), (tier, bits)
    # the root's key is the empty set, every other node's is not: rows of another width would not line up so
    assert not keys[0].any() and all(row.any() for row in keys[1:]), tier


@pytest.mark.parametrize("n,sizes,max_slots,u64,entry,text", [
    (24, [4, 5], 276, False, "ramsey_argmin_data", T_NARROW),       # wide engine, E = 276 > 256
    (34, [3, 3, 3, 3], 170, True, "ramsey_wide_argmin_data", T_WIDE),  # 64-bit engine, E = 561 > 496
], ids=["wide_n24", "u64_n34"])
def test_typed_ramsey_entries_refuse_more_edges_than_their_record_holds(n, sizes, max_slots, u64, entry, text):
    import azdopt_amd as az
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, max_slots=max_slots, u64=u64)
    assert space.tier == ("u64" if u64 else "wide")
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, 1)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(1, 8, kmin=10, kmax=30), model, 8, node_capacity=256)
    st, _ = call(opt, entry)
    assert st == INVALID and opt._L.azd_last_error().decode() == text
    assert call(opt, "ramsey_argmin_any")[0] == OK


# ---------------------------------------------------------------- the recipe tiers of the dense-graph space: every (entry, tier) pair
FAMILIES = ("inv", "invx", "invs")
RECIPE_TIERS = tuple((f, w) for f in FAMILIES for w in (False, True))  # (family, wide)
DENSE_READERS = ("dense", "dense_ah", "dense_ah_wide") + tuple("dense_%s%s" % (f, "_wide" if w else "") for f, w in RECIPE_TIERS)


def flag_of(stem):  # "dense_invx_wide" -> "AZD_ENGINE_DENSE_INVX_WIDE"
    return "AZD_ENGINE_" + stem.upper()


def recipe_engine(az, L, stem, n=4, B=1):
    """an engine made by hand (NablaOptimizer's constructor would set the recipe): (handle, its evaluator, roots)"""
    from azdopt_amd import _lib
    flags = {"dense": 0, "dense_ah": _lib.ENGINE_DENSE_AH, "dense_inv": _lib.ENGINE_DENSE_INV, "dense_invx": _lib.ENGINE_DENSE_INVX, "dense_invs": _lib.ENGINE_DENSE_INVS}
    wide = {"dense_inv_wide": _lib.ENGINE_DENSE_INV_WIDE, "dense_invx_wide": _lib.ENGINE_DENSE_INVX_WIDE, "dense_invs_wide": _lib.ENGINE_DENSE_INVS_WIDE}
    fl = flags[stem[:-5]] | wide[stem] if stem in wide else flags[stem]
    space = az.DenseGraphSpace(n, 0.5)
    model = az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    cfg = _lib.EngineConfig(_lib.SPACE_DENSE, n, B, 0, 0, 0, 0, 0, fl)
    cfg.max_slots, cfg.dense_p = space.E, space.p
    h = C.c_void_p()
    _lib.check(L.azd_engine_create(C.byref(h), C.byref(cfg), model._h), "create")
    adj, slots = space.generate_roots(0, B, kmin=1, kmax=3)
    return h, model, (np.ascontiguousarray(adj, np.uint8), np.ascontiguousarray(slots, np.uint64))


def test_recipe_tiers_every_setter_reader_and_argmin_entry_says_its_text():
    """n = 4, one agent.  The texts are the library's, whole: an entry of another cost names the engine's own flag and the entry that
    serves it; an entry on an engine that takes no recipe says what engine it wants."""
    import azdopt_amd as az
    from azdopt_amd import _lib
    if az.device_count() < 1:
        pytest.fail("no gfx950 device: the GPU tests need the HIP path")
    L = az.lib()
    err = lambda: L.azd_last_error().decode()
    n = 4
    w = dict(edges=1.0)
    recipes = dict(inv=az.InvariantCost(w, eval_scale=0.1).recipe(), invx=az.InvariantCostX(w, eval_scale=0.1).recipe(), invs=az.InvariantCostS(w, eval_scale=0.1).recipe())
    costs = dict(inv=_lib.DenseInvCost, invx=_lib.DenseInvxCost, invs=_lib.DenseInvsCost)
    argmins = dict(dense=_lib.DenseArgmin, dense_ah=_lib.DenseAhArgmin, dense_ah_wide=_lib.DenseAhWideArgmin, dense_inv=_lib.DenseInvArgmin,
                   dense_inv_wide=_lib.DenseInvWideArgmin, dense_invx=_lib.DenseInvxArgmin, dense_invx_wide=_lib.DenseInvxWideArgmin,
                   dense_invs=_lib.DenseInvsArgmin, dense_invs_wide=_lib.DenseInvsWideArgmin)
    setter = lambda f: "azd_engine_set_dense_%s_recipe" % f
    reader = lambda f: "azd_engine_dense_%s_agent_cost" % f
    for stem in ("dense", "dense_ah") + DENSE_READERS[3:]:
        h, model, (a8, s64) = recipe_engine(az, L, stem, n)
        mine = next((f for f in FAMILIES if stem in ("dense_" + f, "dense_" + f + "_wide")), None)  # the engine's family; None: it takes no recipe
        if mine:
            assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == INVALID
            assert err() == "par_new: an %s engine has no cost before %s has given it its recipe" % (flag_of("dense_" + mine), setter(mine)), stem
        for f in FAMILIES:
            st = getattr(L, setter(f))(h, C.byref(recipes[f]))
            if f == mine:
                assert st == OK, (stem, f, err())
            elif mine:
                assert st == UNSUPPORTED and err() == "%s: an %s engine's recipe is set with %s" % (setter(f), flag_of("dense_" + mine), setter(mine)), (stem, f, err())
            else:
                assert st == UNSUPPORTED and err() == "%s: not an %s engine" % (setter(f), flag_of("dense_" + f)), (stem, f, err())
        assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == OK, (stem, err())
        if mine:
            assert getattr(L, setter(mine))(h, C.byref(recipes[mine])) == INVALID
            assert err() == setter(mine) + ": par_new has run: the trees' evals were computed with the recipe in force, which stays", stem
        for f in FAMILIES:
            c = costs[f]()
            st = getattr(L, reader(f))(h, 0, C.byref(c))
            if f == mine:
                assert st == OK and c.computed == 0xFF and c.cost == c.inv[0] > 0.0 and c.eval == np.float32(0.1) * np.float32(c.cost), (stem, c.cost, c.eval)
            elif mine:
                assert st == UNSUPPORTED and err() == "%s: an %s engine's record is read with %s" % (reader(f), flag_of("dense_" + mine), reader(mine)), (stem, f, err())
            else:
                assert st == UNSUPPORTED and err() == "%s: not an %s engine" % (reader(f), flag_of("dense_" + f)), (stem, f, err())
        st = L.azd_engine_dense_ah_agent_cost(h, 0, C.byref(_lib.DenseAhCost()))
        assert st == (OK if stem == "dense_ah" else UNSUPPORTED), stem
        lam = C.c_double()
        st = L.azd_engine_agent_state(h, 0, None, None, None, None, C.byref(lam), None)
        if mine:
            assert err() == "azd_engine_agent_state: lambda_1 / matching_size: an %s engine keeps neither (%s)" % (flag_of("dense_" + mine), reader(mine)), stem
            assert st == UNSUPPORTED
            assert L.azd_engine_dense_ah_agent_cost(h, 0, C.byref(_lib.DenseAhCost())) == UNSUPPORTED
            assert err() == "azd_engine_dense_ah_agent_cost: an %s engine's record is read with %s" % (flag_of("dense_" + mine), reader(mine)), stem
        for entry in DENSE_READERS:
            st = getattr(L, "azd_engine_%s_argmin_data" % entry)(h, C.byref(argmins[entry]()))
            if entry == stem:
                assert st == OK, (stem, entry, err())
                continue
            assert st == UNSUPPORTED, (stem, entry)
            if mine:
                assert err() == "dense argmin read: an %s engine's record is read with azd_engine_%s_argmin_data" % (flag_of(stem), stem), (stem, entry, err())
            elif entry == "dense":
                assert err() == T_DENSE, stem  # (said to an AZD_ENGINE_DENSE_AH engine: the default engine has passed above)
            elif entry != "dense_ah":  # (that entry refuses the default engine without a text)
                assert err() == "azd_engine_%s_argmin_data: not an %s engine" % (entry, flag_of(entry)), (stem, entry, err())
        L.azd_engine_destroy(h)
