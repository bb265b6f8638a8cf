"""Every read-back entry of the C ABI on one engine of every tier, at the smallest shapes: which entry serves which tier, which
refuses it with which status and text, and that the typed Ramsey records and the exported keys have the layout the header gives.
The tiers: c21; Ramsey narrow, wide (max_slots > 0) and 64-bit (AZD_ENGINE_RAMSEY_U64); the dense-graph space with its default cost,
with the Aouchiche-Hansen cost (AZD_ENGINE_DENSE_AH) and with that cost's 64-row form (AZD_ENGINE_DENSE_AH_WIDE)."""
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
