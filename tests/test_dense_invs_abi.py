"""azd_dense_invs_cost, the host form of the spectrum invariant cost (dense_cost_host.cpp), without a GPU: equal to the Python reference
(tests/dense_invs_ref.py) bit for bit -- every field of the record compared as bytes -- on the whole graph set under the five new
recipes, and on the hard case set of the spectral passes (tests/dense_spectral_cases.py) at n = 21, 23, 31, 32 under the heaviest;
azd_dense_invs_spectrum equal to the reference's eigenvalues as bits; equal to azd_dense_invx_cost under the converted INVX
recipes; skipped invariants; and every refusal that needs no device, with its status and the argument or field it names."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import dense_ah_ref as A
import dense_invs_ref as R
import dense_invx_ref as X
import dense_spectral_cases as S

HARD_NS = (21, 23, 31, 32)


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


c_recipe = R.c_recipe


def host_cost(lib, adj, n, recipe):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseInvsCost()
    rc = recipe if isinstance(recipe, _lib.DenseInvsRecipe) else c_recipe(recipe)
    st = lib.azd_dense_invs_cost(_lib.ptr(a), n, C.byref(rc), C.byref(out))
    return st, out


def host_spectrum(lib, adj, n, which):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = np.zeros(n, np.float64)
    st = lib.azd_dense_invs_spectrum(_lib.ptr(a), n, which, _lib.ptr(out))
    return st, out


def reference_bytes(r):
    """the Python reference's record in azd_dense_invs_cost_t's layout"""
    return struct.pack("<21diIff", *[r[k] for k in R.NAMES], r["dist_k"], r["computed"], r["cost"], r["eval"])


def test_symbols_are_exported_and_bound(lib):
    from azdopt_amd import _lib
    for name in ("azd_dense_invs_cost", "azd_dense_invs_spectrum", "azd_debug_probe_invs_cost", "azd_engine_set_dense_invs_recipe",
                 "azd_engine_dense_invs_argmin_data", "azd_engine_dense_invs_agent_cost"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_INVS_MAX_N == 32 and _lib.DENSE_INVS_COUNT == 21 == len(R.NAMES) and _lib.DENSE_INVS_NAMES == R.NAMES
    assert _lib.DENSE_INVS_NAMES[:16] == _lib.DENSE_INVX_NAMES and _lib.ENGINE_DENSE_INVS == 16384 and _lib.DENSE_INVS_ROUNDS == R.ROUNDS == 67
    assert (C.sizeof(_lib.DenseInvsRecipe), C.sizeof(_lib.DenseInvsCost), C.sizeof(_lib.DenseInvsArgmin)) == (304, 184, 512)
    # the INVX structs keep their sizes: index and name are ABI, sixteen doubles
    assert (C.sizeof(_lib.DenseInvxTerm), C.sizeof(_lib.DenseInvxRecipe), C.sizeof(_lib.DenseInvxCost), C.sizeof(_lib.DenseInvxArgmin)) == (24, 264, 144, 472)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "azdopt_amd.h")).read()
    assert "#define AZD_ENGINE_DENSE_INVS 16384u" in hdr and "#define AZD_DENSE_INVS_COUNT 21" in hdr and "#define AZD_DENSE_INVS_ROUNDS 67" in hdr
    assert "#define AZD_DENSE_INVS_NAMES AZD_DENSE_INVX_NAMES, " + ", ".join('"%s"' % k for k in R.NAMES[16:]) in hdr


def test_host_cost_equals_the_python_reference_as_bytes(lib):
    entries = A.graph_set()
    R.prime(entries)
    seen = 0
    for name, n, adj in entries:
        for rname in R.NEW_RECIPES:
            recipe = R.RECIPES[rname](n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, rname, lib.azd_last_error())
            r = R.invs_cost(adj, n, recipe)
            assert bytes(out) == reference_bytes(r), (name, n, rname, list(out.inv), r)
            assert 0.0 <= out.eval <= 1.0, (name, n, rname, out.eval)
            seen += 1
    assert seen == 5 * 560


def test_host_cost_equals_the_python_reference_on_the_hard_spectral_cases(lib):
    """tests/dense_spectral_cases.py (rank-deficient adjacency matrices, every labelling) at n = 21, 23, 31, 32 under ALLE -- all four
    matrices, both finishers each: records as bytes, every invariant finite"""
    entries = [e for e in S.graph_set() if e[1] in HARD_NS]
    assert len(entries) >= 1500
    R.prime(entries, ks_of=lambda n: (1, n - 2, n - 1))
    for name, n, adj in entries:
        recipe = R.RECIPES["ALLE"](n)
        st, out = host_cost(lib, adj, n, recipe)
        assert st == 0, (name, lib.azd_last_error())
        assert all(math.isfinite(x) for x in out.inv) and out.computed == 0xFF | 0xF00 | 0x1F0000, (name, list(out.inv))
        assert bytes(out) == reference_bytes(R.invs_cost(adj, n, recipe)), (name, list(out.inv))
        assert 0.0 <= out.eval <= 1.0, (name, out.eval)


def test_host_spectrum_equals_the_references_as_bits(lib):
    entries = A.graph_set()
    R.prime(entries)
    hard = [e for e in S.graph_set() if e[1] in HARD_NS][::25]
    R.prime(hard)
    seen = 0
    for name, n, adj in list(entries) + hard:
        for w, which in enumerate(R.WHICH):
            st, th = host_spectrum(lib, adj, n, w)
            assert st == 0, (name, which, lib.azd_last_error())
            assert th.tobytes() == np.array(R.spectrum(adj, n, which)).tobytes(), (name, which)
            assert np.all(np.diff(th) >= 0.0), (name, which)  # ascending
            seen += 1
    assert seen >= 4 * 560
    st, _ = host_spectrum(lib, A.path(8), 8, 4)
    assert st == 1 and lib.azd_last_error().decode().split(": ")[1] == "which"
    st, _ = host_spectrum(lib, A.path(33), 33, 0)
    assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n")
    from azdopt_amd import _lib
    a = np.array(A.path(8), dtype=np.uint64)
    assert lib.azd_dense_invs_spectrum(_lib.ptr(a), 8, 0, None) == 1 and "out" in lib.azd_last_error().decode()


def test_the_converted_invx_recipes_give_the_invx_host_function(lib):
    from azdopt_amd import _lib
    import azdopt_amd as az
    seen = 0
    for name, n, adj in A.graph_set():
        a = np.array(adj, dtype=np.uint64)
        for rname in R.INVX_RECIPES:
            xr = X.RECIPES[rname](n)
            invx = _lib.DenseInvxCost()
            rc = X.c_recipe(xr)
            assert lib.azd_dense_invx_cost(_lib.ptr(a), n, C.byref(rc), C.byref(invx)) == 0
            for recipe in (R.RECIPES[rname](n), az.InvariantCostS.from_invariant_cost_x(az.InvariantCostX(xr.weights(), **xr.kwargs())).recipe()):
                st, out = host_cost(lib, adj, n, recipe)
                assert st == 0
                # inv[0 .. 15], dist_k, computed, cost, eval: azd_dense_invx_cost_t's bytes
                assert bytes(out)[:128] + bytes(out)[168:] == bytes(invx), (name, n, rname)
                assert list(out.inv)[16:] == [0.0] * 5
            seen += 1
    assert seen == 9 * 560


def test_skipped_invariants_and_terms_that_name_alone(lib):
    n, adj = 12, A.double_broom(12, 3, 3)
    idx = dict(adj_index=1, dist_index=2, lap_index=n - 2, slap_index=0)
    full = host_cost(lib, adj, n, R.Recipe({k: 1.0 for k in R.NAMES}, **idx))[1]
    assert full.computed == 0x1FFFFF and all(full.inv[i] != 0.0 for i in list(range(8, 15)) + list(range(16, 21)))
    for bit in range(8, 21):
        st, out = host_cost(lib, adj, n, R.Recipe({k: 1.0 for k in R.NAMES if k != R.NAMES[bit]}, **idx))
        assert st == 0 and out.computed == 0x1FFFFF & ~(1 << bit) and out.inv[bit] == 0.0 and math.copysign(1.0, out.inv[bit]) == 1.0
        assert [out.inv[i] for i in range(21) if i != bit] == [full.inv[i] for i in range(21) if i != bit] and out.dist_k == 2
        # the same invariant named by a pair term alone, as either operand: computed again, the others' bits unchanged
        for term in ((0.5, R.NAMES[bit], "*", "edges"), (0.5, "edges", "*", R.NAMES[bit])):
            st, out = host_cost(lib, adj, n, R.Recipe({"edges": 1.0}, terms=[term], **idx))
            assert st == 0 and out.computed == 0xFF | 1 << bit and out.inv[bit] == full.inv[bit], (bit, term)
            v = full.inv[bit] * full.inv[0]
            assert out.cost == np.float32(full.inv[0] + 0.5 * v)
        st, out = host_cost(lib, adj, n, R.Recipe({"edges": 1.0}, terms=[(0.0, R.NAMES[bit], "*", "edges")], **idx))
        assert st == 0 and out.computed == 0xFF and out.cost == full.inv[0]
    # an energy needed and its matrix's *_eig not, and the reverse: one finisher each, the values those of the full record
    for eig, energy in ((8, 16), (9, 17), (10, 18), (11, 19), (8, 20)):
        st, out = host_cost(lib, adj, n, R.Recipe({R.NAMES[energy]: 1.0}, **idx))
        assert st == 0 and out.computed == 0xFF | 1 << energy and out.inv[energy] == full.inv[energy] and out.inv[eig] == 0.0
        st, out = host_cost(lib, adj, n, R.Recipe({R.NAMES[eig]: 1.0}, **idx))
        assert st == 0 and out.computed == 0xFF | 1 << eig and out.inv[eig] == full.inv[eig] and out.inv[energy] == 0.0
    # every new invariant may divide
    for b in range(16, 21):
        st, out = host_cost(lib, adj, n, R.Recipe({}, terms=[(1.0, "edges", "/", R.NAMES[b])], **idx))
        assert st == 0 and out.computed == 0xFF | 1 << b and out.cost == np.float32(full.inv[0] / full.inv[b]), b


def test_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    ok = R.recipe_alle(8)
    for n in (3, 33, 64, 0, -1):
        st, _ = host_cost(lib, A.path(max(n, 4)), n, R.recipe_energy(8))
        assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n"), (n, lib.azd_last_error())
    two_paths = A.from_edges(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)])
    st, _ = host_cost(lib, two_paths, 8, ok)
    assert st == 1 and "adj" in lib.azd_last_error().decode() and "connected" in lib.azd_last_error().decode()
    for bad in ([1 << 1, 0, 0, 0], [0b0011, 0b0001, 0, 0], [1 << 40, 0, 0, 0]):  # asymmetric, loop, neighbour beyond n
        st, _ = host_cost(lib, bad, 4, R.recipe_energy(4))
        assert st == 1 and "adj" in lib.azd_last_error().decode(), bad
    a = np.array(A.path(8), dtype=np.uint64)
    rc = c_recipe(ok)
    assert lib.azd_dense_invs_cost(None, 8, C.byref(rc), C.byref(_lib.DenseInvsCost())) == 1
    assert lib.azd_dense_invs_cost(_lib.ptr(a), 8, C.byref(rc), None) == 1 and "out" in lib.azd_last_error().decode()
    assert lib.azd_dense_invs_cost(_lib.ptr(a), 8, None, C.byref(_lib.DenseInvsCost())) == 1 and "recipe" in lib.azd_last_error().decode()


def bad_recipes(n):
    """(field the refusal names, recipe) for every way a recipe is refused"""
    inf, nan = float("inf"), float("nan")

    def mk(**kw):
        r = c_recipe(R.recipe_eratio(n))  # two terms: adj_energy / edges, adj_spread * proximity
        for k, v in kw.items():
            if k == "w":
                r.weight[v[0]] = v[1]
            elif k == "weights":
                for i, x in enumerate(v):
                    r.weight[i] = x
            elif k == "term":
                for f, x in v.items():
                    setattr(r.term[1], f, x)
            elif k == "coefs":
                for t in range(4):
                    r.term[t].coef = v
            else:
                setattr(r, k, v)
        return r

    out = [("weight", mk(w=(3, inf))), ("weight", mk(w=(20, nan))), ("weight", mk(weights=[0.0] * 21, coefs=0.0)), ("bias", mk(bias=nan)),
           ("bias", mk(bias=-inf)), ("eval_offset", mk(eval_offset=inf)), ("eval_scale", mk(eval_scale=nan)), ("eval_scale", mk(eval_scale=0.0)),
           ("adj_index", mk(adj_index=-1)), ("adj_index", mk(adj_index=n)), ("dist_index", mk(dist_index=n)), ("dist_index", mk(dist_index=-2)),
           ("lap_index", mk(lap_index=-1)), ("lap_index", mk(lap_index=n)), ("slap_index", mk(slap_index=-1)), ("slap_index", mk(slap_index=n)),
           ("n_terms", mk(n_terms=-1)), ("n_terms", mk(n_terms=5)), ("term.coef", mk(term=dict(coef=nan))), ("term.coef", mk(term=dict(coef=inf))),
           ("term.a", mk(term=dict(a=-1))), ("term.a", mk(term=dict(a=21))), ("term.b", mk(term=dict(b=-1))), ("term.b", mk(term=dict(b=21))),
           ("term.op", mk(term=dict(op=2))), ("term.op", mk(term=dict(op=-1)))]
    # the divisor rule: an invariant that can be zero (8 .. 11: eigenvalues, 15: triangles) cannot divide
    out += [("term.b", mk(term=dict(op=X.DIV, b=b))) for b in (8, 9, 10, 11, 15)]
    return out


def test_recipes_are_checked_and_the_field_is_named(lib):
    n = 8
    for field, rc in bad_recipes(n):
        st, _ = host_cost(lib, A.cycle(n), n, rc)
        why = lib.azd_last_error().decode()
        assert st == 1 and why.split(": ")[1] == field, (field, why)
    # the limits themselves are accepted: indices n - 1, the AH rule, a negative scale, -0.0 as a weight of zero, four terms with new divisors,
    # all weights zero beside one coefficient
    terms = [(1.0, "lap_eig", "/", b) for b in ("adj_energy", "lap_energy", "adj_spread", "dist_energy")]
    edge = c_recipe(R.Recipe({"adj_eig": -0.0}, terms=terms, adj_index=n - 1, dist_index=R.INDEX_AH, lap_index=n - 1, slap_index=n - 1, eval_scale=-1.0))
    st, out = host_cost(lib, A.cycle(n), n, edge)
    assert st == 0 and out.computed == 0xFF | 1 << 10 | 1 << 16 | 1 << 17 | 1 << 18 | 1 << 20 and math.isfinite(out.cost), lib.azd_last_error()


def test_probe_checks_graphs_and_recipe_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseInvsCost * 2)()
    rc = c_recipe(R.recipe_alle(8))
    a = np.array(A.path(33) + A.path(33), dtype=np.uint64)
    assert lib.azd_debug_probe_invs_cost(0, _lib.ptr(a), 33, 2, 1, C.byref(rc), out, None) == 1 and "n" in lib.azd_last_error().decode()
    a = np.array(list(A.path(8)) + [0] * 8, dtype=np.uint64)
    assert lib.azd_debug_probe_invs_cost(0, _lib.ptr(a), 8, 2, 1, C.byref(rc), out, None) == 1 and "graph 1" in lib.azd_last_error().decode()
    a = np.array(A.path(8) + A.cycle(8), dtype=np.uint64)
    for field, bad in bad_recipes(8):
        assert lib.azd_debug_probe_invs_cost(0, _lib.ptr(a), 8, 2, 1, C.byref(bad), out, None) == 1
        assert lib.azd_last_error().decode().split(": ")[1] == field, field
    assert lib.azd_debug_probe_invs_cost(0, _lib.ptr(a), 8, 2, 0, C.byref(rc), out, None) == 1
    assert lib.azd_engine_set_dense_invs_recipe(None, C.byref(rc)) == 1
    assert lib.azd_engine_dense_invs_argmin_data(None, C.byref(_lib.DenseInvsArgmin())) == 1
    assert lib.azd_engine_dense_invs_agent_cost(None, 0, C.byref(_lib.DenseInvsCost())) == 1


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_INVS: configuration checks, without a device
def _config(space_id, n, flags, layers=0, max_slots=0, path_kind=0, n_colors=0):
    from azdopt_amd import _lib
    cfg = _lib.EngineConfig(space_id, n, 4, 0, 0, 0, 0, 0, flags)
    cfg.layers, cfg.max_slots, cfg.path_kind, cfg.dense_p, cfg.n_colors = layers, max_slots, path_kind, 0.4, n_colors
    for i in range(n_colors):
        cfg.clique_sizes[i], cfg.color_weights[i] = 3, 1.0
    return cfg


def _create(lib, *args, **kw):
    cfg = _config(*args, **kw)
    h = C.c_void_p()
    st = lib.azd_engine_create(C.byref(h), C.byref(cfg), None)
    if st == 0:
        lib.azd_engine_destroy(h)
    return st, lib.azd_last_error().decode()


def test_engine_flag_is_validated_before_the_device_is_looked_for(lib):
    from azdopt_amd import _lib
    V = _lib.ENGINE_DENSE_INVS
    for extra in (0, _lib.ENGINE_EXT_POOL_F32):  # the pool step's fp32 evaluator is accepted beside it
        st, why = _create(lib, _lib.SPACE_DENSE, 31, V | extra, max_slots=128)
        assert st in (0, 2), why  # created, or "no device"
    st, why = _create(lib, _lib.SPACE_DENSE, 32, V, max_slots=496)
    assert st in (0, 2), why
    for other in (_lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_INV,
                  _lib.ENGINE_DENSE_INV | _lib.ENGINE_DENSE_INV_WIDE, _lib.ENGINE_DENSE_INV_WIDE, _lib.ENGINE_DENSE_INVX,
                  _lib.ENGINE_DENSE_INVX | _lib.ENGINE_DENSE_INVX_WIDE, _lib.ENGINE_DENSE_INVX_WIDE):
        st, why = _create(lib, _lib.SPACE_DENSE, 31, V | other)
        assert st == 1 and why.startswith("flags:") and "AZD_ENGINE_DENSE_INVS" in why, why
    for n in (33, 3, 64):
        st, why = _create(lib, _lib.SPACE_DENSE, n, V)
        assert st == 1 and why.startswith("n:"), why
    st, why = _create(lib, _lib.SPACE_C21, 19, V)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_RAMSEY, 16, V, n_colors=3)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, V, layers=2)
    assert st == 1 and why.startswith("layers:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, V, max_slots=29)  # E = 28
    assert st == 1 and why.startswith("max_slots:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, V, path_kind=1)
    assert st == 1 and why.startswith("path_kind:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, V | _lib.ENGINE_EXT_POOL_F32 | _lib.ENGINE_NO_PERSISTENT_STEP)
    assert st == 1 and "AZD_ENGINE_EXT_POOL_F32" in why, why
    # the flag changes nothing for the other tiers: their limits stand
    assert _create(lib, _lib.SPACE_DENSE, 33, 0)[0] in (0, 2) and _create(lib, _lib.SPACE_DENSE, 31, _lib.ENGINE_DENSE_INVX, max_slots=128)[0] in (0, 2)


def test_the_tier_has_no_pool_step_plan(lib):
    """azd_debug_ext_pool_plan (arithmetic only): the tier builds no pool searchers, and the plan says so instead of reporting one;
    the INV tier's plan stands"""
    from azdopt_amd import _lib
    for max_slots in (128, 256, 465):
        cfg = _config(_lib.SPACE_DENSE, 31, _lib.ENGINE_DENSE_INVS | _lib.ENGINE_EXT_POOL_F32, max_slots=max_slots)
        waves, lds = C.c_int(), C.c_size_t()
        assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 8 and "no searcher-only pool step" in lib.azd_last_error().decode()
    cfg = _config(_lib.SPACE_DENSE, 31, _lib.ENGINE_DENSE_INV | _lib.ENGINE_EXT_POOL_F32, max_slots=128)
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0 and waves.value == 10


def test_python_space_carries_the_recipe():
    import azdopt_amd as az
    cost = az.InvariantCostS({"adj_energy": 1, "max_degree": -0.25}, terms=[(0.5, "lap_energy", "/", "adj_spread"), (2, "adj_eig", "*", "dist_energy")], bias=0.25,
                             adj_index=2, dist_index="ah", lap_index=29, slap_index=3, eval_offset=2.0, eval_scale=0.01)
    sp = az.DenseGraphSpace(31, 0.4, max_slots=600, cost=cost)
    assert sp.COST == "invs" and sp.INVS is cost and sp.INVX is None and sp.INV is None and sp.MAX_SLOTS == 465 and (sp.STATE_DIM, sp.ACTION_DIM) == (1396, 930)
    r = cost.recipe()
    assert list(r.weight) == [0, -0.25] + [0] * 14 + [1, 0, 0, 0, 0] and (r.bias, r.adj_index, r.dist_index, r.lap_index, r.slap_index) == (0.25, 2, -1, 29, 3)
    assert r.n_terms == 2 and [(t.coef, t.a, t.b, t.op) for t in r.term[:2]] == [(0.5, 18, 20, 1), (2.0, 8, 17, 0)]
    with pytest.raises(ValueError, match="matching"):
        az.InvariantCostS({"matching": 1.0})
    with pytest.raises(ValueError, match="triangles"):
        az.InvariantCostS({}, terms=[(1.0, "edges", "/", "triangles")])
    with pytest.raises(ValueError, match="adj_energy"):  # InvariantCostX does not know the new names
        az.InvariantCostX({"adj_energy": 1.0})
    d = {"weights": {"slap_energy": 1}, "terms": [[0.5, "adj_energy", "/", "edges"]], "lap_index": 3, "eval_scale": 0.5}
    assert az.InvariantCostS.from_dict(d).recipe().lap_index == 3 and az.InvariantCostS.from_dict(d).recipe().n_terms == 1
    ref = R.Recipe({"adj_energy": 1, "max_degree": -0.25}, terms=cost.terms, bias=0.25, adj_index=2, lap_index=29, slap_index=3, eval_offset=2.0, eval_scale=0.01)
    got, want = sp.invs_cost(A.cycle(31)), R.invs_cost(A.cycle(31), 31, ref)
    assert all(got[k] == want[k] for k in want), (got, want)
    assert sp.invs_spectrum(A.cycle(31), "lap").tobytes() == np.array(R.spectrum(A.cycle(31), 31, "lap")).tobytes()
    x = az.InvariantCostX({"lap_eig": 1.0, "avg_distance": -1.0}, terms=[(0.5, "remoteness", "/", "radius")], lap_index=29, eval_offset=4.0, eval_scale=0.01)
    s = az.DenseGraphSpace(31, 0.4, cost=az.InvariantCostS.from_invariant_cost_x(x)).invs_cost(A.cycle(31))
    i = az.DenseGraphSpace(31, 0.4, cost=x).invx_cost(A.cycle(31))
    assert all(s[k] == i[k] for k in i) and all(s[k] == 0.0 for k in R.NAMES[16:])


def test_cpp_binding_compiles_with_a_spectrum_invariant_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "invs.cpp"
    src.write_text("""
#include <cmath>
#include "azdopt_amd.hpp"
int main() {
    uint64_t k4[4] = {0xe, 0xd, 0xb, 0x7};
    azdopt::InvariantCostS e;
    e.weight("adj_energy", 1.0).term(0.5, "adj_spread", '/', "lap_energy").scale(0.125f);
    azdopt::DenseGraphInvSSpace space(4, 0.4, 6, e);
    azd_dense_invs_cost_t c = space.cost(k4);  // K4: energy 6, spread 4, Laplacian energy 6
    if (std::fabs(c.inv[16] - 6.0) > 1e-12 || std::fabs(c.inv[20] - 4.0) > 1e-12 || std::fabs(c.inv[18] - 6.0) > 1e-12) return 1;
    if (c.computed != (0xFFu | 1u << 16 | 1u << 18 | 1u << 20) || std::fabs(c.cost - (6.0f + 0.5f * 4.0f / 6.0f)) > 1e-6f) return 2;
    std::vector<double> th = space.spectrum(k4, AZD_DENSE_INVS_MATRIX_ADJ);
    if (th.size() != 4 || std::fabs(th[3] - 3.0) > 1e-12 || std::fabs(th[0] + 1.0) > 1e-12) return 3;
    azdopt::InvariantCostX deg;
    deg.weight("zagreb1", 1.0).term(-1.0, "zagreb2", '/', "edges").offset(1.0f).scale(0.125f);
    uint64_t c5[5] = {0x12, 0x05, 0x0a, 0x14, 0x09};
    azd_dense_invs_cost_t s = azdopt::DenseGraphInvSSpace(5, 0.4, 10, azdopt::InvariantCostS::from_invariant_cost_x(deg)).cost(c5);
    azd_dense_invx_cost_t x = azdopt::DenseGraphInvXSpace(5, 0.4, 10, deg).cost(c5);
    if (s.cost != x.cost || s.eval != x.eval || s.computed != x.computed || s.cost != 16.0f) return 4;
    if (azd_device_count() == 0) return 0;
    azdopt::DenseGraphInvSSpace big(20, 0.2, 128, e.scale(0.01f));
    azdopt::HashStreamModel model(big.STATE_DIM(), big.ACTION_DIM(), 1);
    auto roots = big.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphInvSSpace>::par_new(big, roots, model, 16);
    azdopt::DenseInvsArgmin a = opt.argmin_data();
    return a.cost.cost == big.cost(a.adj.data()).cost ? 0 : 5;
}
""")
    exe = tmp_path / "invs"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
