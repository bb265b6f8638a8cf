"""azd_dense_invx_cost, the host form of the extended invariant cost (dense_cost_host.cpp), without a GPU: equal to the Python reference
(tests/dense_invx_ref.py) bit for bit -- every field of the record compared as bytes -- on the whole graph set under the nine test
recipes, and on the hard case set of the spectral passes (tests/dense_spectral_cases.py) under four of them; equal to azd_dense_inv_cost (and, under the AH recipe, azd_dense_ah_cost) under the converted INV recipes; skipped terms;
and every refusal that needs no device, with its status and the argument or field it names."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as I
import dense_invx_ref as R
import dense_spectral_cases as S


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


c_recipe, c_inv_recipe = R.c_recipe, R.c_inv_recipe


def host_cost(lib, adj, n, recipe):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseInvxCost()
    rc = recipe if isinstance(recipe, _lib.DenseInvxRecipe) else c_recipe(recipe)
    st = lib.azd_dense_invx_cost(_lib.ptr(a), n, C.byref(rc), C.byref(out))
    return st, out


def reference_bytes(r):
    """the Python reference's record in azd_dense_invx_cost_t's layout"""
    return struct.pack("<16diIff", *[r[k] for k in R.NAMES], r["dist_k"], r["computed"], r["cost"], r["eval"])


def test_symbols_are_exported_and_bound(lib):
    from azdopt_amd import _lib
    for name in ("azd_dense_invx_cost", "azd_debug_probe_invx_cost", "azd_engine_set_dense_invx_recipe", "azd_engine_dense_invx_argmin_data",
                 "azd_engine_dense_invx_agent_cost"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_INVX_MAX_N == 32 and _lib.DENSE_INVX_COUNT == 16 == len(R.NAMES) and _lib.DENSE_INVX_NAMES == R.NAMES
    assert _lib.DENSE_INVX_NAMES[:10] == _lib.DENSE_INV_NAMES and _lib.ENGINE_DENSE_INVX == 4096
    assert (_lib.DENSE_INVX_MUL, _lib.DENSE_INVX_DIV, _lib.DENSE_INVX_MAX_TERMS) == (R.MUL, R.DIV, R.MAX_TERMS) == (0, 1, 4)
    assert (C.sizeof(_lib.DenseInvxTerm), C.sizeof(_lib.DenseInvxRecipe), C.sizeof(_lib.DenseInvxCost), C.sizeof(_lib.DenseInvxArgmin)) == (24, 264, 144, 472)
    # the INV structs keep their sizes: index and name are ABI, ten doubles
    assert (C.sizeof(_lib.DenseInvRecipe), C.sizeof(_lib.DenseInvCost), C.sizeof(_lib.DenseInvArgmin)) == (104, 96, 424)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "azdopt_amd.h")).read()
    assert "#define AZD_ENGINE_DENSE_INVX 4096u" in hdr and "#define AZD_DENSE_INVX_COUNT 16" in hdr
    assert "#define AZD_DENSE_INVX_NAMES AZD_DENSE_INV_NAMES, " + ", ".join('"%s"' % k for k in R.NAMES[10:]) in hdr


def test_host_cost_equals_the_python_reference_as_bytes(lib):
    seen = 0
    for name, n, adj in A.graph_set():
        for rname, mk in R.RECIPES.items():
            recipe = mk(n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, rname, lib.azd_last_error())
            r = R.invx_cost(adj, n, recipe)
            assert bytes(out) == reference_bytes(r), (name, n, rname, list(out.inv), r)
            seen += 1
    assert seen == 9 * 560


def test_host_cost_equals_the_python_reference_on_the_hard_spectral_cases(lib):
    """tests/dense_spectral_cases.py (rank-deficient adjacency matrices, every labelling; 186 of them end in NaN without the
    deflation rule) under an adjacency recipe, a both-spectra recipe, the Laplacian recipe (index n - 2) and the signless one
    (index 0): records as bytes, every invariant finite"""
    entries = S.graph_set()
    I.prime(entries, ("adj", "dist", "lap", "slap"), lambda n: (0, 1, n - 2, n - 1))
    seen = 0
    for name, n, adj in entries:
        for rname in ("ADJ", "BOTH", "LAP", "SLAP"):
            recipe = R.RECIPES[rname](n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, rname, lib.azd_last_error())
            assert all(math.isfinite(x) for x in out.inv), (name, rname, list(out.inv))
            assert bytes(out) == reference_bytes(R.invx_cost(adj, n, recipe)), (name, rname, list(out.inv))
            seen += 1
    assert seen == 4 * 3700


def test_the_converted_inv_recipes_give_the_inv_and_the_ah_host_functions(lib):
    from azdopt_amd import _lib
    import azdopt_amd as az
    seen = 0
    for name, n, adj in A.graph_set():
        a = np.array(adj, dtype=np.uint64)
        for rname in R.INV_RECIPES:
            inv = _lib.DenseInvCost()
            rc = c_inv_recipe(I.RECIPES[rname](n))
            assert lib.azd_dense_inv_cost(_lib.ptr(a), n, C.byref(rc), C.byref(inv)) == 0
            for recipe in (R.RECIPES[rname](n), az.InvariantCostX.from_invariant_cost(az.InvariantCost(I.RECIPES[rname](n).weights(), **I.RECIPES[rname](n).kwargs())).recipe()):
                st, out = host_cost(lib, adj, n, recipe)
                assert st == 0
                # inv[0 .. 9], dist_k, computed, cost, eval: azd_dense_inv_cost_t's bytes
                assert bytes(out)[:80] + bytes(out)[128:] == bytes(inv), (name, n, rname)
                assert list(out.inv)[10:] == [0.0] * 6
            if rname == "AH":
                ah = _lib.DenseAhCost()
                assert lib.azd_dense_ah_cost(_lib.ptr(a), n, C.byref(ah)) == 0
                assert struct.pack("<ddiiff", out.inv[5], out.inv[9], int(out.inv[3]), out.dist_k, out.cost, out.eval) == bytes(ah), (name, n)
            seen += 1
    assert seen == 4 * 560


def test_skipped_terms_and_terms_that_name_alone(lib):
    n, adj = 12, A.double_broom(12, 3, 3)
    idx = dict(adj_index=1, dist_index=2, lap_index=n - 2, slap_index=0)
    full = host_cost(lib, adj, n, R.Recipe({k: 1.0 for k in R.NAMES}, **idx))[1]
    assert full.computed == 0xFFFF and all(full.inv[i] != 0.0 for i in range(8, 15))
    for bit in range(8, 16):
        st, out = host_cost(lib, adj, n, R.Recipe({k: 1.0 for k in R.NAMES if k != R.NAMES[bit]}, **idx))
        assert st == 0 and out.computed == 0xFFFF & ~(1 << bit) and out.inv[bit] == 0.0 and math.copysign(1.0, out.inv[bit]) == 1.0
        assert [out.inv[i] for i in range(16) if i != bit] == [full.inv[i] for i in range(16) if i != bit] and out.dist_k == 2
        # the same invariant named by a pair term alone, as either operand: computed again, the others' bits unchanged
        for term in ((0.5, R.NAMES[bit], "*", "edges"), (0.5, "edges", "*", R.NAMES[bit])):
            st, out = host_cost(lib, adj, n, R.Recipe({"edges": 1.0}, terms=[term], **idx))
            assert st == 0 and out.computed == 0xFF | 1 << bit and out.inv[bit] == full.inv[bit], (bit, term)
            v = full.inv[bit] * full.inv[0]
            assert out.cost == np.float32(full.inv[0] + 0.5 * v)
        st, out = host_cost(lib, adj, n, R.Recipe({"edges": 1.0}, terms=[(0.0, R.NAMES[bit], "*", "edges")], **idx))
        assert st == 0 and out.computed == 0xFF and out.cost == full.inv[0]


def test_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    ok = R.recipe_all4(8)
    for n in (3, 33, 64, 0, -1):
        st, _ = host_cost(lib, A.path(max(n, 4)), n, R.recipe_deg(8))
        assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n"), (n, lib.azd_last_error())
    two_paths = A.from_edges(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)])
    st, _ = host_cost(lib, two_paths, 8, ok)
    assert st == 1 and "adj" in lib.azd_last_error().decode() and "connected" in lib.azd_last_error().decode()
    for bad in ([1 << 1, 0, 0, 0], [0b0011, 0b0001, 0, 0], [1 << 40, 0, 0, 0]):  # asymmetric, loop, neighbour beyond n
        st, _ = host_cost(lib, bad, 4, R.recipe_deg(4))
        assert st == 1 and "adj" in lib.azd_last_error().decode(), bad
    a = np.array(A.path(8), dtype=np.uint64)
    rc = c_recipe(ok)
    assert lib.azd_dense_invx_cost(None, 8, C.byref(rc), C.byref(_lib.DenseInvxCost())) == 1
    assert lib.azd_dense_invx_cost(_lib.ptr(a), 8, C.byref(rc), None) == 1 and "out" in lib.azd_last_error().decode()
    assert lib.azd_dense_invx_cost(_lib.ptr(a), 8, None, C.byref(_lib.DenseInvxCost())) == 1 and "recipe" in lib.azd_last_error().decode()


def bad_recipes(n):
    """(field the refusal names, recipe) for every way a recipe is refused"""
    inf, nan = float("inf"), float("nan")

    def mk(**kw):
        r = c_recipe(R.recipe_ratio(n))  # two terms: remoteness / radius, adj_eig * proximity
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

    out = [("weight", mk(w=(3, inf))), ("weight", mk(w=(15, nan))), ("weight", mk(weights=[0.0] * 16, coefs=0.0)), ("bias", mk(bias=nan)),
           ("bias", mk(bias=-inf)), ("eval_offset", mk(eval_offset=inf)), ("eval_scale", mk(eval_scale=nan)), ("eval_scale", mk(eval_scale=0.0)),
           ("adj_index", mk(adj_index=-1)), ("adj_index", mk(adj_index=n)), ("dist_index", mk(dist_index=n)), ("dist_index", mk(dist_index=-2)),
           ("lap_index", mk(lap_index=-1)), ("lap_index", mk(lap_index=n)), ("slap_index", mk(slap_index=-1)), ("slap_index", mk(slap_index=n)),
           ("n_terms", mk(n_terms=-1)), ("n_terms", mk(n_terms=5)), ("term.coef", mk(term=dict(coef=nan))), ("term.coef", mk(term=dict(coef=inf))),
           ("term.a", mk(term=dict(a=-1))), ("term.a", mk(term=dict(a=16))), ("term.b", mk(term=dict(b=-1))), ("term.b", mk(term=dict(b=16))),
           ("term.op", mk(term=dict(op=2))), ("term.op", mk(term=dict(op=-1)))]
    # the divisor rule: an invariant that can be zero (8 .. 11: eigenvalues, 15: triangles) cannot divide
    out += [("term.b", mk(term=dict(op=R.DIV, b=b))) for b in (8, 9, 10, 11, 15)]
    return out


def test_recipes_are_checked_and_the_field_is_named(lib):
    n = 8
    for field, rc in bad_recipes(n):
        st, _ = host_cost(lib, A.cycle(n), n, rc)
        why = lib.azd_last_error().decode()
        assert st == 1 and why.split(": ")[1] == field, (field, why)
    # the limits themselves are accepted: indices n - 1, the AH rule, a negative scale, -0.0 as a weight of zero, every allowed divisor, four
    # terms, all weights zero beside one coefficient
    terms = [(1.0, "lap_eig", "/", b) for b in ("randic", "zagreb1", "zagreb2", "avg_distance")]
    edge = c_recipe(R.Recipe({"adj_eig": -0.0}, terms=terms, adj_index=n - 1, dist_index=R.INDEX_AH, lap_index=n - 1, slap_index=n - 1, eval_scale=-1.0))
    st, out = host_cost(lib, A.cycle(n), n, edge)
    assert st == 0 and out.computed == 0xFF | 1 << 10 | 0x7000 and math.isfinite(out.cost), lib.azd_last_error()
    for b in range(8):
        st, out = host_cost(lib, A.cycle(n), n, R.Recipe({}, terms=[(1.0, "edges", "/", R.NAMES[b])]))
        assert st == 0 and math.isfinite(out.cost) and out.computed == 0xFF, b


def test_probe_checks_graphs_and_recipe_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseInvxCost * 2)()
    rc = c_recipe(R.recipe_all4(8))
    a = np.array(A.path(33) + A.path(33), dtype=np.uint64)
    assert lib.azd_debug_probe_invx_cost(0, _lib.ptr(a), 33, 2, 1, C.byref(rc), out, None) == 1 and "n" in lib.azd_last_error().decode()
    a = np.array(list(A.path(8)) + [0] * 8, dtype=np.uint64)
    assert lib.azd_debug_probe_invx_cost(0, _lib.ptr(a), 8, 2, 1, C.byref(rc), out, None) == 1 and "graph 1" in lib.azd_last_error().decode()
    a = np.array(A.path(8) + A.cycle(8), dtype=np.uint64)
    for field, bad in bad_recipes(8):
        assert lib.azd_debug_probe_invx_cost(0, _lib.ptr(a), 8, 2, 1, C.byref(bad), out, None) == 1
        assert lib.azd_last_error().decode().split(": ")[1] == field, field
    assert lib.azd_debug_probe_invx_cost(0, _lib.ptr(a), 8, 2, 0, C.byref(rc), out, None) == 1
    assert lib.azd_engine_set_dense_invx_recipe(None, C.byref(rc)) == 1
    assert lib.azd_engine_dense_invx_argmin_data(None, C.byref(_lib.DenseInvxArgmin())) == 1
    assert lib.azd_engine_dense_invx_agent_cost(None, 0, C.byref(_lib.DenseInvxCost())) == 1


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_INVX: configuration checks, without a device
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
    X = _lib.ENGINE_DENSE_INVX
    for extra in (0, _lib.ENGINE_EXT_POOL_F32):  # the pool step's fp32 evaluator is accepted beside it
        st, why = _create(lib, _lib.SPACE_DENSE, 31, X | extra, max_slots=128)
        assert st in (0, 2), why  # created, or "no device"
    st, why = _create(lib, _lib.SPACE_DENSE, 32, X, max_slots=496)
    assert st in (0, 2), why
    for other in (_lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_INV,
                  _lib.ENGINE_DENSE_INV | _lib.ENGINE_DENSE_INV_WIDE, _lib.ENGINE_DENSE_INV_WIDE):
        st, why = _create(lib, _lib.SPACE_DENSE, 31, X | other)
        assert st == 1 and why.startswith("flags:") and "AZD_ENGINE_DENSE_INVX" in why, why
    for n in (33, 3):
        st, why = _create(lib, _lib.SPACE_DENSE, n, X)
        assert st == 1 and why.startswith("n:"), why
    st, why = _create(lib, _lib.SPACE_C21, 19, X)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_RAMSEY, 16, X, n_colors=3)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, X, layers=2)
    assert st == 1 and why.startswith("layers:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, X, max_slots=29)  # E = 28
    assert st == 1 and why.startswith("max_slots:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, X, path_kind=1)
    assert st == 1 and why.startswith("path_kind:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, X | _lib.ENGINE_EXT_POOL_F32 | _lib.ENGINE_NO_PERSISTENT_STEP)
    assert st == 1 and "AZD_ENGINE_EXT_POOL_F32" in why, why
    # the flag changes nothing for the other tiers: their limits stand
    assert _create(lib, _lib.SPACE_DENSE, 33, 0)[0] in (0, 2) and _create(lib, _lib.SPACE_DENSE, 31, _lib.ENGINE_DENSE_INV, max_slots=128)[0] in (0, 2)


def test_the_pool_step_plan_is_the_inv_tiers(lib):
    """azd_debug_ext_pool_plan (arithmetic only): 10 / 9 / 7 waves at key widths 2 / 4 / 10, the LDS bytes of the INV tier"""
    from azdopt_amd import _lib
    got = []
    for max_slots in (128, 256, 465):
        plans = []
        for flag in (_lib.ENGINE_DENSE_INVX, _lib.ENGINE_DENSE_INV):
            cfg = _config(_lib.SPACE_DENSE, 31, flag | _lib.ENGINE_EXT_POOL_F32, max_slots=max_slots)
            waves, lds = C.c_int(), C.c_size_t()
            assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0, lib.azd_last_error()
            plans.append((waves.value, lds.value))
        assert plans[0] == plans[1], (max_slots, plans)
        got.append(plans[0][0])
    assert got == [10, 9, 7]


def test_python_space_carries_the_recipe():
    import azdopt_amd as az
    cost = az.InvariantCostX({"lap_eig": 1, "max_degree": -0.25}, terms=[(0.5, "remoteness", "/", "radius"), (2, "adj_eig", "*", "randic")], bias=0.25,
                             adj_index=2, dist_index="ah", lap_index=29, slap_index=3, eval_offset=2.0, eval_scale=0.01)
    sp = az.DenseGraphSpace(31, 0.4, max_slots=600, cost=cost)
    assert sp.COST == "invx" and sp.INVX is cost and sp.INV is None and sp.MAX_SLOTS == 465 and (sp.STATE_DIM, sp.ACTION_DIM) == (1396, 930)
    r = cost.recipe()
    assert list(r.weight) == [0, -0.25, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0] and (r.bias, r.adj_index, r.dist_index, r.lap_index, r.slap_index) == (0.25, 2, -1, 29, 3)
    assert r.n_terms == 2 and [(t.coef, t.a, t.b, t.op) for t in r.term[:2]] == [(0.5, 6, 4, 1), (2.0, 8, 12, 0)]
    with pytest.raises(ValueError, match="matching"):
        az.InvariantCostX({"matching": 1.0})
    with pytest.raises(ValueError, match="triangles"):
        az.InvariantCostX({}, terms=[(1.0, "edges", "/", "triangles")])
    with pytest.raises(ValueError):
        az.InvariantCostX({}, terms=[(1.0, "edges", "+", "radius")])
    with pytest.raises(ValueError):
        az.InvariantCostX({"edges": 1}, terms=[(1.0, "edges", "*", "radius")] * 5)
    d = {"weights": {"zagreb1": 1}, "terms": [[0.5, "zagreb2", "/", "edges"]], "lap_index": 3, "eval_scale": 0.5}
    assert az.InvariantCostX.from_dict(d).recipe().lap_index == 3 and az.InvariantCostX.from_dict(d).recipe().n_terms == 1
    ref = R.Recipe({"lap_eig": 1, "max_degree": -0.25}, terms=cost.terms, bias=0.25, adj_index=2, lap_index=29, slap_index=3, eval_offset=2.0, eval_scale=0.01)
    got, want = sp.invx_cost(A.cycle(31)), R.invx_cost(A.cycle(31), 31, ref)
    assert all(got[k] == want[k] for k in want), (got, want)
    inv = az.InvariantCost({"adj_eig": 1.0, "avg_distance": -1.0}, adj_index=1, eval_offset=4.0, eval_scale=0.01)
    x = az.DenseGraphSpace(31, 0.4, cost=az.InvariantCostX.from_invariant_cost(inv)).invx_cost(A.cycle(31))
    i = az.DenseGraphSpace(31, 0.4, cost=inv).inv_cost(A.cycle(31))
    assert all(x[k] == i[k] for k in i if k != "computed") and x["computed"] == i["computed"]


def test_cpp_binding_compiles_with_an_extended_invariant_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "invx.cpp"
    src.write_text("""
#include "azdopt_amd.hpp"
int main() {
    azdopt::InvariantCost ah = azdopt::InvariantCost::aouchiche_hansen(5);
    azdopt::DenseGraphInvXSpace space(5, 0.4, 10, azdopt::InvariantCostX::from_invariant_cost(ah));
    uint64_t c5[5] = {0x12, 0x05, 0x0a, 0x14, 0x09};
    azd_dense_ah_cost_t c;
    if (azd_dense_ah_cost(c5, 5, &c) != AZD_OK || c.cost != 7.5f) return 1;
    azd_dense_invx_cost_t i = space.cost(c5);
    if (i.cost != c.cost || i.eval != c.eval || i.inv[0] != 5.0 || i.computed != (0xFFu | 1u << 9)) return 3;
    azdopt::InvariantCostX deg;
    deg.weight("zagreb1", 1.0).term(-1.0, "zagreb2", '/', "edges").term(0.5, "triangles", '*', "randic").offset(1.0f).scale(0.125f);
    azd_dense_invx_cost_t d = azdopt::DenseGraphInvXSpace(5, 0.4, 10, deg).cost(c5);  // C5: zagreb1 = 20, zagreb2 / m = 4, no triangle
    if (d.cost != 16.0f || d.computed != (0xFFu | 0xF000u) || d.inv[12] != 2.5) return 4;
    if (azd_device_count() == 0) return 0;
    azdopt::DenseGraphInvXSpace big(20, 0.2, 128, deg.scale(0.0001f));
    azdopt::HashStreamModel model(big.STATE_DIM(), big.ACTION_DIM(), 1);
    auto roots = big.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphInvXSpace>::par_new(big, roots, model, 16);
    azdopt::DenseInvxArgmin a = opt.argmin_data();
    return a.cost.cost == big.cost(a.adj.data()).cost ? 0 : 2;
}
""")
    exe = tmp_path / "invx"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
