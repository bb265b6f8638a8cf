"""The spectrum invariant cost up to 64 vertices without a GPU: azd_dense_invs_cost_wide (dense_cost_host.cpp) equal to the Python reference
(tests/dense_invs_wide_ref.py) as bytes on the 88 graphs of graph_set_wide() under the five new recipes; azd_dense_invs_spectrum_wide
eigenvalue by eigenvalue; equal to azd_dense_invs_cost as bytes on every fifth graph of the n <= 32 set, and under the converted INVX
recipes to azd_dense_invx_cost_wide; the argument checks of the new calls and of AZD_ENGINE_DENSE_INVS_WIDE, made before any device
is looked for; the missing pool plan; the Python and C++ hosts."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import dense_ah_ref as A
import dense_invs_ref as R
import dense_invs_wide_ref as W
import dense_invx_ref as X

c_recipe = R.c_recipe


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


def host_cost(lib, adj, n, recipe, wide=True):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseInvsCost()
    rc = recipe if isinstance(recipe, _lib.DenseInvsRecipe) else c_recipe(recipe)
    st = (lib.azd_dense_invs_cost_wide if wide else lib.azd_dense_invs_cost)(_lib.ptr(a), n, C.byref(rc), C.byref(out))
    return st, out


def host_spectrum(lib, adj, n, which, wide=True):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = np.zeros(max(n, 1), np.float64)
    st = (lib.azd_dense_invs_spectrum_wide if wide else lib.azd_dense_invs_spectrum)(_lib.ptr(a), n, which, _lib.ptr(out))
    return st, out


def reference_bytes(r):
    """the Python reference's record in azd_dense_invs_cost_t's layout"""
    return struct.pack("<21diIff", *[r[k] for k in R.NAMES], r["dist_k"], r["computed"], r["cost"], r["eval"])


def why(lib):
    return lib.azd_last_error().decode()


def test_symbols_are_exported_and_bound(lib):
    import os
    from azdopt_amd import _lib
    for name in ("azd_dense_invs_cost_wide", "azd_dense_invs_spectrum_wide", "azd_debug_probe_invs_cost_wide", "azd_engine_dense_invs_wide_argmin_data"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_INVS_WIDE_MAX_N == 64 == W.INVS_WIDE_MAX_N and _lib.DENSE_INVS_MAX_N == 32
    assert _lib.ENGINE_DENSE_INVS_WIDE == 32768 and _lib.ENGINE_DENSE_INVS == 16384
    # the recipe and the record are the narrow tier's, unchanged; the argmin record: 64 rows, 32 slot words, twenty-one invariants
    assert (C.sizeof(_lib.DenseInvsRecipe), C.sizeof(_lib.DenseInvsCost), C.sizeof(_lib.DenseInvsArgmin)) == (304, 184, 512)
    assert C.sizeof(_lib.DenseInvsWideArgmin) == 8 * 64 + 8 * 32 + 8 * 21 + 4 * 6 == 960
    assert C.sizeof(_lib.DenseInvsWideArgmin) - C.sizeof(_lib.DenseInvsArgmin) == C.sizeof(_lib.DenseInvxWideArgmin) - C.sizeof(_lib.DenseInvxArgmin)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "azdopt_amd.h")).read()
    assert "#define AZD_ENGINE_DENSE_INVS_WIDE 32768u" in hdr and "#define AZD_DENSE_INVS_WIDE_MAX_N 64" in hdr and "#define AZD_DENSE_INVS_MAX_N 32" in hdr


def test_wide_host_cost_equals_the_python_reference_as_bytes(lib):
    entries = W.graph_set_wide()
    W.prime_graphs(entries)
    seen = 0
    for name, n, adj in entries:
        for rname in W.NEW_RECIPES:
            recipe = W.RECIPES[rname](n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, rname, why(lib))
            r = W.invs_cost(adj, n, recipe)
            assert bytes(out) == reference_bytes(r), (name, n, rname, list(out.inv), r)
            assert all(math.isfinite(x) for x in out.inv) and 0.0 <= out.eval <= 1.0, (name, n, rname, out.eval)
            seen += 1
    assert seen == 5 * 88


def test_wide_host_spectrum_equals_the_references_eigenvalue_by_eigenvalue(lib):
    entries = W.graph_set_wide()
    W.prime_graphs(entries)
    seen = 0
    for name, n, adj in entries:
        for w, which in enumerate(R.WHICH):
            st, th = host_spectrum(lib, adj, n, w)
            assert st == 0, (name, which, why(lib))
            want = W.spectrum(adj, n, which)
            for l in range(n):
                assert np.float64(th[l]).view(np.uint64) == np.float64(want[l]).view(np.uint64), (name, n, which, l, th[l], want[l])
            assert np.all(np.diff(th) >= 0.0), (name, which)  # ascending
            seen += 1
    assert seen == 4 * 88
    st, _ = host_spectrum(lib, A.path(40), 40, 4)
    assert st == 1 and why(lib).startswith("azd_dense_invs_spectrum_wide: which")
    for n in (3, 65):
        st, _ = host_spectrum(lib, A.path(min(max(n, 4), 64)), n, 0)
        assert st == 1 and why(lib).startswith("azd_dense_invs_spectrum_wide: n") and "AZD_DENSE_INVS_WIDE_MAX_N" in why(lib), (n, why(lib))
    from azdopt_amd import _lib
    a = np.array(A.path(40), dtype=np.uint64)
    assert lib.azd_dense_invs_spectrum_wide(_lib.ptr(a), 40, 0, None) == 1 and "out" in why(lib)
    # the narrow call keeps its limit and its text
    st, _ = host_spectrum(lib, A.path(33), 33, 0, wide=False)
    assert st == 1 and why(lib) == "azd_dense_invs_spectrum: n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)"


def test_wide_host_calls_are_the_narrow_ones_up_to_32_vertices(lib):
    seen = 0
    for name, n, adj in A.graph_set()[::5]:
        for rname in W.NEW_RECIPES:
            rc = c_recipe(W.RECIPES[rname](n))
            (sw, w), (sn, nr) = host_cost(lib, adj, n, rc), host_cost(lib, adj, n, rc, wide=False)
            assert sw == 0 == sn and bytes(w) == bytes(nr), (name, n, rname)
            seen += 1
        for which in range(4):
            (sw, w), (sn, nr) = host_spectrum(lib, adj, n, which), host_spectrum(lib, adj, n, which, wide=False)
            assert sw == 0 == sn and w.tobytes() == nr.tobytes(), (name, n, which)
    assert seen == 5 * 112


def test_the_converted_invx_recipes_give_the_invx_wide_host_function(lib):
    """inv[0 .. 15], dist_k, computed, cost and eval of azd_dense_invs_cost_wide under a converted INVX recipe == azd_dense_invx_cost_wide's"""
    from azdopt_amd import _lib
    seen = 0
    for name, n, adj in W.graph_set_wide():
        a = np.array(adj, dtype=np.uint64)
        for rname in W.INVX_RECIPES:
            st, s = host_cost(lib, adj, n, W.RECIPES[rname](n))
            x, rx = _lib.DenseInvxCost(), X.c_recipe(X.RECIPES[rname](n))
            assert st == 0 == lib.azd_dense_invx_cost_wide(_lib.ptr(a), n, C.byref(rx), C.byref(x)), (name, n, rname, why(lib))
            assert bytes(s)[:128] + bytes(s)[168:] == bytes(x), (name, n, rname, list(s.inv), list(x.inv))
            assert list(s.inv)[16:] == [0.0] * 5
            seen += 1
    assert seen == 9 * 88


def test_wide_cost_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    for n in (3, 65, 0, -1):
        st, _ = host_cost(lib, A.path(min(max(n, 4), 64)), n, R.recipe_energy(8))
        assert st == 1 and why(lib).startswith("azd_dense_invs_cost_wide: n") and "AZD_DENSE_INVS_WIDE_MAX_N" in why(lib), (n, why(lib))
        assert "the wide spectrum invariant cost needs 4 <= n <= 64" in why(lib)
    st, out = host_cost(lib, A.path(64), 64, R.recipe_alle(64))
    assert st == 0 and out.computed == 0xFF | 0xF00 | 0x1F0000
    # the narrow call keeps its limit and its text
    st, _ = host_cost(lib, A.path(33), 33, R.recipe_energy(33), wide=False)
    assert st == 1 and why(lib) == "azd_dense_invs_cost: n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)"
    ok = R.recipe_alle(40)
    two_paths = A.from_edges(40, [(i, i + 1) for i in range(39) if i != 19])
    st, _ = host_cost(lib, two_paths, 40, ok)
    assert st == 1 and "adj" in why(lib) and "connected" in why(lib)
    beyond = list(A.path(40))
    beyond[0] |= 1 << 40
    for bad in (beyond, [1 << 1] + [0] * 39, [0b0011, 0b0001] + [0] * 38):  # a bit at n, an asymmetric row, a loop
        st, _ = host_cost(lib, bad, 40, ok)
        assert st == 1 and "adj" in why(lib), bad[:2]
    # the recipe's indices are checked against the n of the call: 0 .. n - 1
    four = {"adj_eig": 1.0, "dist_eig": 1.0, "lap_eig": 1.0, "slap_eig": 1.0}
    for field in ("adj_index", "dist_index", "lap_index", "slap_index"):
        for k in (40, 64):
            st, _ = host_cost(lib, A.cycle(40), 40, R.Recipe(four, **{field: k}))
            assert st == 1 and why(lib).split(": ")[1] == field, (field, k, why(lib))
    st, out = host_cost(lib, A.cycle(40), 40, R.Recipe(four, adj_index=39, dist_index=39, lap_index=39, slap_index=39))  # index n - 1 is accepted
    assert st == 0 and out.dist_k == 39 and abs(out.inv[10]) <= 1e-9
    a = np.array(A.path(40), dtype=np.uint64)
    rc = c_recipe(ok)
    assert lib.azd_dense_invs_cost_wide(None, 40, C.byref(rc), C.byref(_lib.DenseInvsCost())) == 1
    assert lib.azd_dense_invs_cost_wide(_lib.ptr(a), 40, C.byref(rc), None) == 1 and why(lib) == "azd_dense_invs_cost_wide: out: null"
    assert lib.azd_dense_invs_cost_wide(_lib.ptr(a), 40, None, C.byref(_lib.DenseInvsCost())) == 1 and "recipe" in why(lib)


def test_wide_probe_checks_graphs_and_recipe_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseInvsCost * 2)()
    rc = c_recipe(R.recipe_alle(40))
    a = np.zeros(2 * 65, dtype=np.uint64)
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 65, 2, 1, C.byref(rc), out, None) == 1 and "n:" in why(lib)
    a = np.array(list(A.path(40)) + [0] * 40, dtype=np.uint64)
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(rc), out, None) == 1
    assert "graph 1" in why(lib) and "azd_debug_probe_invs_cost_wide" in why(lib)
    a = np.array(A.path(40) + A.cycle(40), dtype=np.uint64)
    bad = c_recipe(R.recipe_alle(40))
    bad.lap_index = 40
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(bad), out, None) == 1 and why(lib).split(": ")[1] == "lap_index"
    bad = c_recipe(R.recipe_eratio(40))
    bad.term[0].b = 21
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(bad), out, None) == 1 and why(lib).split(": ")[1] == "term.b"
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 40, 2, 1, None, out, None) == 1 and "recipe" in why(lib)
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 40, 2, 0, C.byref(rc), out, None) == 1
    assert lib.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(rc), None, None) == 1
    a = np.array(A.path(33) + A.path(33), dtype=np.uint64)  # the narrow probe keeps its limit and its text
    assert lib.azd_debug_probe_invs_cost(0, _lib.ptr(a), 33, 2, 1, C.byref(rc), out, None) == 1
    assert why(lib) == "azd_debug_probe_invs_cost: graph 0: n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)"
    assert lib.azd_engine_dense_invs_wide_argmin_data(None, C.byref(_lib.DenseInvsWideArgmin())) == 1


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_INVS_WIDE: configuration checks, without a device
def _cfg(space_id, n, flags, layers=0, max_slots=128, path_kind=0, n_colors=0, batch=4):
    from azdopt_amd import _lib
    cfg = _lib.EngineConfig(space_id, n, batch, 0, 0, 0, 0, 0, flags)
    cfg.layers, cfg.max_slots, cfg.path_kind, cfg.dense_p, cfg.n_colors = layers, max_slots, path_kind, 0.4, n_colors
    for i in range(n_colors):
        cfg.clique_sizes[i], cfg.color_weights[i] = 3, 1.0
    return cfg


def _create(lib, *a, **kw):
    cfg = _cfg(*a, **kw)
    h = C.c_void_p()
    st = lib.azd_engine_create(C.byref(h), C.byref(cfg), None)
    if st == 0:
        lib.azd_engine_destroy(h)
    return st, lib.azd_last_error().decode()


def test_wide_flag_is_validated_before_the_device_is_looked_for(lib):
    from azdopt_amd import _lib
    INVS, WIDE, D = _lib.ENGINE_DENSE_INVS, _lib.ENGINE_DENSE_INVS_WIDE, _lib.SPACE_DENSE
    NO_DEVICE = 2
    import azdopt_amd as az
    accepted = (0,) if az.device_count() > 0 else (NO_DEVICE,)  # without a GPU the accepted configuration gets as far as the device
    for n, ms in ((50, 128), (64, 640), (33, 1), (20, 128), (4, 6), (50, 612)):
        for extra in (0, _lib.ENGINE_EXT_POOL_F32):  # the pool step's fp32 evaluator is accepted beside it (and changes nothing)
            st, text = _create(lib, D, n, INVS | WIDE | extra, max_slots=ms)
            assert st in accepted, (n, ms, st, text)
    st, text = _create(lib, D, 50, WIDE)  # the new flag alone
    assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INVS_WIDE is valid only beside AZD_ENGINE_DENSE_INVS" in text, text
    for space, kw in ((_lib.SPACE_C21, dict(n=19)), (_lib.SPACE_RAMSEY, dict(n=16, n_colors=3))):
        n = kw.pop("n")
        st, text = _create(lib, space, n, WIDE, **kw)
        assert st == 1 and text.startswith("flags:"), text
        st, text = _create(lib, space, n, INVS | WIDE, **kw)
        assert st == 1 and text.startswith("space_id:") and "AZD_ENGINE_DENSE_INVS_WIDE" in text, text
    # beside any AH, INV or INVX flag, with or without the flag it belongs to
    for other in (_lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_INV,
                  _lib.ENGINE_DENSE_INV_WIDE, _lib.ENGINE_DENSE_INV | _lib.ENGINE_DENSE_INV_WIDE, _lib.ENGINE_DENSE_INVX, _lib.ENGINE_DENSE_INVX_WIDE,
                  _lib.ENGINE_DENSE_INVX | _lib.ENGINE_DENSE_INVX_WIDE):
        st, text = _create(lib, D, 50, INVS | WIDE | other)
        assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INVS_WIDE" in text and "cannot be combined" in text, (other, text)
        st, text = _create(lib, D, 50, WIDE | other)
        assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INVS_WIDE" in text, (other, text)
    for n in (3, 65):
        st, text = _create(lib, D, n, INVS | WIDE, max_slots=3)
        assert st == 1 and text == "n: the wide spectrum invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVS_WIDE_MAX_N)", (n, text)
    st, text = _create(lib, D, 50, INVS | WIDE, layers=2)
    assert st == 1 and text.startswith("layers:") and "AZD_ENGINE_DENSE_INVS_WIDE" in text, text
    st, text = _create(lib, D, 50, INVS | WIDE, path_kind=1)  # sequence paths
    assert st == 1 and text.startswith("path_kind:") and "AZD_ENGINE_DENSE_INVS_WIDE" in text, text
    for n, ms in ((50, 641), (64, 641), (50, 0), (50, -1), (8, 29)):  # above 640; below 1; above E = 28
        st, text = _create(lib, D, n, INVS | WIDE, max_slots=ms)
        assert st == 1 and text.startswith("max_slots:") and "640" in text and "AZD_ENGINE_DENSE_INVS_WIDE" in text, (n, ms, text)
    st, text = _create(lib, D, 50, INVS | WIDE | _lib.ENGINE_EXT_POOL_F32 | _lib.ENGINE_NO_PERSISTENT_STEP)
    assert st == 1 and "AZD_ENGINE_EXT_POOL_F32" in text, text
    # AZD_ENGINE_DENSE_INVS alone keeps its limit and its text
    st, text = _create(lib, D, 33, INVS)
    assert st == 1 and text == "n: the spectrum invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVS_MAX_N)", text
    # ... and the other wide tiers theirs
    st, text = _create(lib, D, 65, _lib.ENGINE_DENSE_INVX | _lib.ENGINE_DENSE_INVX_WIDE)
    assert st == 1 and text == "n: the wide extended invariant cost needs 4 <= n <= 64 (AZD_DENSE_INVX_WIDE_MAX_N)", text


def test_the_wide_tier_has_no_pool_step_plan(lib):
    """azd_debug_ext_pool_plan (arithmetic only): no pool searchers are built for this tier either, and the plan says so, with or
    without the fp32 request, exactly as for the narrow tier; the INVX-wide tier's plan stands"""
    from azdopt_amd import _lib
    INVS, WIDE, D = _lib.ENGINE_DENSE_INVS, _lib.ENGINE_DENSE_INVS_WIDE, _lib.SPACE_DENSE
    waves, lds = C.c_int(), C.c_size_t()
    for n, ms in ((50, 128), (50, 256), (64, 640), (20, 128)):
        for extra in (0, _lib.ENGINE_EXT_POOL_F32):
            cfg = _cfg(D, n, INVS | WIDE | extra, max_slots=ms, batch=256)
            assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 8, (n, ms, extra)
            assert why(lib) == "azd_debug_ext_pool_plan: the configuration's tier has no searcher-only pool step"
    cfg = _cfg(D, 31, INVS | _lib.ENGINE_EXT_POOL_F32, max_slots=128)  # the narrow tier's answer, the same text
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 8
    assert why(lib) == "azd_debug_ext_pool_plan: the configuration's tier has no searcher-only pool step"
    cfg = _cfg(D, 65, INVS | WIDE, max_slots=128)  # refused as by azd_engine_create
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1
    cfg = _cfg(D, 50, _lib.ENGINE_DENSE_INVX | _lib.ENGINE_DENSE_INVX_WIDE, max_slots=128, batch=256)
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0 and waves.value == 6


def test_python_space_carries_invs_wide():
    import azdopt_amd as az
    from azdopt_amd import _lib
    recipe = R.recipe_eratio(50)
    cost = az.InvariantCostS(recipe.weights(), terms=recipe.terms, eval_offset=float(recipe.eval_offset), eval_scale=float(recipe.eval_scale))
    sp = az.DenseGraphSpace(50, 0.2, max_slots=128, cost=cost, invs_wide=True)
    assert sp.COST == "invs" and sp.INVS is cost and sp.INVX is None and sp.INVS_WIDE and not sp.AH_WIDE and not sp.INV_WIDE and not sp.INVX_WIDE
    assert not az.DenseGraphSpace(31, cost=cost).INVS_WIDE and not az.DenseGraphSpace(50).INVS_WIDE
    assert (sp.STATE_DIM, sp.ACTION_DIM, sp.MAX_SLOTS) == (3676, 2450, 128)
    assert az.DenseGraphSpace(50, cost=cost, invs_wide=True, max_slots=1024).MAX_SLOTS == 640
    assert az.DenseGraphSpace(8, cost=cost, invs_wide=True, max_slots=1024).MAX_SLOTS == 28
    assert az.DenseGraphSpace(31, cost=cost, max_slots=1024).MAX_SLOTS == 465 and az.DenseGraphSpace(50, max_slots=1024).MAX_SLOTS == 1024
    inv = az.InvariantCost.aouchiche_hansen(50)
    invx = az.InvariantCostX({"lap_eig": 1.0}, lap_index=48)
    for kw in (dict(cost="c21"), dict(cost="ah"), dict(cost="ah", ah_wide=True), dict(cost=inv), dict(cost=inv, inv_wide=True), dict(cost=invx),
               dict(cost=invx, invx_wide=True), dict()):
        with pytest.raises(ValueError, match="invs_wide"):
            az.DenseGraphSpace(50, invs_wide=True, **kw)
    with pytest.raises(ValueError, match="ah_wide"):  # the other wide switches keep their meaning and their errors
        az.DenseGraphSpace(50, cost=cost, ah_wide=True)
    with pytest.raises(ValueError, match="inv_wide=True needs cost=InvariantCost"):
        az.DenseGraphSpace(50, cost=cost, inv_wide=True)
    with pytest.raises(ValueError, match="invx_wide=True needs cost=InvariantCostX"):
        az.DenseGraphSpace(50, cost=cost, invx_wide=True)
    got = sp.invs_cost(A.cycle(50))
    want = W.invs_cost(A.cycle(50), 50, recipe)
    assert all(got[k] == want[k] for k in want), (got, want)
    assert got["computed"] == 0xFF | 1 << 16 | 1 << 20 and got["radius"] == 25.0
    assert sp.invs_spectrum(A.cycle(50), "slap").tobytes() == np.array(W.spectrum(A.cycle(50), 50, "slap")).tobytes()
    narrow = az.DenseGraphSpace(50, cost=cost)
    with pytest.raises(az.AzdError):  # the narrow space's host calls keep their limit
        narrow.invs_cost(A.cycle(50))
    with pytest.raises(az.AzdError):
        narrow.invs_spectrum(A.cycle(50))
    # the flags NablaOptimizer.par_new sets are the configuration the engine accepts
    assert _lib.ENGINE_DENSE_INVS | _lib.ENGINE_DENSE_INVS_WIDE == 49152


def test_cpp_binding_compiles_with_a_wide_spectrum_invariant_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "invsw.cpp"
    src.write_text("""
#include <cmath>
#include "azdopt_amd.hpp"
int main() {
    azdopt::InvariantCostS e;
    e.weight("adj_energy", 1.0).term(0.5, "adj_spread", '/', "lap_energy").scale(0.005f);
    azdopt::DenseGraphInvSSpace space(50, 0.2, 128, e, true);
    azd_engine_config cfg{};
    space.configure(cfg);
    if (cfg.flags != (AZD_ENGINE_DENSE_INVS | AZD_ENGINE_DENSE_INVS_WIDE) || AZD_DENSE_INVS_WIDE_MAX_N != 64 || !space.wide()) return 1;
    azdopt::DenseGraphInvSSpace narrow(20, 0.2, 128, e);
    azd_engine_config ncfg{};
    narrow.configure(ncfg);
    if (ncfg.flags != AZD_ENGINE_DENSE_INVS || narrow.wide()) return 5;
    uint64_t k64[64];
    for (int v = 0; v < 64; ++v) k64[v] = ~0ull ^ (1ull << v);
    azdopt::DenseGraphInvSSpace s64(64, 0.2, 128, e, true);
    azd_dense_invs_cost_t c = s64.cost(k64);  // K_64: energy 126, spread 64, Laplacian energy 126
    if (std::fabs(c.inv[16] - 126.0) > 1e-9 || std::fabs(c.inv[20] - 64.0) > 1e-9 || std::fabs(c.inv[18] - 126.0) > 1e-9) return 3;
    if (c.computed != (0xFFu | 1u << 16 | 1u << 18 | 1u << 20)) return 4;
    std::vector<double> th = s64.spectrum(k64, AZD_DENSE_INVS_MATRIX_ADJ);
    if (th.size() != 64 || std::fabs(th[63] - 63.0) > 1e-9 || std::fabs(th[0] + 1.0) > 1e-9) return 7;
    azd_dense_invs_cost_t o;
    if (azd_dense_invs_cost(k64, 64, &s64.invariant_cost().recipe(), &o) != AZD_ERR_INVALID_ARGUMENT) return 6;
    if (sizeof(azd_dense_invs_wide_argmin) != 960) return 8;
    if (azd_device_count() == 0) return 0;
    azdopt::HashStreamModel model(space.STATE_DIM(), space.ACTION_DIM(), 1);
    auto roots = space.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphInvSSpace>::par_new(space, roots, model, 16);
    azdopt::DenseInvsArgmin a = opt.argmin_data();
    return a.cost.cost == space.cost(a.adj.data()).cost && (int)a.adj.size() == 50 ? 0 : 2;
}
""")
    exe = tmp_path / "invsw"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
