"""The extended invariant cost up to 64 vertices without a GPU: azd_dense_invx_cost_wide (dense_cost_host.cpp) equal to the Python reference
(tests/dense_invx_wide_ref.py) as bytes on the 88 graphs of graph_set_wide() under the five new recipes and BOTH, to
azd_dense_invx_cost as bytes on every fifth graph of the n <= 32 set, and under the converted INV recipes to azd_dense_inv_cost_wide;
the argument checks of the new calls and of AZD_ENGINE_DENSE_INVX_WIDE, made before any device is looked for; the pool plan; the
Python and C++ hosts."""
import ctypes as C
import struct

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as I
import dense_invx_ref as R
import dense_invx_wide_ref as W

c_recipe, c_inv_recipe = R.c_recipe, R.c_inv_recipe


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


def host_cost(lib, adj, n, recipe, wide=True):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseInvxCost()
    rc = recipe if isinstance(recipe, _lib.DenseInvxRecipe) else c_recipe(recipe)
    st = (lib.azd_dense_invx_cost_wide if wide else lib.azd_dense_invx_cost)(_lib.ptr(a), n, C.byref(rc), C.byref(out))
    return st, out


def reference_bytes(r):
    """the Python reference's record in azd_dense_invx_cost_t's layout"""
    return struct.pack("<16diIff", *[r[k] for k in R.NAMES], r["dist_k"], r["computed"], r["cost"], r["eval"])


def why(lib):
    return lib.azd_last_error().decode()


def test_symbols_are_exported_and_bound(lib):
    import os
    from azdopt_amd import _lib
    for name in ("azd_dense_invx_cost_wide", "azd_debug_probe_invx_cost_wide", "azd_engine_dense_invx_wide_argmin_data"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_INVX_WIDE_MAX_N == 64 == W.INVX_WIDE_MAX_N and _lib.DENSE_INVX_MAX_N == 32
    assert _lib.ENGINE_DENSE_INVX_WIDE == 8192 and _lib.ENGINE_DENSE_INVX == 4096
    assert C.sizeof(_lib.DenseInvxWideArgmin) == 8 * 64 + 8 * 32 + 8 * 16 + 4 * 6 == 920
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "azdopt_amd.h")).read()
    assert "#define AZD_ENGINE_DENSE_INVX_WIDE 8192u" in hdr and "#define AZD_DENSE_INVX_WIDE_MAX_N 64" in hdr and "#define AZD_DENSE_INVX_MAX_N 32" in hdr


def test_wide_host_cost_equals_the_python_reference_as_bytes(lib):
    W.prime_graphs(W.graph_set_wide(), ks_of=lambda n: (0, 1, n - 2, n - 1))
    seen = 0
    for name, n, adj in W.graph_set_wide():
        for rname in W.NEW_RECIPES + ("BOTH",):
            recipe = W.RECIPES[rname](n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, rname, why(lib))
            r = W.invx_cost(adj, n, recipe)
            assert bytes(out) == reference_bytes(r), (name, n, rname, list(out.inv), r)
            seen += 1
    assert seen == 6 * 88


def test_wide_host_cost_is_the_narrow_one_up_to_32_vertices(lib):
    seen = 0
    for name, n, adj in A.graph_set()[::5]:
        for rname in W.NEW_RECIPES + ("BOTH",):
            rc = c_recipe(W.RECIPES[rname](n))
            (sw, w), (sn, nr) = host_cost(lib, adj, n, rc), host_cost(lib, adj, n, rc, wide=False)
            assert sw == 0 == sn and bytes(w) == bytes(nr), (name, n, rname)
            seen += 1
    assert seen == 6 * 112


def test_the_converted_inv_recipes_give_the_inv_wide_host_function(lib):
    """inv[0 .. 9], dist_k, computed, cost and eval of azd_dense_invx_cost_wide under a converted INV recipe == azd_dense_inv_cost_wide's"""
    from azdopt_amd import _lib
    seen = 0
    for name, n, adj in W.graph_set_wide():
        a = np.array(adj, dtype=np.uint64)
        for rname in W.INV_RECIPES:
            st, x = host_cost(lib, adj, n, W.RECIPES[rname](n))
            i, ri = _lib.DenseInvCost(), c_inv_recipe(I.RECIPES[rname](n))
            assert st == 0 == lib.azd_dense_inv_cost_wide(_lib.ptr(a), n, C.byref(ri), C.byref(i)), (name, n, rname, why(lib))
            assert bytes(x)[:80] + bytes(x)[128:] == bytes(i), (name, n, rname, list(x.inv), list(i.inv))
            assert list(x.inv)[10:] == [0.0] * 6
            seen += 1
    assert seen == 4 * 88


def test_wide_cost_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    for n in (3, 65, 0, -1):
        st, _ = host_cost(lib, A.path(min(max(n, 4), 64)), n, R.recipe_deg(8))
        assert st == 1 and why(lib).startswith("azd_dense_invx_cost_wide: n") and "AZD_DENSE_INVX_WIDE_MAX_N" in why(lib), (n, why(lib))
    st, out = host_cost(lib, A.path(64), 64, R.recipe_all4(64))
    assert st == 0 and out.computed == 0xFFF
    # the narrow call keeps its limit and its text
    st, _ = host_cost(lib, A.path(33), 33, R.recipe_deg(33), wide=False)
    assert st == 1 and why(lib) == "azd_dense_invx_cost: n: the extended invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVX_MAX_N)"
    ok = R.recipe_all4(40)
    two_paths = A.from_edges(40, [(i, i + 1) for i in range(39) if i != 19])
    st, _ = host_cost(lib, two_paths, 40, ok)
    assert st == 1 and "adj" in why(lib) and "connected" in why(lib)
    beyond = list(A.path(40))
    beyond[0] |= 1 << 40
    for bad in (beyond, [1 << 1] + [0] * 39, [0b0011, 0b0001] + [0] * 38):  # a bit at n, an asymmetric row, a loop
        st, _ = host_cost(lib, bad, 40, ok)
        assert st == 1 and "adj" in why(lib), bad[:2]
    # the recipe's indices are checked against the n of the call: 0 .. n - 1
    for field in ("adj_index", "dist_index", "lap_index", "slap_index"):
        for k in (40, 64):
            st, _ = host_cost(lib, A.cycle(40), 40, R.Recipe({"adj_eig": 1.0, "dist_eig": 1.0, "lap_eig": 1.0, "slap_eig": 1.0}, **{field: k}))
            assert st == 1 and why(lib).split(": ")[1] == field, (field, k, why(lib))
    st, out = host_cost(lib, A.cycle(40), 40, R.Recipe({"adj_eig": 1.0, "dist_eig": 1.0, "lap_eig": 1.0, "slap_eig": 1.0}, adj_index=39, dist_index=39,
                                                     lap_index=39, slap_index=39))  # index n - 1 is accepted
    assert st == 0 and out.dist_k == 39 and abs(out.inv[10]) <= 1e-9
    a = np.array(A.path(40), dtype=np.uint64)
    rc = c_recipe(ok)
    assert lib.azd_dense_invx_cost_wide(None, 40, C.byref(rc), C.byref(_lib.DenseInvxCost())) == 1
    assert lib.azd_dense_invx_cost_wide(_lib.ptr(a), 40, C.byref(rc), None) == 1 and "out" in why(lib)
    assert lib.azd_dense_invx_cost_wide(_lib.ptr(a), 40, None, C.byref(_lib.DenseInvxCost())) == 1 and "recipe" in why(lib)


def test_wide_probe_checks_graphs_and_recipe_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseInvxCost * 2)()
    rc = c_recipe(R.recipe_all4(40))
    a = np.zeros(2 * 65, dtype=np.uint64)
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 65, 2, 1, C.byref(rc), out, None) == 1 and "n:" in why(lib)
    a = np.array(list(A.path(40)) + [0] * 40, dtype=np.uint64)
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(rc), out, None) == 1
    assert "graph 1" in why(lib) and "azd_debug_probe_invx_cost_wide" in why(lib)
    a = np.array(A.path(40) + A.cycle(40), dtype=np.uint64)
    bad = c_recipe(R.recipe_all4(40))
    bad.lap_index = 40
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(bad), out, None) == 1 and why(lib).split(": ")[1] == "lap_index"
    bad = c_recipe(R.recipe_ratio(40))
    bad.term[0].b = 16
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(bad), out, None) == 1 and why(lib).split(": ")[1] == "term.b"
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 40, 2, 1, None, out, None) == 1 and "recipe" in why(lib)
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 40, 2, 0, C.byref(rc), out, None) == 1
    assert lib.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(rc), None, None) == 1
    a = np.array(A.path(33) + A.path(33), dtype=np.uint64)  # the narrow probe keeps its limit and its text
    assert lib.azd_debug_probe_invx_cost(0, _lib.ptr(a), 33, 2, 1, C.byref(rc), out, None) == 1
    assert why(lib) == "azd_debug_probe_invx_cost: graph 0: n: the extended invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVX_MAX_N)"
    assert lib.azd_engine_dense_invx_wide_argmin_data(None, C.byref(_lib.DenseInvxWideArgmin())) == 1


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_INVX_WIDE: configuration checks, without a device
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
    INVX, WIDE, D = _lib.ENGINE_DENSE_INVX, _lib.ENGINE_DENSE_INVX_WIDE, _lib.SPACE_DENSE
    NO_DEVICE = 2
    import azdopt_amd as az
    accepted = (0,) if az.device_count() > 0 else (NO_DEVICE,)  # without a GPU the accepted configuration gets as far as the device
    for n, ms in ((50, 128), (64, 640), (33, 1), (20, 128), (4, 6), (50, 612)):
        for extra in (0, _lib.ENGINE_EXT_POOL_F32):  # the pool step's fp32 evaluator is accepted beside it
            st, text = _create(lib, D, n, INVX | WIDE | extra, max_slots=ms)
            assert st in accepted, (n, ms, st, text)
    st, text = _create(lib, D, 50, WIDE)  # the new flag alone
    assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INVX_WIDE is valid only beside AZD_ENGINE_DENSE_INVX" in text, text
    for space, kw in ((_lib.SPACE_C21, dict(n=19)), (_lib.SPACE_RAMSEY, dict(n=16, n_colors=3))):
        n = kw.pop("n")
        st, text = _create(lib, space, n, WIDE, **kw)
        assert st == 1 and text.startswith("flags:"), text
        st, text = _create(lib, space, n, INVX | WIDE, **kw)
        assert st == 1 and text.startswith("space_id:") and "AZD_ENGINE_DENSE_INVX_WIDE" in text, text
    # beside any AH or INV flag, with or without the flag it belongs to
    for other in (_lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_INV,
                  _lib.ENGINE_DENSE_INV_WIDE, _lib.ENGINE_DENSE_INV | _lib.ENGINE_DENSE_INV_WIDE):
        st, text = _create(lib, D, 50, INVX | WIDE | other)
        assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INVX_WIDE" in text and "cannot be combined" in text, (other, text)
        st, text = _create(lib, D, 50, WIDE | other)
        assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INVX_WIDE" in text, (other, text)
    for n in (3, 65):
        st, text = _create(lib, D, n, INVX | WIDE, max_slots=3)
        assert st == 1 and text.startswith("n:") and "64" in text, (n, text)
    st, text = _create(lib, D, 50, INVX | WIDE, layers=2)
    assert st == 1 and text.startswith("layers:"), text
    st, text = _create(lib, D, 50, INVX | WIDE, path_kind=1)
    assert st == 1 and text.startswith("path_kind:"), text
    for n, ms in ((50, 641), (64, 641), (50, 0), (50, -1), (8, 29)):  # above 640; below 1; above E = 28
        st, text = _create(lib, D, n, INVX | WIDE, max_slots=ms)
        assert st == 1 and text.startswith("max_slots:") and "640" in text, (n, ms, text)
    # AZD_ENGINE_DENSE_INVX alone keeps its limit and its text
    st, text = _create(lib, D, 33, INVX)
    assert st == 1 and text == "n: the extended invariant cost needs 4 <= n <= 32 (AZD_DENSE_INVX_MAX_N)", text


def test_pool_plan_of_a_wide_engine_is_the_inv_wide_tiers(lib):
    """arithmetic only: as many wavefronts per searcher workgroup as a CU's 160 KB hold of the 20-KB blocks -- the INV-wide tier's
    plan, waves and bytes, since the block is that tier's -- for the three key widths"""
    from azdopt_amd import _lib
    INVX, WIDE, D = _lib.ENGINE_DENSE_INVX, _lib.ENGINE_DENSE_INVX_WIDE, _lib.SPACE_DENSE
    waves, lds = C.c_int(0), C.c_size_t(0)
    for n, ms in ((50, 128), (50, 256), (50, 640)):
        cfg = _cfg(D, n, INVX | WIDE, max_slots=ms, batch=256)
        assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0, why(lib)
        iw_waves, iw_lds = C.c_int(0), C.c_size_t(0)
        iw = _cfg(D, n, _lib.ENGINE_DENSE_INV | _lib.ENGINE_DENSE_INV_WIDE, max_slots=ms, batch=256)
        assert lib.azd_debug_ext_pool_plan(C.byref(iw), C.byref(iw_waves), C.byref(iw_lds)) == 0, why(lib)
        assert (waves.value, lds.value) == (iw_waves.value, iw_lds.value) and waves.value == 6, (ms, waves.value, lds.value, iw_waves.value, iw_lds.value)
        assert waves.value * 20000 < lds.value <= 160 * 1024
    cfg = _cfg(D, 50, INVX, max_slots=128)  # n = 50 without the wide flag: refused as by azd_engine_create
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1
    cfg = _cfg(D, 31, INVX, max_slots=128)  # the narrow tier's plan is not asked for by this flag
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1


def test_python_space_carries_invx_wide():
    import azdopt_amd as az
    from azdopt_amd import _lib
    recipe = R.recipe_ratio(50)
    cost = az.InvariantCostX(recipe.weights(), **recipe.kwargs())
    sp = az.DenseGraphSpace(50, 0.2, max_slots=128, cost=cost, invx_wide=True)
    assert sp.COST == "invx" and sp.INVX is cost and sp.INVX_WIDE and not sp.AH_WIDE and not sp.INV_WIDE
    narrow = az.InvariantCostX({"lap_eig": 1.0}, lap_index=29)
    assert not az.DenseGraphSpace(31, cost=narrow).INVX_WIDE and not az.DenseGraphSpace(50).INVX_WIDE
    assert (sp.STATE_DIM, sp.ACTION_DIM, sp.MAX_SLOTS) == (3676, 2450, 128)
    assert az.DenseGraphSpace(50, cost=cost, invx_wide=True, max_slots=1024).MAX_SLOTS == 640
    assert az.DenseGraphSpace(8, cost=cost, invx_wide=True, max_slots=1024).MAX_SLOTS == 28
    assert az.DenseGraphSpace(50, max_slots=1024).MAX_SLOTS == 1024
    inv = az.InvariantCost.aouchiche_hansen(50)
    for kw in (dict(cost="c21"), dict(cost="ah"), dict(cost="ah", ah_wide=True), dict(cost=inv), dict(cost=inv, inv_wide=True), dict()):
        with pytest.raises(ValueError, match="invx_wide"):
            az.DenseGraphSpace(50, invx_wide=True, **kw)
    with pytest.raises(ValueError, match="ah_wide"):  # ah_wide and inv_wide keep their meaning and their errors
        az.DenseGraphSpace(50, cost=cost, ah_wide=True)
    with pytest.raises(ValueError, match="inv_wide=True needs cost=InvariantCost"):
        az.DenseGraphSpace(50, cost=cost, inv_wide=True)
    got = sp.invx_cost(A.cycle(50))
    want = W.invx_cost(A.cycle(50), 50, recipe)
    assert all(got[k] == want[k] for k in want), (got, want)
    assert got["computed"] == 0xFF | 1 << 8 and got["radius"] == 25.0
    with pytest.raises(az.AzdError):  # the narrow space's host cost keeps its limit
        az.DenseGraphSpace(50, cost=cost).invx_cost(A.cycle(50))
    # the flags NablaOptimizer.par_new sets are the configuration the engine accepts
    assert _lib.ENGINE_DENSE_INVX | _lib.ENGINE_DENSE_INVX_WIDE == 12288


def test_cpp_binding_compiles_with_a_wide_extended_invariant_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "invxw.cpp"
    src.write_text("""
#include "azdopt_amd.hpp"
int main() {
    azdopt::InvariantCostX lap;
    lap.weight("lap_eig", 1.0).weight("max_degree", -0.25).term(0.5, "remoteness", '/', "radius").lap_index(48).offset(50.0f).scale(0.005f);
    azdopt::DenseGraphInvXSpace space(50, 0.2, 128, lap, true);
    azd_engine_config cfg{};
    space.configure(cfg);
    if (cfg.flags != (AZD_ENGINE_DENSE_INVX | AZD_ENGINE_DENSE_INVX_WIDE) || AZD_DENSE_INVX_WIDE_MAX_N != 64 || !space.wide()) return 1;
    azdopt::DenseGraphInvXSpace narrow(20, 0.2, 128, azdopt::InvariantCostX().weight("zagreb1", 1.0));
    azd_engine_config ncfg{};
    narrow.configure(ncfg);
    if (ncfg.flags != AZD_ENGINE_DENSE_INVX || narrow.wide()) return 5;
    uint64_t c64[64];
    for (int v = 0; v < 64; ++v) c64[v] = (1ull << ((v + 1) % 64)) | (1ull << ((v + 63) % 64));
    azdopt::InvariantCostX all;
    all.weight("lap_eig", 1.0).weight("zagreb2", 1.0).weight("randic", 1.0).lap_index(0);
    azdopt::DenseGraphInvXSpace s64(64, 0.2, 128, all, true);
    azd_dense_invx_cost_t i = s64.cost(c64);  // C_64: Laplacian index 4, zagreb2 = 4 n, randic = n / 2
    if (i.inv[0] != 64.0 || i.inv[3] != 32.0 || i.inv[14] != 256.0 || i.inv[12] != 32.0 || i.inv[10] < 3.999999 || i.inv[10] > 4.000001) return 3;
    if (i.computed != (0xFFu | 1u << 10 | 1u << 12 | 1u << 14)) return 4;
    azd_dense_invx_cost_t o;
    if (azd_dense_invx_cost(c64, 64, &s64.invariant_cost().recipe(), &o) != AZD_ERR_INVALID_ARGUMENT) return 6;
    if (azd_device_count() == 0) return 0;
    azdopt::HashStreamModel model(space.STATE_DIM(), space.ACTION_DIM(), 1);
    auto roots = space.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphInvXSpace>::par_new(space, roots, model, 16);
    azdopt::DenseInvxArgmin a = opt.argmin_data();
    return a.cost.cost == space.cost(a.adj.data()).cost && (int)a.adj.size() == 50 ? 0 : 2;
}
""")
    exe = tmp_path / "invxw"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
