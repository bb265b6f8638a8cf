"""The weighted-invariant cost up to 64 vertices without a GPU: azd_dense_inv_cost_wide (dense_cost_host.cpp) equal to the Python reference
(tests/dense_inv_wide_ref.py) as bytes on the 88 graphs of graph_set_wide() under the four test recipes, to azd_dense_inv_cost as
bytes on the n <= 32 set, both again on the hard case set of the spectral passes (tests/dense_spectral_cases.py), and under the AH recipe to azd_dense_ah_cost_wide; both spectra against numpy.linalg.eigvalsh within the
project's backward-error tolerance; the argument checks of the new calls and of AZD_ENGINE_DENSE_INV_WIDE, made before any device
is looked for; the pool plan; the Python and C++ hosts."""
import ctypes as C
import struct

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as R
import dense_inv_wide_ref as W
import dense_spectral_cases as S


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


def c_recipe(recipe):
    from azdopt_amd import _lib
    r = _lib.DenseInvRecipe()
    for i, w in enumerate(recipe.weight):
        r.weight[i] = w
    r.bias, r.adj_index, r.dist_index = recipe.bias, recipe.adj_index, recipe.dist_index
    r.eval_offset, r.eval_scale = float(recipe.eval_offset), float(recipe.eval_scale)
    return r


def host_cost(lib, adj, n, recipe, wide=True):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseInvCost()
    rc = recipe if isinstance(recipe, _lib.DenseInvRecipe) else c_recipe(recipe)
    st = (lib.azd_dense_inv_cost_wide if wide else lib.azd_dense_inv_cost)(_lib.ptr(a), n, C.byref(rc), C.byref(out))
    return st, out


def reference_bytes(r):
    """the Python reference's record in azd_dense_inv_cost_t's layout"""
    return struct.pack("<10diIff", *[r[k] for k in R.NAMES], r["dist_k"], r["computed"], r["cost"], r["eval"])


def why(lib):
    return lib.azd_last_error().decode()


def test_symbols_are_exported_and_bound(lib):
    import os
    from azdopt_amd import _lib
    for name in ("azd_dense_inv_cost_wide", "azd_debug_probe_inv_cost_wide", "azd_engine_dense_inv_wide_argmin_data"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_INV_WIDE_MAX_N == 64 == W.INV_WIDE_MAX_N and _lib.DENSE_INV_MAX_N == 32
    assert _lib.ENGINE_DENSE_INV_WIDE == 2048 and _lib.ENGINE_DENSE_INV == 1024
    assert C.sizeof(_lib.DenseInvWideArgmin) == 8 * 64 + 8 * 32 + 8 * 10 + 4 * 6
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "azdopt_amd.h")).read()
    assert "#define AZD_ENGINE_DENSE_INV_WIDE 2048u" in hdr and "#define AZD_DENSE_INV_WIDE_MAX_N 64" in hdr and "#define AZD_DENSE_INV_MAX_N 32" in hdr


def test_wide_host_cost_equals_the_python_reference_as_bytes(lib):
    seen = 0
    for name, n, adj in W.graph_set_wide():
        for rname, mk in sorted(W.RECIPES.items()):
            recipe = mk(n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, rname, why(lib))
            r = W.inv_cost(adj, n, recipe)
            assert bytes(out) == reference_bytes(r), (name, n, rname, list(out.inv), r)
            seen += 1
    assert seen == 4 * 88


def test_wide_host_cost_is_the_narrow_one_up_to_32_vertices(lib):
    seen = 0
    for name, n, adj in A.graph_set():
        for rname, mk in sorted(R.RECIPES.items()):
            rc = c_recipe(mk(n))
            (sw, w), (sn, nr) = host_cost(lib, adj, n, rc), host_cost(lib, adj, n, rc, wide=False)
            assert sw == 0 == sn and bytes(w) == bytes(nr), (name, n, rname)
            seen += 1
    assert seen == 4 * 560


def test_wide_host_cost_on_the_hard_spectral_cases(lib):
    """tests/dense_spectral_cases.py under an adjacency recipe (index 0) and a both-spectra recipe (adjacency n - 1, distance 1):
    beyond 32 vertices (n = 33, 40, 64: graphs other than the two brooms the deflation rule was made for) the wide host function
    equals the Python reference as bytes; up to 32 vertices it equals the narrow host function as bytes; every invariant finite"""
    import math
    wide, narrow = S.graph_set_wide(), S.graph_set()
    R.prime(wide, ("adj", "dist"), lambda n: (0, 1, n - 1))
    seen = 0
    for name, n, adj in wide + narrow:
        for rname in ("ADJ", "BOTH"):
            recipe = R.RECIPES[rname](n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, rname, why(lib))
            assert all(math.isfinite(x) for x in out.inv), (name, rname, list(out.inv))
            if n > 32:
                assert bytes(out) == reference_bytes(W.inv_cost(adj, n, recipe)), (name, rname, list(out.inv))
            else:
                sn, nr = host_cost(lib, adj, n, recipe, wide=False)
                assert sn == 0 and bytes(out) == bytes(nr), (name, rname, list(out.inv), list(nr.inv))
            seen += 1
    assert seen == 2 * (939 + 3700)


def test_the_wide_ah_cost_is_the_ah_recipe(lib):
    from azdopt_amd import _lib
    import azdopt_amd as az
    for name, n, adj in W.graph_set_wide():
        a = np.array(adj, dtype=np.uint64)
        ah = _lib.DenseAhCost()
        assert lib.azd_dense_ah_cost_wide(_lib.ptr(a), n, C.byref(ah)) == 0
        for recipe in (c_recipe(R.recipe_ah(n)), az.InvariantCost.aouchiche_hansen(n).recipe()):
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, why(lib)
            assert struct.pack("<ddiiff", out.inv[5], out.inv[9], int(out.inv[3]), out.dist_k, out.cost, out.eval) == bytes(ah), (name, n)


def test_wide_eigenvalues_against_lapack(lib):
    """both spectra at descending indices 0, 1 and n - 1 on the 88 graphs, within 64 n 2^-53 ||M||_F (the host function, which the
    test above ties to the Python reference byte for byte)"""
    worst = {"adj": (0.0, None), "dist": (0.0, None)}
    values = 0
    for name, n, adj in W.graph_set_wide():
        dist, _, _ = A.bfs_all(adj, n)
        mats = {"adj": np.array(R.adjacency_matrix(adj, n), np.float64), "dist": np.array(dist, np.float64)}
        for which, field, bit in (("adj", "adj_eig", 8), ("dist", "dist_eig", 9)):
            lap = np.linalg.eigvalsh(mats[which])[::-1]
            tol = 64.0 * n * 2.0 ** -53 * np.linalg.norm(mats[which])
            for k in (0, 1, n - 1):
                st, out = host_cost(lib, adj, n, R.Recipe({field: 1.0}, adj_index=k, dist_index=k))
                assert st == 0 and out.computed == 0xFF | 1 << bit and out.dist_k == k, (name, n, which, k, why(lib))
                err = abs(out.inv[bit] - lap[k])
                assert err <= tol, (name, n, which, k, out.inv[bit], lap[k], err / tol)
                if err / tol >= worst[which][0]:
                    worst[which] = (err / tol, (name, n, k))
                values += 1
    print("wide invariant cost vs eigvalsh over %d values: largest error / tolerance: adjacency %.4f at %s, distance %.4f at %s"
          % (values, *worst["adj"], *worst["dist"]))
    assert values == 88 * 6


def test_wide_cost_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    for n in (3, 65, 0, -1):
        st, _ = host_cost(lib, A.path(min(max(n, 4), 64)), n, R.recipe_int(8))
        assert st == 1 and why(lib).startswith("azd_dense_inv_cost_wide: n") and "AZD_DENSE_INV_WIDE_MAX_N" in why(lib), (n, why(lib))
    st, _ = host_cost(lib, A.path(64), 64, R.recipe_both(64))
    assert st == 0
    # the narrow call keeps its limit and its text
    st, _ = host_cost(lib, A.path(33), 33, R.recipe_int(33), wide=False)
    assert st == 1 and why(lib) == "azd_dense_inv_cost: n: the weighted-invariant cost needs 4 <= n <= 32 (AZD_DENSE_INV_MAX_N)"
    ok = R.recipe_both(40)
    two_paths = A.from_edges(40, [(i, i + 1) for i in range(39) if i != 19])
    st, _ = host_cost(lib, two_paths, 40, ok)
    assert st == 1 and "adj" in why(lib) and "connected" in why(lib)
    beyond = list(A.path(40))
    beyond[0] |= 1 << 40
    for bad in (beyond, [1 << 1] + [0] * 39, [0b0011, 0b0001] + [0] * 38):  # a bit at n, an asymmetric row, a loop
        st, _ = host_cost(lib, bad, 40, ok)
        assert st == 1 and "adj" in why(lib), bad[:2]
    for field, kw in (("adj_index", dict(adj_index=40)), ("dist_index", dict(dist_index=40)), ("adj_index", dict(adj_index=64))):
        st, _ = host_cost(lib, A.cycle(40), 40, R.Recipe({"adj_eig": 1.0, "dist_eig": 1.0}, **kw))
        assert st == 1 and why(lib).split(": ")[1] == field, (field, why(lib))
    st, out = host_cost(lib, A.cycle(40), 40, R.Recipe({"adj_eig": 1.0, "dist_eig": 1.0}, adj_index=39, dist_index=39))  # index n - 1 is accepted
    assert st == 0 and out.dist_k == 39
    a = np.array(A.path(40), dtype=np.uint64)
    rc = c_recipe(ok)
    assert lib.azd_dense_inv_cost_wide(None, 40, C.byref(rc), C.byref(_lib.DenseInvCost())) == 1
    assert lib.azd_dense_inv_cost_wide(_lib.ptr(a), 40, C.byref(rc), None) == 1 and "out" in why(lib)
    assert lib.azd_dense_inv_cost_wide(_lib.ptr(a), 40, None, C.byref(_lib.DenseInvCost())) == 1 and "recipe" in why(lib)


def test_wide_probe_checks_graphs_and_recipe_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseInvCost * 2)()
    rc = c_recipe(R.recipe_both(40))
    a = np.zeros(2 * 65, dtype=np.uint64)
    assert lib.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), 65, 2, 1, C.byref(rc), out, None) == 1 and "n:" in why(lib)
    a = np.array(list(A.path(40)) + [0] * 40, dtype=np.uint64)
    assert lib.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(rc), out, None) == 1
    assert "graph 1" in why(lib) and "azd_debug_probe_inv_cost_wide" in why(lib)
    a = np.array(A.path(40) + A.cycle(40), dtype=np.uint64)
    bad = c_recipe(R.recipe_both(40))
    bad.adj_index = 40
    assert lib.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(bad), out, None) == 1 and why(lib).split(": ")[1] == "adj_index"
    assert lib.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), 40, 2, 1, None, out, None) == 1 and "recipe" in why(lib)
    assert lib.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), 40, 2, 0, C.byref(rc), out, None) == 1
    assert lib.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), 40, 2, 1, C.byref(rc), None, None) == 1
    a = np.array(A.path(33) + A.path(33), dtype=np.uint64)  # the narrow probe keeps its limit and its text
    assert lib.azd_debug_probe_inv_cost(0, _lib.ptr(a), 33, 2, 1, C.byref(rc), out, None) == 1
    assert why(lib) == "azd_debug_probe_inv_cost: graph 0: n: the weighted-invariant cost needs 4 <= n <= 32 (AZD_DENSE_INV_MAX_N)"
    assert lib.azd_engine_dense_inv_wide_argmin_data(None, C.byref(_lib.DenseInvWideArgmin())) == 1


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_INV_WIDE: configuration checks, without a device
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
    INV, WIDE, D = _lib.ENGINE_DENSE_INV, _lib.ENGINE_DENSE_INV_WIDE, _lib.SPACE_DENSE
    NO_DEVICE = 2
    import azdopt_amd as az
    accepted = (0,) if az.device_count() > 0 else (NO_DEVICE,)  # without a GPU the accepted configuration gets as far as the device
    for n, ms in ((50, 128), (64, 640), (33, 1), (20, 128), (4, 6), (50, 612)):
        for extra in (0, _lib.ENGINE_EXT_POOL_F32):  # the pool step's fp32 evaluator is accepted beside it
            st, text = _create(lib, D, n, INV | WIDE | extra, max_slots=ms)
            assert st in accepted, (n, ms, st, text)
    st, text = _create(lib, D, 50, WIDE)  # the new flag alone
    assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INV_WIDE is valid only beside AZD_ENGINE_DENSE_INV" in text, text
    for space, kw in ((_lib.SPACE_C21, dict(n=19)), (_lib.SPACE_RAMSEY, dict(n=16, n_colors=3))):
        n = kw.pop("n")
        st, text = _create(lib, space, n, WIDE, **kw)
        assert st == 1 and text.startswith("flags:"), text
        st, text = _create(lib, space, n, INV | WIDE, **kw)
        assert st == 1 and text.startswith("space_id:") and "AZD_ENGINE_DENSE_INV_WIDE" in text, text
    for other in (_lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE):
        st, text = _create(lib, D, 50, INV | WIDE | other)
        assert st == 1 and text.startswith("flags:") and "AZD_ENGINE_DENSE_INV_WIDE" in text and "AZD_ENGINE_DENSE_AH" in text, text
    for n in (3, 65):
        st, text = _create(lib, D, n, INV | WIDE, max_slots=3)
        assert st == 1 and text.startswith("n:") and "64" in text, (n, text)
    st, text = _create(lib, D, 50, INV | WIDE, layers=2)
    assert st == 1 and text.startswith("layers:"), text
    st, text = _create(lib, D, 50, INV | WIDE, path_kind=1)
    assert st == 1 and text.startswith("path_kind:"), text
    for n, ms in ((50, 641), (50, 0), (50, -1), (8, 29)):  # above 640; below 1; above E = 28
        st, text = _create(lib, D, n, INV | WIDE, max_slots=ms)
        assert st == 1 and text.startswith("max_slots:") and "640" in text, (n, ms, text)
    # AZD_ENGINE_DENSE_INV alone keeps its limit and its text
    st, text = _create(lib, D, 33, INV)
    assert st == 1 and text == "n: the weighted-invariant cost needs 4 <= n <= 32 (AZD_DENSE_INV_MAX_N)", text


def test_pool_plan_of_a_wide_engine(lib):
    """arithmetic only: as many wavefronts per searcher workgroup as a CU's 160 KB hold of the 20-KB blocks -- the AH-wide tier's
    count, since the block is that tier's -- at least the form's lower bound of 4, for the three key widths"""
    from azdopt_amd import _lib
    INV, WIDE, D = _lib.ENGINE_DENSE_INV, _lib.ENGINE_DENSE_INV_WIDE, _lib.SPACE_DENSE
    waves, lds = C.c_int(0), C.c_size_t(0)
    for ms in (128, 256, 612):
        cfg = _cfg(D, 50, INV | WIDE, max_slots=ms, batch=256)
        assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0, why(lib)
        assert 4 <= waves.value <= 16 and waves.value * 20000 < lds.value <= 160 * 1024, (ms, waves.value, lds.value)
        ah_waves, ah_lds = C.c_int(0), C.c_size_t(0)
        ah = _cfg(D, 50, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE, max_slots=ms, batch=256)
        assert lib.azd_debug_ext_pool_plan(C.byref(ah), C.byref(ah_waves), C.byref(ah_lds)) == 0, why(lib)
        assert (waves.value, lds.value) == (ah_waves.value, ah_lds.value) and waves.value == 6, (ms, waves.value, ah_waves.value)
    cfg = _cfg(D, 50, INV, max_slots=128)  # n = 50 without the wide flag: refused as by azd_engine_create
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1
    cfg = _cfg(D, 31, INV, max_slots=128)  # the narrow tier's plan is not asked for by this flag
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1


def test_python_space_carries_inv_wide():
    import azdopt_amd as az
    from azdopt_amd import _lib
    cost = az.InvariantCost.aouchiche_hansen(50)
    sp = az.DenseGraphSpace(50, 0.2, max_slots=128, cost=cost, inv_wide=True)
    assert sp.COST == "inv" and sp.INV is cost and sp.INV_WIDE and not sp.AH_WIDE
    assert not az.DenseGraphSpace(31, cost=az.InvariantCost.aouchiche_hansen(31)).INV_WIDE and not az.DenseGraphSpace(50).INV_WIDE
    assert (sp.STATE_DIM, sp.ACTION_DIM, sp.MAX_SLOTS) == (3676, 2450, 128)
    assert az.DenseGraphSpace(50, cost=cost, inv_wide=True, max_slots=1024).MAX_SLOTS == 640
    assert az.DenseGraphSpace(8, cost=az.InvariantCost.aouchiche_hansen(8), inv_wide=True, max_slots=1024).MAX_SLOTS == 28
    assert az.DenseGraphSpace(50, max_slots=1024).MAX_SLOTS == 1024
    for kw in (dict(cost="c21"), dict(cost="ah"), dict(cost="ah", ah_wide=True), dict()):
        with pytest.raises(ValueError, match="inv_wide"):
            az.DenseGraphSpace(50, inv_wide=True, **kw)
    with pytest.raises(ValueError, match="ah_wide"):  # ah_wide keeps its meaning
        az.DenseGraphSpace(50, cost=cost, ah_wide=True)
    got = sp.inv_cost(A.cycle(50))
    want = W.inv_cost(A.cycle(50), 50, R.recipe_ah(50))
    assert all(got[k] == want[k] for k in want), (got, want)
    assert got["cost"] == az.DenseGraphSpace(50, 0.2, cost="ah", ah_wide=True).ah_cost(A.cycle(50))["cost"] and got["diameter"] == 25.0
    with pytest.raises(az.AzdError):  # the narrow space's host cost keeps its limit
        az.DenseGraphSpace(50, cost=cost).inv_cost(A.cycle(50))
    # the flags NablaOptimizer.par_new sets are the configuration the engine accepts
    assert _lib.ENGINE_DENSE_INV | _lib.ENGINE_DENSE_INV_WIDE == 3072


def test_cpp_binding_compiles_with_a_wide_invariant_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "invw.cpp"
    src.write_text("""
#include "azdopt_amd.hpp"
int main() {
    azdopt::DenseGraphInvSpace space(50, 0.2, 128, azdopt::InvariantCost::aouchiche_hansen(50), true);
    azd_engine_config cfg{};
    space.configure(cfg);
    if (cfg.flags != (AZD_ENGINE_DENSE_INV | AZD_ENGINE_DENSE_INV_WIDE) || AZD_DENSE_INV_WIDE_MAX_N != 64 || !space.wide()) return 1;
    azdopt::DenseGraphInvSpace narrow(20, 0.2, 128, azdopt::InvariantCost::aouchiche_hansen(20));
    azd_engine_config ncfg{};
    narrow.configure(ncfg);
    if (ncfg.flags != AZD_ENGINE_DENSE_INV || narrow.wide()) return 5;
    uint64_t c64[64];
    for (int v = 0; v < 64; ++v) c64[v] = (1ull << ((v + 1) % 64)) | (1ull << ((v + 63) % 64));
    azdopt::DenseGraphInvSpace s64(64, 0.2, 128, azdopt::InvariantCost::aouchiche_hansen(64), true);
    azd_dense_ah_cost_t c;
    if (azd_dense_ah_cost_wide(c64, 64, &c) != AZD_OK || c.diameter != 32 || c.k != 20) return 3;
    azd_dense_inv_cost_t i = s64.cost(c64);
    if (i.cost != c.cost || i.eval != c.eval || i.inv[0] != 64.0 || i.inv[3] != 32.0 || i.dist_k != 20 || i.computed != (0xFFu | 1u << 9)) return 4;
    azd_dense_inv_cost_t o;
    if (azd_dense_inv_cost(c64, 64, &s64.invariant_cost().recipe(), &o) != AZD_ERR_INVALID_ARGUMENT) return 6;
    if (azd_device_count() == 0) return 0;
    azdopt::HashStreamModel model(space.STATE_DIM(), space.ACTION_DIM(), 1);
    auto roots = space.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphInvSpace>::par_new(space, roots, model, 16);
    azdopt::DenseInvArgmin a = opt.argmin_data();
    return a.cost.cost == space.cost(a.adj.data()).cost && (int)a.adj.size() == 50 ? 0 : 2;
}
""")
    exe = tmp_path / "invw"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
