"""azd_dense_inv_cost, the host form of the weighted-invariant cost (dense_cost_host.cpp), without a GPU: equal to the Python reference
(tests/dense_inv_ref.py) bit for bit -- every field of the record compared as bytes -- on the whole graph set under the four test
recipes and over a sweep of the spectral indices, and on the hard case set of the spectral passes (tests/dense_spectral_cases.py)
under an adjacency and a both-spectra recipe; skipped terms; azd_dense_ah_cost as one recipe; and every refusal that needs no
device, with its status and the argument it names."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as R
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


def host_cost(lib, adj, n, recipe):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseInvCost()
    rc = recipe if isinstance(recipe, _lib.DenseInvRecipe) else c_recipe(recipe)
    st = lib.azd_dense_inv_cost(_lib.ptr(a), n, C.byref(rc), C.byref(out))
    return st, out


def reference_bytes(r):
    """the Python reference's record in azd_dense_inv_cost_t's layout"""
    return struct.pack("<10diIff", *[r[k] for k in R.NAMES], r["dist_k"], r["computed"], r["cost"], r["eval"])


def test_symbols_are_exported_and_bound(lib):
    from azdopt_amd import _lib
    for name in ("azd_dense_inv_cost", "azd_debug_probe_inv_cost", "azd_engine_set_dense_inv_recipe", "azd_engine_dense_inv_argmin_data",
                 "azd_engine_dense_inv_agent_cost"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_INV_MAX_N == 32 and _lib.DENSE_INV_COUNT == 10 == len(R.NAMES) and _lib.DENSE_INV_NAMES == R.NAMES
    assert _lib.DENSE_INV_INDEX_AH == R.INDEX_AH == -1 and _lib.ENGINE_DENSE_INV == 1024
    assert (C.sizeof(_lib.DenseInvRecipe), C.sizeof(_lib.DenseInvCost), C.sizeof(_lib.DenseInvArgmin)) == (104, 96, 424)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "azdopt_amd.h")).read()
    assert "#define AZD_ENGINE_DENSE_INV 1024u" in hdr and "#define AZD_DENSE_INV_NAMES " + ", ".join('"%s"' % k for k in R.NAMES) in hdr


def test_host_cost_equals_the_python_reference_as_bytes(lib):
    seen = 0
    for name, n, adj in A.graph_set():
        for rname, mk in R.RECIPES.items():
            recipe = mk(n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, rname, lib.azd_last_error())
            r = R.inv_cost(adj, n, recipe)
            assert bytes(out) == reference_bytes(r), (name, n, rname, list(out.inv), r)
            seen += 1
    assert seen == 4 * 560


def test_host_cost_equals_the_python_reference_on_the_hard_spectral_cases(lib):
    """tests/dense_spectral_cases.py (rank-deficient adjacency matrices, every labelling; 186 of them end in NaN without the
    deflation rule) under an adjacency recipe (index 0) and a both-spectra recipe (adjacency n - 1, distance 1): records as bytes,
    every invariant finite"""
    entries = S.graph_set()
    R.prime(entries, ("adj", "dist"), lambda n: (0, 1, n - 1))
    seen = 0
    for name, n, adj in entries:
        for rname in ("ADJ", "BOTH"):
            recipe = R.RECIPES[rname](n)
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, rname, lib.azd_last_error())
            assert all(math.isfinite(x) for x in out.inv), (name, rname, list(out.inv))
            assert bytes(out) == reference_bytes(R.inv_cost(adj, n, recipe)), (name, rname, list(out.inv))
            seen += 1
    assert seen == 2 * 3700


def test_index_sweep_on_every_tenth_graph(lib):
    seen = 0
    for name, n, adj in A.graph_set()[::10]:
        for k in range(n):
            recipe = R.Recipe({"adj_eig": 0.5, "dist_eig": -0.25, "radius": 1.0}, bias=0.125, adj_index=k, dist_index=n - 1 - k, eval_offset=1.0,
                              eval_scale=1.0 / (2 * n + 2))
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0, (name, n, k, lib.azd_last_error())
            assert bytes(out) == reference_bytes(R.inv_cost(adj, n, recipe)), (name, n, k)
            seen += 1
    assert seen > 900


def test_skipped_and_zero_weight_terms(lib):
    n, adj = 12, A.double_broom(12, 3, 3)
    full = host_cost(lib, adj, n, R.Recipe({k: 1.0 for k in R.NAMES}, adj_index=1, dist_index=2))[1]
    assert full.computed == 0x3FF and full.inv[8] != 0.0 and full.inv[9] != 0.0
    for skip, bit in (("adj_eig", 8), ("dist_eig", 9)):
        st, out = host_cost(lib, adj, n, R.Recipe({k: 1.0 for k in R.NAMES if k != skip}, adj_index=1, dist_index=2))
        assert st == 0 and out.computed == 0x3FF & ~(1 << bit) and out.inv[bit] == 0.0 and math.copysign(1.0, out.inv[bit]) == 1.0
        assert [out.inv[i] for i in range(10) if i != bit] == [full.inv[i] for i in range(10) if i != bit] and out.dist_k == 2
    # a zero weight on an integer invariant: still computed and reported, absent from the sum
    st, out = host_cost(lib, adj, n, R.Recipe({"edges": 1.0}, bias=-0.0))
    assert st == 0 and out.computed == 0xFF and list(out.inv)[:8] == list(full.inv)[:8] and out.cost == full.inv[0]
    assert out.dist_k == A.ah_index(int(full.inv[3]), n)  # the index the recipe resolves to is reported either way


def test_the_ah_cost_is_the_ah_recipe(lib):
    from azdopt_amd import _lib
    import azdopt_amd as az
    for name, n, adj in A.graph_set():
        a = np.array(adj, dtype=np.uint64)
        ah = _lib.DenseAhCost()
        assert lib.azd_dense_ah_cost(_lib.ptr(a), n, C.byref(ah)) == 0
        for recipe in (c_recipe(R.recipe_ah(n)), az.InvariantCost.aouchiche_hansen(n).recipe()):
            st, out = host_cost(lib, adj, n, recipe)
            assert st == 0
            assert struct.pack("<ddiiff", out.inv[5], out.inv[9], int(out.inv[3]), out.dist_k, out.cost, out.eval) == bytes(ah), (name, n)


def test_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    ok = R.recipe_both(8)
    for n in (3, 33, 64, 0, -1):
        st, _ = host_cost(lib, A.path(max(n, 4)), n, R.recipe_int(8))
        assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n"), (n, lib.azd_last_error())
    two_paths = A.from_edges(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)])
    st, _ = host_cost(lib, two_paths, 8, ok)
    assert st == 1 and "adj" in lib.azd_last_error().decode() and "connected" in lib.azd_last_error().decode()
    for bad in ([1 << 1, 0, 0, 0], [0b0011, 0b0001, 0, 0], [1 << 40, 0, 0, 0]):  # asymmetric, loop, neighbour beyond n
        st, _ = host_cost(lib, bad, 4, R.recipe_int(4))
        assert st == 1 and "adj" in lib.azd_last_error().decode(), bad
    a = np.array(A.path(8), dtype=np.uint64)
    rc = c_recipe(ok)
    assert lib.azd_dense_inv_cost(None, 8, C.byref(rc), C.byref(_lib.DenseInvCost())) == 1
    assert lib.azd_dense_inv_cost(_lib.ptr(a), 8, C.byref(rc), None) == 1 and "out" in lib.azd_last_error().decode()
    assert lib.azd_dense_inv_cost(_lib.ptr(a), 8, None, C.byref(_lib.DenseInvCost())) == 1 and "recipe" in lib.azd_last_error().decode()


def bad_recipes(n):
    """(field the refusal names, recipe) for every way a recipe is refused"""
    inf, nan = float("inf"), float("nan")

    def mk(**kw):
        r = c_recipe(R.recipe_both(n))
        for k, v in kw.items():
            if k == "w":
                r.weight[v[0]] = v[1]
            elif k == "weights":
                for i, x in enumerate(v):
                    r.weight[i] = x
            else:
                setattr(r, k, v)
        return r

    return [("weight", mk(w=(3, inf))), ("weight", mk(w=(9, nan))), ("weight", mk(weights=[0.0] * 10)), ("bias", mk(bias=nan)), ("bias", mk(bias=-inf)),
            ("eval_offset", mk(eval_offset=inf)), ("eval_scale", mk(eval_scale=nan)), ("eval_scale", mk(eval_scale=0.0)),
            ("adj_index", mk(adj_index=-1)), ("adj_index", mk(adj_index=n)), ("dist_index", mk(dist_index=n)), ("dist_index", mk(dist_index=-2))]


def test_recipes_are_checked_and_the_field_is_named(lib):
    n = 8
    for field, rc in bad_recipes(n):
        st, _ = host_cost(lib, A.cycle(n), n, rc)
        why = lib.azd_last_error().decode()
        assert st == 1 and why.split(": ")[1] == field, (field, why)
    # the limits themselves are accepted: index n - 1, the AH rule, a negative scale, a zero offset, -0.0 as a weight of zero
    edge = c_recipe(R.Recipe({"adj_eig": 1.0, "dist_eig": -0.0, "radius": -1.0}, adj_index=n - 1, dist_index=R.INDEX_AH, eval_scale=-1.0))
    st, out = host_cost(lib, A.cycle(n), n, edge)
    assert st == 0 and out.computed == 0xFF | 1 << 8, lib.azd_last_error()


def test_probe_checks_graphs_and_recipe_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseInvCost * 2)()
    rc = c_recipe(R.recipe_both(8))
    a = np.array(A.path(33) + A.path(33), dtype=np.uint64)
    assert lib.azd_debug_probe_inv_cost(0, _lib.ptr(a), 33, 2, 1, C.byref(rc), out, None) == 1 and "n" in lib.azd_last_error().decode()
    a = np.array(list(A.path(8)) + [0] * 8, dtype=np.uint64)
    assert lib.azd_debug_probe_inv_cost(0, _lib.ptr(a), 8, 2, 1, C.byref(rc), out, None) == 1 and "graph 1" in lib.azd_last_error().decode()
    a = np.array(A.path(8) + A.cycle(8), dtype=np.uint64)
    for field, bad in bad_recipes(8):
        assert lib.azd_debug_probe_inv_cost(0, _lib.ptr(a), 8, 2, 1, C.byref(bad), out, None) == 1
        assert lib.azd_last_error().decode().split(": ")[1] == field, field
    assert lib.azd_debug_probe_inv_cost(0, _lib.ptr(a), 8, 2, 0, C.byref(rc), out, None) == 1
    assert lib.azd_engine_set_dense_inv_recipe(None, C.byref(rc)) == 1
    assert lib.azd_engine_dense_inv_argmin_data(None, C.byref(_lib.DenseInvArgmin())) == 1
    assert lib.azd_engine_dense_inv_agent_cost(None, 0, C.byref(_lib.DenseInvCost())) == 1


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_INV: configuration checks, without a device
def _create(lib, space_id, n, flags, layers=0, max_slots=0, path_kind=0, n_colors=0):
    from azdopt_amd import _lib
    cfg = _lib.EngineConfig(space_id, n, 4, 0, 0, 0, 0, 0, flags)
    cfg.layers, cfg.max_slots, cfg.path_kind, cfg.dense_p, cfg.n_colors = layers, max_slots, path_kind, 0.4, n_colors
    for i in range(n_colors):
        cfg.clique_sizes[i], cfg.color_weights[i] = 3, 1.0
    h = C.c_void_p()
    st = lib.azd_engine_create(C.byref(h), C.byref(cfg), None)
    if st == 0:
        lib.azd_engine_destroy(h)
    return st, lib.azd_last_error().decode()


def test_engine_flag_is_validated_before_the_device_is_looked_for(lib):
    from azdopt_amd import _lib
    INV = _lib.ENGINE_DENSE_INV
    for extra in (0, _lib.ENGINE_EXT_POOL_F32):  # the pool step's fp32 evaluator is accepted beside it
        st, why = _create(lib, _lib.SPACE_DENSE, 31, INV | extra, max_slots=128)
        assert st in (0, 2), why  # created, or "no device"
    st, why = _create(lib, _lib.SPACE_DENSE, 32, INV, max_slots=496)
    assert st in (0, 2), why
    for other in (_lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE, _lib.ENGINE_DENSE_AH_WIDE):
        st, why = _create(lib, _lib.SPACE_DENSE, 31, INV | other)
        assert st == 1 and why.startswith("flags:") and "AZD_ENGINE_DENSE_INV" in why, why
    for n in (33, 3):
        st, why = _create(lib, _lib.SPACE_DENSE, n, INV)
        assert st == 1 and why.startswith("n:"), why
    st, why = _create(lib, _lib.SPACE_C21, 19, INV)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_RAMSEY, 16, INV, n_colors=3)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, INV, layers=2)
    assert st == 1 and why.startswith("layers:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, INV, max_slots=29)  # E = 28
    assert st == 1 and why.startswith("max_slots:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, INV, path_kind=1)
    assert st == 1 and why.startswith("path_kind:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, INV | _lib.ENGINE_EXT_POOL_F32 | _lib.ENGINE_NO_PERSISTENT_STEP)
    assert st == 1 and "AZD_ENGINE_EXT_POOL_F32" in why, why
    # the flag changes nothing for the other tiers: their limits stand
    assert _create(lib, _lib.SPACE_DENSE, 33, 0)[0] in (0, 2) and _create(lib, _lib.SPACE_DENSE, 31, _lib.ENGINE_DENSE_AH, max_slots=128)[0] in (0, 2)


def test_python_space_carries_the_recipe():
    import azdopt_amd as az
    cost = az.InvariantCost({"remoteness": 1, "proximity": -1, "adj_eig": 0.5}, bias=0.25, adj_index=2, dist_index="ah", eval_offset=2.0, eval_scale=0.01)
    sp = az.DenseGraphSpace(31, 0.4, max_slots=600, cost=cost)
    assert sp.COST == "inv" and sp.INV is cost and sp.MAX_SLOTS == 465 and (sp.STATE_DIM, sp.ACTION_DIM) == (1396, 930)
    r = cost.recipe()
    assert list(r.weight) == [0, 0, 0, 0, 0, -1, 1, 0, 0.5, 0] and (r.bias, r.adj_index, r.dist_index) == (0.25, 2, -1)
    with pytest.raises(ValueError, match="matching"):
        az.InvariantCost({"matching": 1.0})
    with pytest.raises(ValueError):
        az.DenseGraphSpace(31, cost="faer")
    assert az.InvariantCost.from_dict({"weights": {"edges": 1}, "dist_index": 3, "eval_scale": 0.5}).recipe().dist_index == 3
    got, want = sp.inv_cost(A.cycle(31)), R.inv_cost(A.cycle(31), 31, R.Recipe({"remoteness": 1, "proximity": -1, "adj_eig": 0.5}, bias=0.25, adj_index=2,
                                                                                eval_offset=2.0, eval_scale=0.01))
    assert all(got[k] == want[k] for k in want), (got, want)
    ah = az.DenseGraphSpace(31, 0.4, cost=az.InvariantCost.aouchiche_hansen(31))
    assert ah.inv_cost(A.cycle(31))["cost"] == az.DenseGraphSpace(31, 0.4, cost="ah").ah_cost(A.cycle(31))["cost"]


def test_cpp_binding_compiles_with_an_invariant_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "inv.cpp"
    src.write_text("""
#include "azdopt_amd.hpp"
int main() {
    azdopt::InvariantCost ah = azdopt::InvariantCost::aouchiche_hansen(5);
    azdopt::DenseGraphInvSpace space(5, 0.4, 10, ah);
    uint64_t c5[5] = {0x12, 0x05, 0x0a, 0x14, 0x09};
    azd_dense_ah_cost_t c;
    if (azd_dense_ah_cost(c5, 5, &c) != AZD_OK || c.cost != 7.5f) return 1;
    azd_dense_inv_cost_t i = space.cost(c5);
    if (i.cost != c.cost || i.eval != c.eval || i.inv[0] != 5.0 || i.computed != (0xFFu | 1u << 9)) return 3;
    azdopt::InvariantCost deg;
    deg.weight("max_degree", 1.0).weight("min_degree", -1.0).offset(1.0f).scale(0.125f);
    if (azdopt::DenseGraphInvSpace(5, 0.4, 10, deg).cost(c5).cost != 0.0f) return 4;
    if (azd_device_count() == 0) return 0;
    azdopt::DenseGraphInvSpace big(20, 0.2, 128, azdopt::InvariantCost::aouchiche_hansen(20));
    azdopt::HashStreamModel model(big.STATE_DIM(), big.ACTION_DIM(), 1);
    auto roots = big.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphInvSpace>::par_new(big, roots, model, 16);
    azdopt::DenseInvArgmin a = opt.argmin_data();
    return a.cost.cost == big.cost(a.adj.data()).cost ? 0 : 2;
}
""")
    exe = tmp_path / "inv"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
