"""The Aouchiche-Hansen cost up to 64 vertices without a GPU: azd_dense_ah_cost_wide (dense_cost_host.cpp) equal to the Python restatement
(tests/dense_ah_wide_ref.py) bit for bit on the 88 graphs of graph_set_wide() -- proximity and eigenvalue as f64 bit patterns,
diameter and k as integers, cost and eval as f32 bit patterns -- and to azd_dense_ah_cost on the n <= 32 set; the argument checks
of the new calls and of AZD_ENGINE_DENSE_AH_WIDE, made before any device is looked for; the Python and C++ hosts."""
import ctypes as C

import numpy as np
import pytest

import dense_ah_ref as R
import dense_ah_wide_ref as W


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


def host_cost(lib, adj, n, wide=True):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseAhCost()
    st = (lib.azd_dense_ah_cost_wide if wide else lib.azd_dense_ah_cost)(_lib.ptr(a), n, C.byref(out))
    return st, out


def test_symbols_are_exported_and_bound(lib):
    from azdopt_amd import _lib
    for name in ("azd_dense_ah_cost_wide", "azd_debug_probe_ah_cost_wide", "azd_engine_dense_ah_wide_argmin_data"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_AH_WIDE_MAX_N == 64 == W.AH_WIDE_MAX_N and _lib.DENSE_AH_MAX_N == 32
    assert _lib.ENGINE_DENSE_AH_WIDE == 256
    assert C.sizeof(_lib.DenseAhWideArgmin) == 8 * 64 + 8 * 32 + 16 + 8 + 8 + 8


def test_graph_set_wide_is_what_the_checks_assume():
    gs = W.graph_set_wide()
    assert len(gs) == 88 and {n for _, n, _ in gs} == {33, 34, 40, 47, 50, 56, 63, 64}
    for fam in ("path", "star", "cycle", "complete", "broom", "gnp0.05+tree", "gnp0.60"):
        assert any(name == fam for name, _, _ in gs), fam
    for name, n, adj in gs:
        assert R.connected(adj, n), name
        assert all(not (adj[v] >> v) & 1 and adj[v] < (1 << n) for v in range(n))
        assert all(((adj[v] >> u) & 1) == ((adj[u] >> v) & 1) for v in range(n) for u in range(n))
    diams = {W.ah_cost(adj, n)["diameter"] for _, n, adj in gs}
    assert min(diams) == 1 and max(diams) == 63


def test_wide_host_cost_equals_the_python_restatement_bit_for_bit(lib):
    for name, n, adj in W.graph_set_wide():
        st, out = host_cost(lib, adj, n)
        assert st == 0, (name, n, lib.azd_last_error())
        r = W.ah_cost(adj, n)
        tag = (name, n)
        assert np.float64(out.proximity).view(np.uint64) == np.float64(r["proximity"]).view(np.uint64), tag
        assert np.float64(out.eigenvalue).view(np.uint64) == np.float64(r["eigenvalue"]).view(np.uint64), (tag, out.eigenvalue, r["eigenvalue"])
        assert (out.diameter, out.k) == (r["diameter"], r["k"]), tag
        assert np.float32(out.cost).view(np.uint32) == r["cost"].view(np.uint32), tag
        assert np.float32(out.eval).view(np.uint32) == r["eval"].view(np.uint32), tag


def test_wide_host_cost_is_the_narrow_one_up_to_32_vertices(lib):
    for name, n, adj in R.graph_set():
        (sw, w), (sn, nr) = host_cost(lib, adj, n), host_cost(lib, adj, n, wide=False)
        assert sw == 0 == sn and bytes(w) == bytes(nr), (name, n)


def test_wide_cost_arguments_are_checked_and_named(lib):
    from azdopt_amd import _lib
    for n in (3, 65, 0, -1):
        st, _ = host_cost(lib, R.path(min(max(n, 4), 64)), n)
        assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n"), (n, lib.azd_last_error())
    st, _ = host_cost(lib, R.path(64), 64)
    assert st == 0
    two_paths = R.from_edges(40, [(i, i + 1) for i in range(39) if i != 19])
    st, _ = host_cost(lib, two_paths, 40)
    assert st == 1 and "adj" in lib.azd_last_error().decode() and "connected" in lib.azd_last_error().decode()
    beyond = list(R.path(40))
    beyond[0] |= 1 << 40
    for bad in (beyond, [1 << 1] + [0] * 39, [0b0011, 0b0001] + [0] * 38):  # neighbour beyond n, asymmetric, loop
        st, _ = host_cost(lib, bad, 40)
        assert st == 1 and "adj" in lib.azd_last_error().decode(), bad[:2]
    assert lib.azd_dense_ah_cost_wide(None, 40, C.byref(_lib.DenseAhCost())) == 1
    a = np.array(R.path(40), dtype=np.uint64)
    assert lib.azd_dense_ah_cost_wide(_lib.ptr(a), 40, None) == 1
    # the narrow call keeps its limit
    st, _ = host_cost(lib, R.path(33), 33, wide=False)
    assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n")


def test_wide_probe_checks_its_graphs_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseAhCost * 2)()
    a = np.zeros(2 * 65, dtype=np.uint64)
    assert lib.azd_debug_probe_ah_cost_wide(0, _lib.ptr(a), 65, 2, 1, out, None) == 1
    assert "n:" in lib.azd_last_error().decode()
    a = np.array(list(R.path(40)) + [0] * 40, dtype=np.uint64)
    assert lib.azd_debug_probe_ah_cost_wide(0, _lib.ptr(a), 40, 2, 1, out, None) == 1
    assert "graph 1" in lib.azd_last_error().decode() and "azd_debug_probe_ah_cost_wide" in lib.azd_last_error().decode()
    a = np.array(R.path(33) + R.path(33), dtype=np.uint64)  # the narrow probe keeps its limit
    assert lib.azd_debug_probe_ah_cost(0, _lib.ptr(a), 33, 2, 1, out, None) == 1 and "n:" in lib.azd_last_error().decode()


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_AH_WIDE: configuration checks, without a device
def _cfg(space_id, n, flags, layers=0, max_slots=0, path_kind=0, n_colors=0, batch=4):
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
    AH, WIDE, D = _lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH_WIDE, _lib.SPACE_DENSE
    for n, ms in ((50, 128), (64, 640), (33, 0), (20, 128), (4, 6)):
        st, why = _create(lib, D, n, AH | WIDE, max_slots=ms)
        assert st in (0, 2), (n, ms, why)  # created, or "no device"
    st, why = _create(lib, D, 50, WIDE)  # the new flag alone
    assert st == 1 and why.startswith("flags:") and "AZD_ENGINE_DENSE_AH" in why, why
    st, why = _create(lib, _lib.SPACE_C21, 19, WIDE)
    assert st == 1 and why.startswith("flags:"), why
    st, why = _create(lib, _lib.SPACE_C21, 19, AH | WIDE)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_RAMSEY, 16, AH | WIDE, n_colors=3)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_RAMSEY, 16, WIDE, n_colors=3)
    assert st == 1 and why.startswith("flags:"), why
    for n in (3, 65):
        st, why = _create(lib, D, n, AH | WIDE)
        assert st == 1 and why.startswith("n:"), (n, why)
    st, why = _create(lib, D, 50, AH | WIDE, layers=2)
    assert st == 1 and why.startswith("layers:"), why
    st, why = _create(lib, D, 50, AH | WIDE, path_kind=1)
    assert st == 1 and why.startswith("path_kind:"), why
    st, why = _create(lib, D, 50, AH | WIDE, max_slots=641)
    assert st == 1 and why.startswith("max_slots:"), why
    st, why = _create(lib, D, 8, AH | WIDE, max_slots=29)  # E = 28
    assert st == 1 and why.startswith("max_slots:"), why
    # AZD_ENGINE_DENSE_AH alone keeps its limit
    st, why = _create(lib, D, 33, AH)
    assert st == 1 and why.startswith("n:") and "32" in why, why


def test_pool_plan_of_a_wide_engine(lib):
    """arithmetic only: as many wavefronts per searcher workgroup as a CU's 160 KB hold of the 20-KB blocks, at least the form's
    lower bound of 4, for the three key widths; a configuration with neither flag is still refused"""
    from azdopt_amd import _lib
    AH, WIDE, D = _lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH_WIDE, _lib.SPACE_DENSE
    for ms in (128, 256, 612):
        cfg = _cfg(D, 50, AH | WIDE, max_slots=ms, batch=256)
        waves, lds = C.c_int(0), C.c_size_t(0)
        assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0, lib.azd_last_error()
        assert 4 <= waves.value <= 16 and waves.value * 20000 < lds.value <= 160 * 1024, (ms, waves.value, lds.value)
    cfg = _cfg(D, 50, AH, max_slots=128)  # n = 50 without the wide flag: refused as by azd_engine_create
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1
    cfg = _cfg(D, 31, AH, max_slots=128)
    assert lib.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 1


def test_python_space_carries_ah_wide():
    import azdopt_amd as az
    sp = az.DenseGraphSpace(50, 0.2, max_slots=128, cost="ah", ah_wide=True)
    assert sp.COST == "ah" and sp.AH_WIDE and not az.DenseGraphSpace(31, cost="ah").AH_WIDE and not az.DenseGraphSpace(50).AH_WIDE
    assert (sp.STATE_DIM, sp.ACTION_DIM, sp.MAX_SLOTS) == (3676, 2450, 128)
    assert az.DenseGraphSpace(50, cost="ah", ah_wide=True, max_slots=1024).MAX_SLOTS == 640
    assert az.DenseGraphSpace(8, cost="ah", ah_wide=True, max_slots=1024).MAX_SLOTS == 28
    assert az.DenseGraphSpace(50, max_slots=1024).MAX_SLOTS == 1024
    with pytest.raises(ValueError):
        az.DenseGraphSpace(50, cost="c21", ah_wide=True)
    r = sp.ah_cost(R.cycle(50))
    want = W.ah_cost(R.cycle(50), 50)
    assert r["cost"] == want["cost"] and r["eval"] == want["eval"] and r["diameter"] == 25 == want["diameter"]
    with pytest.raises(az.AzdError):  # the narrow space's host cost keeps its limit
        az.DenseGraphSpace(50, cost="ah").ah_cost(R.cycle(50))


def test_cpp_binding_compiles_with_a_wide_ah_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "ahw.cpp"
    src.write_text("""
#include "azdopt_amd.hpp"
int main() {
    azdopt::DenseGraphAhSpace space(50, 0.2, 128, true);
    azd_engine_config cfg{};
    space.configure(cfg);
    if (cfg.flags != (AZD_ENGINE_DENSE_AH | AZD_ENGINE_DENSE_AH_WIDE) || AZD_DENSE_AH_WIDE_MAX_N != 64) return 1;
    uint64_t c64[64];
    for (int v = 0; v < 64; ++v) c64[v] = (1ull << ((v + 1) % 64)) | (1ull << ((v + 63) % 64));
    azd_dense_ah_cost_t c;
    if (azd_dense_ah_cost_wide(c64, 64, &c) != AZD_OK || c.diameter != 32 || c.k != 20) return 3;
    if (azd_dense_ah_cost(c64, 64, &c) != AZD_ERR_INVALID_ARGUMENT) return 4;
    if (azd_device_count() == 0) return 0;
    azdopt::HashStreamModel model(space.STATE_DIM(), space.ACTION_DIM(), 1);
    auto roots = space.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphAhSpace>::par_new(space, roots, model, 16);
    azdopt::DenseAhArgmin a = opt.argmin_data();
    return a.cost == space.cost(a.adj.data()).cost ? 0 : 2;
}
""")
    exe = tmp_path / "ahw"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
