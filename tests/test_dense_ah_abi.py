"""azd_dense_ah_cost, the host form of the Aouchiche-Hansen cost (dense_cost_host.cpp), without a GPU: equal to the Python reference
(tests/dense_ah_ref.py) bit for bit on the whole graph set -- proximity and eigenvalue as f64 bit patterns, diameter and k as
integers, cost and eval as f32 bit patterns -- and its argument checks."""
import ctypes as C

import numpy as np
import pytest

import dense_ah_ref as R


@pytest.fixture(scope="module")
def lib():
    import azdopt_amd
    return azdopt_amd.lib()


def host_cost(lib, adj, n):
    from azdopt_amd import _lib
    a = np.array(adj, dtype=np.uint64)
    out = _lib.DenseAhCost()
    st = lib.azd_dense_ah_cost(_lib.ptr(a), n, C.byref(out))
    return st, out


def test_symbols_are_exported_and_bound(lib):
    from azdopt_amd import _lib
    for name in ("azd_dense_ah_cost", "azd_debug_probe_ah_cost", "azd_debug_probe_math_f64"):
        assert getattr(lib, name).argtypes, name
    assert _lib.DENSE_AH_MAX_N == 32 == R.AH_MAX_N
    assert C.sizeof(_lib.DenseAhCost) == 32


def test_host_cost_equals_the_python_reference_bit_for_bit(lib):
    for name, n, adj in R.graph_set():
        st, out = host_cost(lib, adj, n)
        assert st == 0, (name, n, lib.azd_last_error())
        r = R.ah_cost(adj, n)
        tag = (name, n)
        assert np.float64(out.proximity).view(np.uint64) == np.float64(r["proximity"]).view(np.uint64), tag
        assert np.float64(out.eigenvalue).view(np.uint64) == np.float64(r["eigenvalue"]).view(np.uint64), (tag, out.eigenvalue, r["eigenvalue"])
        assert (out.diameter, out.k) == (r["diameter"], r["k"]), tag
        assert np.float32(out.cost).view(np.uint32) == r["cost"].view(np.uint32), tag
        assert np.float32(out.eval).view(np.uint32) == r["eval"].view(np.uint32), tag


def test_arguments_are_checked_and_named(lib):
    for n in (3, 33, 64, 0, -1):
        st, _ = host_cost(lib, R.path(max(n, 4)), n)
        assert st == 1 and lib.azd_last_error().decode().split(": ")[1].startswith("n"), (n, lib.azd_last_error())
    two_paths = R.from_edges(8, [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7)])
    st, _ = host_cost(lib, two_paths, 8)
    assert st == 1 and "adj" in lib.azd_last_error().decode() and "connected" in lib.azd_last_error().decode()
    for bad in ([1 << 1, 0, 0, 0], [0b0011, 0b0001, 0, 0], [1 << 40, 0, 0, 0]):  # asymmetric, loop, neighbour beyond n
        st, _ = host_cost(lib, bad, 4)
        assert st == 1 and "adj" in lib.azd_last_error().decode(), bad
    from azdopt_amd import _lib
    assert lib.azd_dense_ah_cost(None, 8, C.byref(_lib.DenseAhCost())) == 1
    a = np.array(R.path(8), dtype=np.uint64)
    assert lib.azd_dense_ah_cost(_lib.ptr(a), 8, None) == 1


def test_probe_checks_its_graphs_before_it_looks_for_a_device(lib):
    from azdopt_amd import _lib
    out = (_lib.DenseAhCost * 2)()
    a = np.array(R.path(33) + R.path(33), dtype=np.uint64)
    assert lib.azd_debug_probe_ah_cost(0, _lib.ptr(a), 33, 2, 1, out, None) == 1
    assert "n" in lib.azd_last_error().decode()
    a = np.array(list(R.path(8)) + [0] * 8, dtype=np.uint64)
    assert lib.azd_debug_probe_ah_cost(0, _lib.ptr(a), 8, 2, 1, out, None) == 1
    assert "graph 1" in lib.azd_last_error().decode()


# ---------------------------------------------------------------- AZD_ENGINE_DENSE_AH: configuration checks, without a device
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
    AH = _lib.ENGINE_DENSE_AH
    assert AH == 32
    st, _ = _create(lib, _lib.SPACE_DENSE, 31, AH, max_slots=128)
    assert st in (0, 2)  # created, or "no device"
    st, why = _create(lib, _lib.SPACE_DENSE, 33, AH)
    assert st == 1 and why.startswith("n:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 3, AH)
    assert st == 1 and why.startswith("n:"), why
    st, why = _create(lib, _lib.SPACE_C21, 19, AH)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_RAMSEY, 16, AH, n_colors=3)
    assert st == 1 and why.startswith("space_id:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 31, AH, layers=2)
    assert st == 1 and why.startswith("layers:"), why
    st, why = _create(lib, _lib.SPACE_DENSE, 8, AH, max_slots=29)  # E = 28
    assert st == 1 and why.startswith("max_slots:"), why
    # without the flag, every limit is the default dense space's: n = 33 is accepted
    st, _ = _create(lib, _lib.SPACE_DENSE, 33, 0)
    assert st in (0, 2)


def test_python_space_carries_the_cost():
    import azdopt_amd as az
    sp = az.DenseGraphSpace(31, 0.4, max_slots=128, cost="ah")
    assert sp.COST == "ah" and az.DenseGraphSpace(31).COST == "c21"
    assert (sp.STATE_DIM, sp.ACTION_DIM) == (1396, 930)  # 05-ah.rs:39-40 at N = 31
    with pytest.raises(ValueError):
        az.DenseGraphSpace(31, cost="faer")
    r = sp.ah_cost(R.cycle(31))
    want = R.ah_cost(R.cycle(31), 31)
    assert r["cost"] == want["cost"] and r["eval"] == want["eval"] and r["diameter"] == 15 == want["diameter"]


def test_cpp_binding_compiles_with_an_ah_engine(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "ah.cpp"
    src.write_text("""
#include "azdopt_amd.hpp"
int main() {
    azdopt::DenseGraphAhSpace space(31, 0.4, 128);
    uint64_t c5[5] = {0x12, 0x05, 0x0a, 0x14, 0x09};
    azd_dense_ah_cost_t c;
    if (azd_dense_ah_cost(c5, 5, &c) != AZD_OK || c.cost != 7.5f) return 1;
    if (azd_device_count() == 0) return 0;
    azdopt::HashStreamModel model(space.STATE_DIM(), space.ACTION_DIM(), 1);
    auto roots = space.generate_roots(1, 16, 5, 60);
    auto opt = azdopt::NablaOptimizer<azdopt::DenseGraphAhSpace>::par_new(space, roots, model, 16);
    azdopt::DenseAhArgmin a = opt.argmin_data();
    return a.cost == space.cost(a.adj.data()).cost ? 0 : 2;
}
""")
    exe = tmp_path / "ah"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(root, "include"), str(src), "-o", str(exe),
                           "-L" + os.path.join(root, "azdopt_amd"), "-lazdopt_amd", "-Wl,-rpath," + os.path.join(root, "azdopt_amd")])
    assert subprocess.run([str(exe)]).returncode == 0
