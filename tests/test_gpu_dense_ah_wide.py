"""The dense-graph space with the Aouchiche-Hansen cost up to 64 vertices (AZD_ENGINE_DENSE_AH_WIDE; dense_ah_wide_kernels.hip) on
the GPU.
  * the 64-row cost kernel alone (azd_debug_probe_ah_cost_wide) against the host function azd_dense_ah_cost_wide, bit for bit on
    the 88 graphs of tests/dense_ah_wide_ref.py (n = 33 .. 64), one launch per n; and against the 32-row kernel on the n <= 32 set;
  * engines against the Python reference engine (PyDenseWideEngine) with the hash-stream predictions, one launch per phase,
    compared after every call: n = 33 (the first row past 32: the first lane of the wave's second half) with the device root
    policy over two epochs, n = 64 (every lane a row; the BFS mask and the bit shifts at their boundary), n = 50 (the benchmarked
    shape) with roots of up to 612 slots (key width 10).  Sizes are set by the Python side (an eigenproblem per node: 5 ms at
    n = 33, 25 ms at n = 64);
  * a wide engine at n = 20 and n = 31 against the narrow engine: trees, argmin, root-policy report, bit for bit;
  * the pool step (k_pool_search built for as many wavefronts as the LDS holds) against the launch-per-phase form at 256 agents for key
    widths 2, 4 and 10 at n = 40; with a bf16 model at n = 33; an fp32 model falls back with the dense pool step's reason;
  * the argmin record's reads and refusals; the example driver with --wide.
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ah_ref as R
import dense_ah_wide_ref as W
from gpu_parity import C21_CTRS, TOL_REF, PyDenseRef, assert_same_run, assert_tree_equal, az, compare_ah, run_lockstep  # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the cost kernel alone
def test_wide_device_cost_equals_the_host_function_bit_for_bit(az):
    from azdopt_amd import _lib
    L = az.lib()
    by_n = {}
    for name, n, adj in W.graph_set_wide():
        by_n.setdefault(n, []).append((name, adj))
    seen = 0
    for n, graphs in sorted(by_n.items()):
        a = np.array([adj for _, adj in graphs], dtype=np.uint64)
        dev = (_lib.DenseAhCost * len(graphs))()
        _lib.check(L.azd_debug_probe_ah_cost_wide(0, _lib.ptr(a), n, len(graphs), 2, dev, None), "probe_ah_cost_wide")
        for i, (name, adj) in enumerate(graphs):
            host = _lib.DenseAhCost()
            _lib.check(L.azd_dense_ah_cost_wide(_lib.ptr(a[i]), n, C.byref(host)), "ah_cost_wide")
            assert bytes(dev[i]) == bytes(host), (name, n, [(f, getattr(dev[i], f), getattr(host, f)) for f, _ in host._fields_])
            seen += 1
    assert seen == 88


def test_wide_kernel_equals_the_narrow_kernel_up_to_32_vertices(az):
    from azdopt_amd import _lib
    L = az.lib()
    by_n = {}
    for name, n, adj in R.graph_set():
        by_n.setdefault(n, []).append((name, adj))
    for n, graphs in sorted(by_n.items()):
        a = np.array([adj for _, adj in graphs], dtype=np.uint64)
        wide, narrow = (_lib.DenseAhCost * len(graphs))(), (_lib.DenseAhCost * len(graphs))()
        _lib.check(L.azd_debug_probe_ah_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, wide, None), "probe_ah_cost_wide")
        _lib.check(L.azd_debug_probe_ah_cost(0, _lib.ptr(a), n, len(graphs), 1, narrow, None), "probe_ah_cost")
        for i, (name, _) in enumerate(graphs):
            assert bytes(wide[i]) == bytes(narrow[i]), (name, n)


# ---------------------------------------------------------------- engines against the Python reference
def run_wide_parity(az, orc, n, B, p, kmin, kmax, tol, steps, epochs, seed, max_slots=128, **caps):
    """a wide engine, one launch per phase, against PyDenseWideEngine after every call; the device root policy between epochs"""
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost="ah", ah_wide=True)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, model, B, **caps)
    run_lockstep(opt, PyDenseRef(W.PyDenseWideEngine(n, B, cost="ah", p=p)), roots, orc, compare_ah, seed=seed, tol=tol, steps=steps,
                 epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=2, boundary="policy", last_boundary=False, form="dense_per_call",
                 nan_payloads=True)
    return opt


def test_wide_parity_n33_two_epochs_with_the_device_root_policy(az, orc):
    opt = run_wide_parity(az, orc, 33, 12, 0.2, 5, 100, ([50, 20, 10], 5), steps=40, epochs=2, seed=3)
    c = opt.counters()
    print("n = 33:", {k: c[k] for k in C21_CTRS})
    assert c["EXPANSIONS"] > 0


def test_wide_parity_n64_every_lane_a_row(az, orc):
    opt = run_wide_parity(az, orc, 64, 8, 0.1, 5, 128, TOL_REF, steps=20, epochs=1, seed=4)
    assert opt.counters()["EXPANSIONS"] > 0
    # argmin reads: the wide record against the reference (compare() above went through argmin_data()); the narrow call is refused
    from azdopt_amd import _lib
    rec = _lib.DenseAhWideArgmin()
    _lib.check(opt._L.azd_engine_dense_ah_wide_argmin_data(opt._h, C.byref(rec)), "dense_ah_wide_argmin_data")
    a = opt.argmin_data()
    assert np.array_equal(np.array(rec.adj[:], np.uint64), a.state["adj"]) and rec.eval == a.eval and rec.k == a.cost["k"]
    assert any(int(x) >> 63 for x in rec.adj[:63]), "vertex 63 has a neighbour: bit 63 of some row is set"
    assert opt._L.azd_engine_dense_ah_argmin_data(opt._h, C.byref(_lib.DenseAhArgmin())) == 8  # AZD_ERR_UNSUPPORTED
    assert "azd_engine_dense_ah_wide_argmin_data" in opt._L.azd_last_error().decode()
    assert opt._L.azd_engine_dense_argmin_data(opt._h, C.byref(_lib.DenseArgmin())) == 8
    lam, mu = C.c_double(), C.c_int32()
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, C.byref(lam), None) == 8
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, None, C.byref(mu)) == 8


def test_wide_parity_n50_key_width_10(az, orc):
    """the benchmarked shape; roots of 300 .. 612 slots: keys of ten words, slot bitmaps past word 8"""
    opt = run_wide_parity(az, orc, 50, 8, 0.2, 300, 612, TOL_REF, steps=20, epochs=1, seed=6, max_slots=612)
    assert opt.counters()["EXPANSIONS"] > 0


# ---------------------------------------------------------------- wide against narrow where both run
@pytest.mark.parametrize("n,p,kmax", [(20, 0.2, 60), (31, 0.4, 128)])
def test_wide_engine_gives_the_narrow_engines_trees(az, n, p, kmax):
    B, seed, calls = 32, 9, 40
    runs = []
    for wide in (True, False):
        space = az.DenseGraphSpace(n, p, max_slots=128, cost="ah", ah_wide=wide)
        roots = space.generate_roots(seed, B, kmin=5, kmax=kmax)
        o = az.NablaOptimizer.par_new(space, roots, az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B)
        imp = o.par_roll_out_episodes(TOL_REF, n_calls=calls)
        o.par_reset_trees_policy(seed, 0, 5, kmax)
        report = o.root_policy_report()
        imp2 = o.par_roll_out_episodes(TOL_REF, n_calls=20)
        runs.append((o, imp, imp2, report))
    (o0, i0, j0, r0), (o1, i1, j1, r1) = runs
    assert (i0, j0) == (i1, j1) and all(np.array_equal(r0[k], r1[k]) for k in ("branch", "node", "kept"))
    c0, c1 = o0.counters(), o1.counters()
    for k in C21_CTRS:
        assert c0[k] == c1[k], k
    for i in range(B):
        assert_tree_equal(o0.get_tree(i), o1.get_tree(i), f"agent {i}")
        s0, s1 = o0.agent_state(i), o1.agent_state(i)
        assert all(np.array_equal(s0[k], s1[k]) for k in s0), i
    a0, a1 = o0.argmin_data(), o1.argmin_data()
    assert a0.eval == a1.eval and a0.agent == a1.agent and a0.node == a1.node and a0.cost == a1.cost
    assert np.array_equal(a0.state["adj"], a1.state["adj"]) and np.array_equal(a0.state["permitted"], a1.state["permitted"])
    assert np.array_equal(o0.state_vecs(), o1.state_vecs())


# ---------------------------------------------------------------- pool step
@pytest.mark.parametrize("max_slots,kmin,kmax", [(128, 5, 128), (256, 129, 256), (640, 300, 640)])
def test_wide_pool_step_equals_the_launch_per_phase_form_at_256_agents(az, max_slots, kmin, kmax):
    """key widths 2, 4 and 10 at n = 40 (E = 780): the pool step's searchers == one launch per phase -- trees, counters, argmin,
    state vectors -- over an epoch boundary"""
    n, B, seed, calls = 40, 256, 5, 30
    space = az.DenseGraphSpace(n, 0.2, max_slots=max_slots, cost="ah", ah_wide=True)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    runs = []
    for pool in (True, False):
        model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
        if pool:
            model = model.serve_from_pool_evaluators()
        o = az.NablaOptimizer.par_new(space, roots, model, B, pool_step=pool, prediction_capacity=131072)
        imp = o.par_roll_out_episodes(TOL_REF, n_calls=calls)
        form = o.step_form()
        if pool:
            assert form == ("pool", ""), form
            c = o.counters()
            assert c["EVAL_ROWS"] == c["EXPANSIONS"] > 0
        else:
            assert form[0].startswith("per_call"), form
        o.par_reset_trees_policy(seed, 0, kmin, kmax)
        imp2 = o.par_roll_out_episodes(TOL_REF, n_calls=15)
        runs.append((o, imp, imp2))
    (o0, i0, j0), (o1, i1, j1) = runs
    assert (i0, j0) == (i1, j1)
    assert_same_run(o0, o1, B, every=5)


def test_wide_pool_step_with_a_bf16_model_and_the_fp32_fallback(az, monkeypatch):
    """a bf16 ActionModel on the pool step at n = 33 (the searchers' rows gathered into the batched GEMM launches) == one launch
    per phase; an fp32 model falls back with the dense pool step's own reason"""
    n, B, seed, calls = 33, 256, 11, 40
    tol = ([50, 20, 10], 5)
    space = az.DenseGraphSpace(n, 0.2, cost="ah", ah_wide=True)
    roots = space.generate_roots(seed, B)

    def mk(dtype="bf16"):
        model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(128, 128), seed=seed, dtype=dtype)
        return az.NablaOptimizer.par_new(space, roots, model, B, pool_step=True)

    monkeypatch.setenv("AZD_DENSE_NO_POOL", "1")
    ref = mk()
    imp_ref = ref.par_roll_out_episodes(tol, n_calls=calls)
    assert ref.step_form()[0].startswith("per_call")
    monkeypatch.delenv("AZD_DENSE_NO_POOL")
    pool = mk()
    imp_pool = pool.par_roll_out_episodes(tol, n_calls=calls)
    assert pool.step_form() == ("pool", ""), pool.step_form()
    assert imp_pool == imp_ref
    assert_same_run(pool, ref, B, every=3)
    assert pool.counters()["EVAL_ROWS"] == pool.counters()["EXPANSIONS"] > 0
    f32 = mk("f32")
    f32.par_roll_out_episodes(tol, n_calls=5)
    form, why = f32.step_form()
    assert form.startswith("per_call") and "bf16" in why and why.startswith("dense-graph space: the pool step needs"), (form, why)


def test_wide_example_driver_runs(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "ah.py"), "--n", "40", "--wide", "--epochs", "1", "--episodes", "20",
                        "--batch", "32", "--out", str(tmp_path / "ev")], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("==== EPOCH") == 1 and any("AhCost" in l for l in r.stdout.splitlines())
