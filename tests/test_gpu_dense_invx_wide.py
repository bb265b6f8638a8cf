"""The dense-graph space with the extended invariant cost up to 64 vertices (AZD_ENGINE_DENSE_INVX_WIDE; dense_invx_wide_kernels.hip)
on the GPU.
  * the 64-row cost kernel alone (azd_debug_probe_invx_cost_wide) against the host function azd_dense_invx_cost_wide, records equal as
    bytes on the 88 graphs of tests/dense_ah_wide_ref.py (n = 33 .. 64) under LAP, SLAP, DEG, RATIO and ALL4 of tests/dense_invx_ref.py,
    one launch per n; against the 32-row kernel on every fifth graph of the n <= 32 set; and on the hard case set of the spectral
    passes (tests/dense_spectral_cases.py) at n = 23, 32, 33, 64 under ALL4: every invariant finite, adj_eig, lap_eig and slap_eig
    within 64 n 2^-53 ||M||_F of LAPACK's;
  * engines against the Python reference engine (tests/dense_invx_wide_ref.py: PyDenseInvxWideEngine) through gpu_parity.run_lockstep,
    one launch per phase, compared after every call with test_gpu_dense_invx.py's comparison: n = 33 (the first row past 32) with
    the device root policy over two epochs under LAP and DEG, n = 64 (every lane a row; the BFS mask and the bit shifts at their
    boundary) under ALL4, n = 50 (the benchmarked shape) under RATIO with roots of up to 612 slots (key width 10).  Sizes are set by
    the Python side (up to four eigenproblems per node);
  * a wide engine at n = 20 and n = 31 against the narrow INVX engine, and at n = 40 under the converted BOTH recipe against an
    inv_wide=True engine: trees, argmin, root-policy report, bit for bit;
  * the pool step (k_pool_search built for as many wavefronts as the LDS holds) against the launch-per-phase form at 256 agents for
    key widths 2, 4 and 10 at n = 40 under LAP; with a bf16 model at n = 33, and with an fp32 model under AZD_ENGINE_EXT_POOL_F32;
  * refusals and reads on a live engine, both argmin readers; the example driver with --extended --wide.
The seeds and sizes of the lock-step runs were chosen on the Python reference alone, so that every run meets expansions, the n = 33
and n = 64 runs terminals and transpositions too, and every eval lies inside (0, 1); the runs assert that on the reference's counters.
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as I
import dense_invx_ref as R
import dense_invx_wide_ref as W
import dense_spectral_cases as S
from gpu_parity import C21_CTRS, TOL_REF, PyDenseRef, assert_same_run, assert_tree_equal, az, run_lockstep, same_array, same_counters  # noqa: F401
from gpu_parity import f64_bits as bits

pytestmark = pytest.mark.gpu

c_recipe, c_inv_recipe = R.c_recipe, R.c_inv_recipe
NEW = ("LAP", "SLAP", "DEG", "RATIO", "ALL4")


def cost_of(az, recipe):
    return az.InvariantCostX(recipe.weights(), **recipe.kwargs())


# ---------------------------------------------------------------- the cost kernel alone
@pytest.mark.parametrize("name", NEW)
def test_wide_device_cost_equals_the_host_function_as_bytes(az, name):
    from azdopt_amd import _lib
    L = az.lib()
    by_n = {}
    for gname, n, adj in W.graph_set_wide():
        by_n.setdefault(n, []).append((gname, adj))
    seen = 0
    for n, graphs in sorted(by_n.items()):
        rc = c_recipe(R.RECIPES[name](n))
        a = np.array([adj for _, adj in graphs], dtype=np.uint64)
        dev = (_lib.DenseInvxCost * len(graphs))()
        _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, len(graphs), 2, C.byref(rc), dev, None), "probe_invx_cost_wide")
        for i, (gname, adj) in enumerate(graphs):
            host = _lib.DenseInvxCost()
            _lib.check(L.azd_dense_invx_cost_wide(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "invx_cost_wide")
            assert bytes(dev[i]) == bytes(host), (name, gname, n, list(dev[i].inv), list(host.inv), dev[i].cost, host.cost)
            seen += 1
    assert seen == 88


def test_wide_kernel_equals_the_narrow_kernel_up_to_32_vertices(az):
    from azdopt_amd import _lib
    L = az.lib()
    by_n = {}
    for gname, n, adj in A.graph_set()[::5]:
        by_n.setdefault(n, []).append((gname, adj))
    seen = 0
    for n, graphs in sorted(by_n.items()):
        a = np.array([adj for _, adj in graphs], dtype=np.uint64)
        for name in NEW:
            rc = c_recipe(R.RECIPES[name](n))
            wide, narrow = (_lib.DenseInvxCost * len(graphs))(), (_lib.DenseInvxCost * len(graphs))()
            _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), wide, None), "probe_invx_cost_wide")
            _lib.check(L.azd_debug_probe_invx_cost(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), narrow, None), "probe_invx_cost")
            for i, (gname, _) in enumerate(graphs):
                assert bytes(wide[i]) == bytes(narrow[i]), (name, gname, n)
                seen += 1
    assert seen == 5 * 112


@pytest.mark.parametrize("n", [23, 32, 33, 64])
def test_wide_device_cost_on_the_hard_spectral_cases(az, n):
    """every graph of tests/dense_spectral_cases.py on n vertices in one launch of the 64-row kernel (rank-deficient adjacency matrices
    in every labelling) under ALL4 (adjacency index 1, distance 1, Laplacian n - 2, signless Laplacian n - 1): records equal to the
    host function's as bytes, every invariant finite, and the adjacency, Laplacian and signless-Laplacian eigenvalues within
    64 n 2^-53 ||M||_F of LAPACK's (a NaN in the tridiagonal form leaves a finite value far from it)"""
    from azdopt_amd import _lib
    L = az.lib()
    graphs = S.by_size(S.graph_set() if n <= 32 else S.graph_set_wide())[n]
    assert len(graphs) >= 200
    rc = c_recipe(R.recipe_all4(n))
    a = np.array([adj for _, _, adj in graphs], dtype=np.uint64)
    dev = (_lib.DenseInvxCost * len(graphs))()
    _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), dev, None), "probe_invx_cost_wide")
    for i, (gname, _, adj) in enumerate(graphs):
        host = _lib.DenseInvxCost()
        _lib.check(L.azd_dense_invx_cost_wide(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "invx_cost_wide")
        assert dev[i].computed == 0xFFF and all(np.isfinite(x) for x in dev[i].inv), (gname, list(dev[i].inv))
        for m, slot, k in ((I.adjacency_matrix(adj, n), 8, rc.adj_index), (R.laplacian(adj, n, -1), 10, rc.lap_index), (R.laplacian(adj, n, 1), 11, rc.slap_index)):
            m = np.array(m, np.float64)
            assert abs(dev[i].inv[slot] - np.linalg.eigvalsh(m)[::-1][k]) <= 64.0 * n * 2.0 ** -53 * np.linalg.norm(m), (gname, slot, dev[i].inv[slot])
        assert bytes(dev[i]) == bytes(host), (gname, list(dev[i].inv), list(host.inv), dev[i].cost, host.cost)


# ---------------------------------------------------------------- engines against the Python reference
def compare_invx(opt, ref, agents, tag):
    """the extended invariant cost against PyDenseRef(PyDenseInvxWideEngine): the sixteen invariants bit for bit, mask, index, cost,
    the counters the reference keeps, and the argmin's graph re-evaluated through the host function (test_gpu_dense_invx.py's comparison)"""
    same_array(opt.state_vecs(), ref.state_vecs(), f"{tag} state_vecs")
    for i in agents:
        assert_tree_equal(opt.get_tree(i), ref.tree(i), f"{tag} agent {i}")
        sg, sp = opt.agent_state(i), ref.agent_state(i)
        for k in sp:  # (the cost fields are absent while the reference's agent stands on its root)
            if k in R.NAMES:
                assert bits(sg[k]) == bits(sp[k]), (tag, i, k, sg[k], sp[k])
            elif k == "cost":
                assert np.float32(sg[k]).view(np.uint32) == np.float32(sp[k]).view(np.uint32), (tag, i, k)
            else:
                assert np.array_equal(sg[k], sp[k]), (tag, i, k, sg[k], sp[k])
    cp = ref.counters()
    same_counters(opt.counters(), cp, tag, names=cp)
    ag, ap = opt.argmin_data(), ref.argmin()
    assert ag.eval.view(np.uint32) == np.float32(ap["eval"]).view(np.uint32), tag
    for k in R.NAMES:
        assert bits(ag.cost[k]) == bits(ap[k]), (tag, k, ag.cost[k], ap[k])
    assert (ag.cost["dist_k"], ag.cost["computed"]) == (ap["dist_k"], ap["computed"]) and ag.cost["cost"].view(np.uint32) == ap["cost"].view(np.uint32), tag
    assert np.array_equal(ag.state["adj"], ap["adj"]) and np.array_equal(ag.state["permitted"], ap["permitted"]), tag
    again = opt.space.invx_cost(ag.state["adj"])
    assert again["cost"].view(np.uint32) == ag.cost["cost"].view(np.uint32) and again["eval"].view(np.uint32) == ag.eval.view(np.uint32), tag
    assert all(bits(again[k]) == bits(ag.cost[k]) for k in R.NAMES), tag


def run_wide_parity(az, orc, n, name, B, p, kmin, kmax, tol, steps, epochs, seed, max_slots=128, met_all=True):
    """a wide engine, one launch per phase, against PyDenseInvxWideEngine after every call; the device root policy between epochs.
    met_all: the reference run also meets terminals and transpositions (seen to hold on the Python reference engine alone at each
    shape below that asks for it, as are the evals inside (0, 1); the n = 50 run with 300 .. 612 slots meets neither in 20 calls)"""
    recipe = R.RECIPES[name](n)
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost=cost_of(az, recipe), invx_wide=True)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, model, B)
    ref = PyDenseRef(W.PyDenseInvxWideEngine(n, B, recipe, p=p))
    evals = []

    def compare(o, r, agents, tag):
        compare_invx(o, r, agents, tag)
        evals.extend(float(c["eval"]) for c in r.e.costs if c is not None)

    run_lockstep(opt, ref, roots, orc, compare, seed=seed, tol=tol, steps=steps, epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=2,
                 boundary="policy", last_boundary=False, form="dense_per_call", nan_payloads=True)
    c = ref.counters()  # on the reference alone: the run was not vacuous
    print("n = %d %s:" % (n, name), c)
    assert c["EXPANSIONS"] > 0, c
    assert not met_all or (c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0), c
    assert evals and 0.0 < min(evals) and max(evals) < 1.0, (min(evals), max(evals))
    return opt


@pytest.mark.parametrize("name,steps", [("LAP", 20), ("DEG", 40)])
def test_wide_parity_n33_two_epochs_with_the_device_root_policy(az, orc, name, steps):
    """(LAP reduces a 33-row matrix per node on the Python side: half the calls of DEG, which runs no eigen-solve)"""
    run_wide_parity(az, orc, 33, name, 12, 0.2, 5, 100, ([50, 20, 10], 5), steps=steps, epochs=2, seed=3)


def test_wide_parity_n64_every_lane_a_row(az, orc):
    opt = run_wide_parity(az, orc, 64, "ALL4", 4, 0.1, 5, 128, TOL_REF, steps=20, epochs=1, seed=4)
    # argmin reads: the wide record against what argmin_data() gave the comparison above; the narrow call is refused, and the others
    from azdopt_amd import _lib
    rec = _lib.DenseInvxWideArgmin()
    _lib.check(opt._L.azd_engine_dense_invx_wide_argmin_data(opt._h, C.byref(rec)), "dense_invx_wide_argmin_data")
    a = opt.argmin_data()
    assert np.array_equal(np.array(rec.adj[:], np.uint64), a.state["adj"]) and rec.eval == a.eval and rec.dist_k == a.cost["dist_k"] == 1
    assert rec.computed == 0xFFF and all(bits(rec.inv[i]) == bits(a.cost[k]) for i, k in enumerate(R.NAMES))
    assert any(int(x) >> 63 for x in rec.adj[:63]), "vertex 63 has a neighbour: bit 63 of some row is set"
    assert all(int(x) != 0 for x in rec.adj[:]), "every lane is a row"
    assert opt._L.azd_engine_dense_invx_argmin_data(opt._h, C.byref(_lib.DenseInvxArgmin())) == 8  # AZD_ERR_UNSUPPORTED
    assert "azd_engine_dense_invx_wide_argmin_data" in opt._L.azd_last_error().decode()
    for fn, other in ((opt._L.azd_engine_dense_argmin_data, _lib.DenseArgmin()), (opt._L.azd_engine_dense_ah_argmin_data, _lib.DenseAhArgmin()),
                      (opt._L.azd_engine_dense_ah_wide_argmin_data, _lib.DenseAhWideArgmin()), (opt._L.azd_engine_dense_inv_argmin_data, _lib.DenseInvArgmin()),
                      (opt._L.azd_engine_dense_inv_wide_argmin_data, _lib.DenseInvWideArgmin())):
        assert fn(opt._h, C.byref(other)) == 8 and "azd_engine_dense_invx_wide_argmin_data" in opt._L.azd_last_error().decode()
    lam, mu = C.c_double(), C.c_int32()
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, C.byref(lam), None) == 8
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, None, C.byref(mu)) == 8


def test_wide_parity_n50_key_width_10(az, orc):
    """the benchmarked shape under RATIO (two pair terms, adj_eig named by a term alone); roots of 300 .. 612 slots: keys of ten
    words, slot bitmaps past word 8"""
    run_wide_parity(az, orc, 50, "RATIO", 8, 0.2, 300, 612, TOL_REF, steps=20, epochs=1, seed=6, max_slots=612, met_all=False)


# ---------------------------------------------------------------- wide against narrow, and against the INV-wide tier, where both run
def grow(az, space, B, seed, kmin, kmax, calls, more):
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    o = az.NablaOptimizer.par_new(space, roots, az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B)
    imp = o.par_roll_out_episodes(TOL_REF, n_calls=calls)
    if not more:
        return o, imp, 0, None
    o.par_reset_trees_policy(seed, 0, kmin, kmax)
    report = o.root_policy_report()
    return o, imp, o.par_roll_out_episodes(TOL_REF, n_calls=more), report


def assert_same_trees(runs, B, cost_keys=None):
    (o0, i0, j0, r0), (o1, i1, j1, r1) = runs
    assert (i0, j0) == (i1, j1)
    if r0 is not None:
        assert all(np.array_equal(r0[k], r1[k]) for k in ("branch", "node", "kept"))
    c0, c1 = o0.counters(), o1.counters()
    for k in C21_CTRS:
        assert c0[k] == c1[k], k
    assert c0["EXPANSIONS"] > 0 and c0["FAILED"] == 0
    for i in range(B):
        assert_tree_equal(o0.get_tree(i), o1.get_tree(i), f"agent {i}")
        s0, s1 = o0.agent_state(i), o1.agent_state(i)
        for k0, k1 in cost_keys or [(k, k) for k in s0]:
            assert np.array_equal(s0[k0], s1[k1]), (i, k0, s0[k0], s1[k1])
    a0, a1 = o0.argmin_data(), o1.argmin_data()
    assert a0.eval == a1.eval and a0.agent == a1.agent and a0.node == a1.node
    assert np.array_equal(a0.state["adj"], a1.state["adj"]) and np.array_equal(a0.state["permitted"], a1.state["permitted"])
    assert np.array_equal(o0.state_vecs(), o1.state_vecs())
    return a0, a1


@pytest.mark.parametrize("n,p,kmax", [(20, 0.2, 60), (31, 0.4, 128)])
def test_wide_engine_gives_the_narrow_engines_trees(az, n, p, kmax):
    B, seed = 32, 9
    runs = [grow(az, az.DenseGraphSpace(n, p, max_slots=128, cost=cost_of(az, R.recipe_all4(n)), invx_wide=wide), B, seed, 5, kmax, 40, 20)
            for wide in (True, False)]
    a0, a1 = assert_same_trees(runs, B)
    assert a0.cost == a1.cost


def test_a_wide_converted_both_recipe_engine_grows_the_inv_wide_engines_trees(az):
    n, B, seed = 40, 16, 9
    both = I.recipe_both(n)
    inv = az.InvariantCost(both.weights(), **both.kwargs())
    spaces = (az.DenseGraphSpace(n, 0.2, max_slots=128, cost=az.InvariantCostX.from_invariant_cost(inv), invx_wide=True),
              az.DenseGraphSpace(n, 0.2, max_slots=128, cost=inv, inv_wide=True))
    runs = [grow(az, sp, B, seed, 5, 128, 30, 0) for sp in spaces]
    keys = [(k, k) for k in ("parents", "permitted", "path", "state_pos", "dist_k", "computed", "cost") + I.NAMES]
    a0, a1 = assert_same_trees(runs, B, cost_keys=keys)
    assert a0.cost["cost"].view(np.uint32) == a1.cost["cost"].view(np.uint32) and all(bits(a0.cost[k]) == bits(a1.cost[k]) for k in I.NAMES)


# ---------------------------------------------------------------- pool step
@pytest.mark.parametrize("max_slots,kmin,kmax", [(128, 5, 128), (256, 129, 256), (640, 300, 640)])
def test_wide_pool_step_equals_the_launch_per_phase_form_at_256_agents(az, max_slots, kmin, kmax):
    """key widths 2, 4 and 10 at n = 40 (E = 780) under the LAP recipe: the pool step's searchers == one launch per phase -- trees,
    counters, argmin, state vectors -- over an epoch boundary"""
    n, B, seed, calls = 40, 256, 5, 30
    space = az.DenseGraphSpace(n, 0.2, max_slots=max_slots, cost=cost_of(az, R.recipe_lap(n)), invx_wide=True)
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
    a0 = o0.argmin_data()
    assert space.invx_cost(a0.state["adj"])["cost"] == a0.cost["cost"]


def test_wide_pool_step_with_a_bf16_model_and_with_an_fp32_model(az, monkeypatch):
    """a bf16 ActionModel on the pool step at n = 33 (the searchers' rows gathered into the batched GEMM launches) == one launch
    per phase; under AZD_ENGINE_EXT_POOL_F32 an fp32 model on the pool step == one launch per phase too"""
    n, B, seed, calls = 33, 256, 11, 40
    tol = ([50, 20, 10], 5)
    space = az.DenseGraphSpace(n, 0.2, cost=cost_of(az, R.recipe_ratio(n)), invx_wide=True)
    roots = space.generate_roots(seed, B)

    def mk(dtype, **kw):
        model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(128, 128), seed=seed, dtype=dtype)
        return az.NablaOptimizer.par_new(space, roots, model, B, **kw)

    def per_call(ref, tag):
        imp_ref = ref.par_roll_out_episodes(tol, n_calls=calls)
        assert ref.step_form()[0].startswith("per_call"), (tag, ref.step_form())
        return ref, imp_ref

    def same(pool, ref_run, tag):
        ref, imp_ref = ref_run
        imp_pool = pool.par_roll_out_episodes(tol, n_calls=calls)
        assert pool.step_form() == ("pool", ""), (tag, pool.step_form())
        assert imp_pool == imp_ref, tag
        assert_same_run(pool, ref, B, tag, every=3)
        assert pool.counters()["EVAL_ROWS"] == pool.counters()["EXPANSIONS"] > 0

    monkeypatch.setenv("AZD_DENSE_NO_POOL", "1")
    ref_run = per_call(mk("bf16", pool_step=True), "bf16")
    monkeypatch.delenv("AZD_DENSE_NO_POOL")
    same(mk("bf16", pool_step=True), ref_run, "bf16")
    same(mk("f32", pool_step=True, ext_pool_f32=True), per_call(mk("f32", persistent=False), "f32"), "f32")


# ---------------------------------------------------------------- a live engine
def test_wide_refusals_and_reads_on_a_live_engine(az):
    from azdopt_amd import _lib
    L = az.lib()
    n, B = 40, 4
    recipe = R.recipe_all4(n)
    space = az.DenseGraphSpace(n, 0.2, cost=cost_of(az, recipe), invx_wide=True)
    model = az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    adj, slots = space.generate_roots(0, B)
    # par_new before the recipe: refused, and the text names the setter (NablaOptimizer's constructor sets it: this engine is made by hand)
    cfg = _lib.EngineConfig(_lib.SPACE_DENSE, n, B, 0, 0, 0, 0, 0, _lib.ENGINE_DENSE_INVX | _lib.ENGINE_DENSE_INVX_WIDE)
    cfg.max_slots, cfg.dense_p = space.MAX_SLOTS, space.p
    h = C.c_void_p()
    _lib.check(L.azd_engine_create(C.byref(h), C.byref(cfg), model._h), "create")
    a8, s64 = np.ascontiguousarray(adj, np.uint8), np.ascontiguousarray(slots, np.uint64)
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 1
    assert "azd_engine_set_dense_invx_recipe" in L.azd_last_error().decode()
    # the INV setter on this tier: unsupported, naming the right call
    assert L.azd_engine_set_dense_inv_recipe(h, C.byref(c_inv_recipe(I.recipe_both(n)))) == 8 and "azd_engine_set_dense_invx_recipe" in L.azd_last_error().decode()
    bad = c_recipe(recipe)
    bad.lap_index = n  # the indices are checked at the engine's n: n - 1 = 39 is the last
    assert L.azd_engine_set_dense_invx_recipe(h, C.byref(bad)) == 1 and L.azd_last_error().decode().split(": ")[1] == "lap_index"
    rc = c_recipe(recipe)
    assert rc.slap_index == n - 1 and L.azd_engine_set_dense_invx_recipe(h, C.byref(rc)) == 0
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 0
    assert L.azd_engine_set_dense_invx_recipe(h, C.byref(rc)) == 1 and "par_new" in L.azd_last_error().decode()  # fixed once par_new has run
    L.azd_engine_destroy(h)
    opt = az.NablaOptimizer.par_new(space, (adj, slots), model, B)
    # the roots' records as the engine keeps them == the host function on the roots (azd_engine_dense_invx_agent_cost on a wide engine)
    for i in range(B):
        c = _lib.DenseInvxCost()
        assert L.azd_engine_dense_invx_agent_cost(opt._h, i, C.byref(c)) == 0
        st, want = opt.agent_state(i), space.invx_cost(adj[i].view(np.uint64))
        assert all(bits(st[k]) == bits(want[k]) == bits(c.inv[j]) for j, k in enumerate(R.NAMES)) and (st["dist_k"], st["computed"]) == (want["dist_k"], want["computed"])
        assert st["cost"].view(np.uint32) == want["cost"].view(np.uint32) == np.float32(c.cost).view(np.uint32) and np.float32(c.eval) == want["eval"]
    a = opt.argmin_data()
    assert space.invx_cost(a.state["adj"])["cost"] == a.cost["cost"] and a.cost["computed"] == 0xFFF and len(a.state["adj"]) == n
    # both argmin readers: the wide one reads, the narrow one is refused and names it; the INV, AH and default reads likewise
    assert L.azd_engine_dense_invx_wide_argmin_data(opt._h, C.byref(_lib.DenseInvxWideArgmin())) == 0
    assert L.azd_engine_dense_invx_argmin_data(opt._h, C.byref(_lib.DenseInvxArgmin())) == 8 and "azd_engine_dense_invx_wide_argmin_data" in L.azd_last_error().decode()
    assert L.azd_engine_dense_ah_agent_cost(opt._h, 0, C.byref(_lib.DenseAhCost())) == 8 and "azd_engine_dense_invx_agent_cost" in L.azd_last_error().decode()
    assert L.azd_engine_dense_inv_agent_cost(opt._h, 0, C.byref(_lib.DenseInvCost())) == 8 and "azd_engine_dense_invx_agent_cost" in L.azd_last_error().decode()
    # the wide read on a narrow INVX engine names the narrow reader; on an INV-wide, an AH-wide and a default engine it is unsupported
    nsp = az.DenseGraphSpace(20, 0.2, cost=cost_of(az, R.recipe_all4(20)))
    o = az.NablaOptimizer.par_new(nsp, nsp.generate_roots(0, B), az.TrivialModel(nsp.STATE_DIM, nsp.ACTION_DIM), B)
    assert L.azd_engine_dense_invx_wide_argmin_data(o._h, C.byref(_lib.DenseInvxWideArgmin())) == 8
    assert "azd_engine_dense_invx_argmin_data" in L.azd_last_error().decode()
    assert L.azd_engine_dense_invx_argmin_data(o._h, C.byref(_lib.DenseInvxArgmin())) == 0
    both = I.recipe_both(n)
    for kw in (dict(cost=az.InvariantCost(both.weights(), **both.kwargs()), inv_wide=True), dict(cost="ah", ah_wide=True), dict()):
        sp = az.DenseGraphSpace(n, 0.2, **kw)
        o = az.NablaOptimizer.par_new(sp, (adj, slots), az.TrivialModel(sp.STATE_DIM, sp.ACTION_DIM), B)
        assert L.azd_engine_dense_invx_wide_argmin_data(o._h, C.byref(_lib.DenseInvxWideArgmin())) == 8
        assert L.azd_engine_dense_invx_agent_cost(o._h, 0, C.byref(_lib.DenseInvxCost())) == 8
        assert L.azd_engine_set_dense_invx_recipe(o._h, C.byref(rc)) == 8


def test_wide_extended_example_driver_runs(tmp_path):
    """examples/invariants.py --extended --wide --n 40: exits 0 and prints the argmin's invariants for the epoch"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recipe = ('{"weights": {"lap_eig": 1, "max_degree": -0.25, "randic": 0.125}, "terms": [[0.5, "remoteness", "/", "radius"]], "lap_index": 38, '
              '"eval_offset": 40, "eval_scale": 0.00625}')
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "invariants.py"), "--extended", "--wide", "--recipe", recipe, "--n", "40",
                        "--epochs", "1", "--episodes", "20", "--batch", "32"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("==== EPOCH") == 1
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 1 and all(k in lines[0] for k in ("lap_eig:", "randic:", "remoteness:")) and "slap_eig" not in lines[0], lines
