"""The dense-graph space with the weighted-invariant cost (AZD_ENGINE_DENSE_INV; dense_inv_kernels.hip) on the GPU.
  * the cost kernel alone (azd_debug_probe_inv_cost) against the host function azd_dense_inv_cost, records equal as bytes on the
    whole graph set of tests/dense_ah_ref.py (560 connected graphs, n = 4 .. 32) under the four recipes of tests/dense_inv_ref.py,
    and against the Python reference at n = 31; on the hard case set of the spectral passes (tests/dense_spectral_cases.py: rank-deficient
    adjacency matrices in every labelling) at n = 21, 23, 31, 32, one launch per n, every invariant finite; and an engine rooted at
    double_broom(23, 19, 2), whose adjacency reduction ended in NaN before the deflation rule held at every n;
  * an engine with the AH recipe against an AZD_ENGINE_DENSE_AH engine on the same roots: the same trees, bit for bit;
  * engines against the Python reference engine (tests/dense_inv_ref.py: PyDenseInvEngine) through gpu_parity.run_lockstep with
    the comparison below: trees, state vectors, the ten invariants (f64 by bits), mask, cost, counters, and the argmin re-evaluated
    through the host function.  N = 8 after every call; N = 4, 5 (two Householder steps), 20, 32 (all 32 rows);
  * the pool step against the reference at N = 8, and against the launch-per-phase form at 640 agents for key widths 2, 4, 10;
    one fp32 model under AZD_ENGINE_EXT_POOL_F32; refusals and reads on a live engine; the example driver.
Every run asserts on the REFERENCE's counters that it met expansions, terminals and transpositions (N <= 8: root exhaustions too).
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as R
import dense_spectral_cases as S
from gpu_parity import C21_CTRS, TOL_REF, PyDenseRef, assert_same_run, assert_tree_equal, az, run_lockstep, same_array, same_counters  # noqa: F401
from gpu_parity import f64_bits as bits

pytestmark = pytest.mark.gpu

TOL_SMALL = ([6, 3, 2], 1)


def cost_of(az, recipe):
    return az.InvariantCost(recipe.weights(), **recipe.kwargs())


def c_recipe(recipe):
    from azdopt_amd import _lib
    r = _lib.DenseInvRecipe()
    for i, w in enumerate(recipe.weight):
        r.weight[i] = w
    r.bias, r.adj_index, r.dist_index = recipe.bias, recipe.adj_index, recipe.dist_index
    r.eval_offset, r.eval_scale = float(recipe.eval_offset), float(recipe.eval_scale)
    return r


def assert_record_equals_reference(rec, ref, tag):
    for i, name in enumerate(R.NAMES):
        assert bits(rec.inv[i]) == bits(ref[name]), (tag, name, rec.inv[i], ref[name])
    assert (rec.dist_k, rec.computed) == (ref["dist_k"], ref["computed"]), tag
    assert np.float32(rec.cost).view(np.uint32) == ref["cost"].view(np.uint32), (tag, rec.cost, ref["cost"])
    assert np.float32(rec.eval).view(np.uint32) == ref["eval"].view(np.uint32), (tag, rec.eval, ref["eval"])


@pytest.mark.parametrize("name", sorted(R.RECIPES))
def test_device_cost_equals_the_host_function_as_bytes(az, name):
    from azdopt_amd import _lib
    L = az.lib()
    by_n = {}
    for gname, n, adj in A.graph_set():
        by_n.setdefault(n, []).append((gname, adj))
    seen = 0
    for n, graphs in sorted(by_n.items()):
        rc = c_recipe(R.RECIPES[name](n))
        a = np.array([adj for _, adj in graphs], dtype=np.uint64)
        dev = (_lib.DenseInvCost * len(graphs))()
        _lib.check(L.azd_debug_probe_inv_cost(0, _lib.ptr(a), n, len(graphs), 2, C.byref(rc), dev, None), "probe_inv_cost")
        for i, (gname, adj) in enumerate(graphs):
            host = _lib.DenseInvCost()
            _lib.check(L.azd_dense_inv_cost(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "inv_cost")
            assert bytes(dev[i]) == bytes(host), (name, gname, n, list(dev[i].inv), list(host.inv), dev[i].cost, host.cost)
            seen += 1
    assert seen == len(A.graph_set()) == 560


def test_device_cost_equals_the_python_reference_at_n31(az):
    """n = 31, G(31, 0.4) redrawn until connected (the example's roots): device == Python reference under every recipe"""
    from azdopt_amd import _lib
    rng = np.random.default_rng(31)
    graphs = [A.gnp_connected(rng, 31, 0.4) for _ in range(24)]
    a = np.array(graphs, dtype=np.uint64)
    for name, mk in sorted(R.RECIPES.items()):
        recipe = mk(31)
        rc = c_recipe(recipe)
        dev = (_lib.DenseInvCost * len(graphs))()
        _lib.check(az.lib().azd_debug_probe_inv_cost(0, _lib.ptr(a), 31, len(graphs), 1, C.byref(rc), dev, None), "probe_inv_cost")
        for i, adj in enumerate(graphs):
            assert_record_equals_reference(dev[i], R.inv_cost(adj, 31, recipe), (name, i))


@pytest.mark.parametrize("name", ["ADJ", "BOTH"])
@pytest.mark.parametrize("n", [21, 23, 31, 32])
def test_device_cost_on_the_hard_spectral_cases(az, n, name):
    """every graph of the set on n vertices in one launch, under the adjacency recipe (adj_index = 0) and the both-spectra recipe
    (adj_index = n - 1, dist_index = 1): records equal to the host function's as bytes, every invariant finite, adj_eig within 64 n 2^-53 ||A||_F of LAPACK's"""
    from azdopt_amd import _lib
    L = az.lib()
    graphs = S.by_size(S.graph_set())[n]
    assert len(graphs) >= 3 * (7 * n - 21) and any(g[0] in S.PARENT_FAILS for g in graphs)
    rc = c_recipe(R.RECIPES[name](n))
    a = np.array([adj for _, _, adj in graphs], dtype=np.uint64)
    dev = (_lib.DenseInvCost * len(graphs))()
    _lib.check(L.azd_debug_probe_inv_cost(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), dev, None), "probe_inv_cost")
    for i, (gname, _, _) in enumerate(graphs):
        host = _lib.DenseInvCost()
        _lib.check(L.azd_dense_inv_cost(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "inv_cost")
        assert all(np.isfinite(x) for x in dev[i].inv), (name, gname, list(dev[i].inv))
        if dev[i].computed >> 8 & 1:  # adj_eig against LAPACK: a NaN in the tridiagonal form leaves a finite value far from it
            m = np.array(R.adjacency_matrix(graphs[i][2], n), np.float64)
            assert abs(dev[i].inv[8] - np.linalg.eigvalsh(m)[::-1][rc.adj_index]) <= 64.0 * n * 2.0 ** -53 * np.linalg.norm(m), (name, gname, dev[i].inv[8])
        assert bytes(dev[i]) == bytes(host), (name, gname, list(dev[i].inv), list(host.inv), dev[i].cost, host.cost)


def test_an_engine_rooted_at_the_heavy_end_first_brooms_reads_back_the_host_functions_adj_eig(az):
    """AZD_ENGINE_DENSE_INV at n = 23 under {"adj_eig": 1}, rooted through par_new at double_broom(23, 19, 2) and double_broom(23, 20, 1)
    (without the deflation rule: NaN in the tridiagonal form, a finite wrong adj_eig) and at two more graphs of the set: each agent's
    record and the argmin read back the host function's adj_eig, which is LAPACK's within 64 n 2^-53 ||A||_F"""
    n, B = 23, 4
    by_name = {name: adj for name, _, adj in S.by_size(S.graph_set())[n]}
    names = ("broom(19,2)-n23/id", "broom(20,1)-n23/id", "K[11,12]-n23/p1", "star-n23/p2")
    assert set(names[:2]) <= set(S.PARENT_FAILS)
    space = az.DenseGraphSpace(n, 0.3, cost=az.InvariantCost({"adj_eig": 1.0}, adj_index=0, eval_scale=1.0 / n))
    adj, slots = space.generate_roots(0, B)
    adj = np.array(adj, dtype=np.uint8).reshape(B, 8 * n)
    for i, name in enumerate(names):
        adj[i] = np.array(by_name[name], dtype=np.uint64).view(np.uint8)
    opt = az.NablaOptimizer.par_new(space, (adj, slots), az.TrivialModel(space.STATE_DIM, space.ACTION_DIM), B)
    for i, name in enumerate(names):
        st, want = opt.agent_state(i), space.inv_cost(adj[i].view(np.uint64))
        assert np.array_equal(st["parents"], adj[i]), name
        assert bits(st["adj_eig"]) == bits(want["adj_eig"]) and st["computed"] == want["computed"] == 0xFF | 1 << 8, (name, st["adj_eig"], want["adj_eig"])
        assert st["cost"].view(np.uint32) == want["cost"].view(np.uint32), name
        m = np.array(R.adjacency_matrix(by_name[name], n), np.float64)
        assert abs(st["adj_eig"] - np.linalg.eigvalsh(m)[-1]) <= 64.0 * n * 2.0 ** -53 * np.linalg.norm(m), (name, st["adj_eig"])
    a = opt.argmin_data()
    again = space.inv_cost(a.state["adj"])
    assert bits(a.cost["adj_eig"]) == bits(again["adj_eig"]) and a.cost["cost"].view(np.uint32) == again["cost"].view(np.uint32)


# ---------------------------------------------------------------- the AH recipe against the AH tier
def test_an_ah_recipe_engine_grows_the_ah_engines_trees(az):
    """AZD_ENGINE_DENSE_INV under InvariantCost.aouchiche_hansen(n) against AZD_ENGINE_DENSE_AH on the same roots, with the device
    root policy over an epoch boundary: trees, state vectors, observations, counters and the argmin's eval are equal"""
    n, B, p, kmin, kmax, tol, seed = 8, 12, 0.4, 2, 10, ([6, 3], 2), 5
    spaces = (az.DenseGraphSpace(n, p, cost=az.InvariantCost.aouchiche_hansen(n)), az.DenseGraphSpace(n, p, cost="ah"))
    roots = spaces[0].generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opts = [az.NablaOptimizer.par_new(sp, roots, az.HashStreamModel(sp.STATE_DIM, sp.ACTION_DIM, seed), B) for sp in spaces]

    def same(tag):
        o0, o1 = opts
        same_counters(o0.counters(), o1.counters(), tag)
        for i in range(B):
            assert_tree_equal(o0.get_tree(i), o1.get_tree(i), f"{tag} agent {i}")
            s0, s1 = o0.agent_state(i), o1.agent_state(i)
            for k in ("parents", "permitted", "path", "state_pos"):
                assert np.array_equal(s0[k], s1[k]), (tag, i, k)
            assert bits(s0["proximity"]) == bits(s1["proximity"]) and bits(s0["dist_eig"]) == bits(s1["eigenvalue"]), (tag, i)
            assert (s0["diameter"], s0["dist_k"]) == (s1["diameter"], s1["k"]) and s0["cost"].view(np.uint32) == s1["cost"].view(np.uint32), (tag, i)
        same_array(o0.state_vecs(), o1.state_vecs(), f"{tag} state_vecs")
        a0, a1 = o0.argmin_data(), o1.argmin_data()
        assert a0.eval.view(np.uint32) == a1.eval.view(np.uint32) and (a0.agent, a0.node) == (a1.agent, a1.node), tag
        assert np.array_equal(a0.state["adj"], a1.state["adj"]) and np.array_equal(a0.state["permitted"], a1.state["permitted"]), tag

    same("par_new")
    for epoch in range(2):
        for s in range(0, 40, 8):
            imp = [o.par_roll_out_episodes(tol, n_calls=8) for o in opts]
            assert imp[0] == imp[1], (epoch, s, imp)
            same(f"epoch {epoch} step {s + 8}")
        obs = [o.observe(2) for o in opts]
        for x, y, what in zip(obs[0], obs[1], ("rows", "observations", "weights")):
            same_array(x, y, f"epoch {epoch} observe {what}")
        for o in opts:
            o.par_reset_trees_policy(seed, epoch, kmin, kmax)
        same(f"epoch {epoch} reset")
    c = opts[0].counters()
    assert c["FAILED"] == 0 and c["EXPANSIONS"] > 0 and c["TRANSPOSITIONS"] > 0 and c["TERMINALS"] > 0


# ---------------------------------------------------------------- engines against the Python reference
def compare_inv(opt, ref, agents, tag):
    """the weighted-invariant cost against PyDenseRef(PyDenseInvEngine): the ten invariants bit for bit, mask, index, cost, the
    counters the reference keeps, and the argmin's graph re-evaluated through the host function"""
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
    again = opt.space.inv_cost(ag.state["adj"])
    assert again["cost"].view(np.uint32) == ag.cost["cost"].view(np.uint32) and again["eval"].view(np.uint32) == ag.eval.view(np.uint32), tag
    assert all(bits(again[k]) == bits(ag.cost[k]) for k in R.NAMES), tag


def run_inv_parity(az, orc, n, name, B, p, kmin, kmax, tol, steps, epochs, seed, check_every, exhaust=False, max_slots=128, pool=False):
    recipe = R.RECIPES[name](n)
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost=cost_of(az, recipe))
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    caps = {}
    if pool:
        model = model.serve_from_pool_evaluators()
        caps = dict(pool_step=True)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, model, B, **caps)
    ref = PyDenseRef(R.PyDenseInvEngine(n, B, recipe, p=p))
    evals = []

    def compare(o, r, agents, tag):
        compare_inv(o, r, agents, tag)
        evals.extend(float(c["eval"]) for c in r.e.costs if c is not None)

    run_lockstep(opt, ref, roots, orc, compare, seed=seed, tol=tol, steps=steps, epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=2,
                 check_every=check_every, boundary="policy", last_boundary=epochs > 1, form="dense_pool" if pool else "dense_per_call",
                 nan_payloads=True)
    # on the reference alone: the run was not vacuous, and the recipe's offset and scale keep the evals inside (0, 1)
    c = ref.counters()
    assert c["EXPANSIONS"] > 0 and c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0, c
    assert not exhaust or c["ROOT_EXHAUSTED"] > 0, c
    assert evals and 0.0 < min(evals) and max(evals) < 1.0, (min(evals), max(evals))
    return opt


@pytest.mark.parametrize("name", ["INT", "ADJ", "BOTH"])
def test_inv_parity_n8_every_call(az, orc, name):
    run_inv_parity(az, orc, 8, name, 12, 0.4, 2, 10, ([6, 3], 2), steps=40, epochs=2, seed=5, check_every=1, exhaust=True)


@pytest.mark.parametrize("name", ["INT", "ADJ", "BOTH"])
@pytest.mark.parametrize("n", [4, 5])
def test_inv_parity_at_the_smallest_graphs(az, orc, n, name):
    """n = 4 runs two Householder steps, every root slot is modifiable (k up to E)"""
    run_inv_parity(az, orc, n, name, 12, 0.5, 1, n * (n - 1) // 2, TOL_SMALL, steps=12, epochs=2, seed=30 + n, check_every=1, exhaust=True)


@pytest.mark.parametrize("name", ["INT", "ADJ"])
def test_inv_parity_n20_two_epochs_with_the_device_root_policy(az, orc, name):
    run_inv_parity(az, orc, 20, name, 24, 0.2, 5, 60, ([50, 20, 10], 5), steps=60, epochs=2, seed=2, check_every=30)


def test_inv_parity_n20_both_spectra(az, orc):
    run_inv_parity(az, orc, 20, "BOTH", 16, 0.2, 5, 60, ([50, 20, 10], 5), steps=40, epochs=1, seed=2, check_every=20)


@pytest.mark.parametrize("name", ["BOTH", "INT"])
def test_inv_parity_n32_all_rows(az, orc, name):
    """n = 32: every row of the triangle, (1 << n) - 1 at the limit; the reference's tolerances"""
    run_inv_parity(az, orc, 32, name, 8, 0.4, 5, 128, TOL_REF, steps=30, epochs=1, seed=1, check_every=15)


def test_inv_pool_step_against_the_reference(az, orc):
    run_inv_parity(az, orc, 8, "BOTH", 12, 0.4, 2, 10, ([6, 3], 2), steps=40, epochs=2, seed=7, check_every=1, exhaust=True, pool=True)


@pytest.mark.parametrize("max_slots,kmin,kmax", [(128, 5, 128), (256, 129, 256), (465, 300, 465)])
def test_inv_pool_step_equals_the_launch_per_phase_form_at_640_agents(az, max_slots, kmin, kmax):
    """key widths 2, 4 and 10 (N = 31: E = 465) under the ADJ recipe: the pool step's searchers == one launch per phase -- trees,
    counters, argmin, state vectors -- over an epoch boundary"""
    n, B, seed, calls = 31, 640, 5, 40
    space = az.DenseGraphSpace(n, 0.4, max_slots=max_slots, cost=cost_of(az, R.recipe_adj(n)))
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
        imp2 = o.par_roll_out_episodes(TOL_REF, n_calls=20)
        runs.append((o, imp, imp2))
    (o0, i0, j0), (o1, i1, j1) = runs
    assert (i0, j0) == (i1, j1)
    c0, c1 = o0.counters(), o1.counters()
    for k in C21_CTRS:
        assert c0[k] == c1[k], k
    for i in range(0, B, 7):
        assert_tree_equal(o0.get_tree(i), o1.get_tree(i), f"agent {i}")
        s0, s1 = o0.agent_state(i), o1.agent_state(i)
        assert all(np.array_equal(s0[k], s1[k]) for k in s0), i
    a0, a1 = o0.argmin_data(), o1.argmin_data()
    assert a0.eval == a1.eval and a0.agent == a1.agent and a0.node == a1.node and a0.cost == a1.cost
    assert np.array_equal(o0.state_vecs(), o1.state_vecs())
    assert o0.space.inv_cost(a0.state["adj"])["cost"] == a0.cost["cost"]


def test_inv_with_an_fp32_model_on_the_pool_step_equals_the_launch_per_phase_form(az):
    """AZD_ENGINE_EXT_POOL_F32 beside AZD_ENGINE_DENSE_INV: the smallest case of tests/test_gpu_dense_ext_f32.py (n = 8, S = 85)"""
    n, B, calls, seed, hidden = 8, 96, 20, 7, (64, 32)
    space = az.DenseGraphSpace(n, 0.2, max_slots=28, cost=cost_of(az, R.recipe_both(n)))
    kmin, kmax = space.default_permitted_range()
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    runs = []
    for kw in (dict(pool_step=True, ext_pool_f32=True), dict(persistent=False)):
        model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=hidden, seed=seed, dtype="f32")
        o = az.NablaOptimizer.par_new(space, roots, model, B, **kw, **az.tree_capacities(calls + 12, kmax))
        runs.append((o, o.par_roll_out_episodes(TOL_REF, n_calls=calls)))
    (o0, i0), (o1, i1) = runs
    assert o0.step_form() == ("pool", "") and o1.step_form()[0].startswith("per_call"), (o0.step_form(), o1.step_form())
    assert i0 == i1
    assert_same_run(o0, o1, B, "fp32 model")
    c0 = o0.counters()
    assert c0["EVAL_ROWS"] == c0["EXPANSIONS"] > 0 and c0["FAILED"] == 0


def test_inv_refusals_and_reads_on_a_live_engine(az):
    from azdopt_amd import _lib
    L = az.lib()
    n, B = 12, 4
    recipe = R.recipe_both(n)
    space = az.DenseGraphSpace(n, 0.3, cost=cost_of(az, recipe))
    model = az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    adj, slots = space.generate_roots(0, B)
    # par_new before the recipe: refused, and the text names the setter
    # (NablaOptimizer's constructor sets the recipe: this engine is made by hand)
    cfg = _lib.EngineConfig(_lib.SPACE_DENSE, n, B, 0, 0, 0, 0, 0, _lib.ENGINE_DENSE_INV)
    cfg.max_slots, cfg.dense_p = space.MAX_SLOTS, space.p
    h = C.c_void_p()
    _lib.check(L.azd_engine_create(C.byref(h), C.byref(cfg), model._h), "create")
    a8, s64 = np.ascontiguousarray(adj, np.uint8), np.ascontiguousarray(slots, np.uint64)
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 1
    assert "azd_engine_set_dense_inv_recipe" in L.azd_last_error().decode()
    rc = c_recipe(recipe)
    assert L.azd_engine_set_dense_inv_recipe(h, C.byref(rc)) == 0
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 0
    assert L.azd_engine_set_dense_inv_recipe(h, C.byref(rc)) == 1 and "par_new" in L.azd_last_error().decode()  # fixed once par_new has run
    L.azd_engine_destroy(h)
    opt = az.NablaOptimizer.par_new(space, (adj, slots), model, B)
    # the default and the AH reads on this tier: unsupported, naming the right call
    for fn, rec in ((L.azd_engine_dense_argmin_data, _lib.DenseArgmin()), (L.azd_engine_dense_ah_argmin_data, _lib.DenseAhArgmin())):
        assert fn(opt._h, C.byref(rec)) == 8 and "azd_engine_dense_inv_argmin_data" in L.azd_last_error().decode()
    assert L.azd_engine_dense_ah_agent_cost(opt._h, 0, C.byref(_lib.DenseAhCost())) == 8 and "azd_engine_dense_inv_agent_cost" in L.azd_last_error().decode()
    lam = C.c_double()
    assert L.azd_engine_agent_state(opt._h, 0, None, None, None, None, C.byref(lam), None) == 8
    # the roots' records as the engine keeps them == the host function on the roots; the argmin re-evaluated
    for i in range(B):
        st, want = opt.agent_state(i), space.inv_cost(adj[i].view(np.uint64))
        assert all(bits(st[k]) == bits(want[k]) for k in R.NAMES) and (st["dist_k"], st["computed"]) == (want["dist_k"], want["computed"])
        assert st["cost"].view(np.uint32) == want["cost"].view(np.uint32)
    a = opt.argmin_data()
    assert space.inv_cost(a.state["adj"])["cost"] == a.cost["cost"] and a.cost["computed"] == 0x3FF
    # the INV reads and the setter on an AH engine and on a default engine: unsupported
    for cost in ("ah", "c21"):
        sp = az.DenseGraphSpace(n, 0.3, cost=cost)
        o = az.NablaOptimizer.par_new(sp, (adj, slots), az.TrivialModel(sp.STATE_DIM, sp.ACTION_DIM), B)
        assert L.azd_engine_dense_inv_argmin_data(o._h, C.byref(_lib.DenseInvArgmin())) == 8
        assert L.azd_engine_dense_inv_agent_cost(o._h, 0, C.byref(_lib.DenseInvCost())) == 8
        assert L.azd_engine_set_dense_inv_recipe(o._h, C.byref(rc)) == 8


def test_example_driver_runs_two_epochs(tmp_path):
    """examples/invariants.py: exits 0 and prints the argmin's invariants per epoch; an integer recipe reports no eigenvalue"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recipe = '{"weights": {"remoteness": 1, "proximity": -1, "max_degree": 0.25}, "eval_offset": 2, "eval_scale": 0.015625}'
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "invariants.py"), "--recipe", recipe, "--epochs", "2", "--episodes", "20",
                        "--batch", "32"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("==== EPOCH") == 2
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and all("remoteness:" in l and "max_degree:" in l and "adj_eig" not in l and "dist_eig" not in l for l in lines), lines
