"""The dense-graph space with the spectrum invariant cost (AZD_ENGINE_DENSE_INVS; dense_invs_kernels.hip) on the GPU.
  * the cost kernel alone (azd_debug_probe_invs_cost) against the host function azd_dense_invs_cost, records equal as bytes on the
    whole graph set of tests/dense_ah_ref.py (560 connected graphs, n = 4 .. 32) under the five new recipes of
    tests/dense_invs_ref.py and AH, one launch per n; against the Python reference at n = 31 under all fourteen; on the hard
    spectral cases at n = 21, 23, 31, 32 under ALLE; and against the INVX kernel (azd_debug_probe_invx_cost) under INVX's nine
    recipes at n = 4, 5, 20, 32;
  * an engine under the converted ALL4 recipe against an AZD_ENGINE_DENSE_INVX engine on the same roots: the same trees, bit for bit;
  * engines against the Python reference engine (PyDenseInvsEngine) through gpu_parity.run_lockstep with the comparison below:
    trees, state vectors, the twenty-one invariants (f64 by bits), mask, cost, counters, and the argmin re-evaluated through the
    host function.  N = 8 after every call; N = 4, 5 (the shortest reductions), 20, 32 (all 32 rows, lanes 0 .. 31 all live in the
    whole-spectrum finisher);
  * refusals and reads on a live engine; the example driver with --spectrum.
  The tier has no pool step yet (DESIGN.md "The spectrum invariant cost"), so there is no pool-step test here: at 256 agents and
  more its engines run one launch per phase, which test_invs_engines_run_one_launch_per_phase_at_every_population holds.
Every run asserts on the REFERENCE's counters that it met expansions, terminals and transpositions.
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ah_ref as A
import dense_invs_ref as R
import dense_invx_ref as X
import dense_spectral_cases as S
from gpu_parity import C21_CTRS, TOL_REF, PyDenseRef, assert_same_run, assert_tree_equal, az, run_lockstep, same_array, same_counters  # noqa: F401
from gpu_parity import f64_bits as bits

pytestmark = pytest.mark.gpu

TOL_SMALL = ([6, 3, 2], 1)
c_recipe = R.c_recipe


def cost_of(az, recipe):
    return az.InvariantCostS(recipe.weights(), **recipe.kwargs())


def assert_record_equals_reference(rec, ref, tag):
    for i, name in enumerate(R.NAMES):
        assert bits(rec.inv[i]) == bits(ref[name]), (tag, name, rec.inv[i], ref[name])
    assert (rec.dist_k, rec.computed) == (ref["dist_k"], ref["computed"]), tag
    assert np.float32(rec.cost).view(np.uint32) == ref["cost"].view(np.uint32), (tag, rec.cost, ref["cost"])
    assert np.float32(rec.eval).view(np.uint32) == ref["eval"].view(np.uint32), (tag, rec.eval, ref["eval"])


@pytest.mark.parametrize("name", R.NEW_RECIPES + ("AH",))
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
        dev = (_lib.DenseInvsCost * len(graphs))()
        _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), n, len(graphs), 2, C.byref(rc), dev, None), "probe_invs_cost")
        for i, (gname, adj) in enumerate(graphs):
            host = _lib.DenseInvsCost()
            _lib.check(L.azd_dense_invs_cost(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "invs_cost")
            assert bytes(dev[i]) == bytes(host), (name, gname, n, list(dev[i].inv), list(host.inv), dev[i].cost, host.cost)
            seen += 1
    assert seen == len(A.graph_set()) == 560


def test_device_cost_equals_the_python_reference_at_n31(az):
    """n = 31, G(31, 0.4) redrawn until connected (the example's roots): device == Python reference under every recipe"""
    from azdopt_amd import _lib
    rng = np.random.default_rng(31)
    graphs = [A.gnp_connected(rng, 31, 0.4) for _ in range(24)]
    R.prime([("g%d" % i, 31, g) for i, g in enumerate(graphs)], ks_of=lambda n: (0, 1, n - 2, n - 1))
    a = np.array(graphs, dtype=np.uint64)
    for name, mk in sorted(R.RECIPES.items()):
        recipe = mk(31)
        rc = c_recipe(recipe)
        dev = (_lib.DenseInvsCost * len(graphs))()
        _lib.check(az.lib().azd_debug_probe_invs_cost(0, _lib.ptr(a), 31, len(graphs), 1, C.byref(rc), dev, None), "probe_invs_cost")
        for i, adj in enumerate(graphs):
            assert_record_equals_reference(dev[i], R.invs_cost(adj, 31, recipe), (name, i))
    assert len(R.RECIPES) == 14


@pytest.mark.parametrize("n", [21, 23, 31, 32])
def test_device_cost_on_the_hard_spectral_cases(az, n):
    """every graph of tests/dense_spectral_cases.py on n vertices in one launch (rank-deficient adjacency matrices in every labelling)
    under ALLE -- four reductions, both finishers after each: records equal to the host function's as bytes, every invariant finite"""
    from azdopt_amd import _lib
    L = az.lib()
    graphs = S.by_size(S.graph_set())[n]
    assert len(graphs) >= 3 * (7 * n - 21) and any(g[0] in S.PARENT_FAILS for g in graphs)
    rc = c_recipe(R.RECIPES["ALLE"](n))
    a = np.array([adj for _, _, adj in graphs], dtype=np.uint64)
    dev = (_lib.DenseInvsCost * len(graphs))()
    _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), dev, None), "probe_invs_cost")
    for i, (gname, _, _) in enumerate(graphs):
        host = _lib.DenseInvsCost()
        _lib.check(L.azd_dense_invs_cost(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "invs_cost")
        assert all(np.isfinite(x) for x in dev[i].inv) and dev[i].computed == 0xFF | 0xF00 | 0x1F0000, (gname, list(dev[i].inv))
        assert bytes(dev[i]) == bytes(host), (gname, list(dev[i].inv), list(host.inv), dev[i].cost, host.cost)


@pytest.mark.parametrize("n", [4, 5, 20, 32])
def test_device_cost_equals_the_invx_kernel_under_the_invx_recipes(az, n):
    """inv[0 .. 15], dist_k, computed, cost and eval of the INVS probe == azd_debug_probe_invx_cost's, bit for bit; inv[16 .. 20] == 0.0"""
    from azdopt_amd import _lib
    L = az.lib()
    graphs = [adj for _, m, adj in A.graph_set() if m == n]
    assert len(graphs) >= 8
    a = np.array(graphs, dtype=np.uint64)
    for name in R.INVX_RECIPES:
        rs, rx = c_recipe(R.RECIPES[name](n)), X.c_recipe(X.RECIPES[name](n))
        ds, dx = (_lib.DenseInvsCost * len(graphs))(), (_lib.DenseInvxCost * len(graphs))()
        _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rs), ds, None), "probe_invs_cost")
        _lib.check(L.azd_debug_probe_invx_cost(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rx), dx, None), "probe_invx_cost")
        for i in range(len(graphs)):
            assert bytes(ds[i])[:128] + bytes(ds[i])[168:] == bytes(dx[i]), (name, n, i, list(ds[i].inv), list(dx[i].inv))
            assert bytes(ds[i])[128:168] == bytes(40), (name, n, i)
    assert len(R.INVX_RECIPES) == 9


# ---------------------------------------------------------------- the converted ALL4 recipe against the INVX tier
def test_a_converted_all4_recipe_engine_grows_the_invx_engines_trees(az):
    """AZD_ENGINE_DENSE_INVS under InvariantCostS.from_invariant_cost_x(ALL4) against AZD_ENGINE_DENSE_INVX under ALL4 on the same
    roots, with the device root policy over an epoch boundary: trees, state vectors, observations, counters, records and the
    argmin are equal"""
    n, B, p, kmin, kmax, tol, seed = 8, 16, 0.4, 2, 10, ([6, 3], 2), 5
    all4 = X.recipe_all4(n)
    invx = az.InvariantCostX(all4.weights(), **all4.kwargs())
    spaces = (az.DenseGraphSpace(n, p, cost=az.InvariantCostS.from_invariant_cost_x(invx)), az.DenseGraphSpace(n, p, cost=invx))
    roots = spaces[0].generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opts = [az.NablaOptimizer.par_new(sp, roots, az.HashStreamModel(sp.STATE_DIM, sp.ACTION_DIM, seed), B) for sp in spaces]

    def same(tag):
        o0, o1 = opts
        same_counters(o0.counters(), o1.counters(), tag)
        for i in range(B):
            assert_tree_equal(o0.get_tree(i), o1.get_tree(i), f"{tag} agent {i}")
            s0, s1 = o0.agent_state(i), o1.agent_state(i)
            for k in ("parents", "permitted", "path", "state_pos", "dist_k", "computed"):
                assert np.array_equal(s0[k], s1[k]), (tag, i, k)
            assert all(bits(s0[k]) == bits(s1[k]) for k in X.NAMES) and s0["cost"].view(np.uint32) == s1["cost"].view(np.uint32), (tag, i)
            assert all(bits(s0[k]) == bits(0.0) for k in R.NAMES[16:]), (tag, i)
        same_array(o0.state_vecs(), o1.state_vecs(), f"{tag} state_vecs")
        a0, a1 = o0.argmin_data(), o1.argmin_data()
        assert a0.eval.view(np.uint32) == a1.eval.view(np.uint32) and (a0.agent, a0.node) == (a1.agent, a1.node), tag
        assert np.array_equal(a0.state["adj"], a1.state["adj"]) and np.array_equal(a0.state["permitted"], a1.state["permitted"]), tag
        assert all(bits(a0.cost[k]) == bits(a1.cost[k]) for k in X.NAMES), tag

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
def compare_invs(opt, ref, agents, tag):
    """the spectrum invariant cost against PyDenseRef(PyDenseInvsEngine): the twenty-one invariants bit for bit, mask, index, cost,
    the counters the reference keeps, and the argmin's graph re-evaluated through the host function"""
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
    again = opt.space.invs_cost(ag.state["adj"])
    assert again["cost"].view(np.uint32) == ag.cost["cost"].view(np.uint32) and again["eval"].view(np.uint32) == ag.eval.view(np.uint32), tag
    assert all(bits(again[k]) == bits(ag.cost[k]) for k in R.NAMES), tag


def run_invs_parity(az, orc, n, name, B, p, kmin, kmax, tol, steps, epochs, seed, check_every, max_slots=128, pool=False):
    recipe = R.RECIPES[name](n)
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost=cost_of(az, recipe))
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    caps = {}
    if pool:
        model = model.serve_from_pool_evaluators()
        caps = dict(pool_step=True)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, model, B, **caps)
    ref = PyDenseRef(R.PyDenseInvsEngine(n, B, recipe, p=p))
    evals = []

    def compare(o, r, agents, tag):
        compare_invs(o, r, agents, tag)
        evals.extend(float(c["eval"]) for c in r.e.costs if c is not None)

    run_lockstep(opt, ref, roots, orc, compare, seed=seed, tol=tol, steps=steps, epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=2,
                 check_every=check_every, boundary="policy", last_boundary=epochs > 1, form="dense_pool" if pool else "dense_per_call",
                 nan_payloads=True)
    # on the reference alone: the run was not vacuous, and the recipe's offset and scale keep the evals inside [0, 1]
    c = ref.counters()
    assert c["EXPANSIONS"] > 0 and c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0, c
    assert evals and 0.0 <= min(evals) and max(evals) <= 1.0, (min(evals), max(evals))
    return opt


@pytest.mark.parametrize("name", ["ENERGY", "LAPE", "SPREAD", "ERATIO"])
def test_invs_parity_n8_every_call(az, orc, name):
    run_invs_parity(az, orc, 8, name, 12, 0.4, 2, 10, ([6, 3], 2), steps=16, epochs=2, seed=5, check_every=1)


@pytest.mark.parametrize("n", [4, 5])
def test_invs_parity_at_the_smallest_graphs(az, orc, n):
    """the shortest reductions; every root slot is modifiable (k up to E); all four spectra, both finishers after each"""
    run_invs_parity(az, orc, n, "ALLE", 12, 0.5, 1, n * (n - 1) // 2, TOL_SMALL, steps=12, epochs=2, seed=30 + n, check_every=1)


@pytest.mark.parametrize("name", ["LAPE", "ERATIO"])
def test_invs_parity_n20_with_the_device_root_policy(az, orc, name):
    run_invs_parity(az, orc, 20, name, 12, 0.2, 2, 8, ([6, 3], 2), steps=24, epochs=2, seed=2, check_every=12)


def test_invs_parity_n32_all_rows(az, orc):
    """n = 32: every row of the triangle, (1 << n) - 1 at the limit, lanes 0 .. 31 all live in the whole-spectrum finisher"""
    run_invs_parity(az, orc, 32, "ENERGY", 8, 0.4, 2, 8, ([6, 3], 2), steps=20, epochs=1, seed=1, check_every=10)


def test_invs_engines_run_one_launch_per_phase_at_every_population(az):
    """the tier builds no pool searchers: at 256 agents, where the dense-graph space's other tiers take the pool step, and when the
    pool step is asked for, an INVS engine runs the launch-per-phase form and gives the trees a small-population run's rules give"""
    n, B, seed = 8, 256, 3
    space = az.DenseGraphSpace(n, 0.4, max_slots=28, cost=cost_of(az, R.recipe_energy(n)))
    roots = space.generate_roots(seed, B, kmin=2, kmax=10)
    runs = []
    for kw in (dict(), dict(pool_step=True), dict(persistent=False)):
        o = az.NablaOptimizer.par_new(space, roots, az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B, **kw)
        runs.append((o, o.par_roll_out_episodes(([6, 3], 2), n_calls=8)))
        assert o.step_form()[0].startswith("per_call"), o.step_form()
    for o, imp in runs[1:]:
        assert imp == runs[0][1]
        assert_same_run(runs[0][0], o, B, "forms")


def test_invs_refusals_and_reads_on_a_live_engine(az):
    from azdopt_amd import _lib
    L = az.lib()
    n, B = 12, 4
    recipe = R.recipe_eratio(n)
    space = az.DenseGraphSpace(n, 0.3, cost=cost_of(az, recipe))
    model = az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    adj, slots = space.generate_roots(0, B)
    # par_new before the recipe: refused, and the text names the setter
    # (NablaOptimizer's constructor sets the recipe: this engine is made by hand)
    cfg = _lib.EngineConfig(_lib.SPACE_DENSE, n, B, 0, 0, 0, 0, 0, _lib.ENGINE_DENSE_INVS)
    cfg.max_slots, cfg.dense_p = space.MAX_SLOTS, space.p
    h = C.c_void_p()
    _lib.check(L.azd_engine_create(C.byref(h), C.byref(cfg), model._h), "create")
    a8, s64 = np.ascontiguousarray(adj, np.uint8), np.ascontiguousarray(slots, np.uint64)
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 1
    assert "azd_engine_set_dense_invs_recipe" in L.azd_last_error().decode()
    rc = c_recipe(recipe)
    # the INV and INVX setters on this tier: unsupported, naming the right call; a refused recipe names its field
    assert L.azd_engine_set_dense_inv_recipe(h, C.byref(X.c_inv_recipe(X.I.recipe_both(n)))) == 8 and "azd_engine_set_dense_invs_recipe" in L.azd_last_error().decode()
    assert L.azd_engine_set_dense_invx_recipe(h, C.byref(X.c_recipe(X.recipe_ratio(n)))) == 8 and "azd_engine_set_dense_invs_recipe" in L.azd_last_error().decode()
    bad = c_recipe(recipe)
    bad.term[0].a = 21
    assert L.azd_engine_set_dense_invs_recipe(h, C.byref(bad)) == 1 and "term.a" in L.azd_last_error().decode()
    assert L.azd_engine_set_dense_invs_recipe(h, C.byref(rc)) == 0
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 0
    assert L.azd_engine_set_dense_invs_recipe(h, C.byref(rc)) == 1 and "par_new" in L.azd_last_error().decode()  # fixed once par_new has run
    L.azd_engine_destroy(h)
    opt = az.NablaOptimizer.par_new(space, (adj, slots), model, B)
    # the default, the AH, the INV and the INVX reads on this tier: unsupported, naming the right call
    for fn, rec in ((L.azd_engine_dense_argmin_data, _lib.DenseArgmin()), (L.azd_engine_dense_ah_argmin_data, _lib.DenseAhArgmin()),
                    (L.azd_engine_dense_inv_argmin_data, _lib.DenseInvArgmin()), (L.azd_engine_dense_inv_wide_argmin_data, _lib.DenseInvWideArgmin()),
                    (L.azd_engine_dense_invx_argmin_data, _lib.DenseInvxArgmin()), (L.azd_engine_dense_invx_wide_argmin_data, _lib.DenseInvxWideArgmin())):
        assert fn(opt._h, C.byref(rec)) == 8 and "azd_engine_dense_invs_argmin_data" in L.azd_last_error().decode()
    assert L.azd_engine_dense_ah_agent_cost(opt._h, 0, C.byref(_lib.DenseAhCost())) == 8 and "azd_engine_dense_invs_agent_cost" in L.azd_last_error().decode()
    assert L.azd_engine_dense_inv_agent_cost(opt._h, 0, C.byref(_lib.DenseInvCost())) == 8 and "azd_engine_dense_invs_agent_cost" in L.azd_last_error().decode()
    assert L.azd_engine_dense_invx_agent_cost(opt._h, 0, C.byref(_lib.DenseInvxCost())) == 8 and "azd_engine_dense_invs_agent_cost" in L.azd_last_error().decode()
    lam = C.c_double()
    assert L.azd_engine_agent_state(opt._h, 0, None, None, None, None, C.byref(lam), None) == 8
    # the roots' records as the engine keeps them == the host function on the roots; the argmin re-evaluated
    for i in range(B):
        st, want = opt.agent_state(i), space.invs_cost(adj[i].view(np.uint64))
        assert all(bits(st[k]) == bits(want[k]) for k in R.NAMES) and (st["dist_k"], st["computed"]) == (want["dist_k"], want["computed"])
        assert st["cost"].view(np.uint32) == want["cost"].view(np.uint32)
    a = opt.argmin_data()
    assert space.invs_cost(a.state["adj"])["cost"] == a.cost["cost"] and a.cost["computed"] == 0xFF | 1 << 16 | 1 << 20
    # the INVS reads and the setter on an INVX and an INV engine (naming their calls), on an AH engine and on a default engine: unsupported
    for cost in (az.InvariantCostX({"edges": 1.0}), az.InvariantCost({"edges": 1.0}), "ah", "c21"):
        sp = az.DenseGraphSpace(n, 0.3, cost=cost)
        o = az.NablaOptimizer.par_new(sp, (adj, slots), az.TrivialModel(sp.STATE_DIM, sp.ACTION_DIM), B)
        tier = {"invx": "invx", "inv": "inv"}.get(sp.COST)
        assert L.azd_engine_dense_invs_argmin_data(o._h, C.byref(_lib.DenseInvsArgmin())) == 8
        assert tier is None or "azd_engine_dense_%s_argmin_data" % tier in L.azd_last_error().decode()
        assert L.azd_engine_dense_invs_agent_cost(o._h, 0, C.byref(_lib.DenseInvsCost())) == 8
        assert tier is None or "azd_engine_dense_%s_agent_cost" % tier in L.azd_last_error().decode()
        assert L.azd_engine_set_dense_invs_recipe(o._h, C.byref(rc)) == 8
        assert tier is None or "azd_engine_set_dense_%s_recipe" % tier in L.azd_last_error().decode()


def test_example_driver_runs_two_spectrum_epochs(tmp_path):
    """examples/invariants.py --spectrum: exits 0 and prints the argmin's invariants per epoch, the new names and a pair term among them"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recipe = ('{"weights": {"adj_energy": 1, "max_degree": -0.25}, "terms": [[0.5, "adj_spread", "/", "edges"]], '
              '"eval_offset": 8, "eval_scale": 0.015}')
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "invariants.py"), "--spectrum", "--recipe", recipe, "--n", "20", "--epochs", "2",
                        "--episodes", "20", "--batch", "32"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("==== EPOCH") == 2
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and all("adj_energy:" in l and "adj_spread:" in l and "lap_energy" not in l and "adj_eig" not in l for l in lines), lines
