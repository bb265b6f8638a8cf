"""The dense-graph space with the spectrum invariant cost up to 64 vertices (AZD_ENGINE_DENSE_INVS_WIDE; dense_invs_wide_kernels.hip)
on the GPU.
  * the 64-row cost kernel alone (azd_debug_probe_invs_cost_wide) against the host function azd_dense_invs_cost_wide, records equal as
    bytes on the 88 graphs of tests/dense_ah_wide_ref.py (n = 33 .. 64) under ENERGY, LAPE, SPREAD, ERATIO and ALLE of
    tests/dense_invs_ref.py, one launch per n; against the 32-row kernel on every fifth graph of the n <= 32 set; against the
    INVX-wide kernel under INVX's nine recipes at n = 33 and 64; and on the hard case set of the spectral passes
    (tests/dense_spectral_cases.py) at n = 33 and 64 under ALLE: every invariant finite, adj_eig, lap_eig and slap_eig within
    64 n 2^-53 ||M||_F of LAPACK's, every energy within n times that bound, the spread within twice it;
  * engines against the Python reference engine (tests/dense_invs_wide_ref.py: PyDenseInvsWideEngine) through gpu_parity.run_lockstep,
    one launch per phase, compared after every call with test_gpu_dense_invs.py's comparison: n = 33 (the first row past 32) under
    ALLE with the device root policy over two epochs, n = 64 (every lane a row and an eigenvalue; the vertex mask, the spread's
    shuffle from lane 63) under ERATIO, n = 50 under ENERGY with roots of 300 .. 612 slots (key width 10).  Sizes are set by the
    Python side (up to four reductions and four whole spectra per node);
  * a wide engine at n = 20 and n = 31 against the narrow INVS engine under ALLE, and at n = 40 under the converted ALL4 recipe against
    an invx_wide=True engine: trees, argmin, root-policy report, bit for bit;
  * no pool step: one launch per phase at 256 agents and under pool_step=True; azd_debug_ext_pool_plan is AZD_ERR_UNSUPPORTED;
  * refusals and reads on a live engine, both argmin readers; the example driver with --spectrum --wide.
The seeds and sizes of the lock-step runs were chosen on the Python reference alone, so that every run meets expansions, the n = 33
and n = 64 runs terminals and transpositions too, and every eval lies inside (0, 1); the runs assert that on the reference's counters.
No test here runs pool searchers with this cost: none are built (DESIGN.md "No pool step on this tier").
Run with -m gpu on an MI355X."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as I
import dense_invs_ref as R
import dense_invs_wide_ref as W
import dense_invx_ref as X
import dense_spectral_cases as S
from gpu_parity import C21_CTRS, TOL_REF, PyDenseRef, assert_same_run, assert_tree_equal, az, run_lockstep, same_array, same_counters  # noqa: F401
from gpu_parity import f64_bits as bits

pytestmark = pytest.mark.gpu

c_recipe = R.c_recipe
NEW = R.NEW_RECIPES
assert NEW == ("ENERGY", "LAPE", "SPREAD", "ERATIO", "ALLE")


def cost_of(az, recipe):
    return az.InvariantCostS(recipe.weights(), **recipe.kwargs())


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
        dev = (_lib.DenseInvsCost * len(graphs))()
        _lib.check(L.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), n, len(graphs), 2, C.byref(rc), dev, None), "probe_invs_cost_wide")
        for i, (gname, adj) in enumerate(graphs):
            host = _lib.DenseInvsCost()
            _lib.check(L.azd_dense_invs_cost_wide(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "invs_cost_wide")
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
            wide, narrow = (_lib.DenseInvsCost * len(graphs))(), (_lib.DenseInvsCost * len(graphs))()
            _lib.check(L.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), wide, None), "probe_invs_cost_wide")
            _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), narrow, None), "probe_invs_cost")
            for i, (gname, _) in enumerate(graphs):
                assert bytes(wide[i]) == bytes(narrow[i]), (name, gname, n)
                seen += 1
    assert seen == 5 * 112


@pytest.mark.parametrize("n", [33, 64])
def test_wide_device_cost_equals_the_invx_wide_kernel_under_the_invx_recipes(az, n):
    """inv[0 .. 15], dist_k, computed, cost and eval of the wide INVS probe == azd_debug_probe_invx_cost_wide's, bit for bit; inv[16 .. 20] == 0.0"""
    from azdopt_amd import _lib
    L = az.lib()
    graphs = [adj for _, m, adj in W.graph_set_wide() if m == n]
    assert len(graphs) >= 4
    a = np.array(graphs, dtype=np.uint64)
    for name in R.INVX_RECIPES:
        rs, rx = c_recipe(R.RECIPES[name](n)), X.c_recipe(X.RECIPES[name](n))
        ds, dx = (_lib.DenseInvsCost * len(graphs))(), (_lib.DenseInvxCost * len(graphs))()
        _lib.check(L.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rs), ds, None), "probe_invs_cost_wide")
        _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rx), dx, None), "probe_invx_cost_wide")
        for i in range(len(graphs)):
            assert bytes(ds[i])[:128] + bytes(ds[i])[168:] == bytes(dx[i]), (name, n, i, list(ds[i].inv), list(dx[i].inv))
            assert bytes(ds[i])[128:168] == bytes(40), (name, n, i)
    assert len(R.INVX_RECIPES) == 9


@pytest.mark.parametrize("n", [33, 64])
def test_wide_device_cost_on_the_hard_spectral_cases(az, n):
    """every graph of tests/dense_spectral_cases.py on n vertices in one launch of the 64-row kernel (rank-deficient adjacency matrices
    in every labelling) under ALLE (adjacency index 1, distance 1, Laplacian n - 2, signless Laplacian n - 1; four reductions, both
    finishers after each): records equal to the host function's as bytes, every invariant finite; adj_eig, lap_eig and slap_eig within
    64 n 2^-53 ||M||_F of LAPACK's, each energy within n times that bound, the spread within twice it"""
    from azdopt_amd import _lib
    L = az.lib()
    graphs = S.by_size(S.graph_set_wide())[n]
    assert len(graphs) >= 200
    rc = c_recipe(R.recipe_alle(n))
    a = np.array([adj for _, _, adj in graphs], dtype=np.uint64)
    dev = (_lib.DenseInvsCost * len(graphs))()
    _lib.check(L.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), n, len(graphs), 1, C.byref(rc), dev, None), "probe_invs_cost_wide")
    eps = 64.0 * n * 2.0 ** -53
    for i, (gname, _, adj) in enumerate(graphs):
        host = _lib.DenseInvsCost()
        _lib.check(L.azd_dense_invs_cost_wide(_lib.ptr(a[i]), n, C.byref(rc), C.byref(host)), "invs_cost_wide")
        d = dev[i]
        assert d.computed == 0xFF | 0xF00 | 0x1F0000 and all(np.isfinite(x) for x in d.inv), (gname, list(d.inv))
        mats = {k: np.array(m, np.float64) for k, m in S.matrices(adj, n).items()}
        s = sum(X.degrees(adj)) / n
        for which, eig_slot, k, energy_slot in (("adj", 8, rc.adj_index, 16), ("dist", None, None, 17), ("lap", 10, rc.lap_index, 18), ("slap", 11, rc.slap_index, 19)):
            m = mats[which]
            lapack = np.linalg.eigvalsh(m)  # ascending
            tol = eps * np.linalg.norm(m)
            if eig_slot is not None:
                assert abs(d.inv[eig_slot] - lapack[::-1][k]) <= tol, (gname, which, d.inv[eig_slot])
            want = math.fsum(abs(x) for x in (lapack - s if which in ("lap", "slap") else lapack))
            assert abs(d.inv[energy_slot] - want) <= n * tol, (gname, which, d.inv[energy_slot], want)
            if which == "adj":
                assert abs(d.inv[20] - (lapack[-1] - lapack[0])) <= 2 * tol, (gname, d.inv[20])
        assert bytes(d) == bytes(host), (gname, list(d.inv), list(host.inv), d.cost, host.cost)


# ---------------------------------------------------------------- engines against the Python reference
def compare_invs(opt, ref, agents, tag):
    """test_gpu_dense_invs.py's comparison: the spectrum invariant cost against PyDenseRef(PyDenseInvsWideEngine): the twenty-one
    invariants bit for bit, mask, index, cost, the counters the reference keeps, and the argmin's graph re-evaluated through the host
    function (the wide one: the space is an invs_wide one)"""
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


def run_wide_parity(az, orc, n, name, B, p, kmin, kmax, tol, steps, epochs, seed, max_slots=128, met_all=True):
    """a wide engine, one launch per phase, against PyDenseInvsWideEngine after every call; the device root policy between epochs.
    met_all: the reference run also meets terminals and transpositions (seen to hold on the Python reference engine alone at each
    shape below that asks for it, as are the evals inside (0, 1); the n = 50 run with 300 .. 612 slots meets neither in 15 calls)"""
    recipe = R.RECIPES[name](n)
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost=cost_of(az, recipe), invs_wide=True)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, model, B)
    ref = PyDenseRef(W.PyDenseInvsWideEngine(n, B, recipe, p=p))
    evals = []

    def compare(o, r, agents, tag):
        compare_invs(o, r, agents, tag)
        evals.extend(float(c["eval"]) for c in r.e.costs if c is not None)

    run_lockstep(opt, ref, roots, orc, compare, seed=seed, tol=tol, steps=steps, epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=2,
                 boundary="policy", last_boundary=False, form="dense_per_call", nan_payloads=True)
    c = ref.counters()  # on the reference alone: the run was not vacuous
    print("n = %d %s:" % (n, name), c)
    assert c["EXPANSIONS"] > 0, c
    assert not met_all or (c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0), c
    assert evals and 0.0 < min(evals) and max(evals) < 1.0, (min(evals), max(evals))
    return opt


def test_wide_parity_n33_two_epochs_with_the_device_root_policy(az, orc):
    """the first row past 32 under ALLE: four reductions and four whole spectra per node on the Python side, so 4 agents, 2 x 8 calls;
    roots of 2 .. 6 slots and the small tolerances, so that 16 calls meet terminals and transpositions"""
    run_wide_parity(az, orc, 33, "ALLE", 4, 0.2, 2, 6, ([6, 3], 2), steps=8, epochs=2, seed=2)


def test_wide_parity_n64_every_lane_a_row(az, orc):
    """ERATIO: one reduction per node (the adjacency matrix), the energy and the spread from its whole spectrum -- at n = 64 every
    lane owns a row and an eigenvalue, the spread's upper shuffle reads lane 63, the vertex mask is all ones"""
    opt = run_wide_parity(az, orc, 64, "ERATIO", 4, 0.1, 5, 128, TOL_REF, steps=20, epochs=1, seed=4)
    # argmin reads: the wide record against what argmin_data() gave the comparison above; the narrow call is refused, and the others
    from azdopt_amd import _lib
    rec = _lib.DenseInvsWideArgmin()
    _lib.check(opt._L.azd_engine_dense_invs_wide_argmin_data(opt._h, C.byref(rec)), "dense_invs_wide_argmin_data")
    a = opt.argmin_data()
    assert np.array_equal(np.array(rec.adj[:], np.uint64), a.state["adj"]) and rec.eval == a.eval and rec.dist_k == a.cost["dist_k"]
    assert rec.computed == 0xFF | 1 << 16 | 1 << 20 and all(bits(rec.inv[i]) == bits(a.cost[k]) for i, k in enumerate(R.NAMES))
    assert any(int(x) >> 63 for x in rec.adj[:63]), "vertex 63 has a neighbour: bit 63 of some row is set"
    assert all(int(x) != 0 for x in rec.adj[:]), "every lane is a row"
    assert opt._L.azd_engine_dense_invs_argmin_data(opt._h, C.byref(_lib.DenseInvsArgmin())) == 8  # AZD_ERR_UNSUPPORTED
    assert "azd_engine_dense_invs_wide_argmin_data" in opt._L.azd_last_error().decode()
    lam, mu = C.c_double(), C.c_int32()
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, C.byref(lam), None) == 8
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, None, C.byref(mu)) == 8


def test_wide_parity_n50_key_width_10(az, orc):
    """the benchmarked shape under ENERGY; roots of 300 .. 612 slots: keys of ten words, slot bitmaps past word 8"""
    run_wide_parity(az, orc, 50, "ENERGY", 8, 0.2, 300, 612, TOL_REF, steps=15, epochs=1, seed=6, max_slots=612, met_all=False)


# ---------------------------------------------------------------- wide against narrow, and against the INVX-wide tier, where both run
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
    runs = [grow(az, az.DenseGraphSpace(n, p, max_slots=128, cost=cost_of(az, R.recipe_alle(n)), invs_wide=wide), B, seed, 5, kmax, 40, 20)
            for wide in (True, False)]
    a0, a1 = assert_same_trees(runs, B)
    assert a0.cost == a1.cost and a0.cost["computed"] == 0xFF | 0xF00 | 0x1F0000


def test_a_wide_converted_all4_recipe_engine_grows_the_invx_wide_engines_trees(az):
    n, B, seed = 40, 16, 9
    all4 = X.recipe_all4(n)
    invx = az.InvariantCostX(all4.weights(), **all4.kwargs())
    spaces = (az.DenseGraphSpace(n, 0.2, max_slots=128, cost=az.InvariantCostS.from_invariant_cost_x(invx), invs_wide=True),
              az.DenseGraphSpace(n, 0.2, max_slots=128, cost=invx, invx_wide=True))
    runs = [grow(az, sp, B, seed, 5, 128, 30, 15) for sp in spaces]
    keys = [(k, k) for k in ("parents", "permitted", "path", "state_pos", "dist_k", "computed", "cost") + X.NAMES]
    a0, a1 = assert_same_trees(runs, B, cost_keys=keys)
    assert a0.cost["cost"].view(np.uint32) == a1.cost["cost"].view(np.uint32) and all(bits(a0.cost[k]) == bits(a1.cost[k]) for k in X.NAMES)
    assert all(bits(a0.cost[k]) == bits(0.0) for k in R.NAMES[16:])


# ---------------------------------------------------------------- no pool step
def test_wide_engines_run_one_launch_per_phase_at_every_population(az):
    """the tier builds no pool searchers: at 256 agents, where the dense-graph space's other wide tiers take the pool step, and when
    the pool step is asked for, a wide INVS engine runs the launch-per-phase form and grows the same trees; the plan is unsupported"""
    from azdopt_amd import _lib
    n, B, seed = 33, 256, 3
    space = az.DenseGraphSpace(n, 0.2, max_slots=128, cost=cost_of(az, R.recipe_energy(n)), invs_wide=True)
    roots = space.generate_roots(seed, B, kmin=2, kmax=10)
    runs = []
    for kw in (dict(), dict(pool_step=True), dict(persistent=False)):
        o = az.NablaOptimizer.par_new(space, roots, az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B, **kw)
        runs.append((o, o.par_roll_out_episodes(([6, 3], 2), n_calls=8)))
        assert o.step_form()[0].startswith("per_call"), o.step_form()
    for o, imp in runs[1:]:
        assert imp == runs[0][1]
        assert_same_run(runs[0][0], o, B, "forms")
    assert runs[0][0].counters()["EXPANSIONS"] > 0
    cfg = _lib.EngineConfig(_lib.SPACE_DENSE, n, B, 0, 0, 0, 0, 0, _lib.ENGINE_DENSE_INVS | _lib.ENGINE_DENSE_INVS_WIDE)
    cfg.max_slots, cfg.dense_p = 128, 0.2
    waves, lds = C.c_int(), C.c_size_t()
    assert az.lib().azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 8  # AZD_ERR_UNSUPPORTED
    assert "no searcher-only pool step" in az.lib().azd_last_error().decode()


# ---------------------------------------------------------------- a live engine
def test_wide_refusals_and_reads_on_a_live_engine(az):
    from azdopt_amd import _lib
    L = az.lib()
    n, B = 40, 4
    recipe = R.recipe_alle(n)
    space = az.DenseGraphSpace(n, 0.2, cost=cost_of(az, recipe), invs_wide=True)
    model = az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    adj, slots = space.generate_roots(0, B)
    # par_new before the recipe: refused, and the text names the setter (NablaOptimizer's constructor sets it: this engine is made by hand)
    cfg = _lib.EngineConfig(_lib.SPACE_DENSE, n, B, 0, 0, 0, 0, 0, _lib.ENGINE_DENSE_INVS | _lib.ENGINE_DENSE_INVS_WIDE)
    cfg.max_slots, cfg.dense_p = space.MAX_SLOTS, space.p
    h = C.c_void_p()
    _lib.check(L.azd_engine_create(C.byref(h), C.byref(cfg), model._h), "create")
    a8, s64 = np.ascontiguousarray(adj, np.uint8), np.ascontiguousarray(slots, np.uint64)
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 1
    assert "azd_engine_set_dense_invs_recipe" in L.azd_last_error().decode()
    # the INV and INVX setters on this tier: unsupported, naming the right call
    assert L.azd_engine_set_dense_inv_recipe(h, C.byref(X.c_inv_recipe(I.recipe_both(n)))) == 8 and "azd_engine_set_dense_invs_recipe" in L.azd_last_error().decode()
    assert L.azd_engine_set_dense_invx_recipe(h, C.byref(X.c_recipe(X.recipe_ratio(n)))) == 8 and "azd_engine_set_dense_invs_recipe" in L.azd_last_error().decode()
    bad = c_recipe(recipe)
    bad.lap_index = n  # the indices are checked at the engine's n: n - 1 = 39 is the last
    assert L.azd_engine_set_dense_invs_recipe(h, C.byref(bad)) == 1 and L.azd_last_error().decode().split(": ")[1] == "lap_index"
    rc = c_recipe(recipe)
    assert rc.slap_index == n - 1 and L.azd_engine_set_dense_invs_recipe(h, C.byref(rc)) == 0
    assert L.azd_engine_par_new(h, _lib.ptr(a8), _lib.ptr(s64)) == 0
    assert L.azd_engine_set_dense_invs_recipe(h, C.byref(rc)) == 1 and "par_new" in L.azd_last_error().decode()  # fixed once par_new has run
    L.azd_engine_destroy(h)
    opt = az.NablaOptimizer.par_new(space, (adj, slots), model, B)
    # the roots' records as the engine keeps them == the host function on the roots (azd_engine_dense_invs_agent_cost on a wide engine)
    for i in range(B):
        c = _lib.DenseInvsCost()
        assert L.azd_engine_dense_invs_agent_cost(opt._h, i, C.byref(c)) == 0
        st, want = opt.agent_state(i), space.invs_cost(adj[i].view(np.uint64))
        assert all(bits(st[k]) == bits(want[k]) == bits(c.inv[j]) for j, k in enumerate(R.NAMES)) and (st["dist_k"], st["computed"]) == (want["dist_k"], want["computed"])
        assert st["cost"].view(np.uint32) == want["cost"].view(np.uint32) == np.float32(c.cost).view(np.uint32) and np.float32(c.eval) == want["eval"]
    a = opt.argmin_data()
    assert space.invs_cost(a.state["adj"])["cost"] == a.cost["cost"] and a.cost["computed"] == 0xFF | 0xF00 | 0x1F0000 and len(a.state["adj"]) == n
    # both argmin readers: the wide one reads, the narrow one is refused and names it; the readers of the seven other tiers likewise
    assert L.azd_engine_dense_invs_wide_argmin_data(opt._h, C.byref(_lib.DenseInvsWideArgmin())) == 0
    assert L.azd_engine_dense_invs_argmin_data(opt._h, C.byref(_lib.DenseInvsArgmin())) == 8 and "azd_engine_dense_invs_wide_argmin_data" in L.azd_last_error().decode()
    for fn, other in ((L.azd_engine_dense_argmin_data, _lib.DenseArgmin()), (L.azd_engine_dense_ah_argmin_data, _lib.DenseAhArgmin()),
                      (L.azd_engine_dense_ah_wide_argmin_data, _lib.DenseAhWideArgmin()), (L.azd_engine_dense_inv_argmin_data, _lib.DenseInvArgmin()),
                      (L.azd_engine_dense_inv_wide_argmin_data, _lib.DenseInvWideArgmin()), (L.azd_engine_dense_invx_argmin_data, _lib.DenseInvxArgmin()),
                      (L.azd_engine_dense_invx_wide_argmin_data, _lib.DenseInvxWideArgmin())):
        assert fn(opt._h, C.byref(other)) == 8 and "azd_engine_dense_invs_wide_argmin_data" in L.azd_last_error().decode()
    assert L.azd_engine_dense_ah_agent_cost(opt._h, 0, C.byref(_lib.DenseAhCost())) == 8 and "azd_engine_dense_invs_agent_cost" in L.azd_last_error().decode()
    assert L.azd_engine_dense_inv_agent_cost(opt._h, 0, C.byref(_lib.DenseInvCost())) == 8 and "azd_engine_dense_invs_agent_cost" in L.azd_last_error().decode()
    assert L.azd_engine_dense_invx_agent_cost(opt._h, 0, C.byref(_lib.DenseInvxCost())) == 8 and "azd_engine_dense_invs_agent_cost" in L.azd_last_error().decode()
    # the wide read on a narrow INVS engine names the narrow reader; on an INVX-wide, an INV-wide, an AH-wide and a default engine it is unsupported
    nsp = az.DenseGraphSpace(20, 0.2, cost=cost_of(az, R.recipe_alle(20)))
    o = az.NablaOptimizer.par_new(nsp, nsp.generate_roots(0, B), az.TrivialModel(nsp.STATE_DIM, nsp.ACTION_DIM), B)
    assert L.azd_engine_dense_invs_wide_argmin_data(o._h, C.byref(_lib.DenseInvsWideArgmin())) == 8
    assert "azd_engine_dense_invs_argmin_data" in L.azd_last_error().decode()
    assert L.azd_engine_dense_invs_argmin_data(o._h, C.byref(_lib.DenseInvsArgmin())) == 0
    both, all4 = I.recipe_both(n), X.recipe_all4(n)
    for kw in (dict(cost=az.InvariantCostX(all4.weights(), **all4.kwargs()), invx_wide=True), dict(cost=az.InvariantCost(both.weights(), **both.kwargs()), inv_wide=True),
               dict(cost="ah", ah_wide=True), dict()):
        sp = az.DenseGraphSpace(n, 0.2, **kw)
        o = az.NablaOptimizer.par_new(sp, (adj, slots), az.TrivialModel(sp.STATE_DIM, sp.ACTION_DIM), B)
        assert L.azd_engine_dense_invs_wide_argmin_data(o._h, C.byref(_lib.DenseInvsWideArgmin())) == 8
        assert L.azd_engine_dense_invs_agent_cost(o._h, 0, C.byref(_lib.DenseInvsCost())) == 8
        assert L.azd_engine_set_dense_invs_recipe(o._h, C.byref(rc)) == 8


def test_wide_spectrum_example_driver_runs_two_epochs(tmp_path):
    """examples/invariants.py --spectrum --wide --n 40: exits 0 and prints the argmin's invariants per epoch"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recipe = ('{"weights": {"adj_energy": 1, "max_degree": -0.25}, "terms": [[0.5, "adj_spread", "/", "edges"]], '
              '"eval_offset": 10, "eval_scale": 0.006}')
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "invariants.py"), "--spectrum", "--wide", "--recipe", recipe, "--n", "40",
                        "--epochs", "2", "--episodes", "20", "--batch", "32"], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("==== EPOCH") == 2
    lines = [l for l in r.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and all("adj_energy:" in l and "adj_spread:" in l and "lap_energy" not in l and "adj_eig" not in l for l in lines), lines
