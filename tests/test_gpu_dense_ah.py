"""The dense-graph space with the Aouchiche-Hansen cost (AZD_ENGINE_DENSE_AH; dense_ah_kernels.hip) on the GPU.
  * the cost kernel alone (azd_debug_probe_ah_cost) against the host function azd_dense_ah_cost, bit for bit on the whole graph set
    of tests/dense_ah_ref.py (560 connected graphs, n = 4 .. 32), and the f64 primitives it rests on against numpy;
  * engines against the Python reference engine (tests/dense_ah_ref.py: PyDenseEngine, whose glue tests/test_dense_ah_reference.py
    pins to the C++ oracle in "c21" mode) with the hash-stream predictions: trees with keys as action-id sets, state vectors,
    the cost fields per agent, counters, observations, argmin and the device root policy, bit for bit.  Sizes (the Python side
    solves one eigenproblem per node): N = 8: 12 agents x 40 calls x 2 epochs, compared after every call; N = 20: 24 agents x
    120 calls x 2 epochs; N = 31: 16 agents x 60 calls at the reference's tolerances ([200, 50, 50], 25);
  * the pool step against the reference at N = 8, and against the launch-per-phase form at 640 agents for key widths 2, 4, 10;
  * the 1396-256-128-930 fp32 model at N = 31 with the reference fed the device's prediction rows; rejections and reads; the
    example driver.
Run with -m gpu on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ah_ref as R
from gpu_parity import C21_CTRS, TOL_REF, PyDenseRef, assert_tree_equal, az, compare_ah, run_lockstep  # noqa: F401
from gpu_parity import f64_bits as bits

pytestmark = pytest.mark.gpu


def test_f64_primitives_bit_exact(az):
    from azdopt_amd import _lib
    rng = np.random.default_rng(0)
    n = 1 << 16
    x = rng.standard_normal(2 * n) * 10.0 ** rng.integers(-6, 7, 2 * n)
    x[0:2 * 4096:2] = rng.integers(0, 1024, 4096).astype(np.float64)  # small integers over small integers: the cost's own operands
    x[1:2 * 4096:2] = rng.integers(1, 66, 4096).astype(np.float64)
    bits = rng.integers(1, 0x7FE0000000000000, n // 4, dtype=np.uint64)  # every exponent, subnormals included
    x[2 * 8192:2 * 8192 + 2 * (n // 4):2] = bits.view(np.float64)
    x[1::2][x[1::2] == 0.0] = 1.0
    out = np.zeros(3 * n, np.float64)
    _lib.check(az.lib().azd_debug_probe_math_f64(0, _lib.ptr(x), _lib.ptr(out), n), "probe_math_f64")
    a, b = x[0::2], x[1::2]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        q = a / b
        want = (q, np.sqrt(np.abs(a)), a - q * b)
    for i, name in enumerate(("x / y", "sqrt", "x - (x / y) * y")):
        same = out[i::3].view(np.uint64) == want[i].view(np.uint64)
        same |= np.isnan(out[i::3]) & np.isnan(want[i])
        assert same.all(), (name, int((~same).sum()), np.flatnonzero(~same)[:4])


def test_device_cost_equals_the_host_function_bit_for_bit(az):
    from azdopt_amd import _lib
    L = az.lib()
    by_n = {}
    for name, n, adj in R.graph_set():
        by_n.setdefault(n, []).append((name, adj))
    seen = 0
    for n, graphs in sorted(by_n.items()):
        a = np.array([adj for _, adj in graphs], dtype=np.uint64)
        dev = (_lib.DenseAhCost * len(graphs))()
        _lib.check(L.azd_debug_probe_ah_cost(0, _lib.ptr(a), n, len(graphs), 2, dev, None), "probe_ah_cost")
        for i, (name, adj) in enumerate(graphs):
            host = _lib.DenseAhCost()
            _lib.check(L.azd_dense_ah_cost(_lib.ptr(a[i]), n, C.byref(host)), "ah_cost")
            assert bytes(dev[i]) == bytes(host), (name, n, [(f, getattr(dev[i], f), getattr(host, f)) for f, _ in host._fields_])
            seen += 1
    assert seen == len(R.graph_set()) >= 500


def test_device_cost_equals_the_python_reference_at_the_reference_shape(az):
    """n = 31 (ConnectedBitsetGraph<31>, 05-ah.rs), G(31, 0.4) redrawn until connected (05-ah.rs:93): device == Python reference."""
    from azdopt_amd import _lib
    rng = np.random.default_rng(31)
    graphs = [R.gnp_connected(rng, 31, 0.4) for _ in range(24)]
    a = np.array(graphs, dtype=np.uint64)
    dev = (_lib.DenseAhCost * len(graphs))()
    ms = C.c_float(0)
    _lib.check(az.lib().azd_debug_probe_ah_cost(0, _lib.ptr(a), 31, len(graphs), 1, dev, C.byref(ms)), "probe_ah_cost")
    for i, adj in enumerate(graphs):
        r = R.ah_cost(adj, 31)
        assert np.float64(dev[i].proximity).view(np.uint64) == np.float64(r["proximity"]).view(np.uint64)
        assert np.float64(dev[i].eigenvalue).view(np.uint64) == np.float64(r["eigenvalue"]).view(np.uint64), (i, dev[i].eigenvalue, r["eigenvalue"])
        assert (dev[i].diameter, dev[i].k) == (r["diameter"], r["k"])
        assert np.float32(dev[i].cost).view(np.uint32) == r["cost"].view(np.uint32)
        assert np.float32(dev[i].eval).view(np.uint32) == r["eval"].view(np.uint32)


# ---------------------------------------------------------------- engines against the Python reference
def run_ah_parity(az, orc, n, B, p, kmin, kmax, tol, steps, epochs, seed, check_every, max_slots=128, policy=True, pool=False, **caps):
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost="ah")
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    if pool:
        model = model.serve_from_pool_evaluators()
        caps = dict(caps, pool_step=True)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, model, B, **caps)
    run_lockstep(opt, PyDenseRef(R.PyDenseEngine(n, B, cost="ah", p=p)), roots, orc, compare_ah, seed=seed, tol=tol, steps=steps,
                 epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=2, check_every=check_every, boundary="policy" if policy else "fresh",
                 form="dense_pool" if pool else "dense_per_call", nan_payloads=True)
    return opt.counters()


def test_ah_parity_n8_every_call(az, orc):
    c = run_ah_parity(az, orc, 8, 12, 0.4, 2, 10, ([6, 3], 2), steps=40, epochs=2, seed=5, check_every=1)
    assert c["TRANSPOSITIONS"] > 0 and c["TERMINALS"] > 0


def test_ah_parity_n20_two_epochs_with_the_device_root_policy(az, orc):
    c = run_ah_parity(az, orc, 20, 24, 0.2, 5, 60, ([50, 20, 10], 5), steps=120, epochs=2, seed=2, check_every=30)
    assert c["EXPANSIONS"] > 1000 and c["TRANSPOSITIONS"] > 0


def test_ah_parity_n31_reference_tolerances(az, orc):
    """the reference's shape: ConnectedBitsetGraph<31>, G(31, 0.4) roots (05-ah.rs:93), 16 agents x 60 calls"""
    c = run_ah_parity(az, orc, 31, 16, 0.4, 5, 128, TOL_REF, steps=60, epochs=1, seed=1, check_every=20)
    assert c["EXPANSIONS"] > 500


def test_ah_pool_step_against_the_reference(az, orc):
    c = run_ah_parity(az, orc, 8, 12, 0.4, 2, 10, ([6, 3], 2), steps=40, epochs=2, seed=7, check_every=1, pool=True)
    assert c["EXPANSIONS"] > 100


@pytest.mark.parametrize("max_slots,kmin,kmax", [(128, 5, 128), (256, 129, 256), (465, 300, 465)])
def test_ah_pool_step_equals_the_launch_per_phase_form_at_640_agents(az, max_slots, kmin, kmax):
    """key widths 2, 4 and 10 (N = 31: E = 465): the pool step's searchers (fewer than sixteen waves a workgroup: the cost's working
    set is in the wave's block) == one launch per phase -- trees, counters, argmin, state vectors -- over an epoch boundary"""
    n, B, seed, calls = 31, 640, 5, 40
    space = az.DenseGraphSpace(n, 0.4, max_slots=max_slots, cost="ah")
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
    assert o0.space.ah_cost(a0.state["adj"])["cost"] == a0.cost["cost"]


def test_ah_n31_with_the_fp32_model(az, orc):
    """1396-256-128-930 fp32 (05-ah.rs's widths under the live ActionModel head) at N = 31, one launch per phase; the reference is
    fed the GPU's prediction rows and must grow the same trees; then one optimiser step"""
    n, B, seed = 31, 16, 3
    space = az.DenseGraphSpace(n, 0.4, max_slots=128, cost="ah")
    model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(256, 128), seed=seed)
    roots = space.generate_roots(seed, B)
    opt = az.NablaOptimizer.par_new(space, roots, model, B)
    pe = R.PyDenseEngine(n, B, cost="ah", p=0.4)
    pe.new_begin(*roots)
    pe.new_end(opt.predictions())
    for s in range(40):
        opt.par_roll_out_episodes(TOL_REF)
        pe.rollout_begin(*TOL_REF)
        assert np.array_equal(opt.state_vecs(), pe.state_vecs()), s
        pe.rollout_end(opt.predictions())
    assert opt.step_form()[0].startswith("per_call")
    for i in range(B):
        assert_tree_equal(opt.get_tree(i), pe.export_tree(i), f"agent {i}")
    assert opt.argmin_data().eval == pe.argmin["eval"]
    # the same 40 calls in one go: the launches of a call captured in a hipGraph and replayed
    model2 = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(256, 128), seed=seed)
    opt2 = az.NablaOptimizer.par_new(space, roots, model2, B)
    opt2.par_roll_out_episodes(TOL_REF, n_calls=40)
    assert opt2.step_form()[0] == "per_call_graph", opt2.step_form()
    for i in range(B):
        assert_tree_equal(opt2.get_tree(i), opt.get_tree(i), f"graph replay, agent {i}")
    assert opt2.argmin_data().eval == opt.argmin_data().eval and opt2.argmin_data().cost == opt.argmin_data().cost
    loss = opt.par_update_model(2)
    assert np.isfinite(loss) and loss >= 0


def test_ah_rejections_and_reads(az):
    from azdopt_amd import _lib
    space = az.DenseGraphSpace(12, 0.3, cost="ah")
    model = az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    adj, slots = space.generate_roots(0, 4)
    lone = np.zeros((4, 12), np.uint64)  # not connected
    with pytest.raises(az.AzdError):
        az.NablaOptimizer.par_new(space, (lone.view(np.uint8).reshape(4, -1), slots), model, 4)
    many = az.DenseGraphSpace(30, 0.2, cost="ah")  # a root with 300 slots does not fit the default key width
    with pytest.raises(az.AzdError):
        az.NablaOptimizer.par_new(many, many.generate_roots(0, 2, kmin=300, kmax=300), az.TrivialModel(many.STATE_DIM, many.ACTION_DIM), 2)
    with pytest.raises(az.AzdError) as ei:  # n beyond the cost's limit, refused by name
        big = az.DenseGraphSpace(33, 0.2, cost="ah")
        az.NablaOptimizer.par_new(big, big.generate_roots(0, 2), az.TrivialModel(big.STATE_DIM, big.ACTION_DIM), 2)
    assert ei.value.status == 1 and "n:" in str(ei.value)
    opt = az.NablaOptimizer.par_new(space, (adj, slots), model, 4)
    with pytest.raises(az.AzdError):
        opt.par_reset_trees_policy(0, 0, 5, 200)
    rec = _lib.DenseArgmin()
    assert opt._L.azd_engine_dense_argmin_data(opt._h, C.byref(rec)) == 8  # AZD_ERR_UNSUPPORTED
    lam = C.c_double()
    assert opt._L.azd_engine_agent_state(opt._h, 0, None, None, None, None, C.byref(lam), None) == 8
    a = opt.argmin_data()
    assert space.ah_cost(a.state["adj"])["cost"] == a.cost["cost"]
    for i in range(4):  # the roots' costs as the engine keeps them == the host function on the roots
        st = opt.agent_state(i)
        want = space.ah_cost(adj[i].view(np.uint64))
        assert bits(st["proximity"]) == bits(want["proximity"]) and bits(st["eigenvalue"]) == bits(want["eigenvalue"])
        assert (st["diameter"], st["k"]) == (want["diameter"], want["k"])
    # a default dense engine is untouched by all this: the AH reads are unsupported on it
    d = az.DenseGraphSpace(12, 0.3)
    od = az.NablaOptimizer.par_new(d, (adj, slots), az.TrivialModel(d.STATE_DIM, d.ACTION_DIM), 4)
    assert od._L.azd_engine_dense_ah_argmin_data(od._h, C.byref(_lib.DenseAhArgmin())) == 8
    assert "lambda1" in od.agent_state(0)


def test_example_driver_runs_three_epochs(tmp_path):
    """examples/ah.py: exits 0, prints one line per improvement, leaves the four cost scalars (and the losses) in its event file"""
    from azdopt_amd import sinks
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "ev"
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "ah.py"), "--epochs", "3", "--episodes", "30", "--batch", "32",
                        "--out", str(out)], cwd=tmp_path, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if "AhCost" in l]
    ev = sinks.read_events(out / "tfevents-losses")
    assert ev[0][2] == "brain.Event:2"
    tags = [t for e in ev for t, _ in e[3]]
    assert tags.count("loss") == 3 and {"cost/cost", "cost/proximity", "cost/eigenvalue", "cost/diameter"} <= set(tags)
    assert len(lines) >= 1 and tags.count("cost/cost") == len(lines) + 3  # one line and one record per improvement, one record per epoch
    assert r.stdout.count("==== EPOCH") == 3


def test_ah_pool_step_with_a_bf16_model_and_its_abort_recovery(az, monkeypatch):
    """a bf16 ActionModel on the pool step (the searchers' rows gathered into the batched GEMM launches) == one launch per phase;
    and a pool launch whose abort flag is raised (test hook) is completed by the launch-per-phase kernels with the same results"""
    n, B, seed, calls = 20, 300, 11, 60
    tol = ([50, 20, 10], 5)
    space = az.DenseGraphSpace(n, 0.2, cost="ah")
    roots = space.generate_roots(seed, B)

    def mk():
        model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(128, 128), seed=seed, dtype="bf16")
        return az.NablaOptimizer.par_new(space, roots, model, B, pool_step=True)

    monkeypatch.setenv("AZD_DENSE_NO_POOL", "1")
    ref = mk()
    imp_ref = ref.par_roll_out_episodes(tol, n_calls=calls)
    assert ref.step_form()[0].startswith("per_call")
    monkeypatch.delenv("AZD_DENSE_NO_POOL")
    pool = mk()
    imp_pool = pool.par_roll_out_episodes(tol, n_calls=calls)
    assert pool.step_form() == ("pool", ""), pool.step_form()
    monkeypatch.setenv("AZD_POOL_DEBUG_ABORT_CALL", "3")
    opt = mk()
    imp = opt.par_roll_out_episodes(tol, n_calls=calls)
    form, why = opt.step_form()
    monkeypatch.delenv("AZD_POOL_DEBUG_ABORT_CALL")
    assert form.startswith("per_call") and "aborted" in why, (form, why)
    assert imp == imp_ref == imp_pool
    for o in (pool, opt):
        c0, c1 = o.counters(), ref.counters()
        for k in C21_CTRS:
            assert c0[k] == c1[k], k
        for i in range(0, B, 3):
            assert_tree_equal(o.get_tree(i), ref.get_tree(i), f"agent {i}")
        a0, a1 = o.argmin_data(), ref.argmin_data()
        assert a0.eval == a1.eval and a0.agent == a1.agent and a0.node == a1.node and a0.cost == a1.cost
        assert np.array_equal(o.state_vecs(), ref.state_vecs())
    assert pool.counters()["EVAL_ROWS"] == pool.counters()["EXPANSIONS"] > 0
