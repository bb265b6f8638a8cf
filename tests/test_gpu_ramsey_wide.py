"""GPU parity of WIDE Ramsey engines (azd_engine_config::max_slots > 0: N <= 32, E*C <= 1024, nodes of up to max_slots * (C - 1)
actions) against the CPU oracle, bit for bit: exported trees, state vectors, live clique counts, agent state, observations,
argmin and counters -- the reference's R(4,5) shape (05-r45.rs: N 24, [4, 5], every edge may be permitted), the key width 16
instantiation (N = 32; three and four colours), and a wide engine against a narrow one on the same roots."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_parity import MAIN_CTRS, R45_W, TOL, CppRef, assert_tree_equal, az, caps, compare_ramsey, run_lockstep  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_wide_parity(az, orc, n, sizes, weights, B, kmin, kmax, steps, epochs, seed, n_obs_tol=4, check_every=10, sample=None,
                    max_slots=None, persistent=True, threads=16):
    """run_ramsey_parity of tests/test_gpu_ramsey.py for a wide engine: the argmin is read through the wide record"""
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, max_slots=max_slots)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    colors, permitted = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    co, mo = orc.gen_ramsey_roots(seed, 0, 0, B, n, len(sizes), kmin, kmax)
    assert np.array_equal(colors, co) and np.array_equal(permitted, mo)
    opt = az.NablaOptimizer.par_new(space, (colors, permitted), model, B, persistent=persistent,
                                    **caps(steps + 8, space, kmax))
    ref = CppRef(orc, n, sizes, weights, B, threads=threads)
    assert (ref.e.S, ref.e.A, ref.KW) == (space.STATE_DIM, space.ACTION_DIM, space.KEY_WORDS)
    run_lockstep(opt, ref, (colors, permitted), orc, compare_ramsey(space), seed=seed, tol=TOL, steps=steps, epochs=epochs, kmin=kmin,
                 kmax=kmax, n_obs_tol=n_obs_tol, check_every=check_every, sample=sample)
    return opt, ref.e


@pytest.mark.parametrize("persistent", [True, False])
def test_r45_shape_against_the_oracle(az, orc, persistent):
    """N 24, [4, 5], 64 agents, 10..=276 permitted edges (nodes of up to 276 actions: five chunks), two epochs with the device
    root policy between them; the CU-resident step (hash stream in the kernel) and the launch-per-phase form"""
    opt, oe = run_wide_parity(az, orc, 24, [4, 5], R45_W, B=64, kmin=10, kmax=276, steps=30, epochs=2, seed=4,
                              persistent=persistent, sample=range(0, 64, 3))
    c = opt.counters()
    assert c["FAILED"] == 0 and c["EXPANSIONS"] > 0
    assert max(oe.export_tree(i).act_end[0] - oe.export_tree(i).act_begin[0] for i in range(64)) > 128  # nodes beyond two chunks
    assert opt.step_form()[0].startswith("async" if persistent else "per_call"), opt.step_form()


@pytest.mark.parametrize("n,sizes,max_slots,kmax", [(32, [3, 3], 496, 496), (26, [3, 3, 3], 325, 325), (20, [3, 3, 3, 3], 190, 190)])
def test_key_width_16_against_the_oracle(az, orc, n, sizes, max_slots, kmax):
    """RamseyWideSpace<16>: N = 32 (992 actions), three colours at N = 26 (up to 650 actions per node: 11 chunks), four at N = 20"""
    run_wide_parity(az, orc, n, sizes, [1.0] * len(sizes), B=24, kmin=kmax // 2, kmax=kmax, steps=20, epochs=2, seed=7,
                    max_slots=max_slots, persistent=False, sample=range(0, 24, 4))


def test_wide_engine_equals_narrow_on_the_same_roots(az):
    """r44 (N 17, [4, 4]) with max_slots = 136 (RamseyWideSpace<10>) and max_slots = 0 (RamseySpace<5>) on roots of <= 64 permitted
    edges: the wide kernels change nothing but capacity"""
    n, sizes, B, seed = 17, [4, 4], 48, 9
    runs = []
    for ms in (136, 0):
        space = az.RamseySpaceNoEdgeRecolor(n, sizes, max_slots=ms)
        roots = space.generate_roots(seed, B, kmin=12, kmax=64)
        model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
        opt = az.NablaOptimizer.par_new(space, roots, model, B)
        opt.par_roll_out_episodes(TOL, n_calls=60)
        opt.par_reset_trees_policy(seed, 0, 12, 64)
        opt.par_roll_out_episodes(TOL, n_calls=30)
        runs.append(opt)
    w, nw = runs
    assert np.array_equal(w.state_vecs(), nw.state_vecs())
    assert w.counters() == nw.counters()
    for i in range(B):
        assert_tree_equal(w.get_tree(i), nw.get_tree(i), f"agent {i}")
    a, b = w.argmin_data(), nw.argmin_data()
    assert a.eval.tobytes() == b.eval.tobytes() and np.array_equal(a.state["colors"], b.state["colors"])


def test_wide_argmin_record_and_the_narrow_call(az, orc):
    """azd_engine_ramsey_wide_argmin_data equals the oracle's argmin; azd_engine_ramsey_argmin_data refuses E > 256 and names the wide call"""
    import ctypes as C
    from azdopt_amd import _lib
    opt, oe = run_wide_parity(az, orc, 24, [4, 5], R45_W, B=16, kmin=200, kmax=276, steps=12, epochs=1, seed=2, check_every=12)
    rec = _lib.RamseyWideArgmin()
    assert opt._L.azd_engine_ramsey_wide_argmin_data(opt._h, C.byref(rec)) == 0
    ao = oe.argmin()
    assert bytes(rec.colors[:276]) == ao["parents"].tobytes() and not any(rec.colors[276:])
    assert np.array_equal(np.array(rec.permitted[:5], np.uint64), ao["permitted"][:5]) and not any(rec.permitted[5:])
    assert np.float32(rec.eval).tobytes() == ao["eval"].tobytes()
    assert list(rec.totals[:2]) == oe.argmin_totals()[:2].tolist()
    narrow = _lib.RamseyArgmin()
    assert opt._L.azd_engine_ramsey_argmin_data(opt._h, C.byref(narrow)) == 1  # AZD_ERR_INVALID_ARGUMENT
    assert "azd_engine_ramsey_wide_argmin_data" in opt._L.azd_last_error().decode()


FORMS = {"per_call": dict(persistent=False), "async": dict(async_step=True, pool_step=False),
         "barrier": dict(async_step=False, pool_step=False), "pool": dict(pool_step=True)}
# what runs at r45 with the 64-64 model and 32 agents: every plan admits the wide footprint (the pool step's searchers write their
# rows straight to memory), so each form asked for is the form that runs
EXPECTED = {"per_call": "per_call", "async": "async", "barrier": "barrier", "pool": "pool"}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_r45_real_model_in_every_step_form_against_the_oracle(az, orc, form):
    """the real ActionModel (fp32, 64-64) at the r45 shape, each step form forced: the oracle is fed the GPU's predictions, trees
    must match bit for bit and the predictions the oracle's MLP on the same state vectors; the form asked for is the form that ran"""
    n, sizes, B, seed, calls = 24, [4, 5], 32, 5, 25
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, R45_W)
    dims = (space.STATE_DIM, 64, 64, space.ACTION_DIM)
    model = az.ActionModel(B, dims[0], dims[-1], hidden=dims[1:-1], seed=seed)
    om = orc.Mlp(dims, seed=seed, threads=8)
    roots = space.generate_roots(seed, B, kmin=10, kmax=276)
    opt = az.NablaOptimizer.par_new(space, roots, model, B, **FORMS[form], **caps(calls + 4, space, 276))
    oe = orc.Engine(n, B, threads=16, ramsey=(sizes, R45_W))
    oe.new_begin(*roots)
    oe.new_end(opt.predictions())
    worst = 0.0
    for _ in range(calls):
        opt.par_roll_out_episodes(TOL)
        oe.rollout_begin(*TOL)
        sv = oe.state_vecs()
        assert np.array_equal(opt.state_vecs(), sv)
        h = opt.predictions()
        fresh = [i for i in range(B) if oe.agent_state(i)["path"].any()]
        if fresh:
            worst = max(worst, float(np.max(np.abs(h[fresh] - om.forward(sv)[fresh]))))
        oe.rollout_end(h)
    ran, why = opt.step_form()
    print("r45 real model: asked", form, "ran", ran, "--", why)
    assert ran.startswith(EXPECTED[form]), (form, ran, why)
    assert worst < 2e-5, worst
    cg, co = opt.counters(), oe.counters()
    for k in MAIN_CTRS:
        assert cg[k] == co[k], (form, k)
    for i in range(0, B, 2):
        assert_tree_equal(opt.get_tree(i), oe.export_tree(i), f"{form} agent {i}")


def test_r45_driver_writes_the_reference_scalars(tmp_path):
    from azdopt_amd import sinks
    out = tmp_path / "ev"
    subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ramsey.py"), "r45", "--epochs", "2", "--episodes", "40", "--batch",
                    "32", "--hidden", "64", "--stride", "10", "--out", str(out)], cwd=tmp_path, check=True, timeout=600)
    ev = sinks.read_events(out / "tfevents-losses")
    tags = [t for e in ev for t, _ in e[3]]
    assert tags.count("loss") == 2 and {"clique_counts/0", "clique_counts/1"} <= set(tags)


def test_wide_r44_pool_step_every_edge_permitted_against_the_oracle(az, orc):
    """k_pool<RamseyWideSpace<10>> -- the default form of a wide engine from 256 agents: r44 with every edge of a root permitted
    (max_slots = 136, beyond the narrow engine's 64), the real model, 120 calls in one launch against the oracle fed -- call by call --
    with the rows the in-kernel evaluator computes for its states (debug_tile_forward)"""
    n, sizes, weights, B, seed, calls = 17, [4, 4], [1.0, 1.0], 256, 31, 120
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, max_slots=136)
    roots = space.generate_roots(seed, B, kmin=100, kmax=136)
    model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(128, 128), seed=seed)
    opt = az.NablaOptimizer.par_new(space, roots, model, B, pool_step=True, **caps(calls + 4, space, 136))
    oe = orc.Engine(n, B, threads=16, ramsey=(sizes, weights))
    oe.new_begin(*roots)
    oe.new_end(opt.predictions())
    io = 0
    for _ in range(calls):
        oe.rollout_begin(*TOL)
        io += oe.rollout_end(opt.debug_tile_forward(oe.state_vecs()))
    ig = opt.par_roll_out_episodes(TOL, n_calls=calls)
    assert opt.step_form() == ("pool", "") and ig == io
    cg, co = opt.counters(), oe.counters()
    for k in MAIN_CTRS:
        assert cg[k] == co[k], (k, cg[k], co[k])
    assert cg["FAILED"] == 0
    assert np.array_equal(opt.state_vecs(), oe.state_vecs())
    for i in range(0, B, 3):
        assert_tree_equal(opt.get_tree(i), oe.export_tree(i), f"agent {i}")
    ag, ao = opt.argmin_data(), oe.argmin()
    assert ag.eval.tobytes() == ao["eval"].tobytes() and np.array_equal(ag.state["colors"], ao["parents"])


def test_wide_r44_run_ahead_window_hands_out_the_calls_of_separate_launches(az):
    """the run-ahead window on a wide engine (its argmin side record is the wide one): n calls in one pool launch, asked for one at a
    time, give each call's improvement and argmin record as n launches of one call do"""
    n, sizes, B, seed, calls = 17, [4, 4], 256, 8, 60
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, max_slots=136)
    roots = space.generate_roots(seed, B, kmin=12, kmax=136)
    mk = lambda: az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(128, 128), seed=seed)
    rec = lambda a: (a.eval.tobytes(), a.agent, a.node, a.state["colors"].tobytes(), a.state["permitted"].tobytes())
    ref = az.NablaOptimizer.par_new(space, roots, mk(), B, pool_step=True, **caps(calls + 4, space, 136))
    want, want_rec = [], []
    for _ in range(calls):
        want.append(ref.par_roll_out_episodes(TOL, n_calls=1))
        if want[-1]:
            want_rec.append(rec(ref.argmin_data()))
    assert ref.step_form() == ("pool", "") and sum(want) > 0
    opt = az.NablaOptimizer.par_new(space, roots, mk(), B, pool_step=True, **caps(calls + 4, space, 136))
    assert opt.run_ahead(TOL, calls)
    got, got_rec = [], []
    for _ in range(calls):
        got.append(opt.par_roll_out_episodes(TOL, n_calls=1))
        if got[-1]:
            got_rec.append(rec(opt.argmin_data()))
    assert got == want and got_rec == want_rec
    cg, cr = opt.counters(), ref.counters()  # (the evaluator's batch / tick counters depend on how the calls were launched)
    for k in MAIN_CTRS:
        assert cg[k] == cr[k], k
    assert np.array_equal(opt.state_vecs(), ref.state_vecs())
    for i in range(0, B, 5):
        assert_tree_equal(opt.get_tree(i), ref.get_tree(i), f"agent {i}")


def test_r45_bf16_reference_model_runs_the_pool_step_against_the_oracle(az, orc):
    """05-r45.rs's own model (1380-512-1024-512-552) in bf16 storage at r45: the pool plan admits it now that the searchers write
    their rows straight to memory; a launch of calls against the oracle fed with the in-kernel evaluator's rows"""
    n, sizes, B, seed, calls = 24, [4, 5], 256, 12, 12
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, R45_W)
    roots = space.generate_roots(seed, B, kmin=10, kmax=276)
    model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(512, 1024, 512), seed=seed, dtype="bf16")
    opt = az.NablaOptimizer.par_new(space, roots, model, B, pool_step=True, **caps(calls + 4, space, 276))
    oe = orc.Engine(n, B, threads=16, ramsey=(sizes, R45_W))
    oe.new_begin(*roots)
    oe.new_end(opt.predictions())
    io = 0
    for _ in range(calls):
        oe.rollout_begin(*TOL)
        io += oe.rollout_end(opt.debug_tile_forward(oe.state_vecs()))
    ig = opt.par_roll_out_episodes(TOL, n_calls=calls)
    assert opt.step_form() == ("pool", "") and ig == io
    cg, co = opt.counters(), oe.counters()
    for k in MAIN_CTRS:
        assert cg[k] == co[k], (k, cg[k], co[k])
    assert np.array_equal(opt.state_vecs(), oe.state_vecs())
    for i in range(0, B, 8):
        assert_tree_equal(opt.get_tree(i), oe.export_tree(i), f"agent {i}")
