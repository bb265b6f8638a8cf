"""GPU tests of the searcher-only pool step of the Ramsey tiers with max_slots > 0 (AZD_ENGINE_EXT_POOL_STEP; par_new(...,
ext_pool_step=True)): persistent searcher workgroups of eight waves (k_pool_search over RamseyExtSpace), the evaluator a replayed
graph of take -> gathered bf16 GEMMs -> deliver beside them.  Its results are those of the launch-per-phase form bit for bit:
  * with the hash stream against the C++ oracle (r45 on both tiers) and against tests/ramsey64_ref.py (past 32 vertices: N = 33 with
    one searcher workgroup for twelve agents, and the reference's R(3,3,3,3) shape), what tests/test_gpu_ramsey64.py's run_parity
    compares, with the form reported as "pool";
  * with real bf16 models against a persistent=False run of the same engine: trees, rows, prediction bits, argmin, training loss;
  * the fallback with a reason (fp32 storage) and the completion of an aborted launch by the launch-per-phase kernels."""
import numpy as np
import pytest

import mlp_f64 as M
from gpu_parity import (R3333, R3333_DIMS, R45_W, TOL, CppRef, PyRef, assert_same_run, assert_tree_equal, az, caps,  # noqa: F401
                        compare_ramsey, run_lockstep)

pytestmark = pytest.mark.gpu


def run_ext_parity(az, orc, ref, n, sizes, weights, u64, B, kmin, kmax, steps, epochs, seed, n_obs_tol=4, check_every=10, sample=None):
    """run_parity of tests/test_gpu_ramsey64.py with the flag set, on either tier, and the form asserted to be the pool step"""
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, u64=u64)
    assert space.tier == ("u64" if u64 else "wide")
    # (the stream served like a model's rows: posted by the searchers, written by k_ext_hash_rows in the evaluator's graph)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed).serve_from_pool_evaluators()
    colors, permitted = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    co, mo = orc.gen_ramsey_roots(seed, 0, 0, B, n, len(sizes), kmin, kmax)
    assert np.array_equal(colors, co) and np.array_equal(permitted, mo)
    opt = az.NablaOptimizer.par_new(space, (colors, permitted), model, B, ext_pool_step=True, **caps(steps + 8, space, kmax))
    assert ref.KW == space.KEY_WORDS
    opt.taken = set()  # action ids on the agents' paths at the compared moments
    run_lockstep(opt, ref, (colors, permitted), orc, compare_ramsey(space, taken=opt.taken, argmin_any=u64), seed=seed, tol=TOL,
                 steps=steps, epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=n_obs_tol, check_every=check_every, sample=sample,
                 form="pool")
    ev_wgs, search_wgs = opt.pool_split()
    assert ev_wgs == 0 and search_wgs >= 1, (ev_wgs, search_wgs)  # searchers only, as for a dense engine
    return opt, ref


@pytest.mark.parametrize("u64", [False, True], ids=["wide", "u64"])
def test_r45_against_the_cpp_oracle(az, orc, u64):
    """N 24, [4, 5], 48 agents, 10..=276 permitted edges, two epochs of 30 calls with the device root policy between them, on the
    32-bit wide tier (RamseyExtSpace<RamseyWideSpace<10>>) and under AZD_ENGINE_RAMSEY_U64 (RamseyExtSpace<RamseyU64Space>)"""
    opt, ref = run_ext_parity(az, orc, CppRef(orc, 24, [4, 5], R45_W, 48), 24, [4, 5], R45_W, u64, B=48, kmin=10, kmax=276, steps=30,
                              epochs=2, seed=4, sample=range(0, 48, 3))
    assert max(ref.tree(i).act_end[0] - ref.tree(i).act_begin[0] for i in range(48)) > 128  # nodes beyond two chunks


def test_n33_first_shape_past_the_32_bit_word_on_one_workgroup(az, orc, monkeypatch):
    """N = 33, [3, 4], up to 264 permitted edges, one searcher workgroup: twelve agents share its eight waves, and vertex 32 (edge
    positions 496..527) takes part in recoloured edges as in the launch-per-phase test of the same seed"""
    monkeypatch.setenv("AZD_RAMSEY_EXT_POOL_SEARCH_WGS", "1")
    opt, ref = run_ext_parity(az, orc, PyRef(33, [3, 4], [1.0, 1.0], 12), 33, [3, 4], [1.0, 1.0], True, B=12, kmin=100, kmax=264, steps=20,
                              epochs=2, seed=5)
    assert opt.pool_split() == (0, 1)
    E = 33 * 32 // 2
    hit = sum(1 for a in opt.taken if a % E >= 496)
    print("N = 33: %d of %d recoloured edges on the compared paths are at vertex 32" % (hit, len(opt.taken)))
    assert hit >= 4


def test_r3333_shape_against_the_reference(az, orc):
    """03-r3333.rs's shape: N 34, [3,3,3,3], permitted 10..=30, 16 agents, two epochs of 20 calls"""
    n, sizes, w = R3333
    run_ext_parity(az, orc, PyRef(n, sizes, w, 16), n, sizes, w, True, B=16, kmin=10, kmax=30, steps=20, epochs=2, seed=3)


def run_model(az, space, roots, B, calls, kmax, seed, hidden, relu, dtype, **kw):
    model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=hidden, seed=seed, dtype=dtype,
                           **(dict(final_act=M.ACT_RELU, lr=3e-4, l2=1e-6) if relu else {}))
    o = az.NablaOptimizer.par_new(space, roots, model, B, **kw, **caps(calls + 12, space, kmax))
    imp = o.par_roll_out_episodes(TOL, n_calls=calls)
    return o, imp


SMALL, REFERENCE = (64, 64), R3333_DIMS[1:-1]


@pytest.mark.parametrize("shape,hidden,B,calls", [("r3333", SMALL, 96, 20), ("r3333", REFERENCE, 64, 12), ("r45", SMALL, 96, 20),
                                                   ("r45", (512, 1024, 512), 64, 12)])
def test_ext_pool_step_with_a_bf16_model_equals_the_launch_per_phase_form(az, shape, hidden, B, calls):
    """real bf16 models -- a small one and the reference's 512-1024-512 (ReLU head at r3333: 5049-512-1024-512-2244) -- once with the
    flag and once with persistent=False.  A search is chaotic in its predictions, so equal prediction BITS are the condition: the
    gathered GEMM gives every row the sums the whole-batch GEMM gives it, and the bf16 rows the searchers write are the evaluator's
    own rounding of the f32 rows."""
    seed = 7
    n, sizes, w = R3333 if shape == "r3333" else (24, [4, 5], R45_W)
    kmax = 30 if shape == "r3333" else 276
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, w)
    assert space.tier == ("u64" if shape == "r3333" else "wide")
    roots = space.generate_roots(seed, B, kmin=10, kmax=kmax)
    relu = shape == "r3333" and hidden is REFERENCE
    runs = []
    for kw in (dict(ext_pool_step=True), dict(persistent=False)):
        o, imp = run_model(az, space, roots, B, calls, kmax, seed, hidden, relu, "bf16", **kw)
        form = o.step_form()
        assert (form == ("pool", "")) if "ext_pool_step" in kw else form[0].startswith("per_call"), form
        runs.append((o, imp))
    (o0, i0), (o1, i1) = runs
    assert i0 == i1
    assert_same_run(o0, o1, B, "first epoch")
    c0 = o0.counters()
    assert c0["EVAL_ROWS"] == c0["EXPANSIONS"] and c0["FAILED"] == 0 and c0["EXPANSIONS"] > 0
    # (every action taken once counts: after a dozen calls over nodes of 276 actions none has been taken four times, and a training
    # step without a weighted entry has no loss)
    l0, l1 = o0.par_update_model(1), o1.par_update_model(1)
    assert l0 == l1 and np.isfinite(l0), (l0, l1)
    for o in (o0, o1):
        o.par_reset_trees_policy(seed, 0, 10, kmax)
    assert o0.par_roll_out_episodes(TOL, n_calls=10) == o1.par_roll_out_episodes(TOL, n_calls=10)
    assert o0.step_form() == ("pool", "")
    assert_same_run(o0, o1, B, "after the reset")


def test_fp32_model_falls_back_with_a_reason(az):
    """the flag with fp32 weight storage at r3333: the engine runs what it runs without the flag (one launch per phase on the 64-bit
    tier) and the reason opens with the form's name and names the bf16 requirement"""
    n, sizes, w = R3333
    B, seed, calls = 32, 2, 12
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, w)
    roots = space.generate_roots(seed, B, kmin=10, kmax=30)
    o0, i0 = run_model(az, space, roots, B, calls, 30, seed, SMALL, False, "f32", ext_pool_step=True)
    o1, i1 = run_model(az, space, roots, B, calls, 30, seed, SMALL, False, "f32")
    form, why = o0.step_form()
    print("fp32 under the flag:", form, "--", why)
    assert form.startswith("per_call") and form == o1.step_form()[0], (form, o1.step_form())
    assert why.startswith("external pool step") and "bf16" in why, why
    assert i0 == i1
    assert_same_run(o0, o1, B, "fp32")


def test_an_aborted_launch_is_completed_by_the_launch_per_phase_kernels(az, monkeypatch):
    """the pool's own abort flag, raised by the test hook behind the third batch the evaluator hands back (an orderly early exit of
    the searchers): the call succeeds, the launch-per-phase kernels complete it agent by agent from where each one stands -- with
    f32 rows only: the bf16 rows of the form are not theirs -- and the results are those of an undisturbed persistent=False run"""
    B, seed, calls = 64, 11, 40
    space = az.RamseySpaceNoEdgeRecolor(24, [4, 5], R45_W, u64=True)
    roots = space.generate_roots(seed, B, kmin=10, kmax=276)
    ref, imp_ref = run_model(az, space, roots, B, calls, 276, seed, SMALL, False, "bf16", persistent=False)
    monkeypatch.setenv("AZD_POOL_DEBUG_ABORT_CALL", "3")
    opt, imp = run_model(az, space, roots, B, calls, 276, seed, SMALL, False, "bf16", ext_pool_step=True)
    monkeypatch.delenv("AZD_POOL_DEBUG_ABORT_CALL")
    form, why = opt.step_form()
    assert form.startswith("per_call") and "aborted" in why, (form, why)
    assert imp == imp_ref
    assert_same_run(opt, ref, B, "completed")
    # usable afterwards, on the launch-per-phase form
    assert opt.par_roll_out_episodes(TOL, n_calls=5) == ref.par_roll_out_episodes(TOL, n_calls=5)
    assert opt.step_form()[0].startswith("per_call") and "aborted" in opt.step_form()[1]
    for i in range(0, B, 7):
        assert_tree_equal(opt.get_tree(i), ref.get_tree(i), f"agent {i} afterwards")
