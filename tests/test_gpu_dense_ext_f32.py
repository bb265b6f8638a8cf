"""GPU tests of the dense-graph space's pool step with an fp32 model (AZD_ENGINE_EXT_POOL_F32 alone on AZD_SPACE_DENSE;
par_new(..., pool_step=True, ext_pool_f32=True)): the searchers of the bf16 form -- they write the f32 row whatever the model -- and
an evaluator graph of take -> gathered fp32 GEMMs over Arenas::state_vecs -> deliver, on all three tiers (default cost, the
Aouchiche-Hansen cost, its 64-row form).  A search is chaotic in its predictions, so equal prediction BITS are the condition: against
a persistent=False run of the same engine, trees, state rows, prediction bits, argmin, counters and the training loss are equal.

The launch-per-phase form with a real fp32 model is itself held to the references elsewhere (test_ah_n31_with_the_fp32_model in
tests/test_gpu_dense_ah.py feeds tests/dense_ah_ref.py the GPU's rows and grows the same trees; tests/test_gpu_dense.py runs that
form against the C++ oracle), so equality with it ties the new form to the oracle through one link.

The shapes are the smallest at which each path can go wrong: S = 85 and a head of 56 columns (one-float loads, less than a column
tile), key widths 2 and 10, S = 3676 (16-byte loads, config E's model on the drivers' roots), the AH tier's 10 / 9 / 7 waves per
workgroup with the example's model 1396-256-128-930, the wide tier's 6 waves at an odd pitch (S = 1585) and at N = 50, and one searcher
workgroup whose batches are one to a few rows.  Two companions guard the boundary: the flag with a bf16 model is an engine without
the flag, and an fp32 model without the flag still falls back with the reason it always gave."""
import numpy as np
import pytest

from gpu_parity import TOL_REF, assert_same_run, az  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = dict(pool_step=True, ext_pool_f32=True)
NEEDS_BF16 = "dense-graph space: the pool step needs an evaluator that serves gathered bf16 rows (ActionModel with bf16 storage)"


def run_model(az, space, roots, B, calls, kmax, seed, hidden, dtype, **kw):
    model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=hidden, seed=seed, dtype=dtype)
    o = az.NablaOptimizer.par_new(space, roots, model, B, **kw, **az.tree_capacities(calls + 12, kmax))
    imp = o.par_roll_out_episodes(TOL_REF, n_calls=calls)
    return o, imp


def compare_with_the_launch_per_phase_form(az, space, hidden, B, calls, seed=7):
    kmin, kmax = space.default_permitted_range()
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    runs = []
    for kw in (F32, dict(persistent=False)):
        o, imp = run_model(az, space, roots, B, calls, kmax, seed, hidden, "f32", **kw)
        form = o.step_form()
        assert (form == ("pool", "")) if kw is F32 else form[0].startswith("per_call"), form
        runs.append((o, imp))
    (o0, i0), (o1, i1) = runs
    assert i0 == i1
    assert_same_run(o0, o1, B, "first epoch")
    c0 = o0.counters()
    assert c0["EVAL_ROWS"] == c0["EXPANSIONS"] > 0 and c0["FAILED"] == 0, (c0["EVAL_ROWS"], c0["EXPANSIONS"], c0["FAILED"])
    l0, l1 = o0.par_update_model(1), o1.par_update_model(1)
    assert l0 == l1 and np.isfinite(l0), (l0, l1)
    for o in (o0, o1):
        o.par_reset_trees_policy(seed, 0, kmin, kmax)
    assert o0.par_roll_out_episodes(TOL_REF, n_calls=10) == o1.par_roll_out_episodes(TOL_REF, n_calls=10)
    assert o0.step_form() == ("pool", "")
    assert_same_run(o0, o1, B, "after the reset")
    return o0


def check_split(o):
    ev_wgs, search_wgs = o.pool_split()
    assert ev_wgs == 0 and search_wgs >= 1, (ev_wgs, search_wgs)


@pytest.mark.parametrize("n,max_slots,hidden,B,calls", [(8, 28, (64, 32), 96, 20), (20, 128, (256, 128), 96, 20), (50, 612, (512, 512, 512), 64, 12)],
                         ids=["a: n8 S85", "b: n20 S571", "c: n50 S3676 512-512-512"])
def test_default_cost_with_an_fp32_model_equals_the_launch_per_phase_form(az, n, max_slots, hidden, B, calls):
    space = az.DenseGraphSpace(n, 0.1 if n == 50 else 0.2, max_slots=max_slots)
    check_split(compare_with_the_launch_per_phase_form(az, space, hidden, B, calls))


@pytest.mark.parametrize("max_slots", [128, 256, 465], ids=["d: 10 waves", "d: 9 waves", "d: 7 waves"])
def test_ah_n31_with_the_examples_fp32_model_equals_the_launch_per_phase_form(az, max_slots):
    space = az.DenseGraphSpace(31, 0.4, max_slots=max_slots, cost="ah")
    assert (space.STATE_DIM, space.ACTION_DIM) == (1396, 930)
    check_split(compare_with_the_launch_per_phase_form(az, space, (256, 128), 96, 20))


@pytest.mark.parametrize("n", [33, 50], ids=["e: n33 S1585", "e: n50"])
def test_ah_wide_with_an_fp32_model_equals_the_launch_per_phase_form(az, n):
    space = az.DenseGraphSpace(n, 0.2, max_slots=128, cost="ah", ah_wide=True)
    check_split(compare_with_the_launch_per_phase_form(az, space, (256, 128), 64, 12))


def test_one_searcher_workgroup_serves_twenty_four_agents(az, monkeypatch):
    """f: AZD_DENSE_POOL_SEARCH_WGS=1: sixteen waves for twenty-four agents, so the evaluator's batches are one to a few rows"""
    monkeypatch.setenv("AZD_DENSE_POOL_SEARCH_WGS", "1")
    space = az.DenseGraphSpace(20, 0.2, max_slots=128)
    o = compare_with_the_launch_per_phase_form(az, space, (256, 128), 24, 20)
    assert o.pool_split() == (0, 1)


def test_the_flag_with_a_bf16_model_is_an_engine_without_the_flag(az):
    space = az.DenseGraphSpace(20, 0.2, max_slots=128)
    B, calls, seed = 96, 20, 7
    kmin, kmax = space.default_permitted_range()
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    o0, i0 = run_model(az, space, roots, B, calls, kmax, seed, (256, 128), "bf16", **F32)
    o1, i1 = run_model(az, space, roots, B, calls, kmax, seed, (256, 128), "bf16", pool_step=True)
    assert o0.step_form() == ("pool", "") and o1.step_form() == ("pool", "")
    assert i0 == i1
    assert_same_run(o0, o1, B, "bf16 under the flag")
    assert o0.pool_split() == o1.pool_split()


def test_an_fp32_model_without_the_flag_still_falls_back_with_its_reason(az):
    space = az.DenseGraphSpace(20, 0.2, max_slots=128)
    B, calls, seed = 32, 8, 2
    kmin, kmax = space.default_permitted_range()
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    o, _ = run_model(az, space, roots, B, calls, kmax, seed, (256, 128), "f32", pool_step=True)
    form, why = o.step_form()
    assert form.startswith("per_call") and why == NEEDS_BF16, (form, why)
