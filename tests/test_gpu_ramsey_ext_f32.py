"""GPU tests of the searcher-only pool step of the Ramsey tiers with an fp32 model (AZD_ENGINE_EXT_POOL_STEP beside
AZD_ENGINE_EXT_POOL_F32; par_new(..., ext_pool_step=True, ext_pool_f32=True)): the searchers of the bf16 form -- they write the f32
row whatever the model -- and an evaluator graph of take -> gathered fp32 GEMMs over those rows -> deliver.  A search is chaotic in
its predictions, so equal prediction BITS are the condition: against a persistent=False run of the same engine, trees, state rows,
prediction bits, argmin, counters and the training loss are equal.  Both tiers, both node widths' worth of rows, the odd pitch of
r3333 (5049), the reference's 512-1024-512 model, and a single searcher workgroup (batches of one to a few rows).  Two companions
guard the boundary: both flags with a bf16 model are the first flag alone, and the first flag alone with an fp32 model still falls
back with its bf16 reason."""
import numpy as np
import pytest

from gpu_parity import R3333, R45_W, TOL, assert_same_run, az  # noqa: F401
from test_gpu_ramsey_ext_pool import SMALL, run_model

pytestmark = pytest.mark.gpu

F32 = dict(ext_pool_step=True, ext_pool_f32=True)


def shape_space(az, shape, u64):
    n, sizes, w = R3333 if shape == "r3333" else (24, [4, 5], R45_W)
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, w, **(dict(u64=True) if u64 else {}))
    assert space.tier == ("u64" if (u64 or shape == "r3333") else "wide")
    return space, (30 if shape == "r3333" else 276)


def compare_with_the_launch_per_phase_form(az, space, kmax, hidden, B, calls, seed=7):
    roots = space.generate_roots(seed, B, kmin=10, kmax=kmax)
    runs = []
    for kw in (F32, dict(persistent=False)):
        o, imp = run_model(az, space, roots, B, calls, kmax, seed, hidden, False, "f32", **kw)
        form = o.step_form()
        assert (form == ("pool", "")) if kw is F32 else form[0].startswith("per_call"), form
        runs.append((o, imp))
    (o0, i0), (o1, i1) = runs
    assert i0 == i1
    assert_same_run(o0, o1, B, "first epoch")
    c0 = o0.counters()
    assert c0["EVAL_ROWS"] == c0["EXPANSIONS"] and c0["FAILED"] == 0 and c0["EXPANSIONS"] > 0
    l0, l1 = o0.par_update_model(1), o1.par_update_model(1)
    assert l0 == l1 and np.isfinite(l0), (l0, l1)
    for o in (o0, o1):
        o.par_reset_trees_policy(seed, 0, 10, kmax)
    assert o0.par_roll_out_episodes(TOL, n_calls=10) == o1.par_roll_out_episodes(TOL, n_calls=10)
    assert o0.step_form() == ("pool", "")
    assert_same_run(o0, o1, B, "after the reset")
    return o0


@pytest.mark.parametrize("shape,u64,hidden,B,calls", [("r45", False, SMALL, 96, 20), ("r45", True, SMALL, 96, 20), ("r3333", False, SMALL, 96, 20),
                                                       ("r45", False, (512, 1024, 512), 64, 12)],
                         ids=["r45 wide", "r45 u64", "r3333", "r45 wide 512-1024-512"])
def test_ext_pool_step_with_an_fp32_model_equals_the_launch_per_phase_form(az, shape, u64, hidden, B, calls):
    space, kmax = shape_space(az, shape, u64)
    o = compare_with_the_launch_per_phase_form(az, space, kmax, hidden, B, calls)
    ev_wgs, search_wgs = o.pool_split()
    assert ev_wgs == 0 and search_wgs >= 1, (ev_wgs, search_wgs)


def test_one_searcher_workgroup_serves_twelve_agents(az, monkeypatch):
    """AZD_RAMSEY_EXT_POOL_SEARCH_WGS=1: eight waves for twelve agents, so the evaluator's batches are one to a few rows"""
    monkeypatch.setenv("AZD_RAMSEY_EXT_POOL_SEARCH_WGS", "1")
    space, kmax = shape_space(az, "r45", False)
    o = compare_with_the_launch_per_phase_form(az, space, kmax, SMALL, 12, 20)
    assert o.pool_split() == (0, 1)


def test_both_flags_with_a_bf16_model_are_the_first_flag_alone(az):
    space, kmax = shape_space(az, "r45", False)
    B, calls, seed = 96, 20, 7
    roots = space.generate_roots(seed, B, kmin=10, kmax=kmax)
    o0, i0 = run_model(az, space, roots, B, calls, kmax, seed, SMALL, False, "bf16", **F32)
    o1, i1 = run_model(az, space, roots, B, calls, kmax, seed, SMALL, False, "bf16", ext_pool_step=True)
    assert o0.step_form() == ("pool", "") and o1.step_form() == ("pool", "")
    assert i0 == i1
    assert_same_run(o0, o1, B, "bf16 under both flags")


def test_the_first_flag_alone_with_an_fp32_model_still_falls_back(az):
    """(r3333: the 64-bit tier has no other CU-resident form, so what runs without the form is one launch per phase)"""
    space, kmax = shape_space(az, "r3333", False)
    B, calls, seed = 32, 8, 2
    roots = space.generate_roots(seed, B, kmin=10, kmax=kmax)
    o, _ = run_model(az, space, roots, B, calls, kmax, seed, SMALL, False, "f32", ext_pool_step=True)
    form, why = o.step_form()
    assert form.startswith("per_call"), (form, why)
    assert why.startswith("external pool step") and "bf16" in why, why
