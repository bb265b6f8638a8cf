"""GPU tests of clique sizes 6..8 on the 64-bit Ramsey tier (AZD_ENGINE_RAMSEY_BIG_CLIQUES beside AZD_ENGINE_RAMSEY_U64:
RamseyU64BigSpace, count_cliques_inside as fixed-depth nests down to depth 6), bit for bit through the C ABI:
  1. the closed form on monochromatic roots (every per-edge count C(n-2, s-2), total C(n, s)), vertices beyond bit 31 included;
  2. the launch-per-phase form with the hash stream against the C++ oracle and tests/ramsey64_ref.py (pinned on the CPU by
     tests/test_ramsey_big_cliques_reference.py), what tests/test_gpu_ramsey64.py's run_parity compares, over an epoch boundary
     through the device root policy;
  3. the searcher-only pool step: the hash stream against the C++ oracle, and real bf16 / fp32 models against a persistent=False
     run of the same engine, as tests/test_gpu_ramsey_ext_pool.py and tests/test_gpu_ramsey_ext_f32.py compare their tiers;
  4. the deep kernels against the shallow ones at r45;
  5. the r46 driver.
The roots of 2 and 3 are coloured with the big colour at probability p and held to tests/ramsey_big_cases.py's cap on the
reference's values first: on uniformly coloured roots of these sizes there is no K6 to count."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ramsey64_ref as R
import ramsey_big_cases as K
from gpu_parity import (MAIN_CTRS, R45_W, TOL, CppRef, PyRef, assert_same_run, assert_tree_equal, az, caps, compare_ramsey,  # noqa: F401
                        run_lockstep, same_array)
from test_gpu_ramsey_ext_pool import SMALL, run_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMIN, KMAX = 10, 30


def big_space(az, n, sizes, weights=None):
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights)
    assert space.tier == "u64" and space.BIG_CLIQUES
    return space


@pytest.mark.parametrize("n,sizes", [(12, [3, 6]), (14, [4, 7]), (13, [8, 3]), (34, [3, 6])])
def test_closed_form_on_monochromatic_roots(az, n, sizes):
    """every edge in the big colour: per-edge counts C(n-2, s-2), total C(n, s); the other colours count nothing.  At n = 34 the
    common neighbourhoods have vertices beyond bit 31"""
    space = big_space(az, n, sizes)
    big, B = K.big_colour(sizes), 4
    per_edge, total = K.closed_form(n, sizes[big])
    colors = np.full((B, space.E), big, np.uint8)
    permitted = K.pack_permitted([{0, 1, 2}] * B, space.KEY_WORDS)
    opt = az.NablaOptimizer.par_new(space, (colors, permitted), az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, 0), B,
                                    **caps(8, space, 3))
    want = np.zeros((space.C, space.E), np.int64)
    want[big] = per_edge
    for i in range(B):
        counts, totals = opt.ramsey_agent_counts(i)
        assert np.array_equal(np.asarray(counts).reshape(space.C, space.E), want), i
        assert list(totals[:space.C]) == [total if c == big else 0 for c in range(space.C)], (i, totals)
    assert opt.argmin_data().cost["clique_counts"] == [total if c == big else 0 for c in range(space.C)]


class RootView:
    """one root as a reference has it, for ramsey_big_cases.assert_not_vacuous: counts[c][e], and the totals by RamseyCounts::new's
    rule from those counts (the sum over the colour's own edges, divided by C(s,2))"""

    def __init__(self, sizes, colors, counts):
        C = len(sizes)
        self.counts = np.asarray(counts).reshape(C, -1)
        self.totals = [int(self.counts[c][np.asarray(colors) == c].sum()) // (sizes[c] * (sizes[c] - 1) // 2) for c in range(C)]


def run_big_parity(az, orc, make_ref, case, B, steps, seed=1, ext=False, sample=None, check_every=10, after=10, n_obs_tol=4):
    """run_parity of tests/test_gpu_ramsey64.py (run_ext_parity of tests/test_gpu_ramsey_ext_pool.py with ext=True) on roots dense
    in the big colour: `steps` calls, the epoch boundary through the device root policy, `after` calls more"""
    n, sizes, p = K.CASES[case]
    weights = [1.0] * len(sizes)
    space = big_space(az, n, sizes, weights)
    ref = make_ref(n, sizes, weights, B)
    assert ref.KW == space.KEY_WORDS
    colors, perm_sets = K.roots(n, sizes, p, B, seed, KMIN, KMAX)
    permitted = K.pack_permitted(perm_sets, space.KEY_WORDS)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    if ext:
        model = model.serve_from_pool_evaluators()
    opt = az.NablaOptimizer.par_new(space, (colors, permitted), model, B, **(dict(ext_pool_step=True) if ext else {}),
                                    **caps(steps + after + 8, space, KMAX))

    def compare(opt, ref, agents, tag, ramsey=compare_ramsey(space, argmin_any=True)):
        if tag == "par_new":  # the roots as the reference counts them, before anything rests on them
            lo, hi, share = K.assert_not_vacuous(sizes, [RootView(sizes, colors[i], ref.counts(i)) for i in range(B)], case)
            print("%s: big colour's totals %d..%d over %d roots, %.2f of its per-edge counts nonzero (reference)" % (case, lo, hi, B, share))
        ramsey(opt, ref, agents, tag)

    run_lockstep(opt, ref, (colors, permitted), orc, compare, seed=seed, tol=TOL, steps=[steps, after], kmin=KMIN, kmax=KMAX,
                 n_obs_tol=n_obs_tol, check_every=check_every, sample=sample, last_boundary=False, form="pool" if ext else "per_call")
    if ext:
        ev_wgs, search_wgs = opt.pool_split()
        assert ev_wgs == 0 and search_wgs >= 1, (ev_wgs, search_wgs)
    return opt, ref


_ROOTS = {}


def dense_roots(case, B, seed):
    """the case's roots, held to the cap on tests/ramsey64_ref.py's values (once per case: the model tests share them)"""
    if (case, B, seed) not in _ROOTS:
        n, sizes, p = K.CASES[case]
        colors, perm_sets = K.roots(n, sizes, p, B, seed, KMIN, KMAX)
        K.assert_not_vacuous(sizes, [R.IncRamseyState(n, sizes, colors[i].tolist(), perm_sets[i]) for i in range(B)], case)
        _ROOTS[(case, B, seed)] = (colors, perm_sets)
    return _ROOTS[(case, B, seed)]


def cpp_ref(orc):
    return lambda n, sizes, weights, B: CppRef(orc, n, sizes, weights, B)


@pytest.mark.parametrize("case", ["n12_36", "n14_47", "n13_83", "n16_336"])
def test_launch_per_phase_form_against_the_cpp_oracle(az, orc, case):
    """K6 at n = 12, K7 beside K4 at n = 14, K8 in colour 0 at n = 13, K6 as the third colour at n = 16: depths 3..6 of the root
    count, 2..5 and 1..4 of the two adjustments"""
    run_big_parity(az, orc, cpp_ref(orc), case, B=16, steps=20)


def test_launch_per_phase_form_against_the_python_reference_at_n12(az, orc):
    run_big_parity(az, orc, PyRef, "n12_36", B=16, steps=20)


def test_launch_per_phase_form_past_32_vertices(az, orc):
    """n = 34, [3, 6], 8 agents: K6 over 64-bit rows whose common neighbourhoods reach past bit 31 (totals above 10 000)"""
    run_big_parity(az, orc, PyRef, "n34_36", B=8, steps=20, after=5)


def test_pool_step_with_the_hash_stream_against_the_cpp_oracle(az, orc):
    """k_pool_search<RamseyExtSpace<RamseyU64BigSpace>> with the stream served like a model's rows"""
    run_big_parity(az, orc, cpp_ref(orc), "n16_336", B=16, steps=20, ext=True)


@pytest.mark.parametrize("case", ["n16_336", "n34_36"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_pool_step_with_a_model_equals_the_launch_per_phase_form(az, case, dtype):
    """real models, bf16 under AZD_ENGINE_EXT_POOL_STEP and fp32 with AZD_ENGINE_EXT_POOL_F32 beside it, once in the form and once
    with persistent=False: trees, rows, prediction BITS, argmin, counters and the training loss are equal, and the form ran"""
    n, sizes, p = K.CASES[case]
    B, calls, seed = (8 if n > 32 else 16), 20, 1
    space = big_space(az, n, sizes)
    colors, perm_sets = dense_roots(case, B, seed)
    roots = (colors, K.pack_permitted(perm_sets, space.KEY_WORDS))
    form_kw = dict(ext_pool_step=True) if dtype == "bf16" else dict(ext_pool_step=True, ext_pool_f32=True)
    runs = []
    for kw in (form_kw, dict(persistent=False)):
        o, imp = run_model(az, space, roots, B, calls, KMAX, seed, SMALL, False, dtype, **kw)
        form = o.step_form()
        assert (form == ("pool", "")) if kw is form_kw else form[0].startswith("per_call"), form
        runs.append((o, imp))
    (o0, i0), (o1, i1) = runs
    assert i0 == i1
    assert_same_run(o0, o1, B, "first epoch")
    for i in range(B):
        assert np.array_equal(o0.ramsey_agent_counts(i)[0], o1.ramsey_agent_counts(i)[0]), i
    c0 = o0.counters()
    assert c0["EVAL_ROWS"] == c0["EXPANSIONS"] and c0["FAILED"] == 0 and c0["EXPANSIONS"] > 0
    l0, l1 = o0.par_update_model(1), o1.par_update_model(1)
    assert l0 == l1 and np.isfinite(l0), (l0, l1)
    for o in (o0, o1):
        o.par_reset_trees_policy(seed, 0, KMIN, KMAX)
    assert o0.par_roll_out_episodes(TOL, n_calls=10) == o1.par_roll_out_episodes(TOL, n_calls=10)
    assert o0.step_form() == ("pool", "")
    assert_same_run(o0, o1, B, "after the reset")


def test_the_deep_kernels_give_the_shallow_kernels_trees_at_r45(az):
    """r45 (n = 24, [4, 5]) on the 64-bit tier with and without the flag, the same roots and stream: RamseyU64BigSpace's nests at
    depths 0..3 against RamseyU64Space's written-out loops"""
    n, sizes, B, seed, kmin, kmax = 24, [4, 5], 16, 9, 10, 276
    runs = []
    for big in (True, False):
        space = az.RamseySpaceNoEdgeRecolor(n, sizes, R45_W, u64=True, big_cliques=big)
        assert space.tier == "u64" and space.BIG_CLIQUES == big
        roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
        model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
        opt = az.NablaOptimizer.par_new(space, roots, model, B, **caps(40, space, kmax))
        opt.par_roll_out_episodes(TOL, n_calls=20)
        mid = opt.modify_roots(seed, 0, kmin, kmax)
        opt.par_reset_trees_policy(seed, 0, kmin, kmax)
        opt.par_roll_out_episodes(TOL, n_calls=10)
        runs.append((opt, mid))
    (a, ma), (b, mb) = runs
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    same_array(a.state_vecs(), b.state_vecs(), "state_vecs")
    ca, cb = a.counters(), b.counters()
    for k in MAIN_CTRS:
        assert ca[k] == cb[k], k
    for i in range(B):
        assert_tree_equal(a.get_tree(i), b.get_tree(i), f"agent {i}")
        assert np.array_equal(a.ramsey_agent_counts(i)[0], b.ramsey_agent_counts(i)[0])
    x, y = a.argmin_data(), b.argmin_data()
    assert x.eval.tobytes() == y.eval.tobytes() and np.array_equal(x.state["colors"], y.state["colors"]) and x.cost == y.cost
    assert (x.agent, x.node) == (y.agent, y.node)


def test_r46_driver_writes_its_scalars(tmp_path):
    from azdopt_amd import sinks
    out = tmp_path / "ev"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ramsey.py"), "r46", "--epochs", "1", "--episodes", "20", "--batch",
                        "16", "--hidden", "64", "64", "--out", str(out)], cwd=tmp_path, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "TotalCounts([" in r.stdout and "==== EPOCH: 1 ====" in r.stdout and "==== EPISODE: 20 ====" in r.stdout, r.stdout
    ev = sinks.read_events(out / "tfevents-losses")
    tags = [t for e in ev for t, _ in e[3]]
    assert tags.count("loss") == 1 and {"clique_counts/0", "clique_counts/1"} <= set(tags)
