"""The root policy's options without a GPU: the weighted root generator (azd_ramsey_generate_roots_weighted) against its Python
restatement (tests/root_policy_ref.py) bit for bit, equal weights and NULL against the uniform generator, the refusals of
azd_root_policy by name, the defaults, and the reference helper pinned -- with the default rule and no weights -- against the
unmodified oracles' modify_roots before the GPU tests switch its rule."""
import ctypes as C

import numpy as np
import pytest

import ramsey64_ref as R64
import root_policy_ref as RP

R45_P = [0.4685, 0.5315]
WEIGHTS = {2: R45_P, 3: [3, 1, 2], 4: [1e-9, 1, 1, 1e9]}
TOL = ([200, 200, 100, 100, 50, 50, 25, 25], 10)


@pytest.fixture(scope="module", name="az")
def package():  # (no device needed here: tests/gpu_parity.py's `az` is the GPU tests')
    import azdopt_amd
    return azdopt_amd


def weighted(az, seed, epoch, first, count, n, C_, kmin, kmax, w):
    from azdopt_amd import _lib
    E = n * (n - 1) // 2
    colors = np.zeros((count, E), np.uint8)
    permitted = np.zeros((count, az.lib().azd_ramsey_key_words(n, C_)), np.uint64)
    wp = None if w is None else np.ascontiguousarray(w, np.float64)
    st = az.lib().azd_ramsey_generate_roots_weighted(seed, epoch, first, count, n, C_, kmin, kmax, None if w is None else _lib.ptr(wp),
                                                     _lib.ptr(colors), _lib.ptr(permitted))
    return st, colors, permitted


def test_symbols_are_exported_and_bound(az):
    from azdopt_amd import _lib
    L = az.lib()
    for name in ("azd_ramsey_generate_roots_weighted", "azd_engine_set_root_policy", "azd_engine_get_root_policy", "azd_root_policy_check",
                 "azd_engine_root_policy_report"):
        assert getattr(L, name).argtypes, name
    assert C.sizeof(_lib.RootPolicy) == 40 and (_lib.ROOT_RULE_THRESHOLD, _lib.ROOT_RULE_BEST) == (0, 1)


@pytest.mark.parametrize("C_", [2, 3, 4])
def test_weighted_generator_equals_the_python_restatement(az, C_):
    """colours and permitted masks, 64 agents, two epochs, at the r45 probabilities, small integers and weights 18 orders apart"""
    n, kmin, kmax, seed, first = 12, 5, 30, 7, 100
    E = n * (n - 1) // 2
    kw = az.lib().azd_ramsey_key_words(n, C_)
    seen = set()
    for epoch in (0, 1):
        st, colors, permitted = weighted(az, seed, epoch, first, 64, n, C_, kmin, kmax, WEIGHTS[C_])
        assert st == 0
        cr, pr_ = R64.pack_roots(RP.gen_ramsey_roots(seed, epoch, first, 64, n, C_, kmin, kmax, WEIGHTS[C_]), E, kw)
        assert np.array_equal(colors, cr) and np.array_equal(permitted, pr_), epoch
        seen |= set(np.unique(colors).tolist())
        assert all(kmin <= sum(bin(int(x)).count("1") for x in row) <= kmax for row in permitted)
    # (at [1e-9, 1, 1, 1e9] colour 3 has all but 2e-9 of the mass)
    assert seen == ({3} if C_ == 4 else set(range(C_))), seen


def test_thresholds_of_the_restatement():
    assert RP.color_thresholds([1, 1]) == [1 << 31]
    assert RP.color_thresholds([1, 1, 1]) == [(1 << 32) // 3 + 1, 2 * (1 << 32) // 3 + 1]
    assert RP.color_thresholds([1e-9, 1, 1, 1e9])[0] == 1  # ceil of a positive quotient: colour 0 keeps the draw 0
    assert RP.color_thresholds([1e300, 1e-300]) == [1 << 32]  # clamped: colour 1 is never drawn


@pytest.mark.parametrize("C_", [2, 3, 4])
def test_equal_weights_and_null_are_the_uniform_generator(az, orc, C_):
    """ceil(2^32 (c + 1) / C) is the smallest high word hi with (hi C) >> 32 > c: equal weights reproduce below(r, C) exactly"""
    n, kmin, kmax = 13, 4, 40
    for seed, epoch, first in ((0, 0, 0), (5, 1, 77)):
        co, mo = orc.gen_ramsey_roots(seed, epoch, first, 64, n, C_, kmin, kmax)
        sp = az.RamseySpaceNoEdgeRecolor(n, [3] * C_)
        cu, mu = sp.generate_roots(seed, 64, first_agent=first, epoch=epoch, kmin=kmin, kmax=kmax)
        assert np.array_equal(cu, co) and np.array_equal(mu, mo)
        for w in (None, [1.0] * C_, [0.3] * C_, [7] * C_):
            st, c, m = weighted(az, seed, epoch, first, 64, n, C_, kmin, kmax, w)
            assert st == 0 and np.array_equal(c, co) and np.array_equal(m, mo), (C_, w)
        c, m = sp.generate_roots(seed, 64, first_agent=first, epoch=epoch, kmin=kmin, kmax=kmax, color_weights=[2.5] * C_)
        assert np.array_equal(c, co) and np.array_equal(m, mo)
    # every high word, not only the drawn ones: the thresholds sit exactly where below() steps
    thr = RP.color_thresholds([1.0] * C_)
    for c, t in enumerate(thr):
        assert (t * C_) >> 32 == c + 1 and ((t - 1) * C_) >> 32 == c, (C_, c, t)


def test_share_of_colour_0_at_the_r45_probabilities(az):
    """N = 24, 64 agents: 17 664 edges; sigma = sqrt(p (1 - p) / 17664) = 0.00375, the bound 0.02 is five of them -- an inverted
    comparison would give 0.5315"""
    st, colors, _ = weighted(az, 11, 0, 0, 64, 24, 2, 10, 276, R45_P)
    assert st == 0 and colors.size == 17664
    share = float((colors == 0).mean())
    print("share of colour 0: %.4f" % share)
    assert abs(share - 0.4685) <= 0.02, share


def test_generator_refuses_bad_weights_by_name(az):
    L = az.lib()
    for bad in ([0.0, 1.0], [-1.0, 1.0], [float("nan"), 1.0], [float("inf"), 1.0]):
        st, _, _ = weighted(az, 0, 0, 0, 4, 8, 2, 2, 5, bad)
        assert st == 1 and L.azd_last_error().decode().startswith("color_weights"), bad
    sp = az.RamseySpaceNoEdgeRecolor(8, [3, 3])
    with pytest.raises(ValueError):
        sp.generate_roots(0, 4, color_weights=[1, 1, 1])


def check(az, space_id, n_colors, rule, weights):
    from azdopt_amd import _lib
    p = _lib.RootPolicy(rule, len(weights))
    for i, w in enumerate(weights):
        p.color_weights[i] = w
    st = az.lib().azd_root_policy_check(space_id, n_colors, C.byref(p))
    return st, az.lib().azd_last_error().decode()


def test_every_refusal_of_the_policy_is_named(az):
    """azd_root_policy_check is the check azd_engine_set_root_policy makes, callable without an engine (and so without a device)"""
    from azdopt_amd import _lib
    R, C21, D = _lib.SPACE_RAMSEY, _lib.SPACE_C21, _lib.SPACE_DENSE
    for rule in (0, 1):
        assert check(az, R, 2, rule, [])[0] == 0 and check(az, C21, 0, rule, [])[0] == 0 and check(az, D, 0, rule, [])[0] == 0
        assert check(az, R, 2, rule, R45_P)[0] == 0 and check(az, R, 4, rule, [1e-9, 1, 1, 1e9])[0] == 0
    assert az.lib().azd_root_policy_check(R, 2, None) == 0  # NULL: the defaults
    for rule in (2, -1, 7):
        st, why = check(az, R, 2, rule, [])
        assert st == 1 and why.startswith("rule:"), (rule, why)
    for space in (C21, D):
        st, why = check(az, space, 0, 1, [1.0, 1.0])
        assert st == 1 and why.startswith("color_weights:") and "RAMSEY" in why, why
    for n in (1, 3, 4):
        st, why = check(az, R, 2, 0, [1.0] * n)
        assert st == 1 and why.startswith("n_color_weights:"), (n, why)
    for bad in (0.0, -0.5, float("nan"), float("inf"), -float("inf")):
        st, why = check(az, R, 3, 1, [1.0, bad, 1.0])
        assert st == 1 and why.startswith("color_weights:") and "finite and positive" in why, (bad, why)
    assert az.lib().azd_engine_set_root_policy(None, None) == 1
    assert az.lib().azd_engine_root_policy_report(None, None, None, None) == 1


def test_get_returns_the_defaults_before_any_set(az):
    """azd_engine_get_root_policy(NULL, p): the policy of an engine nobody has set one on (tests/test_gpu_root_policy.py reads the
    same from a live engine)"""
    from azdopt_amd import _lib
    p = _lib.RootPolicy(9, 9)
    assert az.lib().azd_engine_get_root_policy(None, C.byref(p)) == 0
    assert (p.rule, p.n_color_weights, list(p.color_weights)) == (_lib.ROOT_RULE_THRESHOLD, 0, [0.0] * 4)
    assert az.lib().azd_engine_get_root_policy(None, None) == 1


def run_calls(orc, ref, eng, roots_packed, roots_ref, A, B, seed, calls):
    eng.new_begin(*roots_packed)
    ref.new_begin(roots_ref)
    h = orc.hash_predictions(seed, 0, B, A, 0)
    eng.new_end(h)
    ref.new_end(h)
    for call in range(1, calls + 1):
        eng.rollout_begin(*TOL)
        ref.rollout_begin(*TOL)
        h = orc.hash_predictions(seed, 0, B, A, call)
        assert eng.rollout_end(h) == ref.rollout_end(h)


def test_helper_at_the_default_rule_equals_the_unmodified_oracles_c21(orc):
    """c21, N = 8: the helper with rule "threshold" == oracle.py_oracle.PyEngine.modify_roots == the C++ oracle's, over two epochs
    that meet the stagnant and the improved branch"""
    import oracle.py_oracle as po
    n, B, seed, kmin, kmax = 8, 16, 3, 2, 9
    parents, permitted = orc.gen_roots(seed, 0, 0, B, n, kmin, kmax)
    eng = orc.Engine(n, B)
    ref = RP.C21PolicyEngine(n, B)
    A = eng.A
    roots = [(list(map(int, parents[i])), {a for a in range(A) if int(permitted[i, a >> 6]) >> (a & 63) & 1}) for i in range(B)]
    run_calls(orc, ref, eng, (parents, permitted), roots, A, B, seed, 12)
    branches = set()
    for epoch in (0, 1):
        mine = ref.modify_roots(seed, epoch, 0, kmin, kmax, rule="threshold")
        branches |= {b for b, _, _ in ref.report}
        theirs = po.PyEngine.modify_roots(ref, seed, epoch, 0, kmin, kmax)
        assert mine == theirs
        pc, mc = eng.modify_roots(seed, epoch, 0, kmin, kmax)
        for i, (p, m) in enumerate(mine):
            assert list(map(int, pc[i])) == p, (epoch, i)
            assert {a for a in range(A) if int(mc[i, a >> 6]) >> (a & 63) & 1} == m, (epoch, i)
    assert {RP.BRANCH_STAGNANT, RP.BRANCH_IMPROVED} <= branches


def test_helper_at_the_default_rule_equals_the_unmodified_oracles_ramsey(orc):
    """Ramsey, N = 8, [3,3,3]: the recounting and the incremental helper == oracle.py_ramsey.PyRamseyEngine.modify_roots == the C++
    oracle's; under "best" the same trees give a different root somewhere (the rule is live)"""
    import oracle.py_ramsey as pr
    n, sizes, w, B, seed, kmin, kmax = 8, [3, 3, 3], [1.0] * 3, 12, 3, 4, 10
    E = n * (n - 1) // 2
    colors, permitted = orc.gen_ramsey_roots(seed, 0, 0, B, n, 3, kmin, kmax)
    eng = orc.Engine(n, B, ramsey=(sizes, w))
    roots = R64.unpack_roots(colors, permitted, E)
    refs = [RP.RamseyPolicyEngine(n, sizes, w, B), RP.Ramsey64PolicyEngine(n, sizes, w, B)]
    for k, ref in enumerate(refs):
        e2 = eng if k == 0 else orc.Engine(n, B, ramsey=(sizes, w))
        run_calls(orc, ref, e2, (colors, permitted), roots, eng.A, B, seed, 10)
    differs = 0
    for epoch in (0, 1):
        theirs = pr.PyRamseyEngine.modify_roots(refs[0], seed, epoch, 0, kmin, kmax)
        cc, mc = eng.modify_roots(seed, epoch, 0, kmin, kmax)
        for ref in refs:
            mine = ref.modify_roots(seed, epoch, 0, kmin, kmax, rule="threshold")
            assert mine == theirs
            pc, pm = R64.pack_roots(mine, E, eng.KW)
            assert np.array_equal(pc, cc) and np.array_equal(pm, mc)
        assert {b for b, _, _ in refs[0].report} >= {RP.BRANCH_IMPROVED}
        best = refs[1].modify_roots(seed, epoch, 0, kmin, kmax, rule="best")
        assert best == refs[0].modify_roots(seed, epoch, 0, kmin, kmax, rule="best")
        for i, (b, node, kept) in enumerate(refs[1].report):
            if b == RP.BRANCH_IMPROVED:
                t = refs[1].trees[i]
                assert kept >= 1 and t.node[node]["c"] == t.node[0]["cs"]
        differs += sum(1 for x, y in zip(best, theirs) if x[0] != y[0])
    assert differs > 0
