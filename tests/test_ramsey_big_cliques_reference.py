"""The yardsticks of the big-clique tests (clique sizes 6..8), pinned on the CPU before the device is compared with them:
  1. tests/ramsey64_ref.py's incrementally maintained counts == RamseyState.recount (the definition) after play-outs of 20
     actions at (12,[3,6]), (14,[4,7]), (13,[8,3]), (16,[3,3,6]), on roots whose big colour is dense (tests/ramsey_big_cases.py);
  2. the C++ oracle engine == PyRamseyEngine over that state, bit for bit, on trees at (12,[3,6]) and (13,[8,3]);
  3. the closed form: a root monochromatic in a colour of clique size s has every per-edge count C(n-2, s-2) and total C(n, s),
     in both references."""
import numpy as np
import pytest

import ramsey64_ref as R
import ramsey_big_cases as K
from oracle import py_ramsey as pr

TOL = ([200, 200, 100, 100, 50, 50, 25, 25], 10)


@pytest.mark.parametrize("case", ["n12_36", "n14_47", "n13_83", "n16_336"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_incremental_counts_match_the_recount_after_20_actions(case, seed):
    n, sizes, p = K.CASES[case]
    E, C = n * (n - 1) // 2, len(sizes)
    colors, _ = K.roots(n, sizes, p, 1, seed, 1, 1)
    st = R.IncRamseyState(n, sizes, colors[0].tolist(), set(range(E)))
    ref = pr.RamseyState(n, sizes, st.colors, st.permitted)
    assert st.counts == ref.counts and st.totals == ref.totals
    assert st.totals[K.big_colour(sizes)] > 0  # (the big colour's cliques exist: the deep counts are exercised)
    rng = np.random.default_rng(seed)
    for k, e in enumerate(rng.permutation(E)[:20]):
        nc = int((st.colors[e] + 1 + rng.integers(0, C - 1)) % C)
        st.act(int(e) + nc * E)
        if k % 5 == 4:
            ref = pr.RamseyState(n, sizes, st.colors, st.permitted)
            assert st.counts == ref.counts and st.totals == ref.totals, k


def _same_trees(ta, tb, tag):
    for f in ta:
        a, b = ta[f], tb[f]
        assert a.shape == b.shape, (tag, f)
        assert np.array_equal(a.view(np.uint32) if a.dtype.kind == "f" else a.astype(np.int64),
                              b.view(np.uint32) if b.dtype.kind == "f" else b.astype(np.int64)), (tag, f)


@pytest.mark.parametrize("case", ["n12_36", "n13_83"])
def test_cpp_oracle_engine_matches_the_python_engine(orc, case):
    n, sizes, p = K.CASES[case]
    B, seed, steps = 6, 1, 20
    E, w = n * (n - 1) // 2, [1.0] * len(sizes)
    ce = orc.Engine(n, B, threads=4, ramsey=(sizes, w))
    pe = R.Ramsey64RefEngine(n, sizes, w, B)
    colors, permitted = K.roots(n, sizes, p, B, seed, 10, 30)
    ce.new_begin(colors, K.pack_permitted(permitted, ce.KW))
    pe.new_begin([(colors[i].tolist(), permitted[i]) for i in range(B)])
    K.assert_not_vacuous(sizes, pe.roots, case)
    h = orc.hash_predictions(seed, 0, B, ce.A, 0)
    ce.new_end(h)
    pe.new_end(h)
    for call in range(1, steps + 1):
        ce.rollout_begin(*TOL)
        pe.rollout_begin(*TOL)
        assert np.array_equal(ce.state_vecs(), pe.vecs)
        h = orc.hash_predictions(seed, 0, B, ce.A, call)
        assert ce.rollout_end(h) == pe.rollout_end(h)
        am = ce.argmin()
        assert am["eval"].tobytes() == np.float32(pe.argmin["eval"]).tobytes()
        assert am["parents"].tolist() == pe.argmin["state"].colors
        assert ce.argmin_totals()[:len(sizes)].tolist() == pe.argmin["state"].totals
    for i in range(B):
        tc = ce.export_tree(i)
        _same_trees({f: getattr(tc, f) for f in tc.FIELDS}, pe.export_tree(i, ce.KW), (case, i))
        assert ce.agent_counts(i).tolist() == pe.states[i].counts


@pytest.mark.parametrize("n,sizes", [(12, [3, 6]), (14, [4, 7]), (13, [8, 3]), (16, [3, 3, 6]), (34, [3, 6])])
def test_closed_form_of_a_monochromatic_root(orc, n, sizes):
    assert K.closed_form(12, 6) == (210, 924)
    big = K.big_colour(sizes)
    E = n * (n - 1) // 2
    per_edge, total = K.closed_form(n, sizes[big])
    st = R.IncRamseyState(n, sizes, [big] * E, set())
    assert st.counts[big] == [per_edge] * E and st.totals[big] == total
    assert all(st.totals[c] == 0 and not any(st.counts[c]) for c in range(len(sizes)) if c != big)
    if n <= 32:  # (the C++ oracle stops at 32 vertices)
        c0, t0 = orc.ramsey_counts_new(n, sizes, np.full(E, big, np.uint8))
        assert c0.tolist() == st.counts and t0.tolist() == st.totals
