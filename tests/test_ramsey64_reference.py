"""The three pins of tests/ramsey64_ref.py (the Ramsey reference past N = 32), on the CPU:
  1. its incrementally maintained counts == the C++ oracle's (orc.ramsey_act_sequence) after every action of full random
     play-outs at N <= 32, clique sizes up to 5;
  2. == RamseyState.recount (the definition, by enumerating vertex subsets) past the 32-bit word: after every action at N = 33
     [3,4] and N = 34 [3,3,3,3], at a fixed handful of states at N = 39 [3,3,4] and N = 48 [4,5] (one recount takes 0.08 s and
     1.4 s there);
  3. the whole engine == oracle.py_ramsey.PyRamseyEngine bit for bit at N = 34 (4 agents, 20 calls, one epoch boundary through
     modify_roots), and == the C++ oracle engine at the R(4,5) shape (N = 24) over two epochs: trees, state vectors,
     observations, argmin."""
import numpy as np
import pytest

import ramsey64_ref as R
from oracle import py_ramsey as pr

TOL = ([200, 200, 100, 100, 50, 50, 25, 25], 10)


def playout(n, C, seed, steps=None):
    """a random colouring and a random order of (edge, new colour != current) over every edge"""
    rng = np.random.default_rng(seed)
    E = n * (n - 1) // 2
    colors = rng.integers(0, C, E).astype(np.uint8)
    order = rng.permutation(E)[:steps]
    cur = colors.copy()
    actions = []
    for e in order:
        nc = int((cur[e] + 1 + rng.integers(0, C - 1)) % C)
        actions.append(int(e) + nc * E)
        cur[e] = nc
    return colors, actions


@pytest.mark.parametrize("n,sizes,seed", [(9, [3, 3], 0), (17, [4, 4], 1), (16, [3, 3, 3], 2), (24, [4, 5], 3), (32, [3, 3], 4),
                                          (20, [3, 3, 3, 3], 5), (14, [5, 5], 6), (19, [2, 5, 3], 7), (32, [5, 4], 8)])
def test_incremental_counts_match_the_cpp_oracle_after_every_action(orc, n, sizes, seed):
    colors, actions = playout(n, len(sizes), seed)
    st = R.IncRamseyState(n, sizes, colors.tolist(), set(range(len(colors))))
    c0, t0 = orc.ramsey_counts_new(n, sizes, colors)
    assert st.counts == c0.tolist() and st.totals == t0.tolist()
    for k, a in enumerate(actions):
        st.act(a)
        co, cn, tt = orc.ramsey_act_sequence(n, sizes, colors, actions[:k + 1])  # (the oracle replays the prefix)
        assert st.colors == co.tolist() and st.counts == cn.tolist() and st.totals == tt.tolist(), k
    assert not st.permitted & {a % len(colors) for a in actions}


def _against_recount(n, sizes, seed, steps, check_at):
    colors, actions = playout(n, len(sizes), seed, steps=steps)
    st = R.IncRamseyState(n, sizes, colors.tolist(), set(range(len(colors))))
    for k, a in enumerate(actions):
        st.act(a)
        if k in check_at:
            ref = pr.RamseyState(n, sizes, st.colors, st.permitted)  # recounts from the definition
            assert st.counts == ref.counts and st.totals == ref.totals, (n, k)


@pytest.mark.parametrize("n,sizes,seed", [(33, [3, 4], 0), (34, [3, 3, 3, 3], 1)])
def test_incremental_counts_match_the_recount_past_32_vertices_after_every_action(n, sizes, seed):
    steps = 60
    _against_recount(n, sizes, seed, steps, set(range(steps)))


@pytest.mark.parametrize("n,sizes,seed,steps,check_at", [(39, [3, 3, 4], 2, 120, {0, 7, 30, 77, 119}), (48, [4, 5], 3, 150, {0, 41, 149})])
def test_incremental_counts_match_the_recount_at_a_handful_of_states(n, sizes, seed, steps, check_at):
    _against_recount(n, sizes, seed, steps, check_at)


def _same_trees(ta, tb, tag):
    for f in ta:
        a, b = ta[f], tb[f]
        assert a.shape == b.shape, (tag, f)
        assert np.array_equal(a.view(np.uint32) if a.dtype.kind == "f" else a.astype(np.int64),
                              b.view(np.uint32) if b.dtype.kind == "f" else b.astype(np.int64)), (tag, f)


def test_engine_matches_the_recounting_engine_at_n34(orc):
    n, sizes, w, B, seed, kmin, kmax = 34, [3, 3, 3, 3], [1.0] * 4, 4, 11, 10, 30
    E, C = n * (n - 1) // 2, 4
    A, KW = E * C, (E * C + 63) // 64
    a, b = R.Ramsey64RefEngine(n, sizes, w, B), pr.PyRamseyEngine(n, sizes, w, B)
    colors, permitted = orc.gen_ramsey_roots(seed, 0, 0, B, n, C, kmin, kmax)
    assert permitted.shape[1] == KW == 36
    for e in (a, b):
        e.new_begin(R.unpack_roots(colors, permitted, E))
    call = 0
    h = orc.hash_predictions(seed, 0, B, A, call)
    for e in (a, b):
        e.new_end(h)

    def same(tag):
        assert np.array_equal(a.vecs.view(np.uint32), b.vecs.view(np.uint32)), tag
        for i in range(B):
            _same_trees(a.export_tree(i, KW), b.export_tree(i, KW), (tag, i))
            assert a.states[i].counts == b.states[i].counts and a.states[i].totals == b.states[i].totals, (tag, i)
        assert np.float32(a.argmin["eval"]).tobytes() == np.float32(b.argmin["eval"]).tobytes(), tag
        assert a.argmin["state"].colors == b.argmin["state"].colors and a.argmin["state"].totals == b.argmin["state"].totals, tag

    for epoch, calls in ((0, 12), (1, 8)):
        for _ in range(calls):
            for e in (a, b):
                e.rollout_begin(*TOL)
            call += 1
            h = orc.hash_predictions(seed, 0, B, A, call)
            assert a.rollout_end(h) == b.rollout_end(h)
        same(("epoch", epoch))
        (oa, wa), (ob, wb) = a.observe(4), b.observe(4)
        assert np.array_equal(wa, wb) and np.array_equal(np.isnan(oa), np.isnan(ob))
        assert np.array_equal(oa[~np.isnan(oa)].view(np.uint32), ob[~np.isnan(ob)].view(np.uint32))
        if epoch == 0:
            ra, rb = a.modify_roots(seed, 0, 0, kmin, kmax), b.modify_roots(seed, 0, 0, kmin, kmax)
            assert [(c, sorted(m)) for c, m in ra] == [(c, sorted(m)) for c, m in rb]
            call += 1
            h = orc.hash_predictions(seed, 0, B, A, call)
            for e, r in ((a, ra), (b, rb)):
                e.reset_begin(r)
                e.reset_end(h)
            same("reset")


def test_engine_matches_the_cpp_oracle_engine_at_r45(orc):
    n, sizes, w, B, seed, kmin, kmax, steps = 24, [4, 5], [1.0, 0.4685 / (1.0 - 0.4685)], 6, 4, 10, 276, 25
    E = n * (n - 1) // 2
    ce = orc.Engine(n, B, threads=4, ramsey=(sizes, w))
    pe = R.Ramsey64RefEngine(n, sizes, w, B)
    colors, permitted = orc.gen_ramsey_roots(seed, 0, 0, B, n, 2, kmin, kmax)
    ce.new_begin(colors, permitted)
    pe.new_begin(R.unpack_roots(colors, permitted, E))
    call = 0
    h = orc.hash_predictions(seed, 0, B, ce.A, call)
    ce.new_end(h)
    pe.new_end(h)
    for epoch in range(2):
        for _ in range(steps):
            ce.rollout_begin(*TOL)
            pe.rollout_begin(*TOL)
            assert np.array_equal(ce.state_vecs(), pe.vecs)
            call += 1
            h = orc.hash_predictions(seed, 0, B, ce.A, call)
            assert ce.rollout_end(h) == pe.rollout_end(h)
            am = ce.argmin()
            assert am["eval"].tobytes() == np.float32(pe.argmin["eval"]).tobytes()
            assert am["parents"].tolist() == pe.argmin["state"].colors
            assert ce.argmin_totals()[:2].tolist() == pe.argmin["state"].totals
        for i in range(B):
            tc = ce.export_tree(i)
            _same_trees({f: getattr(tc, f) for f in tc.FIELDS}, pe.export_tree(i, ce.KW), (epoch, i))
            assert ce.agent_counts(i).tolist() == pe.states[i].counts
        oc, wc = ce.observe(4)
        op, wp = pe.observe(4)
        nan = np.isnan(oc)
        assert np.array_equal(nan, np.isnan(op)) and np.array_equal(wc, wp)
        assert np.array_equal(oc[~nan].view(np.uint32), op[~nan].view(np.uint32))
        rc = ce.modify_roots(seed, epoch, 0, kmin, kmax)
        rp = pe.modify_roots(seed, epoch, 0, kmin, kmax)
        pc = R.pack_roots(rp, E, ce.KW)
        assert np.array_equal(rc[0], pc[0]) and np.array_equal(rc[1], pc[1])
        ce.reset_begin(*rc)
        pe.reset_begin(rp)
        call += 1
        h = orc.hash_predictions(seed, 0, B, ce.A, call)
        ce.reset_end(h)
        pe.reset_end(h)
