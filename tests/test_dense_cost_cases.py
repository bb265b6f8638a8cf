"""The shared case set of the dense-graph space's default cost (dense_cost_cases.py) on the CPU: that it is the set the GPU test
assumes (families, sizes, connected graphs, legal toggles), the oracle's matching procedures against each other on every step
of it, and the oracle's lambda_1 against LAPACK -- split by whether the power iteration ended at its step cap."""
import collections

import numpy as np
import pytest

import dense_cost_cases as D


@pytest.fixture(scope="module")
def stepped(orc):
    """[(case, step, graph, u64 array)] of the whole set"""
    return [(c, j, g, np.array(g, dtype=np.uint64)) for c in D.cases() for j, _, g in D.steps(c)]


def test_the_set_is_what_the_gpu_test_assumes(orc):
    cs = D.cases()
    assert 280 <= len(cs) <= 340, len(cs)
    fams = collections.Counter(c.family for c in cs)
    for name, fn in D.FAMILIES:
        assert {c.n for c in cs if c.family == name and c.kind == "random"} == {n for n in D.SIZES if fn(n) is not None}, name
        assert fams[name] >= 5, name
    for name in D.RANDOM_FAMILIES:
        assert fams[name] >= 20, name
    assert {c.n for c in cs if c.family != "near_tree"} == set(D.SIZES)
    assert any(c.name == "near_tree-trial180" and c.n == 64 and len(D.edges_of(c.adj)) == 64 for c in cs)
    assert {c.n % 2 for c in cs if c.family == "cycle"} == {0, 1}
    for c in cs:
        assert len(c.toggles) == D.n_toggles(c.n) == (16 if c.n >= 8 else {4: 3, 5: 5}[c.n]), c.name
        assert len(set(c.toggles)) == len(c.toggles) and max(c.toggles) < c.n * (c.n - 1) // 2, c.name  # no slot twice
        prev = None
        for j, slot, g in D.steps(c):
            assert D.is_connected(g), (c.name, j)
            assert all(((g[v] >> u) & 1) == ((g[u] >> v) & 1) for v in range(c.n) for u in range(v)) and not any((g[v] >> v) & 1 for v in range(c.n))
            if j:
                u, v = D.from_colex(slot)
                assert D.colex(u, v) == slot
                if (prev[v] >> u) & 1:  # a deletion: never of a cut edge, by the space's own rule
                    assert not orc.dense_is_cut_edge(np.array(prev, dtype=np.uint64), v, u), (c.name, j)
            prev = g


def test_targeted_sequences_start_where_they_say(orc):
    """the first toggle of a targeted sequence, from the greedy start matching (the device's own at step 0 where it is maximum):
    deletions of a matched edge that keep and that lose the matching number, additions between two matched vertices of a graph
    with two or more unmatched ones that raise it and that do not"""
    seen = collections.Counter()
    for c in D.cases():
        if c.kind == "random":
            continue
        mate = D.greedy_matching(c.adj)
        u, v = D.from_colex(c.toggles[0])
        present = bool((c.adj[v] >> u) & 1)
        assert mate[u] != 0xFF and mate[v] != 0xFF, c.name
        assert present == (c.kind == "delete_matched") and (mate[u] == v) == present, c.name
        if c.kind == "add_matched":
            assert mate[:c.n].count(0xFF) >= 2, c.name
        if c.start_mate is not None:
            assert list(c.start_mate) == mate
            g0, g1 = np.array(c.adj, dtype=np.uint64), np.array(D.toggled(c.adj, c.toggles[0]), dtype=np.uint64)
            assert sum(m != 0xFF for m in mate) // 2 == orc.dense_matching_exact(g0)
            seen[D.branch_class(c.n, mate, not present, u, v, orc.dense_matching_exact(g0), orc.dense_matching_exact(g1))] += 1
    for k in (4, 5, 7, 8):
        assert seen[D.CLASSES[k]] > 0, (D.CLASSES[k], seen)


def test_matching_procedures_agree_on_every_step(orc, stepped):
    for c, j, g, a in stepped:
        mu = orc.dense_matching_exact(a)
        assert mu == orc.dense_matching_tutte(a), (c.name, j)
        assert mu == D.matching_number(g), (c.name, j)
        if c.n <= 14:
            assert mu == orc.dense_matching_reference(a), (c.name, j)


def is_near_tree(n, g):
    """at most 18 edges beyond a spanning tree: what a tree of the set, or a near-tree of the generator (two extra pairs at most),
    can have after 16 toggles"""
    return len(D.edges_of(g)) - (n - 1) <= 18


def test_lambda1_against_lapack_below_and_at_the_step_cap(orc, stepped):
    """Below the cap the value's error is of the order of the bracket squared over the spectral gap: 5e-8, and 2e-6 on near-trees
    (the bounds of test_oracle_dense.py's test_lambda1_against_lapack).  A graph whose iteration ends at the cap of 2000 steps has
    no such bound: the bracket has not closed.  Measured on this set: 1 capped graph among 5008 (near_tree-trial180 before any
    toggle: n = 64, 64 edges, lambda_1 = 2.2513, gap to lambda_2 3.6e-3), error 3.189e-05 against numpy.linalg.eigvalsh;
    asserted at twice that (LAPACK's own last bits differ between machines), 6.4e-05 -- about 16 ulp of the f32 cost there."""
    worst = {"dense": (0.0, None), "near-tree": (0.0, None), "capped": (0.0, None)}
    capped = 0
    for c, j, g, a in stepped:
        m = np.zeros((c.n, c.n))
        for u, v in D.edges_of(g):
            m[u, v] = m[v, u] = 1
        err = abs(orc.dense_lambda1(a) - np.linalg.eigvalsh(m)[-1])
        steps = orc.dense_lambda1_steps(a)
        assert steps % 4 == 0 and 4 <= steps <= 2000, (c.name, j, steps)
        kind = "capped" if steps == 2000 else "near-tree" if is_near_tree(c.n, g) else "dense"
        capped += steps == 2000
        if err > worst[kind][0]:
            worst[kind] = (err, (c.name, j))
    print("graphs", len(stepped), "capped", capped, "worst errors", worst)
    assert capped >= 1
    assert worst["dense"][0] < 5e-8, worst
    assert worst["near-tree"][0] < 2e-6, worst
    assert worst["capped"][0] < 2 * 3.189e-05, worst
    assert worst["capped"][0] > 2e-6, worst  # the cap is reached where the documented accuracy does not hold: that is why it is pinned
