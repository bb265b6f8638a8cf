"""The dense-graph space's default cost kernel alone (azd_debug_probe_dense_cost: dense_lambda1_wave, dense_matching_scratch,
dense_matching_update -> dense_augment_from) against the oracle on the shared case set (dense_cost_cases.py), step by step:
lambda_1 as f64 bits, the matching NUMBER (the oracle recomputes it from nothing, the device repairs the previous step's
matching), the device's matching itself as a matching of the current graph, and one hook call per lambda_1.  The branch of the
repair that every step took is derived from the device's own matchings and counted: every branch must occur."""
import collections
import time

import numpy as np
import pytest

import dense_cost_cases as D
from gpu_parity import az  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probed(az):
    """{case name: (lambda_1[steps], mu[steps], mate[steps][64], hooks[steps])} of the whole set: one probe call per vertex count"""
    from azdopt_amd import _lib
    out, t0 = {}, time.time()
    for n, cs in sorted(D.by_size().items()):
        k = D.n_toggles(n)
        adj = np.ascontiguousarray([c.adj for c in cs], dtype=np.uint64)
        tog = np.ascontiguousarray([c.toggles for c in cs], dtype=np.uint16)
        lam = np.zeros((len(cs), k + 1), np.float64)
        mu = np.full((len(cs), k + 1), -1, np.int32)
        hooks = np.full((len(cs), k + 1), -1, np.int32)
        mate = np.zeros((len(cs), k + 1, 64), np.uint8)
        _lib.check(az.lib().azd_debug_probe_dense_cost(0, _lib.ptr(adj), n, len(cs), _lib.ptr(tog), k, _lib.ptr(lam), _lib.ptr(mu), _lib.ptr(mate),
                                                       _lib.ptr(hooks)), "probe_dense_cost")
        for i, c in enumerate(cs):
            out[c.name] = (lam[i], mu[i], mate[i], hooks[i])
    print("probe: %d graphs, %d calls, %.2f s" % (len(out), len(D.by_size()), time.time() - t0))
    return out


@pytest.fixture(scope="module")
def expected(orc):
    """{case name: [(lambda_1, matching number, steps of the iteration)] per step}, from the oracle"""
    out = {}
    for c in D.cases():
        rows = []
        for _, _, g in D.steps(c):
            a = np.array(g, dtype=np.uint64)
            rows.append((orc.dense_lambda1(a), orc.dense_matching_exact(a), orc.dense_lambda1_steps(a)))
        out[c.name] = rows
    return out


def test_lambda1_bits_matching_numbers_and_hook_calls_equal_the_oracle(probed, expected):
    capped = 0
    for c in D.cases():
        lam, mu, _, hooks = probed[c.name]
        for j, (want_lam, want_mu, steps) in enumerate(expected[c.name]):
            tag = (c.name, j)
            assert np.float64(lam[j]).view(np.uint64) == np.float64(want_lam).view(np.uint64), (tag, lam[j], want_lam)
            assert mu[j] == want_mu, (tag, mu[j], want_mu)
            assert hooks[j] == 1, (tag, hooks[j], steps)  # short runs (8 steps or fewer) and runs that end at the cap alike
            capped += steps >= 2000
    assert capped >= 1  # trial 180 of the near-trees: the iteration's last exit, `it + 4 >= DENSE_LAMBDA_ITERS`
    assert any(rows[j][2] <= 8 for rows in expected.values() for j in range(len(rows)))  # ... and its first: the hook after the loop


def test_every_mate_is_a_matching_of_the_current_graph(probed, expected):
    for c in D.cases():
        _, mu, mate, _ = probed[c.name]
        for j, _, g in D.steps(c):
            m, tag = mate[j], (c.name, j)
            assert (m[c.n:] == 0xFF).all(), tag
            matched = 0
            for v in range(c.n):
                u = int(m[v])
                if u == 0xFF:
                    continue
                assert u < c.n and int(m[u]) == v and (g[v] >> u) & 1, (tag, v, u)
                matched += 1
            assert matched == 2 * mu[j] == 2 * expected[c.name][j][1], tag
        if c.start_mate is not None:  # a greedy start that is maximum is what the device holds
            assert mate[0][:c.n].tolist() == list(c.start_mate), c.name


def test_every_branch_of_the_matching_repair_is_taken(probed):
    """from the matching the device held before each toggle: which branch of dense_matching_update the step took, and for a
    search whether it succeeded.  A condition on the case set: an empty class asks for another targeted sequence there."""
    counts = collections.Counter()
    for c in D.cases():
        _, mu, mate, _ = probed[c.name]
        for j, slot, g in D.steps(c):
            if j:
                u, v = D.from_colex(slot)
                counts[D.branch_class(c.n, mate[j - 1], bool((g[v] >> u) & 1), u, v, int(mu[j - 1]), int(mu[j]))] += 1
    for k in D.CLASSES:
        print("%6d  %s" % (counts[k], k))
    assert set(counts) <= set(D.CLASSES)
    for k in D.CLASSES:
        assert counts[k] > 0, k
