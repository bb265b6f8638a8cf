"""The Aouchiche-Hansen cost's Python reference (tests/dense_ah_ref.py) on the CPU:
  1. its all-sources BFS == Floyd-Warshall on every graph of the set;
  2. its eigenvalue (Householder + Sturm-count multisection, one IEEE operation at a time) against numpy.linalg.eigvalsh on the
     whole set -- 560 connected graphs, n = 4 .. 32: paths, stars, cycles, complete graphs, double brooms, G(n, p) for p from 0.05
     to 0.6 -- within 64 n 2^-53 ||D||_F per graph (the backward-error form: LAPACK promises no more than a small multiple of
     n eps ||D||).  Largest ratio seen: 0.0151 (profiles/r08_dense_ah.txt);
  3. closed forms worked from the definition (tests/golden/ah_cost_vectors.json) at 1e-9."""
import json
import os

import numpy as np

import dense_ah_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ah_cost_vectors.json")


def floyd_warshall(adj, n):
    INF = 10 ** 6
    d = [[0 if u == v else (1 if (adj[u] >> v) & 1 else INF) for v in range(n)] for u in range(n)]
    for k in range(n):
        dk = d[k]
        for i in range(n):
            dik, di = d[i][k], d[i]
            for j in range(n):
                if dik + dk[j] < di[j]:
                    di[j] = dik + dk[j]
    return d


def test_graph_set_is_what_the_checks_assume():
    gs = R.graph_set()
    assert len(gs) >= 500
    names = {name.rstrip("0123456789.+tre") for name, _, _ in gs} | {name for name, _, _ in gs}
    for fam in ("path", "star", "cycle", "complete", "broom"):
        assert fam in names
    assert any(name.startswith("gnp0.05") for name, _, _ in gs) and any(name.startswith("gnp0.60") for name, _, _ in gs)
    assert {n for _, n, _ in gs} == set(range(4, 33))
    for name, n, adj in gs:
        assert R.connected(adj, n), name
        assert all(not (adj[v] >> v) & 1 and adj[v] < (1 << n) for v in range(n))
        assert all(((adj[v] >> u) & 1) == ((adj[u] >> v) & 1) for v in range(n) for u in range(n))


def test_bfs_matches_floyd_warshall():
    for name, n, adj in R.graph_set():
        dist, trans, ecc = R.bfs_all(adj, n)
        fw = floyd_warshall(adj, n)
        assert dist == fw, (name, n)
        assert trans == [sum(r) for r in fw] and ecc == [max(r) for r in fw], (name, n)


def test_eigenvalue_against_lapack_on_the_whole_set():
    worst, worst_at = 0.0, None
    diameters, k_branches, cost_moved = set(), set(), 0
    for name, n, adj in R.graph_set():  # no graph is skipped
        r = R.ah_cost(adj, n)
        dist, trans, ecc = R.bfs_all(adj, n)
        D = np.array(dist, dtype=np.float64)
        ev = np.linalg.eigvalsh(D)[::-1]
        assert r["diameter"] == max(ecc) and r["proximity"] == min(trans) / (n - 1)
        q = (2 * r["diameter"]) // 3
        assert r["k"] == (q - 1 if q >= 1 else n - 1) and 0 <= r["k"] < n
        tol = 64.0 * n * 2.0 ** -53 * np.linalg.norm(D)
        err = abs(r["eigenvalue"] - ev[r["k"]])
        if err / tol > worst:
            worst, worst_at = err / tol, (name, n)
        assert err <= tol, (name, n, r["eigenvalue"], ev[r["k"]], err / tol)
        cost_moved += np.float32(r["proximity"] + ev[r["k"]]) != r["cost"]
        assert r["cost"].dtype == np.float32 and r["eval"].dtype == np.float32
        assert r["eval"] == np.float32(1.0) / np.float32(2 * n + 2) * (r["cost"] + np.float32(2.0))
        diameters.add(r["diameter"])
        k_branches.add(q >= 1)
    print("AH eigenvalue vs eigvalsh: largest error / tolerance = %.4f at %s; f32 cost differs from LAPACK's on %d of %d graphs"
          % (worst, worst_at, cost_moved, len(R.graph_set())))
    assert {1, 2, 3} <= diameters and max(diameters) >= 6
    assert k_branches == {True, False}


def test_closed_forms():
    vs = json.load(open(GOLDEN))["vectors"]
    assert len(vs) >= 14
    build = dict(complete=R.complete, star=R.star, cycle=R.cycle, path=R.path)
    for v in vs:
        r = R.ah_cost(build[v["family"]](v["n"]), v["n"])
        assert (r["diameter"], r["k"]) == (v["diameter"], v["k"]), v["name"]
        assert abs(r["proximity"] - v["proximity"]) <= 1e-9 and abs(r["eigenvalue"] - v["eigenvalue"]) <= 1e-9, (v["name"], v["n"], r)
        assert abs(r["proximity"] + r["eigenvalue"] - v["cost"]) <= 1e-9, (v["name"], v["n"], r)
    n = 9
    assert abs(R.ah_cost(R.star(n), n)["eigenvalue"] - (1 + (n - 2) + (n * n - 3 * n + 3) ** 0.5 - 1)) <= 1e-9


def test_tree_sum_is_the_wave_butterfly():
    rng = np.random.default_rng(1)
    for _ in range(20):
        v = [float(x) for x in rng.standard_normal(64) * 10.0 ** rng.integers(-8, 8, 64)]
        lanes = list(v)
        for w in (1, 2, 4, 8, 16, 32):
            lanes = [lanes[l] + lanes[l ^ w] for l in range(64)]
        assert all(x == R.tree_sum64(v) for x in lanes)


# ---------------------------------------------------------------- the helper's engine glue, before its cost is swapped
def _assert_tree_equal(a, b, tag):
    for f in b.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape, (tag, f, x.shape, y.shape)
        same = np.array_equal(x.view(np.uint32), y.view(np.uint32)) if x.dtype.kind == "f" else np.array_equal(x.astype(np.int64), y.astype(np.int64))
        assert same, (tag, f)


def _compare_c21(pe, oe, B, tag):
    assert np.array_equal(pe.state_vecs().view(np.uint32), oe.state_vecs().view(np.uint32)), tag
    for i in range(B):
        _assert_tree_equal(pe.export_tree(i), oe.export_tree(i), f"{tag} agent {i}")
        sp, so = pe.agent_state(i), oe.agent_state(i)
        for k in sp:  # (the cost fields are absent while the agent stands on its root)
            assert np.array_equal(sp[k], so[k]), (tag, i, k, sp[k], so[k])
    cp, co = pe.counters(), oe.counters()
    for k in cp:
        assert cp[k] == co[k], (tag, k, cp[k], co[k])
    ap, ao = pe.argmin, oe.argmin()
    assert ap["eval"] == ao["eval"] and ap["lambda1"] == ao["lambda1"] and ap["matching"] == ao["matching"], tag
    assert np.array_equal(np.array(ap["state"].adj, np.uint64).view(np.uint8), ao["parents"]), tag
    assert np.array_equal(np.array(pe.mask(ap["state"].slots), np.uint64), ao["permitted"]), tag


import pytest  # noqa: E402


@pytest.mark.parametrize("n,B,p,kmin,kmax,tol,steps,seed,every", [
    (8, 12, 0.4, 2, 10, ([6, 3], 2), 40, 5, 1),             # the shapes of tests/test_gpu_dense.py
    (20, 24, 0.2, 5, 60, ([50, 20, 10], 5), 120, 2, 30),
])
def test_c21_mode_reproduces_the_oracle_engine(orc, n, B, p, kmin, kmax, tol, steps, seed, every):
    """The Python dense engine with lambda_1 and the matching number taken from the oracle library's primitives == orc.Engine(dense=True)
    bit for bit over two epochs with the root policy: trees, state vectors, agent states, counters, observations, argmin."""
    A = n * (n - 1)
    roots = orc.gen_dense_roots(seed, 0, 0, B, n, kmin, kmax, p)
    roots = (roots[0].view(np.uint8).reshape(B, 8 * n), roots[1])
    pe = R.PyDenseEngine(n, B, cost="c21", p=0.2)
    oe = orc.Engine(n, B, threads=4, dense=True, dense_p=0.2)
    call = 0
    for eng in (pe, oe):
        eng.new_begin(*roots)
        eng.new_end(orc.hash_predictions(seed, 0, B, A, call))
    _compare_c21(pe, oe, B, "par_new")
    for epoch in range(2):
        for s in range(1, steps + 1):
            call += 1
            h = orc.hash_predictions(seed, 0, B, A, call)
            imp = []
            for eng in (pe, oe):
                eng.rollout_begin(*tol)
                imp.append(eng.rollout_end(h))
            assert imp[0] == imp[1], (epoch, s)
            if s % every == 0:
                _compare_c21(pe, oe, B, f"epoch {epoch} step {s}")
        (op, wp), (oo, wo) = pe.observe(2), oe.observe(2)
        assert np.array_equal(op.view(np.uint32), oo.view(np.uint32)) and np.array_equal(wp, wo)
        rp, ro = pe.modify_roots(seed, epoch, 0, kmin, kmax), oe.modify_roots(seed, epoch, 0, kmin, kmax)
        assert np.array_equal(rp[0], ro[0]) and np.array_equal(rp[1], ro[1]), epoch
        call += 1
        for eng in (pe, oe):
            eng.reset_begin(*ro)
            eng.reset_end(orc.hash_predictions(seed, 0, B, A, call))
        _compare_c21(pe, oe, B, f"epoch {epoch} reset")
    assert pe.counters()["TRANSPOSITIONS"] > 0 and pe.counters()["EXPANSIONS"] > 100
