"""The weighted-invariant cost's Python reference (tests/dense_inv_ref.py) on the CPU:
  1. the integer invariants against Floyd-Warshall and plain degree counts on the whole graph set of tests/dense_ah_ref.py (560
     connected graphs, n = 4 .. 32; no graph is skipped);
  2. adj_eig at descending indices {0, 1, n // 2, n - 2, n - 1} and dist_eig at {0, 1, n - 1, the AH rule} against
     numpy.linalg.eigvalsh, within the project's own bound 64 n 2^-53 ||M||_F (tests/test_dense_ah_reference.py);
  3. the AH recipe == dense_ah_ref.ah_cost bit for bit on the whole set;
  4. closed forms (K_n, star, path, cycle) for every invariant;
  5. PyDenseInvEngine under the AH recipe grows PyDenseEngine(cost="ah")'s trees."""
import math

import numpy as np

import dense_ah_ref as A
import dense_inv_ref as R


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


ONLY = lambda name, **kw: R.Recipe({name: 1.0}, **kw)  # noqa: E731


def bits(x):
    return np.float64(x).view(np.uint64)


def test_integer_invariants_against_floyd_warshall_and_degree_counts():
    seen = 0
    for name, n, adj in A.graph_set():
        r = R.inv_cost(adj, n, R.recipe_int(n))
        fw = floyd_warshall(adj, n)
        deg = [sum((adj[u] >> v) & 1 for v in range(n)) for u in range(n)]
        trans, ecc = [sum(row) for row in fw], [max(row) for row in fw]
        assert r["edges"] == sum(deg) / 2 and r["max_degree"] == max(deg) and r["min_degree"] == min(deg), (name, n)
        assert r["diameter"] == max(ecc) and r["radius"] == min(ecc), (name, n)
        assert r["proximity"] == min(trans) / (n - 1) and r["remoteness"] == max(trans) / (n - 1), (name, n)
        assert r["avg_distance"] == sum(trans) / (n * (n - 1)), (name, n)
        assert r["computed"] == 0xFF and r["adj_eig"] == 0.0 and r["dist_eig"] == 0.0, (name, n)
        seen += 1
    assert seen == 560


def test_eigenvalues_against_lapack_on_the_whole_set():
    worst = {"adj": (0.0, None), "dist": (0.0, None)}
    values = 0
    for name, n, adj in A.graph_set():  # no graph is skipped
        dist, _, ecc = A.bfs_all(adj, n)
        mats = {"adj": np.array(R.adjacency_matrix(adj, n), np.float64), "dist": np.array(dist, np.float64)}
        lap = {k: np.linalg.eigvalsh(m)[::-1] for k, m in mats.items()}
        for k in sorted({0, 1, n // 2, n - 2, n - 1}):
            got = R.inv_cost(adj, n, ONLY("adj_eig", adj_index=k))
            assert got["computed"] == 0xFF | 1 << 8 and got["dist_eig"] == 0.0
            tol = 64.0 * n * 2.0 ** -53 * np.linalg.norm(mats["adj"])
            err = abs(got["adj_eig"] - lap["adj"][k])
            assert err <= tol, (name, n, "adj", k, got["adj_eig"], lap["adj"][k], err / tol)
            worst["adj"] = max(worst["adj"], (err / tol, (name, n, k)))
            values += 1
        for k in sorted({0, 1, n - 1, R.INDEX_AH}):
            got = R.inv_cost(adj, n, ONLY("dist_eig", dist_index=k))
            kk = A.ah_index(max(ecc), n) if k == R.INDEX_AH else k
            assert got["dist_k"] == kk and got["computed"] == 0xFF | 1 << 9 and got["adj_eig"] == 0.0
            tol = 64.0 * n * 2.0 ** -53 * np.linalg.norm(mats["dist"])
            err = abs(got["dist_eig"] - lap["dist"][kk])
            assert err <= tol, (name, n, "dist", k, got["dist_eig"], lap["dist"][kk], err / tol)
            worst["dist"] = max(worst["dist"], (err / tol, (name, n, k)))
            values += 1
    print("invariant cost vs eigvalsh over %d values: largest error / tolerance: adjacency %.4f at %s, distance %.4f at %s"
          % (values, *worst["adj"], *worst["dist"]))
    assert values > 4000


def test_the_ah_recipe_is_the_ah_cost_bit_for_bit():
    for name, n, adj in A.graph_set():
        r, a = R.inv_cost(adj, n, R.recipe_ah(n)), A.ah_cost(adj, n)
        assert bits(r["proximity"]) == bits(a["proximity"]) and bits(r["dist_eig"]) == bits(a["eigenvalue"]), (name, n)
        assert (r["diameter"], r["dist_k"]) == (a["diameter"], a["k"]) and r["computed"] == 0xFF | 1 << 9, (name, n)
        assert r["cost"].view(np.uint32) == a["cost"].view(np.uint32) and r["eval"].view(np.uint32) == a["eval"].view(np.uint32), (name, n)


def test_closed_forms():
    for n in (4, 5, 8, 13, 20, 31, 32):
        both = lambda ai, di: R.Recipe({"adj_eig": 1.0, "dist_eig": 1.0}, adj_index=ai, dist_index=di)  # noqa: E731
        # K_n: adjacency spectrum n - 1, -1 (n - 1 times); the distance matrix is the adjacency matrix
        r = R.inv_cost(A.complete(n), n, both(0, n - 1))
        assert [r[k] for k in R.NAMES[:8]] == [n * (n - 1) / 2, n - 1, n - 1, 1, 1, 1.0, 1.0, 1.0]
        assert abs(r["adj_eig"] - (n - 1)) <= 1e-9 and abs(r["dist_eig"] + 1) <= 1e-9
        assert abs(R.inv_cost(A.complete(n), n, both(n // 2, 0))["adj_eig"] + 1) <= 1e-9  # the repeated eigenvalue, by index
        # star: adjacency +-sqrt(n - 1) and zeros; distance n - 2 +- sqrt(n^2 - 3 n + 3), then -2 (n - 2 times) at the bottom
        r = R.inv_cost(A.star(n), n, both(0, 0))
        assert [r[k] for k in R.NAMES[:5]] == [n - 1, n - 1, 1, 2, 1]
        assert r["proximity"] == 1.0 and r["remoteness"] == (2 * n - 3) / (n - 1) and r["avg_distance"] == (2 * (n - 1) * (n - 1)) / (n * (n - 1))
        assert abs(r["adj_eig"] - math.sqrt(n - 1)) <= 1e-9 and abs(r["dist_eig"] - (n - 2 + math.sqrt(n * n - 3 * n + 3))) <= 1e-9
        r = R.inv_cost(A.star(n), n, both(n - 1, n - 1))
        assert abs(r["adj_eig"] + math.sqrt(n - 1)) <= 1e-9 and abs(r["dist_eig"] + 2) <= 1e-9
        assert abs(R.inv_cost(A.star(n), n, both(0, 1))["dist_eig"] - (n - 2 - math.sqrt(n * n - 3 * n + 3))) <= 1e-9
        assert abs(R.inv_cost(A.star(n), n, both(n // 2, n - 1))["adj_eig"]) <= 1e-9
        # path: adjacency 2 cos(pi j / (n + 1)); transmissions n (n - 1) / 2 at the ends
        r = R.inv_cost(A.path(n), n, both(0, 0))
        assert [r[k] for k in R.NAMES[:5]] == [n - 1, 2, 1, n - 1, n // 2]
        assert r["remoteness"] == (n * (n - 1) / 2) / (n - 1) and r["proximity"] == ((n * n) // 4) / (n - 1)
        assert r["avg_distance"] == ((n - 1) * n * (n + 1) // 3) / (n * (n - 1))
        assert abs(r["adj_eig"] - 2 * math.cos(math.pi / (n + 1))) <= 1e-9
        assert abs(R.inv_cost(A.path(n), n, both(n - 1, 0))["adj_eig"] + 2 * math.cos(math.pi / (n + 1))) <= 1e-9
        # cycle: 2-regular, adjacency 2 cos(2 pi j / n), every transmission floor(n^2 / 4)
        r = R.inv_cost(A.cycle(n), n, both(1, 0))
        assert [r[k] for k in R.NAMES[:5]] == [n, 2, 2, n // 2, n // 2]
        t = (n * n) // 4
        assert r["proximity"] == r["remoteness"] == t / (n - 1) and r["avg_distance"] == (n * t) / (n * (n - 1))
        assert abs(r["adj_eig"] - 2 * math.cos(2 * math.pi / n)) <= 1e-9 and abs(r["dist_eig"] - t) <= 1e-9
        assert abs(R.inv_cost(A.cycle(n), n, both(0, 0))["adj_eig"] - 2) <= 1e-9


def test_the_combination_is_two_operations_in_index_order():
    """weights whose products round: the sum is taken term by term in index order, each product rounded first"""
    n, adj = 9, A.double_broom(9, 2, 3)
    recipe = R.Recipe({"edges": 0.1, "proximity": 1 / 3, "avg_distance": -0.7, "adj_eig": 1e-3, "dist_eig": 3.0}, bias=0.3, adj_index=2, dist_index=1,
                      eval_offset=1.5, eval_scale=0.01)
    r = R.inv_cost(adj, n, recipe)
    c = 0.3
    for name in ("edges", "proximity", "avg_distance", "adj_eig", "dist_eig"):
        c = c + recipe.weights()[name] * r[name]
    assert r["cost"].view(np.uint32) == np.float32(c).view(np.uint32)
    assert r["eval"].view(np.uint32) == (np.float32(0.01) * (np.float32(c) + np.float32(1.5))).view(np.uint32)


def test_the_ah_recipe_engine_reproduces_the_ah_engine(orc):
    """PyDenseInvEngine under the AH recipe == PyDenseEngine(cost="ah"), tree for tree: N = 8, 12 agents, 40 calls, 2 epochs"""
    n, B, p, kmin, kmax, tol, steps, seed = 8, 12, 0.4, 2, 10, ([6, 3], 2), 40, 5
    acts = n * (n - 1)
    roots = orc.gen_dense_roots(seed, 0, 0, B, n, kmin, kmax, p)
    roots = (roots[0].view(np.uint8).reshape(B, 8 * n), roots[1])
    engines = (R.PyDenseInvEngine(n, B, R.recipe_ah(n), p=p), A.PyDenseEngine(n, B, cost="ah", p=p))

    def same(tag):
        e0, e1 = engines
        assert np.array_equal(e0.state_vecs().view(np.uint32), e1.state_vecs().view(np.uint32)), tag
        for i in range(B):
            t0, t1 = e0.export_tree(i), e1.export_tree(i)
            for f in t1.FIELDS:
                x, y = getattr(t0, f), getattr(t1, f)
                assert x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype.kind == "f" else x, y.view(np.uint32) if y.dtype.kind == "f" else y), (tag, i, f)
        assert e0.counters() == e1.counters(), tag
        assert np.float32(e0.argmin["eval"]).view(np.uint32) == np.float32(e1.argmin["eval"]).view(np.uint32), tag

    call = 0
    for e in engines:
        e.new_begin(*roots)
        e.new_end(orc.hash_predictions(seed, 0, B, acts, call))
    same("par_new")
    for epoch in range(2):
        for s in range(steps):
            call += 1
            h = orc.hash_predictions(seed, 0, B, acts, call)
            imp = []
            for e in engines:
                e.rollout_begin(*tol)
                imp.append(e.rollout_end(h))
            assert imp[0] == imp[1], (epoch, s)
            same(f"epoch {epoch} step {s}")
        (o0, w0), (o1, w1) = (e.observe(2) for e in engines)
        assert np.array_equal(o0.view(np.uint32), o1.view(np.uint32)) and np.array_equal(w0, w1)
        r0, r1 = (e.modify_roots(seed, epoch, 0, kmin, kmax) for e in engines)
        assert np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1]), epoch
        call += 1
        for e in engines:
            e.reset_begin(*r0)
            e.reset_end(orc.hash_predictions(seed, 0, B, acts, call))
        same(f"epoch {epoch} reset")
    c = engines[0].counters()
    assert c["EXPANSIONS"] > 100 and c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0 and c["ROOT_EXHAUSTED"] > 0, c
