"""The Python reference of the extended invariant cost up to 64 vertices (tests/dense_invx_wide_ref.py) on the CPU, on the 88 graphs
of dense_ah_wide_ref.graph_set_wide() (n = 33 .. 64) and the complete graphs K_33 .. K_64 (the degree sums' hardest case: every
term of the Randic sum equal); no graph is skipped:
  1. zagreb1, zagreb2 and triangles against plain loops over the edge list;
  2. randic against math.fsum of the same terms within n 2^-52, the bound the invariant was specified with;
  3. lap_eig and slap_eig at descending indices {0, 1, n // 2, n - 2, n - 1} against numpy.linalg.eigvalsh, within the project's own
     bound 64 n 2^-53 ||M||_F, every value finite;
  4. with no new weight and no term the result is dense_inv_wide_ref.inv_cost's, bit for bit;
  5. at n <= 32 the wide reference is the narrow one, bit for bit."""
import math

import numpy as np

import dense_ah_ref as A
import dense_inv_ref as I
import dense_inv_wide_ref as IW
import dense_invx_ref as R
import dense_invx_wide_ref as W

ONLY = lambda name, **kw: R.Recipe({name: 1.0}, **kw)  # noqa: E731
DEGREE_BASED = R.Recipe({"randic": 1.0, "zagreb1": 1.0, "zagreb2": 1.0, "triangles": 1.0})
KS = lambda n: sorted({0, 1, n // 2, n - 2, n - 1})  # noqa: E731


def graphs():
    """the 88 graphs and K_33 .. K_64: 120 entries"""
    out = W.graph_set_wide() + tuple(("K", n, tuple(A.complete(n))) for n in range(33, 65))
    assert len(out) == 120
    return out


def bits(x):
    return np.float64(x).view(np.uint64)


def edge_list(adj, n):
    return [(u, v) for u in range(n) for v in range(u) if (adj[u] >> v) & 1]


def test_integer_degree_invariants_against_plain_loops_over_the_edge_list():
    seen = 0
    for name, n, adj in graphs():
        r = W.invx_cost(adj, n, DEGREE_BASED)
        edges = edge_list(adj, n)
        deg = [sum((adj[u] >> v) & 1 for v in range(n)) for u in range(n)]
        assert r["computed"] == 0xFF | 0xF000 and all(r[k] == 0.0 for k in ("adj_eig", "dist_eig", "lap_eig", "slap_eig")), (name, n)
        assert r["zagreb1"] == sum(d * d for d in deg), (name, n)
        assert r["zagreb2"] == sum(deg[u] * deg[v] for u, v in edges), (name, n)
        nb = [[w for w in range(n) if (adj[u] >> w) & 1] for u in range(n)]
        tri = sum(1 for u, v in edges for w in nb[v] if w < v and (adj[u] >> w) & 1)
        assert r["triangles"] == tri, (name, n, r["triangles"], tri)
        seen += 1
    assert seen == 120


def test_randic_against_fsum_of_the_same_terms_within_n_ulps():
    """The bound n 2^-52 is the invariant's stated one (tests/test_dense_invx_reference.py); the procedure is the narrow tier's, the
    compensated per-vertex sums and the balanced tree.  Measured on these 120 graphs: the largest error is 0.485 x the bound."""
    seen, worst = 0, (0.0, "")
    for name, n, adj in graphs():
        r = W.invx_cost(adj, n, ONLY("randic"))
        deg = [sum((adj[u] >> v) & 1 for v in range(n)) for u in range(n)]
        exact = math.fsum(1.0 / math.sqrt(deg[u] * deg[v]) for u, v in edge_list(adj, n))
        ratio = abs(r["randic"] - exact) / (n * 2.0 ** -52)
        worst = max(worst, (ratio, "%s %d" % (name, n)))
        assert ratio <= 1.0, (name, n, r["randic"], exact, ratio)
        seen += 1
    print("randic vs fsum, n = 33 .. 64: largest error / (n 2^-52) = %.4f at %s" % worst)
    assert seen == 120


def test_laplacian_eigenvalues_against_lapack():
    W.prime_graphs(graphs(), ("lap", "slap"))
    worst = {"lap": (0.0, None), "slap": (0.0, None)}
    values = 0
    for name, n, adj in graphs():
        mats = {"lap": np.array(R.laplacian(adj, n, -1), np.float64), "slap": np.array(R.laplacian(adj, n, 1), np.float64)}
        lapack = {k: np.linalg.eigvalsh(m)[::-1] for k, m in mats.items()}
        for k in KS(n):
            for which, bit in (("lap", 10), ("slap", 11)):
                got = W.invx_cost(adj, n, ONLY(which + "_eig", **{which + "_index": k}))
                assert got["computed"] == 0xFF | 1 << bit, (name, n, which)
                x = got[which + "_eig"]
                assert math.isfinite(x), (name, n, which, k)
                tol = 64.0 * n * 2.0 ** -53 * np.linalg.norm(mats[which])
                err = abs(x - lapack[which][k])
                assert err <= tol, (name, n, which, k, x, lapack[which][k], err / tol)
                worst[which] = max(worst[which], (err / tol, (name, n, k)))
                values += 1
    print("wide extended invariant cost vs eigvalsh over %d values: largest error / tolerance: Laplacian %.4f at %s, signless Laplacian %.4f at %s"
          % (values, *worst["lap"], *worst["slap"]))
    assert values == 120 * 5 * 2


def test_the_numpy_path_gives_the_scalar_reductions_bits():
    """an eigenvalue the caches lack comes from the numpy forms: the same bits as dense_inv_ref's scalar path, on one graph of each
    matrix kind at n = 33 and one at n = 64 (test_dense_spectral_cases.py holds the two forms together on thousands)"""
    for name, n, adj in (W.graph_set_wide()[4], W.graph_set_wide()[-1]):
        for which in ("adj", "dist", "lap", "slap"):
            k = n // 3
            for key in [key for key in I._EIG if key[:3] == (adj, n, which)]:
                del I._EIG[key]
            I._TRI.pop((adj, n, which), None)
            fast = W._eig(adj, n, which, k)
            del I._EIG[(adj, n, which, k)], I._TRI[(adj, n, which)]
            assert bits(I._eig(adj, n, which, k)) == bits(fast), (name, n, which)


def test_without_a_new_weight_or_term_the_cost_is_the_inv_wide_cost_bit_for_bit():
    W.prime_graphs(W.graph_set_wide(), ("adj", "dist"), lambda n: (0, 1, n - 1))
    seen = 0
    for name, n, adj in W.graph_set_wide():
        for rname, mk in I.RECIPES.items():
            x, i = W.invx_cost(adj, n, W.RECIPES[rname](n)), IW.inv_cost(adj, n, mk(n))
            assert all(bits(x[k]) == bits(i[k]) for k in I.NAMES), (name, n, rname)
            assert all(x[k] == 0.0 for k in R.NAMES[10:]), (name, n, rname)
            assert (x["dist_k"], x["computed"]) == (i["dist_k"], i["computed"]), (name, n, rname)
            assert x["cost"].view(np.uint32) == i["cost"].view(np.uint32) and x["eval"].view(np.uint32) == i["eval"].view(np.uint32), (name, n, rname)
            seen += 1
    assert seen == 4 * 88


def test_up_to_32_vertices_the_wide_reference_is_the_narrow_one():
    seen = 0
    for name, n, adj in A.graph_set()[::5]:
        for rname in R.NEW_RECIPES:
            x, y = W.invx_cost(adj, n, R.RECIPES[rname](n)), R.invx_cost(adj, n, R.RECIPES[rname](n))
            assert all(bits(x[k]) == bits(y[k]) for k in R.NAMES) and (x["dist_k"], x["computed"]) == (y["dist_k"], y["computed"]), (name, n, rname)
            assert x["cost"].view(np.uint32) == y["cost"].view(np.uint32) and x["eval"].view(np.uint32) == y["eval"].view(np.uint32), (name, n, rname)
            seen += 1
    assert seen == 5 * 112


def test_the_recipes_keep_the_evals_inside_the_unit_interval():
    """the offsets and scales of the named recipes beyond 32 vertices (the GPU runs assert the same on the states they meet)"""
    W.prime_graphs(W.graph_set_wide()[::4], ks_of=lambda n: (0, 1, n - 2, n - 1))
    for name, n, adj in W.graph_set_wide()[::4]:
        for rname in R.NEW_RECIPES:
            ev = float(W.invx_cost(adj, n, R.RECIPES[rname](n))["eval"])
            assert 0.0 < ev < 1.0, (name, n, rname, ev)
