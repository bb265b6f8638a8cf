"""The invariant costs' Python references (tests/dense_inv_ref.py, dense_invx_ref.py, dense_inv_wide_ref.py) on the hard case set of
the spectral passes (tests/dense_spectral_cases.py), on the CPU:
  1. the set is what its module says: the sizes, every ordered double broom, the multipartite graphs, three labellings, the named
     graphs, the same bitsets on every machine;
  2. the parent-fails list: the entries on which the reduction WITHOUT the deflation rule ends in a non-finite tridiagonal form are
     the ones the module states, there are some, and they reach down to 23 vertices and below -- the set cannot be thinned into
     harmlessness;
  3. with the rule, as the references reduce: every entry of diag and sub is finite, for the adjacency, distance, Laplacian and
     signless-Laplacian matrix of every graph (asserted on the tridiagonal form itself: the final eigenvalue hides a NaN);
  4. eigenvalues at descending indices {0, 1, n // 2, n - 2, n - 1} against numpy.linalg.eigvalsh within the project's own bound
     64 n 2^-53 ||M||_F (tests/test_dense_ah_reference.py), and the cost functions report those values;
  5. dense_ah_ref's forms over many matrices, which fill the references' caches for this set, equal the scalar forms bit for bit.
No case is skipped."""
import hashlib
import math

import numpy as np
import pytest

import dense_ah_ref as A
import dense_inv_ref as R
import dense_inv_wide_ref as W
import dense_invx_ref as X
import dense_spectral_cases as S

KINDS = ("adj", "dist", "lap", "slap")
KIND_NAMES = dict(adj="adjacency", dist="distance", lap="Laplacian", slap="signless Laplacian")


def indices(n):
    return sorted({0, 1, n // 2, n - 2, n - 1})


def finite(diag, sub):
    return all(math.isfinite(z) for z in diag) and all(math.isfinite(z) for z in sub)


def same_bits(xs, ys):
    return np.array_equal(np.array(xs, np.float64).view(np.uint64), np.array(ys, np.float64).view(np.uint64))


@pytest.fixture(scope="module")
def whole_set():
    """both sets with the references' caches filled for all four matrices"""
    entries = S.graph_set() + S.graph_set_wide()
    R.prime(entries, KINDS)
    return entries


def test_the_set_is_what_its_module_says():
    narrow, wide = S.graph_set(), S.graph_set_wide()
    names = {name for name, _, _ in narrow}
    sizes = S.by_size(narrow)
    assert sorted(sizes) == sorted(S.NARROW_NS + (19, 30)) and sorted(S.by_size(wide)) == list(S.WIDE_NS)
    for n in S.NARROW_NS:
        pairs = [(a, b) for a in range(n) for b in range(n) if n - a - b >= 2 and a + b >= n - 8]  # ordered: (a, b) and (b, a)
        assert len(pairs) == 7 * n - 28 and (0, n - 2) in pairs and (n - 2, 0) in pairs
        for lab in S.LABELLINGS:
            assert all("broom(%d,%d)-n%d/%s" % (a, b, n, lab) in names for a, b in pairs), n
            for parts in ([1, 2, n - 3], [2, 3, n - 5], [1, 2, 3, n - 6], [n // 2, (n + 1) // 2], [1, 1, n - 2]):
                assert "K[%s]-n%d/%s" % (",".join(map(str, parts)), n, lab) in names, (n, parts)
            assert "star-n%d/%s" % (n, lab) in names and "complete-n%d/%s" % (n, lab) in names
        assert len([e for e in sizes[n] if not e[0].endswith("/found")]) == 3 * (len(pairs) + 7)
    for n in S.WIDE_NS:
        assert len(S.by_size(wide)[n]) == 3 * (len(S.broom_pairs(n)[::3]) + 7)
    assert {"broom(19,2)-n23/id", "broom(20,1)-n23/id", "broom(14,12)-n30/id", "K[10,11]-n21/found", "K[1,2,19]-n22/found"} <= names
    assert (len(narrow), len(wide)) == (3700, 939)  # a few thousand at most
    for name, n, adj in narrow + wide:
        assert len(adj) == n and A.connected(adj, n), name
    # a relabelling keeps the graph: the degree sequence; and the bitsets are these on every machine
    by_name = {name: adj for name, _, adj in narrow}
    for name in ("broom(19,2)-n23", "K[15,16]-n31", "K[1,2,3,26]-n32"):
        deg = sorted(bin(a).count("1") for a in by_name[name + "/id"])
        assert all(sorted(bin(a).count("1") for a in by_name[name + "/" + lab]) == deg and by_name[name + "/" + lab] != by_name[name + "/id"] for lab in ("p1", "p2"))
    digest = hashlib.sha256(repr(narrow + wide).encode()).hexdigest()
    assert digest[:16] == S.DIGEST, digest


def test_the_parent_fails_list_is_exact_and_reaches_down_to_23_vertices():
    """the reduction as the narrow tiers ran it before: dense_ah_ref.tridiagonalise(M, n), deflate = 0.0"""
    narrow = S.graph_set()
    failing = []
    for n, entries in sorted(S.by_size(narrow).items()):
        diag, sub = A.tridiagonalise_many([R.adjacency_matrix(adj, n) for _, _, adj in entries], n)
        failing += [e[0] for e, ok in zip(entries, np.isfinite(diag).all(axis=1) & np.isfinite(sub).all(axis=1)) if not ok]
    assert sorted(failing) == sorted(S.PARENT_FAILS)
    assert len(S.PARENT_FAILS) > 100 and {"broom(19,2)-n23/id", "broom(20,1)-n23/id", "broom(14,12)-n30/id", "K[10,11]-n21/found"} <= set(S.PARENT_FAILS)
    per_n = {}
    for name in S.PARENT_FAILS:
        n = int(name.split("-n")[1].split("/")[0])
        per_n[n] = per_n.get(n, 0) + 1
    print("non-finite adjacency reductions without the rule, per n:", sorted(per_n.items()))
    assert min(per_n) <= 23 and sum(c for n, c in per_n.items() if n <= 23) >= 4
    # the named ones through the scalar form itself, and what a caller saw: a finite eigenvalue far from LAPACK's
    by_name = {name: (n, adj) for name, n, adj in narrow}
    for name in ("K[9,10]-n19/found", "K[10,11]-n21/found", "K[1,2,19]-n22/found", "broom(19,2)-n23/id", "broom(20,1)-n23/id", "broom(14,12)-n30/id"):
        n, adj = by_name[name]
        assert not finite(*A.tridiagonalise(R.adjacency_matrix(adj, n), n)), name
    n, adj = by_name["broom(14,12)-n30/id"]
    diag, sub = A.tridiagonalise(R.adjacency_matrix(adj, n), n)
    assert finite(diag[:20], sub[:19]) and not any(math.isfinite(z) for z in diag[21:])
    wrong, right = A.kth_eigenvalue(diag, sub, n, 0), np.linalg.eigvalsh(np.array(R.adjacency_matrix(adj, n), np.float64))[-1]
    assert math.isfinite(wrong) and abs(wrong - 5.898) < 1e-3 and abs(right - 3.887) < 1e-3
    assert abs(R.inv_cost(adj, n, R.Recipe({"adj_eig": 1.0}, adj_index=0))["adj_eig"] - right) < 1e-12


def test_every_tridiagonal_form_is_finite(whole_set):
    """zero non-finite entries over the whole set, all four matrix kinds, as the references reduce them"""
    bad, seen = [], 0
    for name, n, adj in whole_set:
        for kind in KINDS:
            diag, sub = R._tridiagonal(adj, n, kind)
            assert len(diag) == len(sub) == n
            if not finite(diag, sub):
                bad.append((name, kind))
            seen += 1
    assert seen == 4 * (3700 + 939)
    assert not bad, (len(bad), bad[:20])


def test_eigenvalues_against_lapack_on_the_whole_set(whole_set):
    worst = {kind: (0.0, None) for kind in KINDS}
    values = 0
    for name, n, adj in whole_set:  # no graph is skipped
        for kind in KINDS:
            m = np.array(R.MATRICES[kind](adj, n), np.float64)
            lapack = np.linalg.eigvalsh(m)[::-1]
            tol = 64.0 * n * 2.0 ** -53 * np.linalg.norm(m)
            for k in indices(n):
                x = R._eig(adj, n, kind, k)
                assert math.isfinite(x), (name, kind, k)
                err = abs(x - lapack[k])
                assert err <= tol, (name, kind, k, x, lapack[k], err / tol)
                worst[kind] = max(worst[kind], (err / tol, (name, k)))
                values += 1
    print("hard spectral cases vs eigvalsh over %d values: largest error / tolerance: " % values
          + ", ".join("%s %.4f at %s" % (KIND_NAMES[kind], *worst[kind]) for kind in KINDS))
    assert values == 5 * 4 * (3700 + 939)


def test_the_cost_functions_report_these_eigenvalues(whole_set):
    """inv_cost, invx_cost and the wide inv_cost under one-eigenvalue recipes: the values held to LAPACK above, bit for bit"""
    seen = 0
    for name, n, adj in whole_set[::5] + tuple(e for e in whole_set if e[0] in S.PARENT_FAILS):
        cost = R.inv_cost if n <= 32 else W.inv_cost
        for k in indices(n):
            got = cost(adj, n, R.Recipe({"adj_eig": 1.0, "dist_eig": 1.0}, adj_index=k, dist_index=k))
            assert got["computed"] == 0x3FF and same_bits([got["adj_eig"], got["dist_eig"]], [R._eig(adj, n, "adj", k), R._eig(adj, n, "dist", k)]), (name, k)
            if n <= 32:
                gx = X.invx_cost(adj, n, X.Recipe({"adj_eig": 1.0, "dist_eig": 1.0, "lap_eig": 1.0, "slap_eig": 1.0}, adj_index=k, dist_index=k, lap_index=k, slap_index=k))
                assert same_bits([gx[key + "_eig"] for key in KINDS], [R._eig(adj, n, kind, k) for kind in KINDS]), (name, k)
            seen += 1
    assert seen > 5000


def test_the_forms_over_many_matrices_equal_the_scalar_forms_bit_for_bit(whole_set):
    """what prime() left in the caches against tridiagonalise and kth_eigenvalue themselves: every 50th entry and every named one,
    all four kinds; and without the rule, NaN for NaN, on the entries the parent fails on"""
    sample = whole_set[::50] + tuple(e for e in whole_set if e[0].endswith("/found") or e[0] in ("broom(19,2)-n23/id", "broom(14,12)-n30/id"))
    for name, n, adj in sample:
        for kind in KINDS:
            diag, sub = A.tridiagonalise(R.MATRICES[kind](adj, n), n, R.INV_DEFLATE)
            held = R._tridiagonal(adj, n, kind)
            assert same_bits(diag, held[0]) and same_bits(sub, held[1]), (name, kind)
            for k in indices(n):
                assert same_bits([A.kth_eigenvalue(diag, sub, n, k)], [R._eig(adj, n, kind, k)]), (name, kind, k)
    by_name = {e[0]: e for e in whole_set}
    for name in S.PARENT_FAILS[::9]:
        _, n, adj = by_name[name]
        m = R.adjacency_matrix(adj, n)
        diag, sub = A.tridiagonalise(m, n)
        many = A.tridiagonalise_many([m, m], n)
        assert np.array_equal(np.isnan(diag), np.isnan(many[0][1])) and np.array_equal(np.isnan(sub), np.isnan(many[1][1])), name
        ok = ~np.isnan(diag)
        assert same_bits(np.array(diag)[ok], many[0][1][ok]), name
        assert same_bits([A.kth_eigenvalue(diag, sub, n, k) for k in indices(n)], A.kth_eigenvalues_many(many[0], many[1], n, indices(n))[1]), name
