"""The Python reference of the spectrum invariant cost up to 64 vertices (tests/dense_invs_wide_ref.py) on the CPU:
  1. the whole spectrum of all four matrices against numpy.linalg.eigvalsh on the 88 graphs of dense_ah_wide_ref.graph_set_wide()
     (n = 33 .. 64) and on the hard spectral cases at n = 33 and n = 64 -- every eigenvalue within the project's per-eigenvalue bound
     64 n 2^-53 ||M||_F, every energy within n times that bound, the spread within twice it, every value finite: the bounds of
     tests/test_dense_invs_reference.py;
  2. closed forms beyond 32 vertices to the same bounds: K_33, K_64, the star, K_{a,b} and C_n at n = 33 and 64;
  3. under INVX's recipes, converted, the cost is dense_invx_wide_ref.invx_cost's, bit for bit;
  4. at n <= 32 the wide reference is the narrow one, bit for bit; the named recipes keep the evals inside the unit interval."""
import math

import numpy as np

import dense_ah_ref as A
import dense_invs_ref as R
import dense_invs_wide_ref as W
import dense_invx_ref as X
import dense_invx_wide_ref as XW
import dense_spectral_cases as S

ENERGY_OF = dict(adj="adj_energy", dist="dist_energy", lap="lap_energy", slap="slap_energy")
ALL5 = R.Recipe({k: 1.0 for k in R.NAMES[16:]})


def bits(x):
    return np.float64(x).view(np.uint64)


def eig_bound(m, n):
    """the project's per-eigenvalue bound (tests/test_dense_ah_reference.py): 64 n 2^-53 ||M||_F"""
    return 64.0 * n * 2.0 ** -53 * np.linalg.norm(m)


def check_against_lapack(entries):
    """-> (values checked, largest eigenvalue error / bound, largest energy error / bound)"""
    W.prime_graphs(entries)
    worst_eig, worst_energy, values = (0.0, None), (0.0, None), 0
    for name, n, adj in entries:
        mats = {k: np.array(m, np.float64) for k, m in S.matrices(adj, n).items()}
        s = sum(X.degrees(adj)) / n
        r = W.invs_cost(adj, n, ALL5)
        assert r["computed"] == 0xFF | 0x1F0000, name
        for which in R.WHICH:
            lapack = np.linalg.eigvalsh(mats[which])  # ascending
            th = np.array(W.spectrum(adj, n, which))
            assert len(th) == n and np.all(np.isfinite(th)) and np.all(np.diff(th) >= 0.0), (name, which)
            tol = eig_bound(mats[which], n)
            err = np.abs(th - lapack).max()
            assert err <= tol, (name, n, which, err / tol)
            worst_eig = max(worst_eig, (err / tol, (name, n, which)), key=lambda w: w[0])
            shifted = lapack - s if which in ("lap", "slap") else lapack
            want = math.fsum(abs(x) for x in shifted)
            got = r[ENERGY_OF[which]]
            assert math.isfinite(got) and got > 0.0, (name, which)
            e_err = abs(got - want)
            assert e_err <= n * tol, (name, n, which, e_err / (n * tol))
            worst_energy = max(worst_energy, (e_err / (n * tol), (name, n, which)), key=lambda w: w[0])
            values += n
        lap_a = np.linalg.eigvalsh(mats["adj"])
        assert abs(r["adj_spread"] - (lap_a[-1] - lap_a[0])) <= 2 * eig_bound(mats["adj"], n), name
        assert r["adj_spread"] > 0.0
    return values, worst_eig, worst_energy


def test_whole_spectrum_against_lapack_on_the_wide_set():
    entries = W.graph_set_wide()
    assert len(entries) == 88 and {33, 64} <= {e[1] for e in entries} <= set(range(33, 65))  # no graph is skipped
    values, we, wn = check_against_lapack(entries)
    print("whole spectrum vs eigvalsh, n = 33 .. 64, %d eigenvalues: largest error / bound %.4f at %s; energies: %.4f at %s" % (values, *we, *wn))


def test_whole_spectrum_against_lapack_on_the_hard_spectral_cases_at_33_and_64():
    """every eighth of the hard cases at n = 33 and n = 64 (the rank-deficient adjacency matrices among them)"""
    full = [e for e in S.graph_set_wide() if e[1] in (33, 64)]
    entries = full[::8]
    assert len(entries) >= 40 and {e[1] for e in entries} == {33, 64}
    values, we, wn = check_against_lapack(entries)
    print("hard cases at n = 33, 64, %d eigenvalues: largest error / bound %.4f at %s; energies: %.4f at %s" % (values, *we, *wn))


def test_the_vectorised_procedure_is_the_scalar_definition_as_bits_at_64_rows():
    for name, n, adj in (W.graph_set_wide()[0], W.graph_set_wide()[-1]):
        adj = tuple(int(a) for a in adj)
        for which in R.WHICH:
            diag, sub = R.I._tridiagonal(adj, n, which)
            want = R.whole_spectrum_scalar(diag, sub, n)
            assert np.array(W.spectrum(adj, n, which)).tobytes() == np.array(want).tobytes(), (name, n, which)


def test_closed_forms_beyond_32_vertices():
    def tols(adj, n):
        return {k: eig_bound(np.array(m, np.float64), n) for k, m in S.matrices(adj, n).items()}

    for n in (33, 64):
        # K_n: A has n - 1 and -1 (n - 1 times); D = A; L has n (n - 1 times) and 0, s = n - 1: all energies 2 (n - 1); spread n
        adj = A.complete(n)
        r, t = W.invs_cost(adj, n, ALL5), tols(adj, n)
        for which in ("adj", "dist", "lap", "slap"):
            assert abs(r[ENERGY_OF[which]] - 2 * (n - 1)) <= n * t[which], (n, which)
        assert abs(r["adj_spread"] - n) <= 2 * t["adj"]
        th = W.spectrum(adj, n, "adj")
        assert len(th) == n and all(abs(x + 1.0) <= t["adj"] for x in th[:-1]) and abs(th[-1] - (n - 1)) <= t["adj"]
        # star: A has +-sqrt(n - 1) and 0 (n - 2 times)
        adj = A.star(n)
        r, t = W.invs_cost(adj, n, ALL5), tols(adj, n)
        assert abs(r["adj_energy"] - 2 * math.sqrt(n - 1)) <= n * t["adj"] and abs(r["adj_spread"] - 2 * math.sqrt(n - 1)) <= 2 * t["adj"]
        th = W.spectrum(adj, n, "adj")
        assert all(abs(x) <= t["adj"] for x in th[1:-1])
        # K_{a,b}: +-sqrt(a b), 0 otherwise
        for a in sorted({1, 2, n // 2}):
            b = n - a
            adj = S.multipartite([a, b])
            r, t = W.invs_cost(adj, n, ALL5), tols(adj, n)
            assert abs(r["adj_energy"] - 2 * math.sqrt(a * b)) <= n * t["adj"], (n, a)
            assert abs(r["adj_spread"] - 2 * math.sqrt(a * b)) <= 2 * t["adj"], (n, a)
        # C_n: 2 cos(2 pi k / n); L - 2 I = -A and Q - 2 I = A, so the Laplacian energies are the graph energy
        adj = A.cycle(n)
        r, t = W.invs_cost(adj, n, ALL5), tols(adj, n)
        want = math.fsum(abs(2 * math.cos(2 * math.pi * k / n)) for k in range(n))
        assert abs(r["adj_energy"] - want) <= n * t["adj"], n
        assert abs(r["lap_energy"] - want) <= n * t["lap"] and abs(r["slap_energy"] - want) <= n * t["slap"], n


def test_the_converted_invx_recipes_give_the_invx_wide_cost_bit_for_bit():
    XW.prime_graphs(W.graph_set_wide(), ks_of=lambda n: (0, 1, n // 2, n - 2, n - 1))
    seen = 0
    for name, n, adj in W.graph_set_wide():
        for rname, mk in X.RECIPES.items():
            s, x = W.invs_cost(adj, n, W.RECIPES[rname](n)), XW.invx_cost(adj, n, mk(n))
            assert all(bits(s[k]) == bits(x[k]) for k in X.NAMES), (name, n, rname)
            assert all(bits(s[k]) == bits(0.0) for k in R.NAMES[16:]), (name, n, rname)
            assert (s["dist_k"], s["computed"]) == (x["dist_k"], x["computed"]), (name, n, rname)
            assert s["cost"].view(np.uint32) == x["cost"].view(np.uint32) and s["eval"].view(np.uint32) == x["eval"].view(np.uint32), (name, n, rname)
            seen += 1
    assert seen == 9 * 88


def test_up_to_32_vertices_the_wide_reference_is_the_narrow_one():
    entries = A.graph_set()[::5]
    R.prime(entries)
    seen = 0
    for name, n, adj in entries:
        for rname in R.NEW_RECIPES:
            x, y = W.invs_cost(adj, n, R.RECIPES[rname](n)), R.invs_cost(adj, n, R.RECIPES[rname](n))
            assert all(bits(x[k]) == bits(y[k]) for k in R.NAMES) and (x["dist_k"], x["computed"]) == (y["dist_k"], y["computed"]), (name, n, rname)
            assert x["cost"].view(np.uint32) == y["cost"].view(np.uint32) and x["eval"].view(np.uint32) == y["eval"].view(np.uint32), (name, n, rname)
            seen += 1
    assert seen == 5 * 112


def test_the_recipes_keep_the_evals_inside_the_unit_interval_beyond_32_vertices():
    """the offsets and scales of the named recipes at n = 33 .. 64 (the GPU runs assert the same on the states they meet)"""
    entries = W.graph_set_wide()
    W.prime_graphs(entries)
    for name, n, adj in entries:
        for rname in R.NEW_RECIPES:
            ev = float(W.invs_cost(adj, n, R.RECIPES[rname](n))["eval"])
            assert 0.0 <= ev <= 1.0, (name, n, rname, ev)
