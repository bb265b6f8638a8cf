"""The spectrum invariant cost's Python reference (tests/dense_invs_ref.py) on the CPU:
  1. the whole spectrum of all four matrices against numpy.linalg.eigvalsh -- every eigenvalue within the project's per-eigenvalue
     bound 64 n 2^-53 ||M||_F, every energy within n times that bound -- on the 560 graphs of tests/dense_ah_ref.py and on a
     fixed-seed sample of 360 of the hard spectral cases (tests/dense_spectral_cases.py: rank-deficient adjacency matrices), every
     value finite; the vectorised form of the procedure against its scalar definition as bits;
  2. closed forms at n = 4, 5, 19, 32 to the same bounds: K_n, the star, K_{a,b}, C_n;
  3. the combination: two operations per weight, three per pair term, in order, as bits; the converted INVX recipes give
     dense_invx_ref.invx_cost bit for bit on the whole set; PyDenseInvsEngine under a converted recipe grows PyDenseInvxEngine's
     trees."""
import math

import numpy as np

import dense_ah_ref as A
import dense_invs_ref as R
import dense_invx_ref as X
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
    R.prime(entries)
    worst_eig, worst_energy, values = (0.0, None), (0.0, None), 0
    for name, n, adj in entries:
        mats = {k: np.array(m, np.float64) for k, m in S.matrices(adj, n).items()}
        s = sum(X.degrees(adj)) / n
        r = R.invs_cost(adj, n, ALL5)
        assert r["computed"] == 0xFF | 0x1F0000, name
        for which in R.WHICH:
            lapack = np.linalg.eigvalsh(mats[which])  # ascending
            th = np.array(R.spectrum(adj, n, which))
            assert np.all(np.isfinite(th)) and np.all(np.diff(th) >= 0.0), (name, which)
            tol = eig_bound(mats[which], n)
            err = np.abs(th - lapack).max()
            assert err <= tol, (name, which, err / tol)
            worst_eig = max(worst_eig, (err / tol, (name, which)), key=lambda w: w[0])
            shifted = lapack - s if which in ("lap", "slap") else lapack
            want = math.fsum(abs(x) for x in shifted)
            got = r[ENERGY_OF[which]]
            assert math.isfinite(got) and got > 0.0, (name, which)
            e_err = abs(got - want)
            assert e_err <= n * tol, (name, which, e_err / (n * tol))
            worst_energy = max(worst_energy, (e_err / (n * tol), (name, which)), key=lambda w: w[0])
            values += n
        lap_a = np.linalg.eigvalsh(mats["adj"])
        assert abs(r["adj_spread"] - (lap_a[-1] - lap_a[0])) <= 2 * eig_bound(mats["adj"], n), name
        assert r["adj_spread"] > 0.0
    return values, worst_eig, worst_energy


def test_whole_spectrum_against_lapack_on_the_whole_set():
    entries = A.graph_set()
    assert len(entries) == 560  # no graph is skipped
    values, we, wn = check_against_lapack(entries)
    print("whole spectrum vs eigvalsh over %d eigenvalues: largest error / bound %.4f at %s; energies: %.4f at %s" % (values, *we, *wn))


def test_whole_spectrum_against_lapack_on_a_sample_of_the_hard_spectral_cases():
    """360 of the hard cases, drawn with a fixed seed over every size (the rank-deficient brooms at n = 20 .. 32 among them)"""
    full = S.graph_set()
    pick = np.random.default_rng(20261021).choice(len(full), size=360, replace=False)
    entries = [full[i] for i in sorted(pick)]
    assert len(entries) >= 300 and {e[1] for e in entries} >= set(S.NARROW_NS)
    values, we, wn = check_against_lapack(entries)
    print("hard cases, %d eigenvalues: largest error / bound %.4f at %s; energies: %.4f at %s" % (values, *we, *wn))


def test_the_vectorised_procedure_is_the_scalar_definition_as_bits():
    picks = [e for e in A.graph_set()[::40]] + [e for e in S.graph_set() if e[1] in (21, 32)][::150]
    assert len(picks) >= 20
    for name, n, adj in picks:
        adj = tuple(int(a) for a in adj)
        for which in R.WHICH:
            diag, sub = R.I._tridiagonal(adj, n, which)
            want = R.whole_spectrum_scalar(diag, sub, n)
            assert np.array(R.spectrum(adj, n, which)).tobytes() == np.array(want).tobytes(), (name, which)


def test_closed_forms():
    def tols(adj, n):
        return {k: eig_bound(np.array(m, np.float64), n) for k, m in S.matrices(adj, n).items()}

    for n in (4, 5, 19, 32):
        # K_n: A has n - 1 and -1 (n - 1 times); D = A; L has n (n - 1 times) and 0, s = n - 1: all three energies 2 (n - 1); spread n.
        # The eigenvalue of multiplicity n - 1 exercises the `c <= l` rule and the TINY pivot guard.
        adj = A.complete(n)
        r, t = R.invs_cost(adj, n, ALL5), tols(adj, n)
        for which in ("adj", "dist", "lap"):
            assert abs(r[ENERGY_OF[which]] - 2 * (n - 1)) <= n * t[which], (n, which)
        assert abs(r["slap_energy"] - 2 * (n - 1)) <= n * t["slap"]  # Q: 2 n - 2, n - 2 (n - 1 times); s = n - 1
        assert abs(r["adj_spread"] - n) <= 2 * t["adj"]
        th = R.spectrum(adj, n, "adj")
        assert all(abs(x + 1.0) <= t["adj"] for x in th[:-1]) and abs(th[-1] - (n - 1)) <= t["adj"]
        # star: A has +-sqrt(n - 1) and 0 (n - 2 times)
        adj = A.star(n)
        r, t = R.invs_cost(adj, n, ALL5), tols(adj, n)
        assert abs(r["adj_energy"] - 2 * math.sqrt(n - 1)) <= n * t["adj"] and abs(r["adj_spread"] - 2 * math.sqrt(n - 1)) <= 2 * t["adj"]
        th = R.spectrum(adj, n, "adj")
        assert all(abs(x) <= t["adj"] for x in th[1:-1])
        # K_{a,b}: +-sqrt(a b), 0 otherwise
        for a in sorted({1, 2, n // 2}):
            b = n - a
            adj = S.multipartite([a, b])
            r, t = R.invs_cost(adj, n, ALL5), tols(adj, n)
            assert abs(r["adj_energy"] - 2 * math.sqrt(a * b)) <= n * t["adj"], (n, a)
            assert abs(r["adj_spread"] - 2 * math.sqrt(a * b)) <= 2 * t["adj"], (n, a)
        # C_n: 2 cos(2 pi k / n); L - 2 I = -A and Q - 2 I = A, so the Laplacian energies are the graph energy
        adj = A.cycle(n)
        r, t = R.invs_cost(adj, n, ALL5), tols(adj, n)
        want = math.fsum(abs(2 * math.cos(2 * math.pi * k / n)) for k in range(n))
        assert abs(r["adj_energy"] - want) <= n * t["adj"], n
        assert abs(r["lap_energy"] - want) <= n * t["lap"] and abs(r["slap_energy"] - want) <= n * t["slap"], n


def test_the_combination_is_two_operations_per_weight_and_three_per_term_in_order():
    n, adj = 9, A.double_broom(9, 2, 3)
    recipe = R.Recipe({"edges": 0.1, "proximity": 1 / 3, "lap_eig": -0.7, "randic": 1e-3, "adj_energy": 1 / 7, "slap_energy": -0.3, "adj_spread": 3.0},
                      terms=[(0.3, "remoteness", "/", "lap_energy"), (-1 / 7, "dist_energy", "*", "avg_distance")], bias=0.3, lap_index=n - 2, slap_index=1,
                      eval_offset=1.5, eval_scale=0.01)
    r = R.invs_cost(adj, n, recipe)
    c = 0.3
    for name in ("edges", "proximity", "lap_eig", "randic", "adj_energy", "slap_energy", "adj_spread"):
        c = c + recipe.weights()[name] * r[name]
    v = r["remoteness"] / r["lap_energy"]
    c = c + 0.3 * v
    v = r["dist_energy"] * r["avg_distance"]
    c = c + (-1 / 7) * v
    assert r["cost"].view(np.uint32) == np.float32(c).view(np.uint32)
    assert r["eval"].view(np.uint32) == (np.float32(0.01) * (np.float32(c) + np.float32(1.5))).view(np.uint32)
    # named by a pair term alone: computed, bit set (lap_energy, dist_energy); neither weighted nor named: 0.0, bit clear
    assert r["computed"] == 0xFF | 1 << 10 | 1 << 12 | 0x1F0000
    assert r["lap_energy"] > 0.0 and r["dist_energy"] > 0.0 and r["adj_eig"] == 0.0 and r["dist_eig"] == 0.0 and r["slap_eig"] == 0.0
    # an energy needed with its *_eig not needed, and the reverse
    e = R.invs_cost(adj, n, R.Recipe({"lap_energy": 1.0}, lap_index=n - 2))
    assert e["computed"] == 0xFF | 1 << 18 and e["lap_eig"] == 0.0 and bits(e["lap_energy"]) == bits(r["lap_energy"])
    e = R.invs_cost(adj, n, R.Recipe({"lap_eig": 1.0}, lap_index=n - 2))
    assert e["computed"] == 0xFF | 1 << 10 and e["lap_energy"] == 0.0 and bits(e["lap_eig"]) == bits(r["lap_eig"])
    # a term whose coefficient is zero asks for nothing and adds nothing
    q = R.invs_cost(adj, n, R.Recipe({"edges": 1.0}, terms=[(0.0, "adj_energy", "*", "adj_spread")]))
    assert q["computed"] == 0xFF and q["cost"] == r["edges"]


def test_the_converted_invx_recipes_give_the_invx_cost_bit_for_bit():
    seen = 0
    for name, n, adj in A.graph_set():
        for rname, mk in X.RECIPES.items():
            s, x = R.invs_cost(adj, n, R.RECIPES[rname](n)), X.invx_cost(adj, n, mk(n))
            assert all(bits(s[k]) == bits(x[k]) for k in X.NAMES), (name, n, rname)
            assert all(bits(s[k]) == bits(0.0) for k in R.NAMES[16:]), (name, n, rname)
            assert (s["dist_k"], s["computed"]) == (x["dist_k"], x["computed"]), (name, n, rname)
            assert s["cost"].view(np.uint32) == x["cost"].view(np.uint32) and s["eval"].view(np.uint32) == x["eval"].view(np.uint32), (name, n, rname)
            seen += 1
    assert seen == 9 * 560


def test_the_recipes_keep_the_evals_inside_the_unit_interval():
    """the offsets and scales of the named recipes (the GPU runs assert the same on the states they meet)"""
    entries = A.graph_set()[::7]
    R.prime(entries)
    for name, n, adj in entries:
        for rname in R.NEW_RECIPES:
            ev = float(R.invs_cost(adj, n, R.RECIPES[rname](n))["eval"])
            assert 0.0 <= ev <= 1.0, (name, n, rname, ev)


def test_the_converted_all4_recipe_engine_reproduces_the_invx_engine(orc):
    """PyDenseInvsEngine under converted ALL4 == PyDenseInvxEngine under ALL4, tree for tree: N = 8, 12 agents, 30 calls, 2 epochs"""
    n, B, p, kmin, kmax, tol, steps, seed = 8, 12, 0.4, 2, 10, ([6, 3], 2), 30, 5
    acts = n * (n - 1)
    roots = orc.gen_dense_roots(seed, 0, 0, B, n, kmin, kmax, p)
    roots = (roots[0].view(np.uint8).reshape(B, 8 * n), roots[1])
    engines = (R.PyDenseInvsEngine(n, B, R.RECIPES["ALL4"](n), p=p), X.PyDenseInvxEngine(n, B, X.recipe_all4(n), p=p))

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
    assert c["EXPANSIONS"] > 100 and c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0, c
