"""The Aouchiche-Hansen cost's Python restatement (tests/dense_ah_ref.py's primitives, through tests/dense_ah_wide_ref.py) at
33 .. 64 vertices, on the CPU, against numpy.linalg.eigvalsh on the 88 graphs of graph_set_wide():
  * |eigenvalue - eigvalsh| <= 64 n 2^-53 ||D||_F per graph -- the bound tests/test_dense_ah_reference.py uses up to 32 vertices
    (the backward-error form: LAPACK promises no more than a small multiple of n eps ||D||).  The procedure is unchanged: 11
    rounds, the 2^-512 pivot floor, the Gershgorin bracket.  The largest ratio and its graph are printed
    (profiles/r11_dense_ah_wide.txt records them);
  * the f32 cost differs from the one formed with LAPACK's eigenvalue only on complete graphs (true cost 0: a sum that cancels,
    so the last bits of the eigenvalue are all the f32 sees) -- as on the n <= 32 set."""
import numpy as np

import dense_ah_ref as R
import dense_ah_wide_ref as W


def test_bfs_matches_matrix_powers_of_the_adjacency():
    """distances at 33 .. 64 vertices: d(u, v) = the first power of (A + I) with a non-zero (u, v) entry"""
    for name, n, adj in W.graph_set_wide():
        dist, trans, ecc = R.bfs_all(adj, n)
        M = np.array([[1 if (u == v or (adj[u] >> v) & 1) else 0 for v in range(n)] for u in range(n)], dtype=np.int64)
        want = np.where(np.eye(n, dtype=bool), 0, -1)
        P = np.eye(n, dtype=np.int64)
        for d in range(1, n):
            P = np.minimum(P @ M, 1)
            want[(want < 0) & (P > 0)] = d
        assert (want >= 0).all() and np.array_equal(np.array(dist), want), (name, n)
        assert trans == [int(s) for s in want.sum(1)] and ecc == [int(m) for m in want.max(1)], (name, n)


def test_eigenvalue_against_lapack_up_to_64_vertices():
    worst, worst_at = 0.0, None
    moved = []
    for name, n, adj in W.graph_set_wide():  # no graph is skipped
        r = W.ah_cost(adj, n)
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
        if np.float32(r["proximity"] + ev[r["k"]]) != r["cost"]:
            moved.append((name, n))
        assert r["cost"].dtype == np.float32 and r["eval"].dtype == np.float32
        assert r["eval"] == np.float32(1.0) / np.float32(2 * n + 2) * (r["cost"] + np.float32(2.0))
    print("AH eigenvalue vs eigvalsh, n = 33 .. 64: largest error / tolerance = %.4f at %s; f32 cost differs from LAPACK's on %d of %d graphs: %s"
          % (worst, worst_at, len(moved), len(W.graph_set_wide()), moved))
    assert all(name == "complete" for name, _ in moved), moved
