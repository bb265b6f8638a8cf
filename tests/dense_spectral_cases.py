"""The hard case set of the invariant costs' spectral passes (dense_inv_ref, dense_invx_ref, dense_inv_wide_ref and the host and
device forms they are held to): connected graphs whose ADJACENCY matrix has few distinct eigenvalues -- double brooms with most
vertices in the two bunches, complete multipartite graphs, the star, K_n -- each as generated and under two seeded relabellings.
On such a matrix the Householder reduction uses the rank up after a few steps and goes on in rounding noise that shrinks by about
2^-53 every other step; without the deflation rule (dense_cost_host.h: DENSE_INV_DEFLATE) the squares reach the subnormals after some
twenty steps and the tridiagonal form ends in NaN, which the multisection turns into a finite, wrong eigenvalue.  Which labelling
a graph comes in decides: a double broom with the lighter bunch first passes, the same broom with the heavier bunch first fails.
Shared by test_dense_spectral_cases.py (the references, CPU), the three test_dense_inv*_abi.py (host functions, CPU) and the
three test_gpu_dense_inv*.py (probe kernels).  Pure Python and numpy, seeded: the same set on every machine.

An entry is (name, n, adj), adj a tuple of n neighbourhood bitsets.  Names: "broom(a,b)-n23", "K[1,2,20]-n23", "star-n23",
"complete-n23", then "/id" (as generated) or "/p1", "/p2" (relabelled)."""
import functools
import zlib

import numpy as np

import dense_ah_ref as A

NARROW_NS = (20, 21, 22, 23, 24, 27, 31, 32)  # around the smallest failures (21 .. 24), one in between, the last two rows
WIDE_NS = (33, 40, 64)                        # the 64-row form's own branch: the first row past 32, one in between, the last
BROOM_SLACK = 8                               # brooms with a + b >= n - 8: a path of at most 8 vertices between the bunches
WIDE_THINNING = 3                             # beyond 32 vertices every third ordered pair (a, b)
LABELLINGS = ("id", "p1", "p2")


def multipartite(parts):
    """the complete multipartite graph, the parts in the order given: vertices 0 .. parts[0] - 1 first"""
    n, lab = sum(parts), []
    for i, p in enumerate(parts):
        assert p >= 1
        lab += [i] * p
    return A.from_edges(n, [(u, v) for u in range(n) for v in range(u) if lab[u] != lab[v]])


def relabel(adj, n, perm):
    """vertex u becomes perm[u]"""
    return A.from_edges(n, [(int(perm[u]), int(perm[v])) for u in range(n) for v in range(u) if (adj[u] >> v) & 1])


def permutation(name):
    """the seeded relabelling of the entry `name` (the whole name, "/p1" or "/p2" included)"""
    n = int(name.split("-n")[1].split("/")[0])
    return tuple(int(x) for x in np.random.default_rng([20261021, zlib.crc32(name.encode())]).permutation(n))


def broom_pairs(n):
    """every ORDERED (a, b) with a + b >= n - BROOM_SLACK that leaves a path of two vertices or more; a = 0 and b = 0 included"""
    return [(a, b) for a in range(n - 1) for b in range(n - 1 - a) if a + b >= n - BROOM_SLACK]


def multipartite_parts(n):
    return ([1, 2, n - 3], [2, 3, n - 5], [1, 2, 3, n - 6], [n // 2, n - n // 2], [1, 1, n - 2])


def base_graphs(n):
    """[(name, adj)] as generated"""
    pairs = broom_pairs(n)
    if n > A.AH_MAX_N:
        pairs = pairs[::WIDE_THINNING]
    out = [("broom(%d,%d)-n%d" % (a, b, n), A.double_broom(n, a, b)) for a, b in pairs]
    out += [("K[%s]-n%d" % (",".join(str(p) for p in parts), n), multipartite(parts)) for parts in multipartite_parts(n)]
    out += [("star-n%d" % n, A.star(n)), ("complete-n%d" % n, A.complete(n))]
    return out


# Named by the report that opened this set.  broom(19,2)-n23/id -- the smallest double broom that fails as generated -- is in the
# regular set.  The others are not: n = 30 is no size of it, and the smallest failures of all are complete multipartite graphs
# under relabellings other than the seeded ones, kept here as a search over random labellings found them (K(9,10) on 19 vertices
# is the smallest known: nothing failed at n = 18 in 15 000 labellings of five such graphs).  (name, n, base graph, relabelling)
NAMED = (
    ("broom(14,12)-n30/id", 30, A.double_broom(30, 14, 12), None),
    ("K[9,10]-n19/found", 19, multipartite([9, 10]), (5, 10, 4, 11, 0, 12, 16, 3, 6, 7, 13, 15, 9, 2, 17, 1, 8, 14, 18)),
    ("K[10,11]-n21/found", 21, multipartite([10, 11]), (1, 11, 20, 15, 7, 12, 18, 17, 16, 2, 10, 3, 4, 5, 8, 0, 9, 14, 13, 6, 19)),
    ("K[1,2,19]-n22/found", 22, multipartite([1, 2, 19]), (0, 10, 18, 1, 14, 19, 17, 21, 6, 12, 5, 2, 13, 7, 3, 15, 11, 20, 4, 8, 16, 9)),
)


def _entries(ns):
    out = []
    for n in ns:
        for name, adj in base_graphs(n):
            assert A.connected(adj, n), name
            for lab in LABELLINGS:
                full = name + "/" + lab
                out.append((full, n, tuple(adj if lab == "id" else relabel(adj, n, permutation(full)))))
    return out


@functools.lru_cache(maxsize=None)
def graph_set():
    """the narrow tiers' set: NARROW_NS and the named graphs, n <= 32"""
    out = _entries(NARROW_NS)
    for name, n, base, perm in NAMED:
        out.append((name, n, tuple(base if perm is None else relabel(base, n, perm))))
    assert len({name for name, _, _ in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def graph_set_wide():
    """the 64-row form's set beyond 32 vertices: WIDE_NS (at n <= 32 it takes graph_set())"""
    return tuple(_entries(WIDE_NS))


def by_size(entries):
    """{n: [entries]}: what one probe launch takes (one vertex count per launch)"""
    out = {}
    for e in entries:
        out.setdefault(e[1], []).append(e)
    return out


def matrices(adj, n):
    """the four matrices the invariant costs reduce, as lists of rows: adjacency, distance, Laplacian D - A, signless Laplacian D + A"""
    a = [[(adj[u] >> v) & 1 for v in range(n)] for u in range(n)]
    deg = [sum(row) for row in a]
    return dict(adj=a, dist=A.bfs_all(adj, n)[0],
                lap=[[deg[u] if u == v else -a[u][v] for v in range(n)] for u in range(n)],
                slap=[[deg[u] if u == v else a[u][v] for v in range(n)] for u in range(n)])


# The entries of graph_set() on which the reduction WITHOUT the deflation rule -- dense_ah_ref.tridiagonalise(M, n), deflate = 0.0,
# the procedure the narrow tiers ran before -- leaves a non-finite entry in the adjacency matrix's tridiagonal form.
# test_dense_spectral_cases.py recomputes the list and holds it to this one, so the set cannot be thinned into harmlessness.
PARENT_FAILS = (
    "broom(19,2)-n23/id", "broom(20,1)-n23/id", "broom(13,7)-n24/id", "broom(18,3)-n24/p1", "broom(18,4)-n24/id", "broom(20,2)-n24/id",
    "broom(20,2)-n24/p2", "broom(1,24)-n27/p1", "broom(5,20)-n27/p2", "broom(6,19)-n27/p1", "broom(7,18)-n27/p2", "broom(8,16)-n27/p1",
    "broom(8,17)-n27/p1", "broom(9,16)-n27/p2", "broom(10,15)-n27/p2", "broom(11,14)-n27/p1", "broom(14,10)-n27/p1", "broom(14,11)-n27/p2",
    "broom(16,7)-n27/id", "broom(16,9)-n27/p2", "broom(17,6)-n27/id", "broom(17,8)-n27/p2", "broom(19,6)-n27/id", "broom(22,1)-n27/id",
    "broom(22,3)-n27/id", "broom(24,1)-n27/id", "K[1,2,24]-n27/p1", "K[13,14]-n27/p1", "K[13,14]-n27/p2", "broom(0,24)-n31/p1",
    "broom(0,27)-n31/p2", "broom(3,26)-n31/p1", "broom(4,25)-n31/p2", "broom(5,24)-n31/p1", "broom(5,24)-n31/p2", "broom(6,23)-n31/p1",
    "broom(6,23)-n31/p2", "broom(8,20)-n31/p1", "broom(8,21)-n31/p2", "broom(9,19)-n31/p1", "broom(9,19)-n31/p2", "broom(9,20)-n31/p2",
    "broom(10,19)-n31/p2", "broom(11,15)-n31/p2", "broom(11,18)-n31/p1", "broom(11,18)-n31/p2", "broom(12,16)-n31/p1", "broom(12,17)-n31/p2",
    "broom(13,16)-n31/p1", "broom(14,15)-n31/p1", "broom(15,11)-n31/p2", "broom(15,14)-n31/p1", "broom(15,14)-n31/p2", "broom(17,6)-n31/id",
    "broom(18,5)-n31/id", "broom(18,11)-n31/p2", "broom(19,4)-n31/id", "broom(19,8)-n31/id", "broom(19,10)-n31/id", "broom(19,10)-n31/p1",
    "broom(20,5)-n31/id", "broom(20,9)-n31/id", "broom(20,9)-n31/p2", "broom(21,2)-n31/id", "broom(21,7)-n31/p1", "broom(21,8)-n31/id",
    "broom(21,8)-n31/p1", "broom(22,3)-n31/id", "broom(22,5)-n31/id", "broom(22,7)-n31/id", "broom(22,7)-n31/p1", "broom(22,7)-n31/p2",
    "broom(23,4)-n31/id", "broom(23,5)-n31/p1", "broom(23,5)-n31/p2", "broom(23,6)-n31/id", "broom(23,6)-n31/p1", "broom(24,3)-n31/id",
    "broom(24,3)-n31/p1", "broom(25,3)-n31/p2", "broom(25,4)-n31/id", "broom(26,0)-n31/p2", "broom(26,3)-n31/id", "broom(27,2)-n31/p1",
    "K[2,3,26]-n31/p1", "broom(0,27)-n32/p1", "broom(0,27)-n32/p2", "broom(0,28)-n32/p2", "broom(0,29)-n32/p2", "broom(1,28)-n32/p1",
    "broom(1,28)-n32/p2", "broom(1,29)-n32/p2", "broom(2,27)-n32/p2", "broom(2,28)-n32/p2", "broom(3,25)-n32/p2", "broom(3,26)-n32/p2",
    "broom(3,27)-n32/p1", "broom(3,27)-n32/p2", "broom(4,26)-n32/p1", "broom(4,26)-n32/p2", "broom(5,24)-n32/p1", "broom(5,25)-n32/p2",
    "broom(6,23)-n32/p1", "broom(6,23)-n32/p2", "broom(6,24)-n32/p2", "broom(7,23)-n32/p1", "broom(7,23)-n32/p2", "broom(8,22)-n32/p1",
    "broom(8,22)-n32/p2", "broom(9,20)-n32/p1", "broom(9,20)-n32/p2", "broom(9,21)-n32/p2", "broom(10,18)-n32/p2", "broom(10,20)-n32/p1",
    "broom(10,20)-n32/p2", "broom(11,17)-n32/p2", "broom(12,15)-n32/p1", "broom(12,16)-n32/p1", "broom(12,17)-n32/p1", "broom(13,15)-n32/p2",
    "broom(13,16)-n32/p1", "broom(13,17)-n32/p1", "broom(13,17)-n32/p2", "broom(14,15)-n32/p1", "broom(14,16)-n32/p1", "broom(14,16)-n32/p2",
    "broom(15,12)-n32/p1", "broom(15,15)-n32/p1", "broom(15,15)-n32/p2", "broom(16,11)-n32/p2", "broom(16,12)-n32/id", "broom(16,13)-n32/p2",
    "broom(16,14)-n32/p1", "broom(16,14)-n32/p2", "broom(17,13)-n32/p2", "broom(18,10)-n32/id", "broom(18,10)-n32/p2", "broom(18,11)-n32/p2",
    "broom(18,12)-n32/p1", "broom(19,7)-n32/id", "broom(19,9)-n32/id", "broom(19,9)-n32/p2", "broom(19,10)-n32/p2", "broom(19,11)-n32/p1",
    "broom(19,11)-n32/p2", "broom(20,10)-n32/id", "broom(21,3)-n32/id", "broom(21,9)-n32/id", "broom(21,9)-n32/p1", "broom(21,9)-n32/p2",
    "broom(22,6)-n32/p2", "broom(22,7)-n32/p1", "broom(22,7)-n32/p2", "broom(22,8)-n32/id", "broom(22,8)-n32/p2", "broom(23,1)-n32/id",
    "broom(23,3)-n32/id", "broom(23,6)-n32/p1", "broom(23,6)-n32/p2", "broom(23,7)-n32/id", "broom(23,7)-n32/p1", "broom(23,7)-n32/p2",
    "broom(24,5)-n32/p1", "broom(24,6)-n32/id", "broom(25,5)-n32/id", "broom(25,5)-n32/p1", "broom(25,5)-n32/p2", "broom(26,2)-n32/p1",
    "broom(26,4)-n32/p1", "broom(26,4)-n32/p2", "broom(27,1)-n32/p1", "broom(27,2)-n32/p1", "broom(27,3)-n32/id", "broom(27,3)-n32/p1",
    "broom(27,3)-n32/p2", "broom(28,0)-n32/p1", "broom(28,1)-n32/p1", "broom(28,2)-n32/p1", "broom(29,0)-n32/p2", "K[1,2,29]-n32/p1",
    "K[1,2,29]-n32/p2", "K[2,3,27]-n32/p2", "broom(14,12)-n30/id", "K[9,10]-n19/found", "K[10,11]-n21/found", "K[1,2,19]-n22/found",
)

# sha256(repr(graph_set() + graph_set_wide()))[:16]: the seeded relabellings are these on every machine
DIGEST = "15d764b3675a7725"
