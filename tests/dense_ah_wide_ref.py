"""Python reference of the Aouchiche-Hansen cost up to 64 vertices (AZD_ENGINE_DENSE_AH_WIDE, azd_dense_ah_cost_wide; test
infrastructure).  Nothing is restated here: tests/dense_ah_ref.py's primitives (bfs_all, tridiagonalise, kth_eigenvalue, the
whole of _ah_cost_cached) are generic in n; only its ah_cost's assert, AH_MAX_N and graph_set stop at 32.  This module lifts the
limit to 64, gives the Python engine a cost that uses it, and holds the graph set of the 64-row checks."""
import functools
import math

import numpy as np

import dense_ah_ref as R

AH_WIDE_MAX_N = 64
WIDE_NS = (33, 34, 40, 47, 50, 56, 63, 64)  # the first rows past 32, the benchmarked shape (50), the last two
WIDE_PS = (0.05, 0.1, 0.2, 0.4, 0.6)


def ah_cost(adj, n):
    """The whole objective of one connected graph on 4 <= n <= 64 vertices: dense_ah_ref's sequence of operations, unchanged."""
    assert 4 <= n <= AH_WIDE_MAX_N
    return R._ah_cost_cached(tuple(int(a) for a in adj), n)


def gnp_over_tree(rng, n, p):
    """G(n, p) over a random spanning tree (dense_ah_ref.graph_set's variant below the connectivity threshold)"""
    adj = [0] * n
    order = rng.permutation(n)
    for a in range(1, n):
        u, v = int(order[a]), int(order[int(rng.integers(0, a))])
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    for v in range(1, n):
        for u in range(v):
            if rng.random() < p:
                adj[v] |= 1 << u
                adj[u] |= 1 << v
    return adj


@functools.lru_cache(maxsize=None)
def graph_set_wide():
    """(name, n, adj): per n of WIDE_NS a path, a star, a cycle, the complete graph, two double brooms and G(n, p) for p of
    WIDE_PS (over a spanning tree below 1.5 ln n / n) -- 88 connected graphs, diameters 1 .. 63, from a fixed seed."""
    out = []
    rng = np.random.default_rng(20250711)
    for n in WIDE_NS:
        out.append(("path", n, R.path(n)))
        out.append(("star", n, R.star(n)))
        out.append(("cycle", n, R.cycle(n)))
        out.append(("complete", n, R.complete(n)))
        out.append(("broom", n, R.double_broom(n, (n - 2) // 3, (n - 2) // 3)))
        out.append(("broom", n, R.double_broom(n, 1, n - 4)))
        for p in WIDE_PS:
            if p < 1.5 * math.log(n) / n:
                out.append(("gnp%.2f+tree" % p, n, gnp_over_tree(rng, n, p)))
            else:
                out.append(("gnp%.2f" % p, n, R.gnp_connected(rng, n, p)))
    assert len(out) == 88
    return tuple((name, n, tuple(adj)) for name, n, adj in out)


class PyDenseWideEngine(R.PyDenseEngine):
    """dense_ah_ref.PyDenseEngine with the cost up to 64 vertices; everything else (space, tree, root policy) is the parent's."""

    def cost(self, st):
        assert self.cost_kind == "ah"
        return dict(ah_cost(st.adj, self.n))
