"""Python reference of the weighted-invariant cost up to 64 vertices (AZD_ENGINE_DENSE_INV_WIDE, azd_dense_inv_cost_wide; test
infrastructure).  The image of tests/dense_ah_wide_ref.py: the stages of tests/dense_inv_ref.py (_stages, dist_index_of, the
recipes) and of tests/dense_ah_ref.py (kth_eigenvalue) are generic in n; only dense_inv_ref.inv_cost's assert stops at 32.
inv_cost below is that function's sequence with the limit at 64.  One thing differs beyond 32 vertices, in all three forms of the
cost (c21_host.h: DENSE_INV_DEFLATE): the Householder reduction skips a column whose tail is below 2^-200 as it skips one whose
tail is zero -- a rank-deficient adjacency matrix (a double broom on 50 vertices) otherwise runs the reduction into subnormal
squares and NaN, which 32 rows are too few steps to reach.  tridiagonalise below is dense_ah_ref's with that one condition; up to 32
vertices it is not used.  The pure-Python reduction is slow at n = 64 and does not depend on the index wanted, so it is cached
per (graph, matrix): the four test recipes share it, where dense_inv_ref._eig redoes it per index.  The graphs of the 64-row checks
are dense_ah_wide_ref.graph_set_wide()."""
import functools
import math

import dense_ah_ref as A
import dense_ah_wide_ref as W
import dense_inv_ref as R

INV_WIDE_MAX_N = 64
INV_DEFLATE = 2.0 ** -200
graph_set_wide = W.graph_set_wide
RECIPES = R.RECIPES


def tridiagonalise(m, n):
    """dense_ah_ref.tridiagonalise, operation for operation, with the deflation threshold of the rows beyond 32"""
    assert n > A.AH_MAX_N
    M = [[float(x) for x in row] for row in m]
    diag, sub = [0.0] * n, [0.0] * n
    for i in range(n - 2):
        x = [M[r][i] if r > i else 0.0 for r in range(n)]
        tail = A.tree_sum64([x[r] * x[r] if r > i + 1 else 0.0 for r in range(n)])
        x1 = x[i + 1]
        diag[i] = M[i][i]
        if tail == 0.0 or tail < INV_DEFLATE:
            sub[i] = x1
            continue
        sigma = tail + x1 * x1
        s = math.sqrt(sigma)
        alpha = -s if x1 >= 0.0 else s
        v = list(x)
        v1 = x1 - alpha
        v[i + 1] = v1
        beta = 2.0 / (tail + v1 * v1)
        p = [0.0] * n
        for r in range(i + 1, n):
            acc = 0.0
            Mr = M[r]
            for c in range(i + 1, n):
                acc = acc + Mr[c] * v[c]
            p[r] = beta * acc
        vp = A.tree_sum64([v[r] * p[r] if r > i else 0.0 for r in range(n)])
        K = (0.5 * beta) * vp
        q = [p[r] - K * v[r] if r > i else 0.0 for r in range(n)]
        for r in range(i + 1, n):
            Mr, vr, qr = M[r], v[r], q[r]
            for c in range(i + 1, n):
                Mr[c] = Mr[c] - (vr * q[c] + qr * v[c])
        sub[i] = alpha
    diag[n - 2] = M[n - 2][n - 2]
    sub[n - 2] = M[n - 1][n - 2]
    diag[n - 1] = M[n - 1][n - 1]
    return diag, sub


@functools.lru_cache(maxsize=None)
def _tridiagonal(adj, n, which):
    m = R._stages(adj, n)[0] if which == "dist" else R.adjacency_matrix(adj, n)
    return tridiagonalise(m, n) if n > A.AH_MAX_N else A.tridiagonalise(m, n)


@functools.lru_cache(maxsize=None)
def _eig(adj, n, which, k):
    diag, sub = _tridiagonal(adj, n, which)
    return A.kth_eigenvalue(diag, sub, n, k)


def inv_cost(adj, n, recipe):
    """The whole objective of one connected graph on 4 <= n <= 64 vertices under `recipe`: dense_inv_ref.inv_cost's sequence."""
    assert 4 <= n <= INV_WIDE_MAX_N
    adj = tuple(int(a) for a in adj)
    _, s = R._stages(adj, n)
    dist_k = R.dist_index_of(recipe, s["diam"], n)
    inv = [float(s["m"]), float(s["max_deg"]), float(s["min_deg"]), float(s["diam"]), float(s["rad"]),
           float(s["min_t"]) / float(n - 1), float(s["max_t"]) / float(n - 1), float(s["sum_t"]) / float(n * (n - 1)), 0.0, 0.0]
    computed = R.ALWAYS
    if recipe.weight[R.ADJ_EIG] != 0.0:
        inv[R.ADJ_EIG] = _eig(adj, n, "adj", recipe.adj_index)
        computed |= 1 << R.ADJ_EIG
    if recipe.weight[R.DIST_EIG] != 0.0:
        inv[R.DIST_EIG] = _eig(adj, n, "dist", dist_k)
        computed |= 1 << R.DIST_EIG
    c = recipe.bias
    for w, x in zip(recipe.weight, inv):
        if w != 0.0:
            term = w * x
            c = c + term
    cost = R.F(c)
    ev = recipe.eval_scale * (cost + recipe.eval_offset)
    out = dict(zip(R.NAMES, inv))
    out.update(dist_k=dist_k, computed=computed, cost=cost, eval=ev)
    return out


class PyDenseInvWideEngine(R.PyDenseInvEngine):
    """dense_inv_ref.PyDenseInvEngine with the cost up to 64 vertices; everything else (space, tree, root policy) is the parent's."""

    def cost(self, st):
        return dict(inv_cost(st.adj, self.n, self.recipe))
