"""Python reference of the weighted-invariant cost up to 64 vertices (AZD_ENGINE_DENSE_INV_WIDE, azd_dense_inv_cost_wide; test
infrastructure).  The image of tests/dense_ah_wide_ref.py: the stages of tests/dense_inv_ref.py (_stages, _tridiagonal, _eig,
dist_index_of, the recipes) and of tests/dense_ah_ref.py (tridiagonalise, kth_eigenvalue) are generic in n; only
dense_inv_ref.inv_cost's assert stops at 32.  inv_cost below is that function's sequence with the limit at 64, and nothing else
differs: the Householder reduction skips a column whose tail is below 2^-200 (dense_inv_ref.INV_DEFLATE; dense_cost_host.h:
DENSE_INV_DEFLATE) at every n, in the narrow reference as here -- the condition was found on double brooms of 50 and 56 vertices
and first held beyond 32 vertices only, until rank-deficient adjacency matrices on 21 vertices and more turned out to starve the
same way.  The pure-Python reduction is slow at n = 64 and does not depend on the index wanted: dense_inv_ref caches it per
(graph, matrix), so the four test recipes share it.  The graphs of the 64-row checks are dense_ah_wide_ref.graph_set_wide()."""
import dense_ah_wide_ref as W
import dense_inv_ref as R

INV_WIDE_MAX_N = 64
INV_DEFLATE = R.INV_DEFLATE
graph_set_wide = W.graph_set_wide
RECIPES = R.RECIPES
_tridiagonal, _eig = R._tridiagonal, R._eig


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
