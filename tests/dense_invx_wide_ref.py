"""Python reference of the extended invariant cost up to 64 vertices (AZD_ENGINE_DENSE_INVX_WIDE, azd_dense_invx_cost_wide; test
infrastructure).  The image of tests/dense_inv_wide_ref.py: the stages of tests/dense_invx_ref.py (degree_invariants, the recipes,
the Laplacian matrices it adds to dense_inv_ref.MATRICES) and of tests/dense_inv_ref.py (_stages, _eig, dist_index_of) are generic
in n; only dense_invx_ref.invx_cost's assert stops at 32.  invx_cost below is that function's sequence with the limit at 64, and
nothing else differs: the caches, the recipes and degree_invariants are shared with the narrow reference, and the Householder
reduction skips a column whose tail is below 2^-200 at every n (dense_inv_ref.INV_DEFLATE), there as here.
The pure-Python reduction takes tens of milliseconds a matrix at n = 64 and a node of a tree under the ALL4 recipe needs four: an
eigenvalue that the caches do not hold yet is computed through dense_inv_ref.prime, that is through dense_ah_ref's numpy forms of
the two spectral stages, which test_dense_spectral_cases.py holds to the scalar forms bit for bit.  prime_graphs fills the caches
for a whole graph set at once.  The graphs of the 64-row checks are dense_ah_wide_ref.graph_set_wide()."""
import dense_ah_ref as A
import dense_ah_wide_ref as W
import dense_inv_ref as I
import dense_invx_ref as R

INVX_WIDE_MAX_N = 64
graph_set_wide = W.graph_set_wide
RECIPES, NEW_RECIPES, INV_RECIPES, NAMES = R.RECIPES, R.NEW_RECIPES, R.INV_RECIPES, R.NAMES
degree_invariants = R.degree_invariants
WHICH = {R.ADJ_EIG: "adj", R.DIST_EIG: "dist", R.LAP_EIG: "lap", R.SLAP_EIG: "slap"}


def prime_graphs(entries, whiches=("adj", "dist", "lap", "slap"), ks_of=lambda n: (0, 1, n // 2, n - 2, n - 1)):
    """fill dense_inv_ref's caches for entries of (name, n, adj) through the numpy forms"""
    I.prime(entries, whiches, ks_of)


def _eig(adj, n, which, k):
    """dense_inv_ref._eig; a value the caches lack comes from the numpy forms (the same operations, the same bits)"""
    if (adj, n, which, k) not in I._EIG:
        if (adj, n, which) in I._TRI:  # (reduced already, for another index)
            diag, sub = I._TRI[(adj, n, which)]
            I._EIG[(adj, n, which, k)] = float(A.kth_eigenvalues_many([diag], [sub], n, [k])[0, 0])
        else:
            I.prime([(None, n, adj)], (which,), lambda n: (k,))
    return I._EIG[(adj, n, which, k)]


def invx_cost(adj, n, recipe):
    """The whole objective of one connected graph on 4 <= n <= 64 vertices under `recipe`: dense_invx_ref.invx_cost's sequence."""
    assert 4 <= n <= INVX_WIDE_MAX_N
    adj = tuple(int(a) for a in adj)
    _, s = I._stages(adj, n)
    dist_k = I.dist_index_of(recipe, s["diam"], n)
    inv = [float(s["m"]), float(s["max_deg"]), float(s["min_deg"]), float(s["diam"]), float(s["rad"]),
           float(s["min_t"]) / float(n - 1), float(s["max_t"]) / float(n - 1), float(s["sum_t"]) / float(n * (n - 1))] + [0.0] * 8
    need = recipe.needed()
    index = {R.ADJ_EIG: recipe.adj_index, R.DIST_EIG: dist_k, R.LAP_EIG: recipe.lap_index, R.SLAP_EIG: recipe.slap_index}
    for i in (R.ADJ_EIG, R.DIST_EIG, R.LAP_EIG, R.SLAP_EIG):
        if need >> i & 1:
            inv[i] = _eig(adj, n, WHICH[i], index[i])
    if need >> R.RANDIC:
        d = degree_invariants(adj, n)
        for i in range(4):
            if need >> (R.RANDIC + i) & 1:
                inv[R.RANDIC + i] = float(d[i])
    c = recipe.bias
    for w, x in zip(recipe.weight, inv):
        if w != 0.0:
            term = w * x
            c = c + term
    for coef, a, op, b in recipe.terms:
        if coef != 0.0:
            x, y = inv[NAMES.index(a)], inv[NAMES.index(b)]
            v = x / y if op == "/" else x * y
            term = coef * v
            c = c + term
    cost = R.F(c)
    ev = recipe.eval_scale * (cost + recipe.eval_offset)
    out = dict(zip(NAMES, inv))
    out.update(dist_k=dist_k, computed=R.ALWAYS | need, cost=cost, eval=ev)
    return out


class PyDenseInvxWideEngine(R.PyDenseInvxEngine):
    """dense_invx_ref.PyDenseInvxEngine with the cost up to 64 vertices; everything else (space, tree, root policy) is the parent's."""

    def cost(self, st):
        return dict(invx_cost(st.adj, self.n, self.recipe))
