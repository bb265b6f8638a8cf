"""Python reference of the spectrum invariant cost up to 64 vertices (AZD_ENGINE_DENSE_INVS_WIDE, azd_dense_invs_cost_wide; test
infrastructure).  The image of tests/dense_invx_wide_ref.py: the stages of tests/dense_invs_ref.py (spectrum, energy, spread, prime,
the recipes) and of the references below it are generic in n; only dense_invs_ref.invs_cost's assert stops at 32.  invs_cost below
is that function's sequence with the limit at 64, and nothing else differs: the caches and the recipes are shared with the narrow
reference, and the Householder reduction skips a column whose tail is below 2^-200 at every n (dense_inv_ref.INV_DEFLATE).
A *_eig that the caches do not hold yet comes from dense_invx_wide_ref._eig, that is through the numpy forms of the two spectral
stages, which test_dense_spectral_cases.py holds to the scalar forms bit for bit; a whole spectrum from dense_invs_ref.spectrum.
prime_graphs fills the caches for a whole graph set at once.  The graphs of the 64-row checks are dense_ah_wide_ref.graph_set_wide()."""
import dense_ah_wide_ref as W
import dense_inv_ref as I
import dense_invs_ref as S
import dense_invx_ref as X
import dense_invx_wide_ref as XW

INVS_WIDE_MAX_N = 64
graph_set_wide = W.graph_set_wide
RECIPES, NEW_RECIPES, INVX_RECIPES, NAMES = S.RECIPES, S.NEW_RECIPES, S.INVX_RECIPES, S.NAMES
c_recipe = S.c_recipe
spectrum, energy, spread = S.spectrum, S.energy, S.spread


def prime_graphs(entries, whiches=S.WHICH, ks_of=lambda n: (0, 1, n - 2, n - 1)):
    """fill the caches (tridiagonal forms, *_eig at ks_of(n), whole spectra) for entries of (name, n, adj) through the numpy forms"""
    S.prime(entries, whiches, ks_of)


def invs_cost(adj, n, recipe):
    """The whole objective of one connected graph on 4 <= n <= 64 vertices under `recipe`: dense_invs_ref.invs_cost's sequence."""
    assert 4 <= n <= INVS_WIDE_MAX_N
    adj = tuple(int(a) for a in adj)
    _, s = I._stages(adj, n)
    dist_k = I.dist_index_of(recipe, s["diam"], n)
    inv = [float(s["m"]), float(s["max_deg"]), float(s["min_deg"]), float(s["diam"]), float(s["rad"]),
           float(s["min_t"]) / float(n - 1), float(s["max_t"]) / float(n - 1), float(s["sum_t"]) / float(n * (n - 1))] + [0.0] * 13
    need = recipe.needed()
    index = dict(dist=dist_k, adj=recipe.adj_index, lap=recipe.lap_index, slap=recipe.slap_index)
    for which, eig_i, energy_i in S.PASSES:
        if need >> eig_i & 1:
            inv[eig_i] = XW._eig(adj, n, which, index[which])
        if need >> energy_i & 1:
            inv[energy_i] = energy(adj, n, which)
    if need >> S.ADJ_SPREAD & 1:
        inv[S.ADJ_SPREAD] = spread(adj, n)
    if need >> X.RANDIC & 0xF:
        d = X.degree_invariants(adj, n)
        for i in range(4):
            if need >> (X.RANDIC + i) & 1:
                inv[X.RANDIC + i] = float(d[i])
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
    cost = S.F(c)
    ev = recipe.eval_scale * (cost + recipe.eval_offset)
    out = dict(zip(NAMES, inv))
    out.update(dist_k=dist_k, computed=S.ALWAYS | need, cost=cost, eval=ev)
    return out


class PyDenseInvsWideEngine(S.PyDenseInvsEngine):
    """dense_invs_ref.PyDenseInvsEngine with the cost up to 64 vertices; everything else (space, tree, root policy) is the parent's."""

    def cost(self, st):
        return dict(invs_cost(st.adj, self.n, self.recipe))
