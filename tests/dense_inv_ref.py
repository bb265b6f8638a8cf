"""Python reference of the dense-graph space's weighted-invariant cost (test infrastructure; DESIGN.md "The invariant cost").

BUILD-DEFINED.  Ten invariants of a connected graph, in ABI order (NAMES), from tests/dense_ah_ref.py's stages -- bfs_all,
tridiagonalise, kth_eigenvalue -- one IEEE f64 operation at a time:

    edges, max_degree, min_degree, diameter, radius                       integers
    proximity = min t / (n - 1), remoteness = max t / (n - 1)             one f64 division each
    avg_distance = sum t / (n (n - 1))                                    integer sum, one f64 division
    adj_eig  = adjacency eigenvalue at descending index adj_index         Householder + multisection
    dist_eig = distance eigenvalue at descending index dist_index, or the AH rule (INDEX_AH)
               (the reduction with INV_DEFLATE: a column whose tail is below 2^-200 is skipped like a zero one -- without it a
               rank-deficient adjacency matrix ends in NaN from 19 vertices on; the AH cost itself keeps deflate = 0)

and a recipe (weight[10], bias, adj_index, dist_index, eval_offset, eval_scale):

    c = bias;  for i in 0 .. 9: if weight[i] != 0: c = c + weight[i] * I_i;  cost = f32(c);  eval = eval_scale * (cost + eval_offset)

A spectral invariant whose weight is zero is not computed: 0.0, and its bit of `computed` is clear.  azd_dense_inv_cost
(dense_cost_host.cpp) and dense_inv_cost_wave (dense_inv_cost.inc) run the same sequence: the three agree bit for bit.
Also here: the four recipes the tests use, and PyDenseInvEngine, tests/dense_ah_ref.py's engine with this cost."""
import functools

import numpy as np

import dense_ah_ref as A

F = np.float32
NAMES = ("edges", "max_degree", "min_degree", "diameter", "radius", "proximity", "remoteness", "avg_distance", "adj_eig", "dist_eig")
ADJ_EIG, DIST_EIG = 8, 9
INDEX_AH = -1
ALWAYS = 0xFF
INV_DEFLATE = 2.0 ** -200  # a Householder column whose tail is below this is skipped (dense_cost_host.h: DENSE_INV_DEFLATE)


class Recipe:
    def __init__(self, weights, bias=0.0, adj_index=0, dist_index=INDEX_AH, eval_offset=0.0, eval_scale=1.0):
        assert set(weights) <= set(NAMES), weights
        self.weight = tuple(float(weights.get(k, 0.0)) for k in NAMES)
        self.bias, self.adj_index, self.dist_index = float(bias), int(adj_index), int(dist_index)
        self.eval_offset, self.eval_scale = F(eval_offset), F(eval_scale)

    def key(self):
        return (self.weight, self.bias, self.adj_index, self.dist_index, float(self.eval_offset), float(self.eval_scale))

    def weights(self):
        return {k: w for k, w in zip(NAMES, self.weight) if w != 0.0}

    def kwargs(self):
        """as InvariantCost's keyword arguments"""
        return dict(bias=self.bias, adj_index=self.adj_index, dist_index="ah" if self.dist_index == INDEX_AH else self.dist_index,
                    eval_offset=self.eval_offset, eval_scale=self.eval_scale)


# ---------------------------------------------------------------- the recipes the tests use; scales are 1 / (2 n + 2)
def recipe_ah(n):
    """the Aouchiche-Hansen cost: scale as an f32 quotient, as dense_ah_ref.eval_slope"""
    return Recipe({"proximity": 1.0, "dist_eig": 1.0}, dist_index=INDEX_AH, eval_offset=2.0, eval_scale=F(1.0) / F(2 * n + 2))


def recipe_int(n):
    return Recipe({"remoteness": 1.0, "proximity": -1.0, "max_degree": 0.25, "edges": -0.03125, "diameter": 0.5, "radius": -0.5},
                  eval_offset=2.0, eval_scale=1.0 / (2 * n + 2))


def recipe_adj(n):
    return Recipe({"adj_eig": 1.0, "avg_distance": -1.0, "min_degree": 0.125}, adj_index=0, eval_offset=4.0, eval_scale=1.0 / (2 * n + 2))


def recipe_both(n):
    return Recipe({"adj_eig": -1.0, "dist_eig": 0.25}, adj_index=n - 1, dist_index=1, eval_offset=2.0, eval_scale=1.0 / (2 * n + 2))


RECIPES = dict(AH=recipe_ah, INT=recipe_int, ADJ=recipe_adj, BOTH=recipe_both)


# ---------------------------------------------------------------- the cost
def adjacency_matrix(adj, n):
    return [[(adj[u] >> v) & 1 for v in range(n)] for u in range(n)]


@functools.lru_cache(maxsize=None)
def _stages(adj, n):
    """what does not depend on the recipe: the BFS and the integer reductions"""
    dist, trans, ecc = A.bfs_all(adj, n)
    deg = [bin(a).count("1") for a in adj]
    return dist, dict(m=sum(deg) // 2, max_deg=max(deg), min_deg=min(deg), diam=max(ecc), rad=min(ecc),
                      min_t=min(trans), max_t=max(trans), sum_t=sum(trans))


# The matrices a spectral pass reduces, by name: f(adj, n) -> rows.  dense_invx_ref adds "lap" and "slap".
MATRICES = {"adj": adjacency_matrix, "dist": lambda adj, n: _stages(adj, n)[0]}
_TRI, _EIG = {}, {}  # (adj, n, which) -> (diag, sub);  (adj, n, which, k) -> the eigenvalue


def _tridiagonal(adj, n, which):
    """(diag, sub) of the matrix `which` of the graph: it does not depend on the index wanted, so the indices share it.  The
    reduction skips a column whose tail is below INV_DEFLATE, at every n (dense_cost_host.h: DENSE_INV_DEFLATE)."""
    key = (adj, n, which)
    if key not in _TRI:
        _TRI[key] = A.tridiagonalise(MATRICES[which](adj, n), n, INV_DEFLATE)
    return _TRI[key]


def _eig(adj, n, which, k):
    key = (adj, n, which, k)
    if key not in _EIG:
        diag, sub = _tridiagonal(adj, n, which)
        _EIG[key] = A.kth_eigenvalue(diag, sub, n, k)
    return _EIG[key]


def prime(entries, whiches, ks_of=lambda n: (0, 1, n // 2, n - 2, n - 1)):
    """Fill the two caches for many graphs at once -- entries of (name, n, adj), the matrices `whiches`, the descending indices
    ks_of(n) -- through dense_ah_ref's forms over many matrices: the same operations, the same bits (test_dense_spectral_cases.py),
    some twenty times faster.  The hard case set has thousands of graphs; nothing else needs this."""
    by_n = {}
    for _, n, adj in entries:
        by_n.setdefault(n, []).append(tuple(int(a) for a in adj))
    for n, graphs in by_n.items():
        ks = sorted(set(ks_of(n)))
        for which in whiches:
            todo = [g for g in graphs if any((g, n, which, k) not in _EIG for k in ks)]
            if not todo:
                continue
            diag, sub = A.tridiagonalise_many([MATRICES[which](g, n) for g in todo], n, INV_DEFLATE)
            eig = A.kth_eigenvalues_many(diag, sub, n, ks)
            for i, g in enumerate(todo):
                _TRI[(g, n, which)] = (diag[i].tolist(), sub[i].tolist())
                for j, k in enumerate(ks):
                    _EIG[(g, n, which, k)] = float(eig[i, j])


def dist_index_of(recipe, diam, n):
    return recipe.dist_index if recipe.dist_index != INDEX_AH else A.ah_index(diam, n)


def inv_cost(adj, n, recipe):
    """The whole objective of one connected graph under `recipe`; adj = n neighbourhood bitsets (ints)."""
    assert 4 <= n <= A.AH_MAX_N
    adj = tuple(int(a) for a in adj)
    _, s = _stages(adj, n)
    dist_k = dist_index_of(recipe, s["diam"], n)
    inv = [float(s["m"]), float(s["max_deg"]), float(s["min_deg"]), float(s["diam"]), float(s["rad"]),
           float(s["min_t"]) / float(n - 1), float(s["max_t"]) / float(n - 1), float(s["sum_t"]) / float(n * (n - 1)), 0.0, 0.0]
    computed = ALWAYS
    if recipe.weight[ADJ_EIG] != 0.0:
        inv[ADJ_EIG] = _eig(adj, n, "adj", recipe.adj_index)
        computed |= 1 << ADJ_EIG
    if recipe.weight[DIST_EIG] != 0.0:
        inv[DIST_EIG] = _eig(adj, n, "dist", dist_k)
        computed |= 1 << DIST_EIG
    c = recipe.bias
    for w, x in zip(recipe.weight, inv):
        if w != 0.0:
            term = w * x
            c = c + term
    cost = F(c)
    ev = recipe.eval_scale * (cost + recipe.eval_offset)
    out = dict(zip(NAMES, inv))
    out.update(dist_k=dist_k, computed=computed, cost=cost, eval=ev)
    return out


# ---------------------------------------------------------------- the engine
class PyDenseInvEngine(A.PyDenseEngine):
    """tests/dense_ah_ref.py's engine of the dense-graph space with the weighted-invariant cost under one recipe"""

    def __init__(self, n, batch, recipe, p=0.2):
        super().__init__(n, batch, cost="inv", p=p)
        self.recipe = recipe

    def cost(self, st):
        return dict(inv_cost(st.adj, self.n, self.recipe))
