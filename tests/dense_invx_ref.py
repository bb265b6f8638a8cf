"""Python reference of the dense-graph space's extended invariant cost (test infrastructure; DESIGN.md "The extended invariant cost").

BUILD-DEFINED.  Sixteen invariants of a connected graph, in ABI order (NAMES).  The first ten are tests/dense_inv_ref.py's, from
the same stages; then, one IEEE f64 operation at a time:

    lap_eig  = eigenvalue of L = D - A at descending index lap_index      tridiagonalise + kth_eigenvalue (tests/dense_ah_ref.py)
    slap_eig = eigenvalue of Q = D + A at descending index slap_index     the same
    randic   = sum over edges uv of 1 / sqrt(d_u d_v)                     vertex u over its neighbours v < u ascending, a compensated
                                                                          sum: x = 1.0 / sqrt(float(d_u * d_v)), (r, e) = TwoSum(r, x),
                                                                          c = c + e; the vertex's part is r + c; then tree_sum64
    zagreb1 = sum_u d_u^2,  zagreb2 = sum_{uv} d_u d_v,  triangles = (sum_{uv} |N(u) & N(v)|) / 3        integers

and a recipe (weight[16], bias, adj_index, dist_index, lap_index, slap_index, eval_offset, eval_scale, up to four pair terms
(coef, a, op, b), op "*" or "/"):

    c = bias;  for i in 0 .. 15: if weight[i] != 0: c = c + weight[i] * I_i
    for each term in order: if coef != 0: v = I_a * I_b or I_a / I_b;  c = c + coef * v
    cost = f32(c);  eval = eval_scale * (cost + eval_offset)

Invariants 0 .. 7 are always computed; each of 8 .. 15 only when its weight is not zero or a term with a non-zero coefficient names
it -- otherwise 0.0, and its bit of `computed` is clear.  azd_dense_invx_cost (dense_cost_host.cpp) and dense_invx_cost_wave
(dense_invx_cost.inc) run the same sequence: the three agree bit for bit.  With weights 10 .. 15 zero and no term the sequence is
dense_inv_ref.inv_cost's.
Also here: the nine recipes the tests use, their ctypes forms, and PyDenseInvxEngine, tests/dense_ah_ref.py's engine with this cost."""
import functools
import math

import numpy as np

import dense_ah_ref as A
import dense_inv_ref as I

F = np.float32
NAMES = I.NAMES + ("lap_eig", "slap_eig", "randic", "zagreb1", "zagreb2", "triangles")
ADJ_EIG, DIST_EIG, LAP_EIG, SLAP_EIG, RANDIC, ZAGREB1, ZAGREB2, TRIANGLES = range(8, 16)
INDEX_AH = I.INDEX_AH
ALWAYS = 0xFF
MUL, DIV = 0, 1
OPS = {"*": MUL, "/": DIV}
DIVISORS = NAMES[:8] + ("randic", "zagreb1", "zagreb2")
MAX_TERMS = 4


class Recipe:
    def __init__(self, weights, terms=(), bias=0.0, adj_index=0, dist_index=INDEX_AH, lap_index=0, slap_index=0, eval_offset=0.0, eval_scale=1.0):
        assert set(weights) <= set(NAMES), weights
        self.weight = tuple(float(weights.get(k, 0.0)) for k in NAMES)
        self.terms = tuple((float(c), a, op, b) for c, a, op, b in terms)
        assert len(self.terms) <= MAX_TERMS and all(a in NAMES and b in NAMES and op in OPS and (op == "*" or b in DIVISORS) for _, a, op, b in self.terms)
        self.bias, self.adj_index, self.dist_index = float(bias), int(adj_index), int(dist_index)
        self.lap_index, self.slap_index = int(lap_index), int(slap_index)
        self.eval_offset, self.eval_scale = F(eval_offset), F(eval_scale)

    @classmethod
    def from_inv(cls, r):
        """tests/dense_inv_ref.py's Recipe, converted"""
        return cls(r.weights(), bias=r.bias, adj_index=r.adj_index, dist_index=r.dist_index, eval_offset=r.eval_offset, eval_scale=r.eval_scale)

    def weights(self):
        return {k: w for k, w in zip(NAMES, self.weight) if w != 0.0}

    def needed(self):
        """bits 8 .. 15 of `computed`"""
        m = 0
        for i in range(ADJ_EIG, len(NAMES)):
            if self.weight[i] != 0.0:
                m |= 1 << i
        for c, a, _, b in self.terms:
            if c != 0.0:
                m |= (1 << NAMES.index(a) | 1 << NAMES.index(b)) & ~ALWAYS
        return m

    def kwargs(self):
        """as InvariantCostX's keyword arguments"""
        return dict(terms=list(self.terms), bias=self.bias, adj_index=self.adj_index, dist_index="ah" if self.dist_index == INDEX_AH else self.dist_index,
                    lap_index=self.lap_index, slap_index=self.slap_index, eval_offset=self.eval_offset, eval_scale=self.eval_scale)


def c_recipe(recipe):
    """`recipe` as an azd_dense_invx_recipe"""
    from azdopt_amd import _lib
    r = _lib.DenseInvxRecipe()
    for i, w in enumerate(recipe.weight):
        r.weight[i] = w
    r.bias, r.adj_index, r.dist_index, r.lap_index, r.slap_index = recipe.bias, recipe.adj_index, recipe.dist_index, recipe.lap_index, recipe.slap_index
    r.eval_offset, r.eval_scale = float(recipe.eval_offset), float(recipe.eval_scale)
    for t, (coef, a, op, b) in enumerate(recipe.terms):
        r.term[t].coef, r.term[t].a, r.term[t].b, r.term[t].op = coef, NAMES.index(a), NAMES.index(b), OPS[op]
    r.n_terms = len(recipe.terms)
    return r


def c_inv_recipe(recipe):
    """a tests/dense_inv_ref.py Recipe as an azd_dense_inv_recipe"""
    from azdopt_amd import _lib
    r = _lib.DenseInvRecipe()
    for i, w in enumerate(recipe.weight):
        r.weight[i] = w
    r.bias, r.adj_index, r.dist_index = recipe.bias, recipe.adj_index, recipe.dist_index
    r.eval_offset, r.eval_scale = float(recipe.eval_offset), float(recipe.eval_scale)
    return r


# ---------------------------------------------------------------- the recipes the tests use; scales keep the evals inside (0, 1)
def recipe_lap(n):
    """algebraic connectivity - max_degree / 4: in (-n / 4, n]"""
    return Recipe({"lap_eig": 1.0, "max_degree": -0.25}, lap_index=n - 2, eval_offset=float(n), eval_scale=1.0 / (4 * n))


def recipe_slap(n):
    """signless-Laplacian index - zagreb1 / 64: q_1 <= 2 (n - 1), zagreb1 <= n (n - 1)^2"""
    return Recipe({"slap_eig": 1.0, "zagreb1": -0.015625}, slap_index=0, eval_offset=float(n * n * n) / 64.0, eval_scale=1.0 / (n * n * n / 32.0 + 4 * n))


def recipe_deg(n):
    """randic - min_degree / 2 + zagreb2 / 100 - triangles / 8"""
    return Recipe({"randic": 1.0, "min_degree": -0.5, "zagreb2": 0.01, "triangles": -0.125}, eval_offset=float(n * n * n) / 32.0 + n,
                  eval_scale=1.0 / (n ** 4 / 100.0 + n * n * n / 16.0 + 4 * n))


def recipe_ratio(n):
    """remoteness / radius + adj_eig * proximity / 8, weight on edges: one DIV and one MUL term (a spectral invariant named by a term alone)"""
    return Recipe({"edges": -0.0078125}, terms=[(1.0, "remoteness", "/", "radius"), (0.125, "adj_eig", "*", "proximity")], adj_index=0,
                  eval_offset=8.0, eval_scale=1.0 / (n * n / 4.0 + 3 * n + 16.0))


def recipe_all4(n):
    """all four spectra, at indices 1, 1, n - 2, n - 1"""
    return Recipe({"adj_eig": 1.0, "dist_eig": -0.125, "lap_eig": 0.5, "slap_eig": -0.25}, adj_index=1, dist_index=1, lap_index=n - 2, slap_index=n - 1,
                  eval_offset=4.0 * n, eval_scale=1.0 / (8 * n))


RECIPES = dict({k: (lambda n, mk=mk: Recipe.from_inv(mk(n))) for k, mk in I.RECIPES.items()},
               LAP=recipe_lap, SLAP=recipe_slap, DEG=recipe_deg, RATIO=recipe_ratio, ALL4=recipe_all4)
INV_RECIPES = tuple(sorted(I.RECIPES))
NEW_RECIPES = ("LAP", "SLAP", "DEG", "RATIO", "ALL4")


# ---------------------------------------------------------------- the cost
def degrees(adj):
    return [bin(a).count("1") for a in adj]


def laplacian(adj, n, sign):
    """D - A (sign = -1) or D + A (sign = +1)"""
    deg = degrees(adj)
    return [[deg[u] if u == v else sign * ((adj[u] >> v) & 1) for v in range(n)] for u in range(n)]


# L and Q join the matrices dense_inv_ref reduces: one reduction (with INV_DEFLATE), one pair of caches, for all four
I.MATRICES.update(lap=lambda adj, n: laplacian(adj, n, -1), slap=lambda adj, n: laplacian(adj, n, 1))
_eig = I._eig


@functools.lru_cache(maxsize=None)
def degree_invariants(adj, n):
    """(randic, zagreb1, zagreb2, triangles)"""
    deg = degrees(adj)
    part = [0.0] * n
    z2 = tri = 0
    for u in range(n):
        r = c = 0.0
        for v in range(u):
            if (adj[u] >> v) & 1:
                x = 1.0 / math.sqrt(float(deg[u] * deg[v]))
                t = r + x  # TwoSum (Knuth): t + e == r + x exactly; the errors are kept in c
                bp = t - r
                ap = t - bp
                e = (r - ap) + (x - bp)
                c = c + e
                r = t
                z2 += deg[u] * deg[v]
                tri += bin(adj[u] & adj[v]).count("1")
        part[u] = r + c
    return A.tree_sum64(part), sum(d * d for d in deg), z2, tri // 3


def invx_cost(adj, n, recipe):
    """The whole objective of one connected graph under `recipe`; adj = n neighbourhood bitsets (ints)."""
    assert 4 <= n <= A.AH_MAX_N
    adj = tuple(int(a) for a in adj)
    _, s = I._stages(adj, n)
    dist_k = I.dist_index_of(recipe, s["diam"], n)
    inv = [float(s["m"]), float(s["max_deg"]), float(s["min_deg"]), float(s["diam"]), float(s["rad"]),
           float(s["min_t"]) / float(n - 1), float(s["max_t"]) / float(n - 1), float(s["sum_t"]) / float(n * (n - 1))] + [0.0] * 8
    need = recipe.needed()
    if need >> ADJ_EIG & 1:
        inv[ADJ_EIG] = I._eig(adj, n, "adj", recipe.adj_index)
    if need >> DIST_EIG & 1:
        inv[DIST_EIG] = I._eig(adj, n, "dist", dist_k)
    if need >> LAP_EIG & 1:
        inv[LAP_EIG] = _eig(adj, n, "lap", recipe.lap_index)
    if need >> SLAP_EIG & 1:
        inv[SLAP_EIG] = _eig(adj, n, "slap", recipe.slap_index)
    if need >> RANDIC:
        d = degree_invariants(adj, n)
        for i in range(4):
            if need >> (RANDIC + i) & 1:
                inv[RANDIC + i] = float(d[i])
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
    cost = F(c)
    ev = recipe.eval_scale * (cost + recipe.eval_offset)
    out = dict(zip(NAMES, inv))
    out.update(dist_k=dist_k, computed=ALWAYS | need, cost=cost, eval=ev)
    return out


# ---------------------------------------------------------------- the engine
class PyDenseInvxEngine(A.PyDenseEngine):
    """tests/dense_ah_ref.py's engine of the dense-graph space with the extended invariant cost under one recipe"""

    def __init__(self, n, batch, recipe, p=0.2):
        super().__init__(n, batch, cost="invx", p=p)
        self.recipe = recipe

    def cost(self, st):
        return dict(invx_cost(st.adj, self.n, self.recipe))
