"""Python reference of the dense-graph space's spectrum invariant cost (test infrastructure; DESIGN.md "The spectrum invariant cost").

BUILD-DEFINED.  Twenty-one invariants of a connected graph, in ABI order (NAMES).  The first sixteen are tests/dense_invx_ref.py's,
from the same stages; then functions of a matrix's WHOLE spectrum theta_0 <= .. <= theta_{n-1}:

    adj_energy  = sum_l |theta_l(A)|          dist_energy = sum_l |theta_l(D)|
    lap_energy  = sum_l |theta_l(L) - s|      slap_energy = sum_l |theta_l(Q) - s|      s = float(sum of degrees) / float(n)
    adj_spread  = theta_{n-1}(A) - theta_0(A)

The whole-spectrum procedure, one IEEE f64 operation at a time, on the tridiagonal form of dense_inv_ref's one reduction of the matrix
(the same Householder steps, INV_DEFLATE at every n): R the Gershgorin bound as in dense_ah_ref.kth_eigenvalue; eigenvalue l starts
from hi = R + 1.0, lo = -hi and makes ROUNDS = 67 rounds of

    x = (lo + hi) * 0.5;  c = sturm_count(x);  if c <= l: lo = x  else: hi = x

then theta_l = (lo + hi) * 0.5.  An energy is dense_ah_ref.tree_sum64 over the n absolute values (64 slots, the rest 0.0).
A matrix's *_eig comes from the multisection, its energy from the procedure above, each only when needed: a weight that is not zero
or a term with a non-zero coefficient names it -- otherwise 0.0, and its bit (8 .. 20) of `computed` is clear.  The combination is
dense_invx_ref's over twenty-one weights.  azd_dense_invs_cost (dense_cost_host.cpp) and dense_invs_cost_wave (dense_invs_cost.inc) run the
same sequence: the three agree bit for bit.  With weights 16 .. 20 zero and no term naming them the sequence is
dense_invx_ref.invx_cost's.
Also here: the five recipes the tests add and INVX's nine converted, their ctypes form, and PyDenseInvsEngine."""
import math

import numpy as np

import dense_ah_ref as A
import dense_inv_ref as I
import dense_invx_ref as X

F = np.float32
NAMES = X.NAMES + ("adj_energy", "dist_energy", "lap_energy", "slap_energy", "adj_spread")
ADJ_ENERGY, DIST_ENERGY, LAP_ENERGY, SLAP_ENERGY, ADJ_SPREAD = range(16, 21)
INDEX_AH = I.INDEX_AH
ALWAYS = 0xFF
ROUNDS = 67
DIVISORS = X.DIVISORS + NAMES[16:]
WHICH = ("adj", "dist", "lap", "slap")  # azd_dense_invs_spectrum's `which`
# pass order of the cost: (matrix, its *_eig, its energy)
PASSES = (("dist", X.DIST_EIG, DIST_ENERGY), ("adj", X.ADJ_EIG, ADJ_ENERGY), ("lap", X.LAP_EIG, LAP_ENERGY), ("slap", X.SLAP_EIG, SLAP_ENERGY))


class Recipe(X.Recipe):
    def __init__(self, weights, terms=(), bias=0.0, adj_index=0, dist_index=INDEX_AH, lap_index=0, slap_index=0, eval_offset=0.0, eval_scale=1.0):
        assert set(weights) <= set(NAMES), weights
        self.weight = tuple(float(weights.get(k, 0.0)) for k in NAMES)
        self.terms = tuple((float(c), a, op, b) for c, a, op, b in terms)
        assert len(self.terms) <= X.MAX_TERMS and all(a in NAMES and b in NAMES and op in X.OPS and (op == "*" or b in DIVISORS) for _, a, op, b in self.terms)
        self.bias, self.adj_index, self.dist_index = float(bias), int(adj_index), int(dist_index)
        self.lap_index, self.slap_index = int(lap_index), int(slap_index)
        self.eval_offset, self.eval_scale = F(eval_offset), F(eval_scale)

    @classmethod
    def from_invx(cls, r):
        """tests/dense_invx_ref.py's Recipe, converted"""
        return cls(r.weights(), terms=r.terms, bias=r.bias, adj_index=r.adj_index, dist_index=r.dist_index, lap_index=r.lap_index, slap_index=r.slap_index,
                   eval_offset=r.eval_offset, eval_scale=r.eval_scale)

    def weights(self):
        return {k: w for k, w in zip(NAMES, self.weight) if w != 0.0}

    def needed(self):
        """bits 8 .. 20 of `computed`"""
        m = 0
        for i in range(X.ADJ_EIG, len(NAMES)):
            if self.weight[i] != 0.0:
                m |= 1 << i
        for c, a, _, b in self.terms:
            if c != 0.0:
                m |= (1 << NAMES.index(a) | 1 << NAMES.index(b)) & ~ALWAYS
        return m


def c_recipe(recipe):
    """`recipe` as an azd_dense_invs_recipe"""
    from azdopt_amd import _lib
    r = _lib.DenseInvsRecipe()
    for i, w in enumerate(recipe.weight):
        r.weight[i] = w
    r.bias, r.adj_index, r.dist_index, r.lap_index, r.slap_index = recipe.bias, recipe.adj_index, recipe.dist_index, recipe.lap_index, recipe.slap_index
    r.eval_offset, r.eval_scale = float(recipe.eval_offset), float(recipe.eval_scale)
    for t, (coef, a, op, b) in enumerate(recipe.terms):
        r.term[t].coef, r.term[t].a, r.term[t].b, r.term[t].op = coef, NAMES.index(a), NAMES.index(b), X.OPS[op]
    r.n_terms = len(recipe.terms)
    return r


# ---------------------------------------------------------------- the recipes the tests use; scales keep the evals inside [0, 1]
# Bounds on a connected graph with n >= 4 vertices: adj_energy <= n (1 + sqrt n) / 2 (Koolen-Moulton); adj_spread <= 2 lambda_1 <=
# 2 (n - 1); lap_energy, slap_energy <= sum_l (theta_l + s) = 2 * 2m <= 2 n (n - 1) (the eigenvalues of L and Q are >= 0, their sum
# is 2m); dist_energy <= sqrt(n) ||D||_F <= n^(3/2) (n - 1); an eigenvalue of A lies in [-(n - 1), n - 1], of L and Q in [0, 2 (n - 1)],
# of D in [-(n - 1)^2, (n - 1)^2].
def koolen_moulton(n):
    return n * (1.0 + math.sqrt(n)) / 2.0


def recipe_energy(n):
    """the graph energy alone: in (0, n (1 + sqrt n) / 2]"""
    return Recipe({"adj_energy": 1.0}, eval_scale=1.0 / (koolen_moulton(n) + 1.0))


def recipe_lape(n):
    """the Laplacian energy - max_degree / 4: in (-n / 4, 2 n (n - 1)]"""
    return Recipe({"lap_energy": 1.0, "max_degree": -0.25}, eval_offset=float(n), eval_scale=1.0 / (2.0 * n * n + 2.0 * n))


def recipe_spread(n):
    """the adjacency spread alone: in (0, 2 (n - 1)]"""
    return Recipe({"adj_spread": 1.0}, eval_scale=1.0 / (2.0 * n))


def recipe_eratio(n):
    """adj_energy / edges + adj_spread * proximity / 8, weight on max_degree: one DIV and one MUL term, each naming an invariant no
    weight names; energy / m <= n (1 + sqrt n) / 2 / (n - 1) < n, spread * proximity / 8 <= 2 n * n / 8"""
    return Recipe({"max_degree": -0.125}, terms=[(1.0, "adj_energy", "/", "edges"), (0.125, "adj_spread", "*", "proximity")],
                  eval_offset=float(n), eval_scale=1.0 / (n * n / 4.0 + 3.0 * n))


def recipe_alle(n):
    """all four energies, the spread and all four *_eig (at indices 1, 1, n - 2, n - 1): the heaviest recipe"""
    return Recipe({"adj_energy": 1.0, "dist_energy": -0.03125, "lap_energy": 0.25, "slap_energy": -0.125, "adj_spread": 0.5, "adj_eig": 1.0, "dist_eig": -0.125,
                   "lap_eig": 0.5, "slap_eig": -0.25}, adj_index=1, dist_index=1, lap_index=n - 2, slap_index=n - 1,
                  eval_offset=float(n ** 2.5) / 32.0 + n * n / 2.0 + 4.0 * n, eval_scale=1.0 / (n ** 2.5 / 16.0 + 2.0 * n * n + 12.0 * n))


NEW_RECIPES = ("ENERGY", "LAPE", "SPREAD", "ERATIO", "ALLE")
INVX_RECIPES = tuple(sorted(X.RECIPES))
RECIPES = dict({k: (lambda n, mk=mk: Recipe.from_invx(mk(n))) for k, mk in X.RECIPES.items()},
               ENERGY=recipe_energy, LAPE=recipe_lape, SPREAD=recipe_spread, ERATIO=recipe_eratio, ALLE=recipe_alle)


# ---------------------------------------------------------------- the whole-spectrum procedure
def whole_spectrum_scalar(diag, sub, n):
    """theta_0 .. theta_{n-1} of the tridiagonal matrix, the definition itself: Python floats, dense_ah_ref.sturm_count"""
    sub2 = [sub[i] * sub[i] for i in range(n)]
    R = 0.0
    for i in range(n):
        g = (abs(diag[i]) + (abs(sub[i - 1]) if i > 0 else 0.0)) + abs(sub[i])
        if g > R:
            R = g
    theta = []
    for l in range(n):
        hi = R + 1.0
        lo = -hi
        for _ in range(ROUNDS):
            x = (lo + hi) * 0.5
            if A.sturm_count(diag, sub2, n, x) <= l:
                lo = x
            else:
                hi = x
        theta.append((lo + hi) * 0.5)
    return theta


def whole_spectrum_many(diag, sub, n):
    """whole_spectrum_scalar(diag[g], sub[g], n) for every row g: a float64 array [rows, n].  Where the scalar form has one Python
    float operation this has one elementwise float64 numpy operation, in the same order (as dense_ah_ref.kth_eigenvalues_many)."""
    diag, sub = np.asarray(diag, np.float64).reshape(-1, n), np.asarray(sub, np.float64).reshape(-1, n)
    sub2 = sub * sub
    below = np.zeros_like(sub)
    below[:, 1:] = np.abs(sub[:, :-1])
    g = (np.abs(diag) + below) + np.abs(sub)
    R = np.fmax.reduce(np.concatenate([np.zeros((len(diag), 1)), g], axis=1), axis=1)
    hi = np.repeat((R + 1.0)[:, None], n, axis=1)
    lo = -hi
    l = np.arange(n, dtype=np.int64)[None, :]
    with np.errstate(all="ignore"):
        for _ in range(ROUNDS):
            x = (lo + hi) * 0.5
            q = diag[:, 0, None] - x
            q = np.where(np.abs(q) < A.AH_TINY, -A.AH_TINY, q)
            c = (q < 0.0).astype(np.int64)
            for i in range(1, n):
                q = (diag[:, i, None] - x) - sub2[:, i - 1, None] / q
                q = np.where(np.abs(q) < A.AH_TINY, -A.AH_TINY, q)
                c += q < 0.0
            up = c <= l
            lo, hi = np.where(up, x, lo), np.where(up, hi, x)
    return (lo + hi) * 0.5


_SPEC = {}  # (adj, n, which) -> theta, a tuple of n floats


def spectrum(adj, n, which):
    """theta_0 .. theta_{n-1} of the matrix `which` ("adj", "dist", "lap", "slap") of the graph"""
    adj = tuple(int(a) for a in adj)
    key = (adj, n, which)
    if key not in _SPEC:
        diag, sub = I._tridiagonal(adj, n, which)
        _SPEC[key] = tuple(float(t) for t in whole_spectrum_many([diag], [sub], n)[0])
    return _SPEC[key]


def prime(entries, whiches=WHICH, ks_of=lambda n: (0, 1, n - 2, n - 1)):
    """Fill the caches (the tridiagonal forms, the *_eig at the descending indices ks_of(n), the spectra) for many graphs at once:
    entries of (name, n, adj).  The same operations, the same bits, many times faster than one graph at a time."""
    I.prime(entries, whiches, ks_of)
    by_n = {}
    for _, n, adj in entries:
        by_n.setdefault(n, set()).add(tuple(int(a) for a in adj))
    for n, graphs in by_n.items():
        for which in whiches:
            todo = [g for g in sorted(graphs) if (g, n, which) not in _SPEC]
            if not todo:
                continue
            tri = [I._tridiagonal(g, n, which) for g in todo]
            th = whole_spectrum_many([t[0] for t in tri], [t[1] for t in tri], n)
            for i, g in enumerate(todo):
                _SPEC[(g, n, which)] = tuple(float(t) for t in th[i])


def mean_degree(adj, n):
    return float(sum(X.degrees(adj))) / float(n)


def energy(adj, n, which):
    """sum_l |theta_l| (adjacency, distance) or sum_l |theta_l - s| (the Laplacians), by the tree sum over 64 slots"""
    th = spectrum(adj, n, which)
    if which in ("lap", "slap"):
        s = mean_degree(adj, n)
        return A.tree_sum64([abs(t - s) for t in th])
    return A.tree_sum64([abs(t) for t in th])


def spread(adj, n):
    th = spectrum(adj, n, "adj")
    return th[n - 1] - th[0]


# ---------------------------------------------------------------- the cost
def invs_cost(adj, n, recipe):
    """The whole objective of one connected graph under `recipe`; adj = n neighbourhood bitsets (ints)."""
    assert 4 <= n <= A.AH_MAX_N
    adj = tuple(int(a) for a in adj)
    _, s = I._stages(adj, n)
    dist_k = I.dist_index_of(recipe, s["diam"], n)
    inv = [float(s["m"]), float(s["max_deg"]), float(s["min_deg"]), float(s["diam"]), float(s["rad"]),
           float(s["min_t"]) / float(n - 1), float(s["max_t"]) / float(n - 1), float(s["sum_t"]) / float(n * (n - 1))] + [0.0] * 13
    need = recipe.needed()
    index = dict(dist=dist_k, adj=recipe.adj_index, lap=recipe.lap_index, slap=recipe.slap_index)
    for which, eig_i, energy_i in PASSES:
        if need >> eig_i & 1:
            inv[eig_i] = I._eig(adj, n, which, index[which])
        if need >> energy_i & 1:
            inv[energy_i] = energy(adj, n, which)
    if need >> ADJ_SPREAD & 1:
        inv[ADJ_SPREAD] = spread(adj, n)
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
    cost = F(c)
    ev = recipe.eval_scale * (cost + recipe.eval_offset)
    out = dict(zip(NAMES, inv))
    out.update(dist_k=dist_k, computed=ALWAYS | need, cost=cost, eval=ev)
    return out


# ---------------------------------------------------------------- the engine
class PyDenseInvsEngine(A.PyDenseEngine):
    """tests/dense_ah_ref.py's engine of the dense-graph space with the spectrum invariant cost under one recipe"""

    def __init__(self, n, batch, recipe, p=0.2):
        super().__init__(n, batch, cost="invs", p=p)
        self.recipe = recipe

    def cost(self, st):
        return dict(invs_cost(st.adj, self.n, self.recipe))
