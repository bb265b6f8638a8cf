"""Python reference of the Aouchiche-Hansen cost of the dense-graph space (test infrastructure; DESIGN.md "The AH cost").

The objective is restated from the reference's ConnectedBitsetGraph::ah_cost
(graph-state/src/simple_graph/connected_bitset_graph/mod.rs:156-198), not ported:

    BFS from every vertex -> distance matrix d(u, v), transmissions t(u) = sum_v d(u, v), diameter D = max d
    proximity   pi  = min_u t(u) / (n - 1)                        one f64 division
    index       k   = floor(2 D / 3) - 1 if floor(2 D / 3) >= 1 else n - 1      (checked_sub(1).unwrap_or(N - 1))
    eigenvalue  d_k = entry k (0-based) of the distance matrix's eigenvalues sorted descending
    cost        = (f32)(pi + d_k)                                 the sum in f64, cast once

BUILD-DEFINED, in the image of the dense space: eval = slope * (cost + 2.0f) with slope = 1.0f / (2 n + 2).

The eigenvalue procedure stands in for faer: Householder reduction of the distance matrix to tridiagonal form, then a
Sturm-count multisection (64 shifts per round, AH_ROUNDS rounds) for the one eigenvalue wanted.  It is written one IEEE f64
operation at a time with every reduction in a fixed order (tree_sum64 = the xor-butterfly of a 64-lane wave), the same sequence
as azd_dense_ah_cost (dense_cost_host.cpp) and dense_ah_cost_wave (dense_ah_cost.inc): the three agree bit for bit.  Plain Python floats
are IEEE binary64 and Python never contracts a * b + c.
"""
import functools
import math

import numpy as np

AH_MAX_N = 32
AH_ROUNDS = 11           # 64 shifts cut the bracket by 65 a round: 65^11 > 2^66
AH_TINY = 2.0 ** -512    # a Sturm pivot below this in magnitude is replaced by -AH_TINY (no division by zero, no overflow)


def tree_sum64(vals):
    """Balanced binary tree over 64 slots, adjacent pairs first: what `v += shfl_xor(v, w)` for w = 1, 2, .. 32 leaves in every lane."""
    v = list(vals) + [0.0] * (64 - len(vals))
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def bfs_all(adj, n):
    """Distance matrix, transmissions and eccentricities of the connected graph adj (neighbourhood bitsets): integer work."""
    dist = [[0] * n for _ in range(n)]
    trans, ecc = [0] * n, [0] * n
    for u in range(n):
        seen = frontier = 1 << u
        d = 0
        while True:
            nxt = 0
            f = frontier
            while f:
                w = (f & -f).bit_length() - 1
                f &= f - 1
                nxt |= adj[w]
            nxt &= ~seen
            if not nxt:
                break
            d += 1
            m = nxt
            while m:
                v = (m & -m).bit_length() - 1
                m &= m - 1
                dist[u][v] = d
            trans[u] += d * bin(nxt).count("1")
            seen |= nxt
            frontier = nxt
        assert seen == (1 << n) - 1, "graph is not connected"
        ecc[u] = d
    return dist, trans, ecc


def ah_index(diam, n):
    q = (2 * diam) // 3
    return q - 1 if q >= 1 else n - 1


def tridiagonalise(dist, n, deflate=0.0):
    """Householder reduction of the symmetric matrix to tridiagonal (diag, sub): step i annihilates column i below row i + 1.
    deflate: a column whose tail is below it is left as it is, like one whose tail is zero.  0.0 (none) for the AH cost, whose
    bits tests/golden/ah_cost_vectors.json pins; the invariant costs pass dense_inv_ref.INV_DEFLATE at every n."""
    A = [[float(x) for x in row] for row in dist]
    diag, sub = [0.0] * n, [0.0] * n  # sub[i] couples i and i + 1; sub[n - 1] = 0
    for i in range(n - 2):
        x = [A[r][i] if r > i else 0.0 for r in range(n)]
        tail = tree_sum64([x[r] * x[r] if r > i + 1 else 0.0 for r in range(n)])
        x1 = x[i + 1]
        diag[i] = A[i][i]
        if tail == 0.0 or tail < deflate:  # already tridiagonal in this column, or rounding noise of a matrix whose rank is used up
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
            Ar = A[r]
            for c in range(i + 1, n):
                acc = acc + Ar[c] * v[c]
            p[r] = beta * acc
        vp = tree_sum64([v[r] * p[r] if r > i else 0.0 for r in range(n)])
        K = (0.5 * beta) * vp
        q = [p[r] - K * v[r] if r > i else 0.0 for r in range(n)]
        for r in range(i + 1, n):
            Ar, vr, qr = A[r], v[r], q[r]
            for c in range(i + 1, n):
                Ar[c] = Ar[c] - (vr * q[c] + qr * v[c])
        sub[i] = alpha
    diag[n - 2] = A[n - 2][n - 2]
    sub[n - 2] = A[n - 1][n - 2]
    diag[n - 1] = A[n - 1][n - 1]
    return diag, sub


def sturm_count(diag, sub2, n, x):
    """Number of eigenvalues of the tridiagonal matrix below x (sub2 = squared subdiagonal)."""
    q = diag[0] - x
    if abs(q) < AH_TINY:
        q = -AH_TINY
    c = 1 if q < 0.0 else 0
    for i in range(1, n):
        q = (diag[i] - x) - sub2[i - 1] / q
        if abs(q) < AH_TINY:
            q = -AH_TINY
        if q < 0.0:
            c += 1
    return c


def kth_eigenvalue(diag, sub, n, k):
    """Entry k of the eigenvalues sorted descending = ascending index j = n - 1 - k, by multisection."""
    j = n - 1 - k
    sub2 = [sub[i] * sub[i] for i in range(n)]
    R = 0.0
    for i in range(n):
        g = (abs(diag[i]) + (abs(sub[i - 1]) if i > 0 else 0.0)) + abs(sub[i])
        if g > R:
            R = g
    hi = R + 1.0
    lo = -hi
    for _ in range(AH_ROUNDS):
        w = hi - lo
        xs = [lo + (w * float(l + 1)) / 65.0 for l in range(64)]
        m = sum(1 for l in range(64) if sturm_count(diag, sub2, n, xs[l]) <= j)
        new_lo = xs[m - 1] if m > 0 else lo
        new_hi = xs[m] if m < 64 else hi
        lo, hi = new_lo, new_hi
    return (lo + hi) * 0.5


# ---------------------------------------------------------------- the two spectral stages over many matrices at once
# tridiagonalise and kth_eigenvalue again, with the matrices of one size along the leading axis of numpy arrays: where the scalar
# form has one Python float operation, these have one elementwise float64 numpy operation (IEEE, never fused), in the same order,
# with the same fixed-order sums.  They exist because the scalar forms take tens of milliseconds a matrix and the hard case set
# (tests/dense_spectral_cases.py) has thousands; test_dense_spectral_cases.py holds them to the scalar forms bit for bit.
def _tree_sum64_many(v):
    """tree_sum64 along the last axis (at most 64 slots)"""
    pad = np.zeros(v.shape[:-1] + (64,))
    pad[..., :v.shape[-1]] = v
    while pad.shape[-1] > 1:
        pad = pad[..., 0::2] + pad[..., 1::2]
    return pad[..., 0]


def tridiagonalise_many(mats, n, deflate=0.0):
    """tridiagonalise(m, n, deflate) for every m of mats: (diag, sub), two float64 arrays [len(mats), n]"""
    M = np.array(mats, dtype=np.float64).reshape(-1, n, n)
    G = M.shape[0]
    diag, sub = np.zeros((G, n)), np.zeros((G, n))
    with np.errstate(all="ignore"):  # (a column that is skipped still goes through the arithmetic; its results are dropped)
        for i in range(n - 2):
            x = np.zeros((G, n))
            x[:, i + 1:] = M[:, i + 1:, i]
            sq = x * x
            sq[:, :i + 2] = 0.0
            tail = _tree_sum64_many(sq)
            x1 = x[:, i + 1]
            diag[:, i] = M[:, i, i]
            skip = (tail == 0.0) | (tail < deflate)
            sigma = tail + x1 * x1
            s = np.sqrt(sigma)
            alpha = np.where(x1 >= 0.0, -s, s)
            v = x.copy()
            v1 = x1 - alpha
            v[:, i + 1] = v1
            beta = 2.0 / (tail + v1 * v1)
            acc = np.zeros((G, n))
            for c in range(i + 1, n):
                acc = acc + M[:, :, c] * v[:, c:c + 1]
            p = beta[:, None] * acc
            p[:, :i + 1] = 0.0
            vp = _tree_sum64_many(v * p)
            K = (0.5 * beta) * vp
            q = p - K[:, None] * v
            q[:, :i + 1] = 0.0
            B = M[:, i + 1:, i + 1:]
            new = B - (v[:, i + 1:, None] * q[:, None, i + 1:] + q[:, i + 1:, None] * v[:, None, i + 1:])
            M[:, i + 1:, i + 1:] = np.where(skip[:, None, None], B, new)
            sub[:, i] = np.where(skip, x1, alpha)
    diag[:, n - 2] = M[:, n - 2, n - 2]
    sub[:, n - 2] = M[:, n - 1, n - 2]
    diag[:, n - 1] = M[:, n - 1, n - 1]
    return diag, sub


def kth_eigenvalues_many(diag, sub, n, ks):
    """kth_eigenvalue(diag[g], sub[g], n, k) for every row g and every k of ks: a float64 array [rows, len(ks)]"""
    diag, sub = np.asarray(diag, np.float64), np.asarray(sub, np.float64)
    j = (n - 1 - np.asarray(ks, np.int64))[None, :, None]
    sub2 = sub * sub
    below = np.zeros_like(sub)
    below[:, 1:] = np.abs(sub[:, :-1])
    g = (np.abs(diag) + below) + np.abs(sub)
    R = np.fmax.reduce(np.concatenate([np.zeros((len(diag), 1)), g], axis=1), axis=1)  # (`if g > R`: a NaN is passed over)
    hi = np.repeat((R + 1.0)[:, None], len(ks), axis=1)
    lo = -hi
    lanes = np.arange(1, 65, dtype=np.float64)
    with np.errstate(all="ignore"):
        for _ in range(AH_ROUNDS):
            w = hi - lo
            xs = lo[:, :, None] + (w[:, :, None] * lanes) / 65.0
            q = diag[:, 0, None, None] - xs
            q = np.where(np.abs(q) < AH_TINY, -AH_TINY, q)
            c = (q < 0.0).astype(np.int64)
            for i in range(1, n):
                q = (diag[:, i, None, None] - xs) - sub2[:, i - 1, None, None] / q
                q = np.where(np.abs(q) < AH_TINY, -AH_TINY, q)
                c += q < 0.0
            m = (c <= j).sum(axis=2)
            x_lo = np.take_along_axis(xs, np.maximum(m - 1, 0)[:, :, None], axis=2)[:, :, 0]
            x_hi = np.take_along_axis(xs, np.minimum(m, 63)[:, :, None], axis=2)[:, :, 0]
            lo, hi = np.where(m > 0, x_lo, lo), np.where(m < 64, x_hi, hi)
    return (lo + hi) * 0.5


def eval_slope(n):
    return np.float32(1.0) / np.float32(2 * n + 2)


@functools.lru_cache(maxsize=None)
def _ah_cost_cached(adj, n):
    dist, trans, ecc = bfs_all(adj, n)
    diam = max(ecc)
    prox = float(min(trans)) / float(n - 1)
    k = ah_index(diam, n)
    diag, sub = tridiagonalise(dist, n)
    eig = kth_eigenvalue(diag, sub, n, k)
    cost = np.float32(prox + eig)
    ev = eval_slope(n) * (cost + np.float32(2.0))
    return dict(proximity=prox, eigenvalue=eig, diameter=diam, k=k, cost=cost, eval=ev)


def ah_cost(adj, n):
    """The whole objective of one connected graph; adj = n neighbourhood bitsets (ints)."""
    assert 4 <= n <= AH_MAX_N
    return _ah_cost_cached(tuple(int(a) for a in adj), n)


# ---------------------------------------------------------------- graphs
def from_edges(n, edges):
    adj = [0] * n
    for u, v in edges:
        assert u != v
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    return adj


def path(n):
    return from_edges(n, [(i, i + 1) for i in range(n - 1)])


def star(n):
    return from_edges(n, [(0, i) for i in range(1, n)])


def cycle(n):
    return from_edges(n, [(i, (i + 1) % n) for i in range(n)])


def complete(n):
    return from_edges(n, [(i, j) for i in range(n) for j in range(i)])


def double_broom(n, a, b):
    """A path with a pendant vertices on one end and b on the other (n = path length + a + b)."""
    L = n - a - b
    assert L >= 2
    e = [(i, i + 1) for i in range(L - 1)]
    e += [(0, L + i) for i in range(a)] + [(L - 1, L + a + i) for i in range(b)]
    return from_edges(n, e)


def connected(adj, n):
    seen = frontier = 1
    while frontier:
        nxt = 0
        f = frontier
        while f:
            w = (f & -f).bit_length() - 1
            f &= f - 1
            nxt |= adj[w]
        frontier = nxt & ~seen
        seen |= nxt
    return seen == (1 << n) - 1


def gnp_connected(rng, n, p):
    """G(n, p) redrawn until connected (05-ah.rs:93 draws its roots this way)."""
    while True:
        adj = [0] * n
        for v in range(1, n):
            for u in range(v):
                if rng.random() < p:
                    adj[v] |= 1 << u
                    adj[u] |= 1 << v
        if connected(adj, n):
            return adj


@functools.lru_cache(maxsize=None)
def graph_set():
    """The graphs every AH check runs over: (name, n, adj) -- structured families and G(n, p), n = 4 .. 32, 560 in all."""
    out = []
    for n in range(4, AH_MAX_N + 1):
        out.append(("path", n, path(n)))
        out.append(("star", n, star(n)))
        out.append(("cycle", n, cycle(n)))
        out.append(("complete", n, complete(n)))
        if n >= 6:
            out.append(("broom", n, double_broom(n, (n - 2) // 3, (n - 2) // 3)))
            out.append(("broom", n, double_broom(n, 1, n - 4)))
    rng = np.random.default_rng(20240531)
    ps = (0.05, 0.1, 0.15, 0.2, 0.3, 0.4, 0.5, 0.6)
    i = 0
    while len(out) < 560:
        n = 4 + i % (AH_MAX_N - 3)
        p = ps[(i // 7) % len(ps)]
        if p < 1.5 * math.log(n) / n:
            # below the connectivity threshold a redraw-until-connected loop does not end: G(n, p) over a random spanning tree
            # instead (sparse, long diameters)
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
            out.append(("gnp%.2f+tree" % p, n, adj))
        else:
            out.append(("gnp%.2f" % p, n, gnp_connected(rng, n, p)))
        i += 1
    return tuple((name, n, tuple(adj)) for name, n, adj in out)


# ---------------------------------------------------------------- the dense-graph space under the search tree
# A Python engine of the dense-graph space over oracle.py_oracle's tree (selection, cascade), the way oracle/py_ramsey.py plugs
# the Ramsey space in: state, act, legal actions, state vector and root policy restated from the space's definition
# (oracle/dense_graph.inc's header), the cost either the AH procedure above ("ah") or, for validating this glue against the C++
# oracle engine, lambda_1 + matching number taken from the oracle library's own primitives ("c21": bit-exact by construction).
from oracle import py_oracle as po  # noqa: E402

F = np.float32
CTRS = ("EXPANSIONS", "TERMINALS", "TRANSPOSITIONS", "VISITED_STEPS", "ROOT_EXHAUSTED")


def from_colex(e):  # simple_graph/edge.rs:55-65
    v = 1
    while v * (v + 1) // 2 <= e:
        v += 1
    return v, e - v * (v - 1) // 2


def is_cut_edge(adj, v, u):  # connected_bitset_graph/mod.rs:47-71
    new = adj[v] ^ (1 << u)
    explored = 1 << v
    while new:
        if (new >> u) & 1:
            return False
        explored |= new
        recent, new = new, 0
        while recent:
            w = (recent & -recent).bit_length() - 1
            recent &= recent - 1
            new |= adj[w]
        new &= ~explored
    return True


class DenseState:
    def __init__(self, adj, slots):
        self.adj, self.slots = [int(a) for a in adj], set(slots)

    def clone(self):
        return DenseState(self.adj, self.slots)


class Tree:
    FIELDS = ("c", "c_star", "n_t", "exhausted", "act_begin", "act_end", "keys", "e_src", "e_dst", "e_pp", "p_aid", "p_g", "p_edge")

    def __init__(self, **kw):
        self.__dict__.update(kw)


class PyDenseEngine(po.PyEngine):
    """NablaOptimizer<dense-graph space, M, ActionSet> with an injectable model.  cost: "ah" | "c21".  p: the edge probability of
    the root policy's fresh roots, rounded the way the engine rounds azd_engine_config::dense_p (a float)."""

    def __init__(self, n, batch, cost="ah", p=0.2):
        self.n, self.B, self.seq, self.cost_kind = n, batch, False, cost
        self.E = n * (n - 1) // 2
        self.S, self.A = 3 * self.E + 1, 2 * self.E
        self.KW = (self.A + 63) // 64
        self.p24 = int(float(np.float32(p)) * 16777216.0 + 0.5)
        self.pairs = [from_colex(e) for e in range(self.E)]
        self.ctr = dict.fromkeys(CTRS, 0)
        self.set_layers(1)

    def clone_state(self, st):
        return st.clone()

    # ---- space
    def act(self, st, a):  # AddOrDeleteEdge (action.rs:20-27); the slot is used up
        slot = a % self.E
        mx, mn = self.pairs[slot]
        st.adj[mx] ^= 1 << mn
        st.adj[mn] ^= 1 << mx
        st.slots.discard(slot)

    def legal(self, st):  # action_kinds (mod.rs:139-158) over the remaining slots, ascending action id
        adds, dels = [], []
        for slot in sorted(st.slots):
            mx, mn = self.pairs[slot]
            if not (st.adj[mx] >> mn) & 1:
                adds.append(slot)
            elif not is_cut_edge(st.adj, mx, mn):
                dels.append(self.E + slot)
        return adds + dels

    def inner_vec(self, st):
        E = self.E
        v = np.zeros(self.S_inner, F)
        for e, (mx, mn) in enumerate(self.pairs):
            if (st.adj[mx] >> mn) & 1:
                v[e] = 1
        for slot in st.slots:
            mx, mn = self.pairs[slot]
            v[(2 * E if (st.adj[mx] >> mn) & 1 else E) + slot] = 1
        v[3 * E] = F(len(st.slots)) / F(E)
        return v

    def cost(self, st):
        if self.cost_kind == "ah":
            return dict(ah_cost(st.adj, self.n))
        from oracle import orc
        lam, mu = orc.dense_lambda1(st.adj), orc.dense_matching_exact(st.adj)
        return dict(lambda1=lam, matching=mu, eval=po.evaluate(self.n, lam, mu))

    # ---- roots: (adj bytes [B, 8 n], slot masks u64 [B, KW]) as DenseGraphSpace.generate_roots hands them over
    def unpack(self, adj_bytes, slots):
        adj = np.ascontiguousarray(adj_bytes, np.uint8).view(np.uint64).reshape(self.B, self.n)
        slots = np.ascontiguousarray(slots, np.uint64).reshape(self.B, -1)
        return [DenseState(adj[i], {e for e in range(self.E) if (int(slots[i, e >> 6]) >> (e & 63)) & 1}) for i in range(self.B)]

    def pack(self, states):
        adj = np.array([st.adj for st in states], np.uint64)
        return adj.view(np.uint8).reshape(self.B, 8 * self.n), np.array([self.mask(st.slots) for st in states], np.uint64)

    def mask(self, ids):
        m = [0] * self.KW
        for a in ids:
            m[a >> 6] |= 1 << (a & 63)
        return m

    # ---- optimizer
    def _begin(self, adj_bytes, slots):
        self.roots = self.unpack(adj_bytes, slots)
        self.states = [r.clone() for r in self.roots]
        self.costs = [self.cost(r) for r in self.roots]
        self.paths = [[] for _ in self.roots]
        self.posn = [0] * self.B
        self.older = [[] for _ in range(self.B)]
        for i in range(self.B):
            self.write_row(i, self.states[i], [])

    def new_begin(self, adj_bytes, slots):
        self._begin(adj_bytes, slots)
        self.inspected = [0] * self.B

    reset_begin = _begin

    def _root_tree(self, i, h_row):
        t = po.PyTree()
        t.add_node(self.key([]), self.costs[i]["eval"])
        t.add_actions(0, self.legal(self.roots[i]), h_row)
        return t

    def new_end(self, h):
        self.trees = [self._root_tree(i, h[i]) for i in range(self.B)]
        best = min(range(self.B), key=lambda i: (self.costs[i]["eval"], i))
        self.argmin = dict(self.cost(self.states[best]), state=self.states[best].clone())

    def _step(self, i, tol, tol_default):
        t, st, path = self.trees[i], self.states[i], self.paths[i]
        while True:
            tl = tol[len(path)] if len(path) < len(tol) else tol_default
            ch = t.select(self.posn[i], tl)
            if ch is None:
                assert not path
                self.ctr["ROOT_EXHAUSTED"] += 1
                return
            if ch[0] == "V":
                _, dst, pp = t.edge[ch[1]]
                a = t.pred[pp][0]
                path.append(a)
                self.act(st, a)
                self.posn[i] = dst
                self.ctr["VISITED_STEPS"] += 1
                continue
            pp = ch[1]
            a = t.pred[pp][0]
            path.append(a)
            key = self.key(path)
            hit = t.pos.get(key)
            if hit is not None:
                self.ctr["TRANSPOSITIONS"] += 1
                t.cascade(t.add_edge(self.posn[i], hit, pp), True)
            else:
                self.act(st, a)
                self.costs[i] = self.cost(st)
                v = t.add_node(key, self.costs[i]["eval"])
                e = t.add_edge(self.posn[i], v, pp)
                if self.legal(st):
                    self.posn[i] = v
                    self.ctr["EXPANSIONS"] += 1  # (a new node that takes predictions; a terminal one counts as TERMINALS)
                    return
                self.ctr["TERMINALS"] += 1
                t.cascade(e, False)
            st = self.states[i] = self.roots[i].clone()
            self.costs[i] = None  # (the agent's record is the last NEW node's; back at the root it is not read)
            path.clear()
            self.posn[i] = 0

    def rollout_end(self, h):
        for i in range(self.B):
            if self.paths[i]:
                self.trees[i].add_actions(self.posn[i], self.legal(self.states[i]), h[i])
        best = None
        for i, t in enumerate(self.trees):  # optimizer/mod.rs:194-246; cross-tree ties -> lowest tree index
            for j in range(self.inspected[i], len(t.node)):
                c = t.node[j]["c"]
                if c < self.argmin["eval"] and (best is None or c < best[0]):
                    best = (c, i, j)
            self.inspected[i] = len(t.node)
        if best is None:
            return 0
        _, i, j = best
        st = self.roots[i].clone()
        for a in self.actions_taken(next(k for k, v in self.trees[i].pos.items() if v == j)):
            self.act(st, a)
        self.argmin = dict(self.cost(st), state=st, agent=i, node=j)
        return 1

    def fresh_root(self, seed, domain, agent, k):
        """oracle gen_dense_root: G(n, p) redrawn until connected, then k of the E slots"""
        n, E = self.n, self.E
        t = 0
        while True:
            adj = [0] * n
            for e, (mx, mn) in enumerate(self.pairs):
                if (po.key4(seed, domain, agent, 4096 + t * E + e) >> 40) < self.p24:
                    adj[mx] |= 1 << mn
                    adj[mn] |= 1 << mx
            if connected(adj, n):
                return DenseState(adj, po.shuffle_prefix(seed, domain, agent, E, k))
            t += 1

    def modify_roots(self, seed, epoch, first_agent, kmin, kmax):  # 04-c21-tree.rs:172-206 over this space, seeded
        domain = po.D_RESET ^ ((epoch << 32) & po.M64)
        out = []
        for i, t in enumerate(self.trees):
            agent = first_agent + i
            r0, r1 = po.key4(seed, domain, agent, 0), po.key4(seed, domain, agent, 1)
            st = self.roots[i].clone()
            order = sorted(t.pos.items(), key=lambda kv: self.actions_taken(kv[0]))  # BTreeMap order
            c_root, c_root_star = t.node[0]["c"], t.node[0]["cs"]
            if c_root == c_root_star:
                kcur = len(st.slots)
                if kcur == kmax:
                    out.append(self.fresh_root(seed, domain, agent, kmin + po.below(r1, kmax - kmin + 1)))
                    continue
                keep = [k for k, v in order if t.node[v]["c"] == c_root]
                k_new = kcur + po.below(r1, kmax - kcur + 1)
            else:
                thr = (c_root + F(3.0) * c_root_star) / F(4.0)
                keep = [k for k, v in order if t.node[v]["c"] <= thr]
                k_new = kmin + po.below(r1, kmax - kmin + 1)
            for a in self.actions_taken(keep[po.below(r0, len(keep))]):
                self.act(st, a)
            out.append(DenseState(st.adj, po.shuffle_prefix(seed, domain, agent, self.E, k_new)))
        return self.pack(out)

    # ---- reads, in the engines' formats
    def state_vecs(self):
        return self.vecs.copy()

    def export_tree(self, i):
        return Tree(**po.PyEngine.export_tree(self, i, self.KW))

    def counters(self):
        return dict(self.ctr)

    def agent_state(self, i):
        st = self.states[i]
        out = dict(parents=np.array(st.adj, np.uint64).view(np.uint8), permitted=np.array(self.mask(st.slots), np.uint64),
                   path=np.array(self.mask(self.paths[i]), np.uint64), state_pos=self.posn[i])
        if self.costs[i] is not None:
            out.update({k: v for k, v in self.costs[i].items() if k != "eval"})
        return out
