"""A Ramsey reference that keeps up past N = 32: oracle.py_ramsey.PyRamseyEngine (the tree, the space glue and the root policy
are its own, imported) over a state that MAINTAINS the per-edge clique counts instead of recounting them from the definition
after every action.  A test helper, not a conftest.

The state is written from the reference's update (graph-state/src/ramsey_counts/mod.rs:78-160: reassign_color and
reassign_color_count_adjustment; RamseyCounts::new, mod.rs:20-68, for a root) on Python-int bitsets, so a neighbourhood has
whatever width N asks for -- there is no 32- or 64-bit word in it.  tests/test_ramsey64_reference.py pins it against the C++
oracle (N <= 32) and against RamseyState.recount (N = 33 .. 48) before anything on the device is compared with it."""
from oracle import py_ramsey as pr


def bits(x):
    while x:
        b = x & -x
        yield b.bit_length() - 1
        x ^= b


def pos(a, b):  # simple_graph/edge.rs:48-53 colex_position
    return a * (a - 1) // 2 + b if a > b else b * (b - 1) // 2 + a


def cliques_inside(nb, s, k):
    """number of k-cliques of the graph `nb` (neighbourhood bitsets) inside the vertex set `s`"""
    if k == 0:
        return 1
    if k == 1:
        return bin(s).count("1")
    total = 0
    for u in bits(s):
        total += cliques_inside(nb, s & nb[u] & ((1 << u) - 1), k - 1)
    return total


class IncRamseyState(pr.RamseyState):
    """RamseyState with incrementally maintained counts; `recount` (inherited) stays the definition to check against"""

    def __init__(self, n, sizes, colors, permitted):
        self.n, self.sizes = n, sizes
        self.colors = list(colors)
        self.permitted = set(permitted)
        C = len(sizes)
        self.nb = [[0] * n for _ in range(C)]
        for e, (v, u) in enumerate(pr.edges(n)):
            self.nb[self.colors[e]][v] |= 1 << u
            self.nb[self.colors[e]][u] |= 1 << v
        self.counts, self.totals = [], []
        for c, k in enumerate(sizes):  # mod.rs:20-68
            nb, row, tot = self.nb[c], [], 0
            for v, u in pr.edges(n):
                cnt = cliques_inside(nb, nb[v] & nb[u], k - 2)
                row.append(cnt)
                if (nb[v] >> u) & 1:
                    tot += cnt
            self.counts.append(row)
            self.totals.append(tot // (k * (k - 1) // 2))

    def clone(self):
        s = IncRamseyState.__new__(IncRamseyState)
        s.n, s.sizes, s.colors, s.permitted = self.n, self.sizes, list(self.colors), set(self.permitted)
        s.counts, s.totals = [list(r) for r in self.counts], list(self.totals)
        s.nb = [list(r) for r in self.nb]
        return s

    def _adjust(self, sign, u, v, c):  # mod.rs:101-160, the edge uv absent from colour c's graph
        size = self.sizes[c]
        if size <= 2:
            return
        nb, cnt = self.nb[c], self.counts[c]
        n_u, n_v = nb[u], nb[v]
        n_uv = n_u & n_v
        for w in bits(n_u):  # edge {v, w}
            cnt[pos(v, w)] += sign * cliques_inside(nb, n_uv & nb[w], size - 3)
        for w in bits(n_v):  # edge {u, w}
            cnt[pos(u, w)] += sign * cliques_inside(nb, n_uv & nb[w], size - 3)
        if size == 3:
            return
        common = list(bits(n_uv))
        for i, w in enumerate(common):  # edge {w, x}, w < x both in n_uv
            n_uvw = n_uv & nb[w]
            for x in common[i + 1:]:
                cnt[pos(w, x)] += sign * cliques_inside(nb, n_uvw & nb[x], size - 4)

    def act(self, a):  # space.rs:71-86: reassign_color (mod.rs:78-99) + permitted_edges.remove
        E = len(self.colors)
        e, nc = a % E, a // E
        v, u = edge_of(e)
        oc = self.colors[e]
        self.nb[oc][v] ^= 1 << u
        self.nb[oc][u] ^= 1 << v
        self._adjust(-1, u, v, oc)
        self._adjust(+1, u, v, nc)
        self.nb[nc][v] ^= 1 << u
        self.nb[nc][u] ^= 1 << v
        self.totals[oc] -= self.counts[oc][e]
        self.totals[nc] += self.counts[nc][e]
        self.colors[e] = nc
        self.permitted.discard(e)


def edge_of(e):
    v = 1
    while v * (v + 1) // 2 <= e:
        v += 1
    return v, e - v * (v - 1) // 2


class Ramsey64RefEngine(pr.PyRamseyEngine):
    """PyRamseyEngine whose roots (and so every state cloned from them) are IncRamseyState: the two methods that build roots
    are restated with the other state class, everything else is inherited"""

    def new_begin(self, roots):  # roots: list of (colors, permitted edge set)
        self.inspected = [0] * self.B
        self.reset_begin(roots)

    def reset_begin(self, roots):
        self.roots = [IncRamseyState(self.n, self.sizes, c, m) for c, m in roots]
        self.states = [r.clone() for r in self.roots]
        self.costs = [self.evaluate(r) for r in self.roots]
        self.paths = [[] for _ in roots]
        self.posn = [0] * self.B
        self.older = [[] for _ in range(self.B)]
        for i in range(self.B):
            self.write_row(i, self.states[i], [])


# ---- packed roots <-> the engines' (colors list, permitted edge set)
def unpack_roots(colors, permitted, E):
    out = []
    for i in range(colors.shape[0]):
        mask = sum(int(permitted[i, w]) << (64 * w) for w in range(permitted.shape[1]))
        out.append(([int(c) for c in colors[i]], {e for e in range(E) if mask >> e & 1}))
    return out


def pack_roots(roots, E, kw):
    import numpy as np
    colors = np.zeros((len(roots), E), np.uint8)
    permitted = np.zeros((len(roots), kw), np.uint64)
    for i, (c, m) in enumerate(roots):
        colors[i] = c
        for e in m:
            permitted[i, e >> 6] |= np.uint64(1 << (e & 63))
    return colors, permitted
