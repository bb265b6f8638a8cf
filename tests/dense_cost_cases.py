"""The case set of the dense-graph space's default cost (lambda_1 + matching number): connected graphs of the families on which
a matching repair or a power iteration goes wrong first, each with 16 seeded edge toggles that keep it connected.  Shared by
test_dense_cost_cases.py (the oracle's procedures against each other and against LAPACK, CPU) and test_gpu_dense_cost.py (the
device's cost kernel against the oracle, step by step).  Pure Python and numpy, seeded: the same set on every machine.

A graph is a list of n Python ints, the neighbourhood bitsets; an edge slot is the colex position v (v - 1) / 2 + u of {u, v},
u < v.  A toggle ADDS the edge at its slot if it is absent and DELETES it if it is present; no slot is used twice in a sequence,
and no deletion removes a cut edge (the rule of the space: action_kinds)."""
import functools
import zlib
from collections import namedtuple

import numpy as np

SIZES = (4, 5, 8, 9, 20, 31, 32, 33, 50, 63, 64)
N_TOGGLES = 16
GNP = (0.03, 0.1, 0.4)
NEAR_TREE_TRIALS = tuple(range(20)) + (180,)  # trial 180: n = 64, 64 edges, gap to lambda_2 3.6e-3 -- the iteration ends at its step cap

# kind: "random" (16 random toggles) or "delete_matched" / "add_matched" (a targeted first toggle, then 15 random ones).
# start_mate: the greedy start matching where it is already maximum -- then it IS the matching the device holds at step 0
# (a search that fails changes nothing) -- else None.
Case = namedtuple("Case", "name family n adj toggles kind start_mate")


def n_toggles(n):
    """16; below 8 vertices half the slots there are (n = 4: 3 of 6, n = 5: 5 of 10)"""
    return N_TOGGLES if n >= 8 else n * (n - 1) // 4


# ---------------------------------------------------------------- graphs
def from_edges(n, edges):
    adj = [0] * n
    for u, v in edges:
        assert u != v and 0 <= u < n and 0 <= v < n, (n, u, v)
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    return adj


def edges_of(adj):
    return [(u, v) for v in range(len(adj)) for u in range(v) if (adj[v] >> u) & 1]


def colex(u, v):
    u, v = min(u, v), max(u, v)
    return v * (v - 1) // 2 + u


def from_colex(slot):
    v = 1
    while v * (v + 1) // 2 <= slot:
        v += 1
    return slot - v * (v - 1) // 2, v


def is_connected(adj):
    n = len(adj)
    seen = frontier = 1
    while frontier:
        nxt = 0
        for v in range(n):
            if (frontier >> v) & 1:
                nxt |= adj[v]
        frontier = nxt & ~seen
        seen |= nxt
    return seen == (1 << n) - 1


def toggled(adj, slot):
    u, v = from_colex(slot)
    out = list(adj)
    out[u] ^= 1 << v
    out[v] ^= 1 << u
    return out


def greedy_matching(adj):
    """dense_matching_scratch's start (and the oracle's): every vertex in ascending order, if still free, takes its lowest free neighbour"""
    n = len(adj)
    mate = [0xFF] * n
    for v in range(n):
        if mate[v] != 0xFF:
            continue
        for u in range(n):
            if (adj[v] >> u) & 1 and mate[u] == 0xFF:
                mate[v], mate[u] = u, v
                break
    return mate


def matching_number(adj):
    """the matching number by the textbook blossom search, in plain Python: the generators ask it whether a greedy matching is
    maximum (test_dense_cost_cases.py holds it against the oracle's three procedures over the whole set)"""
    n = len(adj)
    mate = greedy_matching(adj)
    mate = [-1 if m == 0xFF else m for m in mate]

    def find_path(root):
        p, base = [-1] * n, list(range(n))
        used, q = {root}, [root]

        def lca(a, b):
            mark = set()
            while True:
                a = base[a]
                mark.add(a)
                if mate[a] < 0:
                    break
                a = p[mate[a]]
            while True:
                b = base[b]
                if b in mark:
                    return b
                b = p[mate[b]]

        for v in q:  # (q grows while it is walked)
            for to in range(n):
                if not (adj[v] >> to) & 1 or base[v] == base[to] or mate[v] == to:
                    continue
                if to == root or (mate[to] >= 0 and p[mate[to]] >= 0):
                    cur, blossom = lca(v, to), set()
                    for x, child in ((v, to), (to, v)):
                        while base[x] != cur:
                            blossom.add(base[x])
                            blossom.add(base[mate[x]])
                            p[x] = child
                            child = mate[x]
                            x = p[mate[x]]
                    for i in range(n):
                        if base[i] in blossom:
                            base[i] = cur
                            if i not in used:
                                used.add(i)
                                q.append(i)
                elif p[to] < 0:
                    p[to] = v
                    if mate[to] < 0:
                        return to, p
                    used.add(mate[to])
                    q.append(mate[to])
        return -1, p

    for root in range(n):
        if mate[root] >= 0:
            continue
        x, p = find_path(root)
        while x >= 0:
            pv = p[x]
            ppv = mate[pv]
            mate[x], mate[pv] = pv, x
            x = ppv
    return sum(m >= 0 for m in mate) // 2


# ---------------------------------------------------------------- families: n -> edge list, or None where the family has no member of that size
def path(n):
    return [(i, i + 1) for i in range(n - 1)]


def cycle(n):  # odd and even with n
    return [(i, (i + 1) % n) for i in range(n)]


def star(n):
    return [(0, i) for i in range(1, n)]


def double_star(n, p=None):
    """hub 0 with leaves 1 .. p, hub p + 1 with the leaves above it, the hubs joined"""
    p = (n - 2) // 2 if p is None else p
    return [(0, i) for i in range(1, p + 1)] + [(0, p + 1)] + [(p + 1, i) for i in range(p + 2, n)]


def spider2(n):
    """hub 0, legs 0 - (2i - 1) - 2i of length 2"""
    if n % 2 == 0:
        return None
    return [e for i in range(1, (n - 1) // 2 + 1) for e in ((0, 2 * i - 1), (2 * i - 1, 2 * i))]


def caterpillar(n):
    return [(i, i + 1) for i in range(n // 2 - 1)] + [(i, n // 2 + i) for i in range(n - n // 2)]


def complete(n):
    return [(u, v) for v in range(n) for u in range(v)]


def k_ab(n):
    a = max(2, n // 3)
    if a == n - a:
        return None
    return [(u, v) for u in range(a) for v in range(a, n)]


def flower(n):
    """triangles 0 - (2i - 1) - 2i at the hub 0"""
    if n % 2 == 0:
        return None
    return [e for i in range(1, (n - 1) // 2 + 1) for e in ((0, 2 * i - 1), (0, 2 * i), (2 * i - 1, 2 * i))]


def odd_cycles_sharing_a_vertex(n):
    """a chain of 5- and 3-cycles, each sharing the vertex opposite to where it was entered with the next"""
    if n % 2 == 0:
        return None
    edges, a, used, k = [], 0, 1, 0
    while used < n:
        length = 5 if n - used >= 4 and k % 3 != 2 else 3
        ring = [a] + list(range(used, used + length - 1))
        edges += [(ring[i], ring[(i + 1) % length]) for i in range(length)]
        used += length - 1
        a = ring[length // 2]
        k += 1
    return edges


def odd_cycles_sharing_an_edge(n):
    """a chain of odd cycles, each sharing an EDGE with the next: a search that closes the last one finds blossoms nested in blossoms"""
    first = 5 if n >= 5 else 3
    edges = [(i, (i + 1) % first) for i in range(first)]
    p, q, used = first // 2, first // 2 + 1, first
    while used < n:
        new = 3 if n - used >= 3 else 1  # a 5-cycle over the edge {p, q}, or a triangle
        chain = [p] + list(range(used, used + new)) + [q]
        edges += [(chain[i], chain[i + 1]) for i in range(len(chain) - 1)]
        used += new
        p, q = (chain[2], chain[3]) if new == 3 else (chain[1], q)
    return edges


def odd_cycle_with_pendant_paths(n):
    """an odd cycle, the largest that divides n properly, with a path of the same length hanging from every vertex"""
    c = next((c for c in range(n // 2, 2, -1) if c % 2 == 1 and n % c == 0), None)
    if c is None:
        return None
    ell = n // c - 1
    edges = [(i, (i + 1) % c) for i in range(c)]
    for i in range(c):
        prev = i
        for j in range(ell):
            edges.append((prev, c + i * ell + j))
            prev = c + i * ell + j
    return edges


def barbell(n, a=None, b=None):
    """K_a and K_b joined by a path through the vertices between them (by an edge when there are none)"""
    if a is None:  # equal
        if n % 2 or n < 8:
            return None
        a = b = n // 2
    edges = [(u, v) for v in range(a) for u in range(v)] + [(u, v) for v in range(n - b, n) for u in range(n - b, v)]
    return edges + [(i, i + 1) for i in range(a - 1, n - b)]


def unequal_barbell(n):
    if n < 8:
        return None
    a = max(3, n // 3)
    return barbell(n, a, max(a + 1, n // 2 - 1))


def lollipop(n):
    k = max(3, n // 2)
    if k >= n:
        return None
    return [(u, v) for v in range(k) for u in range(v)] + [(i, i + 1) for i in range(k - 1, n - 1)]


def tree_plus_gnp(rng, n, p):
    order = rng.permutation(n)
    es = {tuple(sorted((int(order[i]), int(order[rng.integers(0, i)])))) for i in range(1, n)}
    es |= {(u, v) for v in range(n) for u in range(v) if rng.random() < p}
    return sorted(es)


def near_trees(trials):
    """the near-tree stream: default_rng(3); per trial n in 8 .. 64, a random order, every vertex joined to one of the two before it
    in that order, then 0 .. 2 extra pairs.  {trial: (n, edges)} for the trials asked for (the stream is drawn from its start)"""
    rng = np.random.default_rng(3)
    out = {}
    for trial in range(max(trials) + 1):
        n = int(rng.integers(8, 65))
        order = rng.permutation(n)
        es = {tuple(sorted((int(order[i]), int(order[rng.integers(max(0, i - 2), i)])))) for i in range(1, n)}
        for _ in range(int(rng.integers(0, 3))):
            u, v = (int(x) for x in rng.choice(n, 2, replace=False))
            es.add((min(u, v), max(u, v)))
        if trial in trials:
            out[trial] = (n, sorted(es))
    return out


FAMILIES = (
    ("path", path), ("cycle", cycle), ("star", star), ("double_star", double_star), ("spider2", spider2), ("caterpillar", caterpillar),
    ("complete", complete), ("k_ab", k_ab), ("flower", flower), ("odd_cycles_sharing_a_vertex", odd_cycles_sharing_a_vertex),
    ("odd_cycles_sharing_an_edge", odd_cycles_sharing_an_edge), ("odd_cycle_with_pendant_paths", odd_cycle_with_pendant_paths),
    ("barbell", barbell), ("unequal_barbell", unequal_barbell), ("lollipop", lollipop),
)
RANDOM_FAMILIES = tuple("tree_gnp_%g" % p for p in GNP) + ("near_tree",)


# ---------------------------------------------------------------- targeted graphs: labelled so that the greedy matching is maximum
def spider_with_free_leaves(n):
    """hub 0, three legs of length 1 (vertices 1, 2, 3: the hub takes 1, the other two stay unmatched), legs 0 - a - b of length 2"""
    if n < 8 or n % 2:
        return None
    return [(0, 1), (0, 2), (0, 3)] + [e for a in range(4, n, 2) for e in ((0, a), (a, a + 1))]


def flower_with_petals_removed(n):
    """hub 0 with triangles, two of them without their outer edge (vertices 1 .. 4 hang from the hub: it takes 1, three stay unmatched)"""
    if n < 9 or n % 2 == 0:
        return None
    return [(0, i) for i in range(1, n)] + [(a, a + 1) for a in range(5, n, 2)]


def _targets(family, n, adj, mate):
    """[(kind, first slot)] of a targeted graph whose step-0 matching `mate` is known"""
    if family in ("cycle", "k_ab", "odd_cycles_sharing_a_vertex", "odd_cycles_sharing_an_edge"):
        # a matched edge that is no cut edge: the lowest and the highest
        es = [(u, v) for u, v in edges_of(adj) if mate[u] == v and is_connected(toggled(adj, colex(u, v)))]
        return [("delete_matched", colex(*e)) for e in ([es[0], es[-1]] if len(es) > 1 else es)]
    if family == "double_star":  # 0 - 1 and hub - its first leaf are matched
        hub = next(v for v in range(1, n) if bin(adj[v]).count("1") > 1)
        return [("add_matched", colex(1, mate[hub])), ("add_matched", colex(0, mate[hub]))]  # an augmenting path through the new edge; none
    if family == "spider_with_free_leaves":
        return [("add_matched", colex(4, 6)), ("add_matched", colex(1, 5)), ("add_matched", colex(5, 7))]
    if family == "flower_with_petals_removed":
        return [("add_matched", colex(1, 5)), ("add_matched", colex(5, 7)), ("delete_matched", colex(5, 6))]
    raise KeyError(family)


TARGETED = (
    ("cycle", cycle, (4, 8, 20, 32, 50, 64)), ("k_ab", k_ab, (5, 9, 20, 33, 64)),
    ("odd_cycles_sharing_a_vertex", odd_cycles_sharing_a_vertex, (9, 33, 63)), ("odd_cycles_sharing_an_edge", odd_cycles_sharing_an_edge, (8, 9, 32, 63, 64)),
    ("double_star", double_star, (8, 9, 32, 63, 64)), ("spider_with_free_leaves", spider_with_free_leaves, (8, 20, 32, 64)),
    ("flower_with_petals_removed", flower_with_petals_removed, (9, 31, 33, 63)),
)


# ---------------------------------------------------------------- toggle sequences
def _rng(name):
    return np.random.default_rng([20240607, zlib.crc32(name.encode())])


def toggle_sequence(name, adj, first=()):
    """n_toggles(n) slots: `first`, then random unused ones -- an absent edge is added, a present one deleted unless it is a cut edge
    (then another slot is drawn)"""
    n = len(adj)
    E = n * (n - 1) // 2
    rng, g, seq = _rng(name), list(adj), []
    for slot in first:
        g = toggled(g, slot)
        assert is_connected(g), name
        seq.append(slot)
    while len(seq) < n_toggles(n):
        for slot in (int(x) for x in rng.permutation(E)):
            u, v = from_colex(slot)
            if slot not in seq and not ((g[v] >> u) & 1 and not is_connected(toggled(g, slot))):
                break
        else:
            raise AssertionError("no legal toggle left: " + name)
        g = toggled(g, slot)
        seq.append(slot)
    return tuple(seq)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, family, n, edges, kind="random", first=(), start_mate=None):
        adj = from_edges(n, edges)
        assert is_connected(adj), name
        out.append(Case(name, family, n, tuple(adj), toggle_sequence(name, adj, first), kind, start_mate))

    for family, fn in FAMILIES:
        for n in SIZES:
            edges = fn(n)
            if edges is not None:
                add("%s-%d" % (family, n), family, n, edges)
    for p in GNP:
        for n in SIZES:
            for rep in range(3):
                name = "tree_gnp_%g-%d-%d" % (p, n, rep)
                add(name, "tree_gnp_%g" % p, n, tree_plus_gnp(_rng("graph " + name), n, p))
    for trial, (n, edges) in sorted(near_trees(NEAR_TREE_TRIALS).items()):
        add("near_tree-trial%d" % trial, "near_tree", n, edges)
    for family, fn, sizes in TARGETED:
        for n in sizes:
            adj = from_edges(n, fn(n))
            mate = greedy_matching(adj)
            known = sum(m != 0xFF for m in mate) // 2 == matching_number(adj)
            for k, (kind, slot) in enumerate(_targets(family, n, adj, mate)):
                add("%s-%d-%s%d" % (family, n, kind, k), family, n, fn(n), kind, (slot,), tuple(mate) if known else None)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_size():
    """{n: [cases]}: what one probe call takes (one vertex count per call)"""
    out = {}
    for c in cases():
        out.setdefault(c.n, []).append(c)
    return out


def adjacency_array(case):
    return np.array(case.adj, dtype=np.uint64)


def steps(case):
    """the graphs of a case: before any toggle, and after each"""
    g = list(case.adj)
    yield 0, None, g
    for j, slot in enumerate(case.toggles, 1):
        g = toggled(g, slot)
        yield j, slot, g


# ---------------------------------------------------------------- the branch of dense_matching_update a step takes
CLASSES = (
    "add, both ends free",
    "add, one end free, search succeeded", "add, one end free, search failed",
    "add, both ends matched, fewer than two free",
    "add, both ends matched, two or more free, search succeeded", "add, both ends matched, two or more free, search failed",
    "delete, unmatched edge",
    "delete, matched edge, size restored", "delete, matched edge, size lost",
)


def branch_class(n, prev_mate, added, u, v, mu_before, mu_after):
    """from the matching held BEFORE the toggle (64 bytes, 0xFF: unmatched), the toggled edge and the matching numbers"""
    mu_, mv = int(prev_mate[u]), int(prev_mate[v])
    free = sum(1 for i in range(n) if int(prev_mate[i]) == 0xFF)
    if added:
        if mu_ == 0xFF and mv == 0xFF:
            return CLASSES[0]
        grew = mu_after > mu_before
        if mu_ == 0xFF or mv == 0xFF:
            return CLASSES[1] if grew else CLASSES[2]
        if free < 2:
            return CLASSES[3]
        return CLASSES[4] if grew else CLASSES[5]
    if mu_ != v:
        return CLASSES[6]
    return CLASSES[7] if mu_after == mu_before else CLASSES[8]
