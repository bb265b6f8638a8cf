"""What the big-clique tests share (AZD_ENGINE_RAMSEY_BIG_CLIQUES: clique sizes up to 8 on the 64-bit Ramsey tier): the shapes, and
roots whose big colour is dense enough that its cliques exist.  A test helper, not a conftest.

At small n a uniformly coloured root has no K6 at all -- a [6,6] root at n = 12 with p = 0.5 has total 0 and no nonzero count --
and a parity test on it would say nothing about count_cliques_inside at depth >= 4.  So every case colours its edges with the
big colour at probability p (the other colours share the rest evenly), and `assert_not_vacuous` holds the roots to a cap before
anything is compared on them: the big colour's total > 0 in every root and at least 90 % of its per-edge counts nonzero, on the
REFERENCE's values."""
from math import comb

import numpy as np

# (n, sizes, p of the big colour)
CASES = {"n12_36": (12, [3, 6], 0.85), "n14_47": (14, [4, 7], 0.9), "n13_83": (13, [8, 3], 0.93), "n16_336": (16, [3, 3, 6], 0.8),
         "n34_36": (34, [3, 6], 0.75)}


def big_colour(sizes):
    return max(range(len(sizes)), key=lambda c: sizes[c])


def colour_weights(sizes, p):
    big, C = big_colour(sizes), len(sizes)
    return [p if c == big else (1.0 - p) / (C - 1) for c in range(C)]


def roots(n, sizes, p, B, seed, kmin, kmax):
    """B roots: (colors u8 [B, E], list of permitted edge sets), the colours drawn with colour_weights(sizes, p)"""
    rng = np.random.default_rng([seed, n, len(sizes)])
    E = n * (n - 1) // 2
    colors = rng.choice(len(sizes), size=(B, E), p=colour_weights(sizes, p)).astype(np.uint8)
    permitted = [set(int(e) for e in rng.permutation(E)[:int(rng.integers(kmin, kmax + 1))]) for _ in range(B)]
    return colors, permitted


def pack_permitted(permitted, kw):
    out = np.zeros((len(permitted), kw), np.uint64)
    for i, m in enumerate(permitted):
        for e in m:
            out[i, e >> 6] |= np.uint64(1 << (e & 63))
    return out


def assert_not_vacuous(sizes, states, tag=""):
    """states: the case's roots as the REFERENCE has them (objects with counts[c][e] and totals[c]): every root has cliques of the
    big colour, and at least 90 % of the roots' per-edge counts of that colour are nonzero"""
    big = big_colour(sizes)
    totals = [st.totals[big] for st in states]
    rows = np.asarray([st.counts[big] for st in states])
    share = np.count_nonzero(rows) / rows.size
    assert min(totals) > 0 and share >= 0.9, (tag, "the big colour has too few cliques for the case to say anything", totals, share)
    return min(totals), max(totals), share


def closed_form(n, s):
    """a root monochromatic in a colour of clique size s: (every per-edge count, the total)"""
    return comb(n - 2, s - 2), comb(n, s)
