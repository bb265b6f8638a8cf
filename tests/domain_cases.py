"""The edges of the domain check_engine_config accepts, as one table (a helper like tests/dense_cost_cases.py: numpy only, no test
lives here).  tests/test_domain_cases.py holds every row to the engine's argument check, the oracle's dimensions and the row's
non-vacuity conditions on the CPU; tests/test_gpu_domain_cases.py runs every row on the device against the oracle through
gpu_parity.run_lockstep, one launch per phase and in the engine's default form.

A row: id, family ("c21" | "ramsey" | "dense"), the space's constructor arguments, B, (kmin, kmax), the n_as_tol table, calls per
epoch, epochs (two: the observations, the device root policy and a reset are each compared once), seed, and the instantiation the
row is there for, with the device key width that selects it.
    conditions   what makes the row non-vacuous, evaluated ON THE ORACLE ALONE (run_oracle below; names: CONDITIONS).  The seeds
                 were chosen on the CPU so that the oracle meets them; the comment beside a row records what the oracle gives.
    default      the step form the engine's default takes for the row and a substring of the reason it gives for a form it did
                 not take, from the units' tables (the 64-bit Ramsey tier and the dense-graph space build no CU-resident form with
                 the evaluator in the kernel: ramsey64_phase.inc, launchers.inc) -- asserted through step_form(), never assumed
    refuse       a refusal row: (status, message substring) of par_new on roots the oracle's generator draws beyond the limit
    roots        "all_legal": the generator's trees with kmax permitted actions drawn (seeded, numpy) among the LEGAL ones only
Tolerance tables: TOL_SMALL on the minima; the reference drivers' tables elsewhere (gpu_parity.TOL, TOL_REF)."""
from collections import namedtuple

import numpy as np

TOL_SMALL = ([6, 3, 2], 1)
TOL = ([200, 200, 100, 100, 50, 50, 25, 25], 10)  # 02-r44.rs:128-130 (= gpu_parity.TOL)
TOL_REF = ([200, 50, 50], 25)                     # 04-c21-tree.rs:136-138 (= gpu_parity.TOL_REF)
INVALID = 1                                       # AZD_ERR_INVALID_ARGUMENT
MAX_NODE_ACTIONS = 128                            # engine_types.h: what a c21 or narrow Ramsey node holds

ASYNC = ("async", "")
U64_PER_CALL = ("per_call", "not built for the 64-bit Ramsey tier")
DENSE_PER_CALL = ("per_call", "dense-graph space")
# c21 from N = 22: a wave's lambda_1 columns in LDS are 512 (N - 2) bytes (space_c21.inc: lds_pq), 16 waves' no longer fit a CU's
# 160 KB beside the rest, and the engine steps down to one launch per phase -- the asynchronous step's plan says so
LDS_PER_CALL = ("per_call", "asynchronous step: 16 rows of activations do not fit the CU's 160 KB of LDS")
C21_LDS_PER_CALL = LDS_PER_CALL

Case = namedtuple("Case", "id family ctor B k tol calls epochs seed inst kw conditions default first_agent n_obs_tol check_every refuse roots")


def case(id, family, ctor, B, k, tol, calls, seed, inst, kw, conditions=(), default=ASYNC, first_agent=0, n_obs_tol=2, check_every=None,
         refuse=None, epochs=2, roots=None):
    return Case(id, family, ctor, B, k, tol, calls, epochs, seed, inst, kw, tuple(conditions), default, first_agent, n_obs_tol,
                check_every or calls // 2, refuse, roots)


def ramsey(n, sizes, weights=None, **kw):
    return dict(n=n, sizes=sizes, weights=[1.0] * len(sizes) if weights is None else weights, **kw)


SMALL = ("terminals", "transpositions")
MINIMUM = SMALL + ("root_exhausted",)
R20 = dict(B=8, k=(100, 128), tol=TOL, calls=24, kw=6, conditions=("vertex19",))
R15 = dict(family="ramsey", ctor=ramsey(15, [4, 4]), k=(12, 52), tol=TOL, calls=20, seed=3, inst="RamseySpace<4>", kw=4)
C23 = dict(family="c21", ctor=dict(n=23), k=(5, 115), tol=TOL_REF, calls=20, seed=5, inst="C21Space<4>", kw=4, default=C21_LDS_PER_CALL)

CASES = [
    # ---- c21 (ROTModifyParentsOnce): minimum, ceiling, fullest node
    # S = 4, A = 2: both actions re-parent vertex 2, which may be re-parented once -- every new node is terminal and no two paths
    # meet, so a transposition cannot occur at this size.  The oracle: 0 expansions, 17 terminals, 384 root exhaustions
    case("c21_n4", "c21", dict(n=4), 16, (1, 2), TOL_SMALL, 12, 11, "C21Space<1>", 1, ("terminals", "root_exhausted")),
    case("c21_n23", **C23, B=8),                                    # A = 230, S = 460: lambda1_impl<FULL, 0> in a search
    case("c21_n24", "c21", dict(n=24), 8, (5, 126), TOL_REF, 20, 6, "C21Space<4>", 4, default=C21_LDS_PER_CALL),  # AZD_C21_MAX_N: A = 252, S = 504
    # upload_roots (engine.hip) lets a root bring MAX_NODE_ACTIONS = 128 permitted actions ("more permitted actions than a node can
    # hold" beyond): kmin = kmax = 128 of the 252.  A permitted action that names a vertex's current parent is not legal (21 of the
    # 252), so the generator's roots hold about 119 predictions; "all_legal" roots hold 128, the prediction count's maximum
    case("c21_n24_full", "c21", dict(n=24), 4, (128, 128), TOL_REF, 16, 7, "C21Space<4>", 4, ("full_node",), roots="all_legal",
         default=C21_LDS_PER_CALL),
    case("c21_n24_over", "c21", dict(n=24), 4, (129, 129), TOL_REF, 0, 7, "C21Space<4>", 4,
         refuse=(INVALID, "more permitted actions than a node can hold")),
    # ---- narrow Ramsey tier (max_slots = 0): minima, RamseySpace<4>, four colours, the tier's ceiling
    case("r_n3", "ramsey", ramsey(3, [3, 3]), 16, (1, 3), TOL_SMALL, 12, 1, "RamseySpace<1>", 1, MINIMUM),        # E = 3, A = 6
    case("r_n4c4", "ramsey", ramsey(4, [3, 3, 3, 3]), 16, (1, 6), TOL_SMALL, 16, 2, "RamseySpace<1>", 1, MINIMUM),  # E = 6, A = 24
    case("r_n12c3", "ramsey", ramsey(12, [3, 4, 3]), 16, (12, 33), TOL, 20, 4, "RamseySpace<4>", 4),               # A = 198
    case("r_n15c2", **R15, B=16),                                                                                 # A = 210
    case("r_n13c4", "ramsey", ramsey(13, [3, 3, 3, 3]), 16, (12, 39), TOL, 20, 5, "RamseySpace<5>", 5),            # A = 312
    # E*C = 364 of the tier's 384; a root at the node limit of 128 / (C - 1) = 42 edges holds 126 of 128 predictions
    case("r_n14c4_full", "ramsey", ramsey(14, [3, 3, 3, 3], [1.0, 0.5, 2.0, 1.0]), 16, (42, 42), TOL, 24, 6, "RamseySpace<6>", 6,
         ("all_colours", "full_node")),
    case("r_n14c4_over", "ramsey", ramsey(14, [3, 3, 3, 3]), 4, (43, 43), TOL, 0, 6, "RamseySpace<6>", 6,
         refuse=(INVALID, "more permitted actions than a node can hold")),
    # N = 20, two colours: E = 190, A = 380, KW = 6, 190 of the 192 bits of the three permitted words in use; vertex 19's edges are
    # positions 171..189.  [3, 5]: K5 over the top vertices
    case("r_n20_k4", "ramsey", ramsey(20, [4, 4]), seed=8, inst="RamseySpace<6>", **R20),
    case("r_n20_k35", "ramsey", ramsey(20, [3, 5]), seed=9, inst="RamseySpace<6>", **R20),
    # ---- wide tier: both sides of `a.A <= 640 ? 10 : 16` (engine.hip: engine_shape)
    case("w_n25", "ramsey", ramsey(25, [3, 3], max_slots=300), 8, (150, 300), TOL, 16, 10, "RamseyWideSpace<10>", 10),  # A = 600
    # A = 650.  RamseyWideSpace<16> keeps 512 * 16 bytes of selection scratch and 4 E C bytes of clique counts per wave; E C > 640
    # makes that more than 10752 bytes, 16 waves' more than a CU's 160 KB: no CU-resident form takes a key width of 16, at any shape
    case("w_n26", "ramsey", ramsey(26, [3, 3], max_slots=325), 8, (160, 325), TOL, 16, 11, "RamseyWideSpace<16>", 16, default=LDS_PER_CALL),
    # ---- N = 3 with max_slots = 3 on the wide and the 64-bit tier (tests/test_ramsey64_abi.py: accepted)
    case("w_n3", "ramsey", ramsey(3, [3, 3], max_slots=3), 16, (1, 3), TOL_SMALL, 12, 1, "RamseyWideSpace<10>", 10, MINIMUM),
    case("u_n3", "ramsey", ramsey(3, [3, 3], max_slots=3, u64=True), 16, (1, 3), TOL_SMALL, 12, 1, "RamseyU64Space", 36, MINIMUM,
         default=U64_PER_CALL),
    # ---- dense-graph space: minima (default cost n = 4..7; Aouchiche-Hansen cost n = 4, 5)
    *[case("d_n%d" % n, "dense", dict(n=n, p=0.5), 12, (1, n * (n - 1) // 2), TOL_SMALL, 12, 20 + n, "DenseSpace<2> c21", 2,
           MINIMUM if n <= 5 else SMALL, default=DENSE_PER_CALL) for n in (4, 5, 6, 7)],
    *[case("d_n%d_ah" % n, "dense", dict(n=n, p=0.5, cost="ah"), 12, (1, n * (n - 1) // 2), TOL_SMALL, 12, 30 + n, "DenseSpace<2> ah", 2,
           MINIMUM, default=DENSE_PER_CALL) for n in (4, 5)],
    # ---- ragged populations: one agent (one live wave of a workgroup's 16), and four workgroups of 16 agents plus one agent, as the
    # shard of a larger population that starts at agent 3
    case("b1_r_n15c2", **R15, B=1),
    case("b65_r_n15c2", **R15, B=65, first_agent=3),
    case("b1_c21_n23", **C23, B=1),
    case("b65_c21_n23", **C23, B=65, first_agent=3),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def make_space(az, c):
    if c.family == "c21":
        return az.ROTModifyParentsOnce(c.ctor["n"])
    if c.family == "ramsey":
        t = c.ctor
        return az.RamseySpaceNoEdgeRecolor(t["n"], t["sizes"], t["weights"], max_slots=t.get("max_slots"), u64=t.get("u64"))
    return az.DenseGraphSpace(c.ctor["n"], c.ctor["p"], cost=c.ctor.get("cost", "c21"))


def oracle_roots(orc, c):
    """the row's roots from the oracle's seeded generators, in the layout par_new and the references take (a refusal row's are
    beyond what the engine's own generators draw)"""
    n, (kmin, kmax) = c.ctor["n"], c.k
    if c.family == "c21":
        parents, permitted = orc.gen_roots(c.seed, 0, c.first_agent, c.B, n, kmin, kmax)
        if c.roots == "all_legal":  # action id of (parent, child) = child (child - 1) / 2 - 1 + parent, children 2 .. n - 2
            rng = np.random.default_rng(c.seed)
            for i in range(c.B):
                legal = [ch * (ch - 1) // 2 - 1 + p for ch in range(2, n - 1) for p in range(ch) if p != parents[i, ch]]
                permitted[i] = 0
                for a in rng.choice(legal, kmax, replace=False):
                    permitted[i, a >> 6] |= np.uint64(1 << (int(a) & 63))
        return parents, permitted
    if c.family == "ramsey":
        return orc.gen_ramsey_roots(c.seed, 0, c.first_agent, c.B, n, len(c.ctor["sizes"]), kmin, kmax)
    adj, slots = orc.gen_dense_roots(c.seed, 0, c.first_agent, c.B, n, kmin, kmax, c.ctor["p"])
    return adj.view(np.uint8).reshape(c.B, 8 * n), slots


def make_ref(orc, c):
    """the row's reference engine behind gpu_parity's interface (imported here: gpu_parity needs pytest)"""
    import gpu_parity as G
    n = c.ctor["n"]
    if c.family == "c21":
        return G.OracleRef.c21(orc, n, c.B)
    if c.family == "ramsey":
        return G.CppRef(orc, n, c.ctor["sizes"], c.ctor["weights"], c.B)
    if c.ctor.get("cost") == "ah":
        import dense_ah_ref as R
        return G.PyDenseRef(R.PyDenseEngine(n, c.B, cost="ah", p=c.ctor["p"]))
    return G.OracleRef.dense(orc, n, c.B, c.ctor["p"])


def path_bits(ref, i):
    return {64 * w + b for w, x in enumerate(ref.agent_state(i)["path"]) for b in range(64) if (int(x) >> b) & 1}


def run_oracle(orc, c):
    """The row on the reference alone, with run_lockstep's calls in run_lockstep's order (new, the epochs' calls, observe,
    modify_roots, reset).  -> dict(counters, taken: the action ids on the agents' paths at the moments run_lockstep compares,
    widest: the most predictions of a node at the end of an epoch's calls, roots: every epoch's roots, ref)"""
    ref = make_ref(orc, c)
    roots = oracle_roots(orc, c)
    call = 0
    A = ref.e.A
    h = lambda: orc.hash_predictions(c.seed, c.first_agent, c.B, A, call)
    ref.new(roots, h())
    taken, all_roots, widest = set(), [roots], 0
    for epoch in range(c.epochs):
        for s in range(c.calls):
            call += 1
            ref.step(c.tol, h())
            if (s + 1) % c.check_every == 0 or s + 1 == c.calls:
                for i in range(c.B):
                    taken |= path_bits(ref, i)
        widest = max([widest] + [int((t.act_end - t.act_begin).max()) for t in (ref.tree(i) for i in range(c.B))])
        ref.observe(c.n_obs_tol)
        roots = ref.modify_roots(c.seed, epoch, c.first_agent, *c.k)
        all_roots.append(roots)
        call += 1
        ref.reset(roots, h())
    return dict(counters=ref.counters(), taken=taken, widest=widest, roots=all_roots, ref=ref)


def node_limit(c):
    """the most predictions a node of the row's engine can hold at the row's kmax"""
    if c.family == "ramsey":
        return c.k[1] * (len(c.ctor["sizes"]) - 1)
    return c.k[1]


def _vertex19(c, r):
    E = c.ctor["n"] * (c.ctor["n"] - 1) // 2
    return sum(1 for a in r["taken"] if a % E >= 171) >= 4


def _all_colours(c, r):
    E = c.ctor["n"] * (c.ctor["n"] - 1) // 2
    return {a // E for a in r["taken"]} == set(range(len(c.ctor["sizes"])))


CONDITIONS = {
    "terminals": lambda c, r: r["counters"]["TERMINALS"] > 0,
    "transpositions": lambda c, r: r["counters"]["TRANSPOSITIONS"] > 0,
    "root_exhausted": lambda c, r: r["counters"]["ROOT_EXHAUSTED"] > 0,
    "vertex19": _vertex19,        # at least 4 recoloured edges at vertex 19 (position >= 171) on the compared paths
    "all_colours": _all_colours,  # every new colour taken at least once on the compared paths
    "full_node": lambda c, r: r["widest"] == node_limit(c),  # a node with the maximum prediction count
}
