"""tests/domain_cases.py on the CPU: every row is accepted by the engine's argument check (or is a pinned refusal), its dimensions
and key width are the oracle's and the named instantiation's, the oracle alone meets the row's non-vacuity conditions over the
whole case, and the new Ramsey shapes do not rest on the C++ oracle's incremental counts alone (oracle/py_ramsey.py's recount,
tests/test_oracle_ramsey.py's brute-force counter).  Every dense-graph row runs in a child process under a time limit."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import domain_cases as D
from test_oracle_cross import _pack_ramsey, _unpack_ramsey, assert_same_trees
from test_oracle_ramsey import brute_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.id for c in D.CASES]
RUN = [c for c in D.CASES if not c.refuse]
RAMSEY = [c for c in RUN if c.family == "ramsey"]
DENSE = [c for c in D.CASES if c.family == "dense"]
NO_DEVICE = 2  # AZD_ERR_NO_DEVICE


def device_key_words(c, space):
    """engine_shape (engine.hip): the host's key words on c21 and the narrow Ramsey tier; 10 or 16 by ACTION_DIM on the wide tier,
    36 on the 64-bit tier; 2 / 4 / 10 / 16 by max_slots on the dense-graph space"""
    if c.family == "dense":
        ms = space.MAX_SLOTS if space.MAX_SLOTS > 0 else 128
        return 2 if ms <= 128 else 4 if ms <= 256 else 10 if ms <= 640 else 16
    if c.family == "ramsey" and space.tier == "u64":
        return 36
    if c.family == "ramsey" and space.tier == "wide":
        return 10 if space.ACTION_DIM <= 640 else 16
    return space.KEY_WORDS


@pytest.mark.parametrize("c", D.CASES, ids=IDS)
def test_row_is_accepted_and_has_the_oracles_dimensions(orc, c):
    import azdopt_amd as az
    space = D.make_space(az, c)
    # azd_engine_create checks the configuration before it looks for a device (tests/test_ramsey64_abi.py relies on the same)
    for persistent in (False, True):
        try:
            az.NablaOptimizer(space, None, c.B, first_agent=c.first_agent, persistent=persistent)
        except az.AzdError as e:
            assert e.status == NO_DEVICE, (c.id, str(e))
    ref = D.make_ref(orc, c)
    assert (space.STATE_DIM, space.ACTION_DIM, space.KEY_WORDS) == (ref.e.S, ref.e.A, ref.KW), c.id
    assert device_key_words(c, space) == c.kw, c.id
    width = re.search(r"<(\d+)>", c.inst)
    assert (int(width.group(1)) if width else 36) == c.kw, c.inst
    tier = {"RamseySpace": "narrow", "RamseyWideSpace": "wide", "RamseyU64Space": "u64"}.get(c.inst.split("<")[0])
    assert tier == (space.tier if c.family == "ramsey" else None), (c.id, c.inst)
    roots = D.oracle_roots(orc, c)
    per_root = [sum(bin(int(w)).count("1") for w in row) for row in roots[1]]
    assert all(c.k[0] <= k <= c.k[1] for k in per_root), c.id
    if c.refuse:  # one beyond what a node holds: the engine's own generators do not draw such roots
        per_slot = len(c.ctor["sizes"]) - 1 if c.family == "ramsey" else 1  # actions a permitted edge / action brings
        assert all(k * per_slot > D.MAX_NODE_ACTIONS >= (k - 1) * per_slot for k in per_root), c.id
        if c.family == "c21":
            with pytest.raises(az.AzdError):
                space.generate_roots(c.seed, c.B, kmin=c.k[0], kmax=c.k[1])
    elif c.roots is None:  # the engine's host generator draws the oracle's roots
        mine = space.generate_roots(c.seed, c.B, first_agent=c.first_agent, kmin=c.k[0], kmax=c.k[1])
        assert np.array_equal(mine[0], roots[0]) and np.array_equal(mine[1], roots[1]), c.id


@pytest.mark.parametrize("c", [c for c in RUN if c.family != "dense"], ids=lambda c: c.id)
def test_oracle_alone_meets_the_rows_conditions(orc, c):
    t0 = time.time()
    r = D.run_oracle(orc, c)
    assert r["counters"]["FAILED"] == 0, c.id
    for name in c.conditions:
        assert D.CONDITIONS[name](c, r), (c.id, name, r["counters"], r["widest"])
    assert time.time() - t0 < 5.0, c.id  # the reference side of a GPU case: cheap


CHILD = """
import sys
sys.path[:0] = [%r, %r]
from oracle import orc
import domain_cases as D
c = D.BY_ID[sys.argv[1]]
r = D.run_oracle(orc, c)
assert r["counters"].get("FAILED", 0) == 0, r["counters"]
bad = [n for n in c.conditions if not D.CONDITIONS[n](c, r)]
assert not bad, (bad, r["counters"], r["widest"])
print("finished", c.id, r["counters"]["EXPANSIONS"])
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("c", DENSE, ids=lambda c: c.id)
def test_dense_row_finishes_in_a_child_process(orc, c):
    """the oracle over the whole dense-graph case, conditions included, in a process of its own with a 20 s limit: a search that
    does not return at a tiny n fails here, by name, and never reaches a device"""
    try:
        p = subprocess.run([sys.executable, "-c", CHILD, c.id], capture_output=True, text=True, timeout=20)
    except subprocess.TimeoutExpired:
        pytest.fail("dense row %s did not finish on the oracle within 20 s" % c.id)
    assert p.returncode == 0 and ("finished %s" % c.id) in p.stdout, (c.id, p.stdout, p.stderr)


def test_oracle_binding_takes_u64_rows_and_refuses_a_short_block(orc):
    """orc.gen_dense_roots hands the neighbourhoods over as u64 [B, n].  Engine.new_begin used to cast them to u8 BY VALUE -- a
    block an eighth of the size the library reads, graphs with neighbours beyond n, and a first roll-out that never
    returned at n = 4 and 5.  The rows are now taken as the bytes they are; a block of the wrong size is refused."""
    n, B = 4, 16
    E = n * (n - 1) // 2
    adj, slots = orc.gen_dense_roots(1, 0, 0, B, n, 1, E, 0.5)
    assert adj.dtype == np.uint64 and adj.shape == (B, n)
    runs = []
    for rows in (adj, adj.view(np.uint8).reshape(B, 8 * n)):
        e = orc.Engine(n, B, threads=2, dense=True, dense_p=0.5)
        e.new_begin(rows, slots)
        e.new_end(orc.hash_predictions(1, 0, B, e.A, 0))
        for call in range(1, 7):
            e.rollout_begin(*D.TOL_SMALL)
            e.rollout_end(orc.hash_predictions(1, 0, B, e.A, call))
        runs.append(e)
    assert runs[0].counters() == runs[1].counters() and runs[0].counters()["EXPANSIONS"] > 0
    assert np.array_equal(runs[0].state_vecs(), runs[1].state_vecs())
    e = orc.Engine(n, B, threads=1, dense=True, dense_p=0.5)
    with pytest.raises(ValueError):
        e.new_begin(adj.astype(np.uint8), slots)  # B x n bytes where B x 8 n are read
    with pytest.raises(ValueError):
        e.reset_begin(adj, slots[:, :0])
    c21 = orc.Engine(8, 4)
    with pytest.raises(ValueError):
        c21.new_begin(np.zeros((4, 7), np.uint8), np.zeros((4, c21.KW), np.uint64))


# ---------------------------------------------------------------- the new Ramsey shapes beside the incremental C++ counts
@pytest.mark.parametrize("c", RAMSEY, ids=lambda c: c.id)
def test_ramsey_row_root_counts_against_the_brute_force_counter(orc, c):
    """the first root of every Ramsey row (every root at N <= 9): the oracle engine's per-edge counts, the counts section of its state
    vector and the root's cost against tests/test_oracle_ramsey.py:brute_counts (under a second per root at every row's size)"""
    n, sizes, w = c.ctor["n"], c.ctor["sizes"], c.ctor["weights"]
    ref = D.make_ref(orc, c)
    colors, permitted = D.oracle_roots(orc, c)
    ref.e.new_begin(colors, permitted)
    ref.e.new_end(orc.hash_predictions(c.seed, c.first_agent, c.B, ref.e.A, 0))
    E, C = n * (n - 1) // 2, len(sizes)
    for i in range(c.B if n <= 9 else 1):
        counts, totals = brute_counts(n, sizes, colors[i])
        assert np.array_equal(ref.counts(i), counts), (c.id, i)
        assert np.array_equal(ref.state_vecs()[i, :C * E], counts.reshape(-1).astype(np.float32)), (c.id, i)
        cost = np.float32(0)
        for col in range(C):
            cost = np.float32(cost + np.float32(totals[col]) * np.float32(w[col]))
        assert ref.tree(i).c[0] == cost, (c.id, i)


@pytest.mark.parametrize("c", [c for c in RAMSEY if c.ctor["n"] <= 9], ids=lambda c: c.id)
def test_small_ramsey_rows_against_the_recounting_restatement(orc, c):
    """N <= 9: the whole case -- calls, observations, root policy, resets -- on the C++ oracle and on oracle/py_ramsey.py, which
    recounts every clique from the definition after every action"""
    from oracle import py_ramsey as pr
    n, sizes, w = c.ctor["n"], c.ctor["sizes"], c.ctor["weights"]
    E = n * (n - 1) // 2
    ce = orc.Engine(n, c.B, threads=2, ramsey=(sizes, w))
    pe = pr.PyRamseyEngine(n, sizes, w, c.B)
    colors, permitted = D.oracle_roots(orc, c)
    ce.new_begin(colors, permitted)
    pe.new_begin(_unpack_ramsey(colors, permitted, E))
    call = 0
    h = lambda: orc.hash_predictions(c.seed, c.first_agent, c.B, ce.A, call)
    ce.new_end(h())
    pe.new_end(h())
    assert_same_trees(ce, pe, c.B)
    for epoch in range(c.epochs):
        for _ in range(c.calls):
            ce.rollout_begin(*c.tol)
            pe.rollout_begin(*c.tol)
            assert np.array_equal(ce.state_vecs(), pe.vecs)
            call += 1
            assert ce.rollout_end(h()) == pe.rollout_end(h())
            assert ce.argmin()["eval"].tobytes() == np.float32(pe.argmin["eval"]).tobytes()
            assert ce.argmin_totals()[:len(sizes)].tolist() == pe.argmin["state"].totals
        assert_same_trees(ce, pe, c.B)
        for i in range(c.B):
            assert ce.agent_counts(i).tolist() == pe.states[i].counts
        oc, wc = ce.observe(c.n_obs_tol)
        op, wp = pe.observe(c.n_obs_tol)
        nan = np.isnan(oc)
        assert np.array_equal(nan, np.isnan(op)) and np.array_equal(wc, wp)
        assert np.array_equal(oc[~nan].view(np.uint32), op[~nan].view(np.uint32))
        rc = ce.modify_roots(c.seed, epoch, c.first_agent, *c.k)
        rp = pe.modify_roots(c.seed, epoch, c.first_agent, *c.k)
        pc = _pack_ramsey(rp, E, ce.KW)
        assert np.array_equal(rc[0], pc[0]) and np.array_equal(rc[1], pc[1])
        ce.reset_begin(*rc)
        pe.reset_begin(rp)
        call += 1
        ce.reset_end(h())
        pe.reset_end(h())
        assert_same_trees(ce, pe, c.B)


def test_r_n12c3_states_against_the_recount(orc):
    """RamseySpace<4> at three colours with a K4: the live counts and totals of a handful of agents, after the row's first epoch of
    calls, against oracle/py_ramsey.py's recount of their colourings"""
    from oracle import py_ramsey as pr
    c = D.BY_ID["r_n12c3"]
    ref = D.make_ref(orc, c)
    ref.new(D.oracle_roots(orc, c), orc.hash_predictions(c.seed, 0, c.B, ref.e.A, 0))
    for call in range(1, c.calls + 1):
        ref.step(c.tol, orc.hash_predictions(c.seed, 0, c.B, ref.e.A, call))
    moved = [i for i in range(c.B) if ref.agent_state(i)["path"].any()][:5]
    assert len(moved) == 5
    for i in moved:
        st = pr.RamseyState(c.ctor["n"], c.ctor["sizes"], ref.agent_state(i)["parents"], ())
        assert ref.counts(i).tolist() == st.counts, i
        assert ref.e.agent_totals(i)[:3].tolist() == st.totals, i
