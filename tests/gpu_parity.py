"""Shared scaffolding of the GPU parity tests (a helper like tests/bf16_exact.py: no test lives here).
  * the `az` fixture, the counter lists, the tolerance tables and shapes several families share;
  * same_array / assert_tree_equal / caps / assert_same_run;
  * the reference engines behind one small interface (new, step, state_vecs, tree, agent_state, observe, counters, argmin,
    modify_roots, reset): OracleRef (the C++ oracle: c21 and dense), CppRef (the C++ oracle's Ramsey engine), PyRef
    (tests/ramsey64_ref.py), PyDenseRef (tests/dense_ah_ref.py's and tests/dense_ah_wide_ref.py's engines);
  * the three family comparisons (compare_c21, compare_ramsey, compare_ah);
  * run_lockstep, the one loop that drives an optimizer and a reference through the same hash-stream predictions and compares them
    after par_new, after every chunk of calls and after every reset.
tests/test_parity_harness.py shows on the CPU that each item compared here fails the run when it is wrong."""
import numpy as np
import pytest

import ramsey64_ref as R

MAIN_CTRS = ("EXPANSIONS", "TERMINALS", "TRANSPOSITIONS", "VISITED_STEPS", "SELECT_CALLS", "SUM_DEG", "SUM_ACTIONS",
             "CASCADE_NODES", "NEW_PREDS", "ROOT_EXHAUSTED", "MAX_FRONTIER", "MAX_DEPTH", "CURIOSITY_PAIRS", "FAILED")
# the c21 and dense-graph families' list: MAX_FRONTIER is no per-call parity quantity there (after the first call of an N = 5 c21
# run, and of an N = 8 dense pool run, the device reports 1 and the oracle 0; later in a run the two maxima meet)
C21_CTRS = tuple(k for k in MAIN_CTRS if k != "MAX_FRONTIER")
TOL = ([200, 200, 100, 100, 50, 50, 25, 25], 10)  # 02-r44.rs:128-130, 05-r45.rs
TOL_REF = ([200, 50, 50], 25)  # 04-c21-tree.rs:136-138, the live drivers' tolerances
R45_W = [1.0, 0.4685 / (1.0 - 0.4685)]  # 05-r45.rs:84-85,101-103: [W_RED, P_RED / P_BLUE]
R3333 = (34, [3, 3, 3, 3], [1.0] * 4)
R3333_DIMS = (5049, 512, 1024, 512, 2244)
AGENT_KEYS = ("parents", "permitted", "path", "state_pos")


@pytest.fixture(scope="module")
def az():
    import azdopt_amd
    if azdopt_amd.device_count() < 1:
        pytest.fail("no gfx950 device: the GPU tests need the HIP path")
    return azdopt_amd


def _bits(x):
    return x.view("u%d" % x.dtype.itemsize) if x.dtype.kind == "f" else x.astype(np.int64)


def same_array(a, b, tag):
    """shape, then floats by bit pattern and integers as int64; a failure names the first mismatching indices and both values"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    x, y = _bits(a), _bits(b)
    if not np.array_equal(x, y):
        idx = np.argwhere(x != y) if x.shape == y.shape else []
        where = f"first mismatch at {idx[:3].tolist()} gpu={a[tuple(idx[0])]} reference={b[tuple(idx[0])]}" if len(idx) else f"{a.dtype} != {b.dtype}"
        raise AssertionError(f"{tag}: {where}")


def assert_tree_equal(tg, to, tag=""):
    """an exported tree against a reference's, given as an object with the fields or as a dict"""
    for f in tg.FIELDS:
        same_array(getattr(tg, f), to[f] if isinstance(to, dict) else getattr(to, f), f"{tag} field {f}")


def same_counters(cg, co, tag, names=MAIN_CTRS):
    for k in names:
        assert cg[k] == co[k], (tag, k, cg[k], co[k])


def caps(calls, space, kmax):
    """arenas for `calls` calls of nodes of up to kmax * (C - 1) actions (the default 32768 predictions fill within ~120 calls at r45)"""
    return dict(node_capacity=2 * calls + 256, arc_capacity=min(65535, 8 * calls + 256),
                prediction_capacity=(calls + 2) * kmax * (space.C - 1) + 256)


def assert_same_run(o0, o1, B, tag="", every=1, predictions=True):
    """two optimizers after the same calls: counters, every `every`-th agent's tree and state, state vectors, prediction bits
    (predictions=False: the models' rows are not comparable), the argmin and its cost -- re-evaluated where the space can"""
    same_counters(o0.counters(), o1.counters(), tag)
    for i in range(0, B, every):
        assert_tree_equal(o0.get_tree(i), o1.get_tree(i), f"{tag} agent {i}")
        s0, s1 = o0.agent_state(i), o1.agent_state(i)
        for k in s0:
            assert np.array_equal(s0[k], s1[k]), (tag, i, k, s0[k], s1[k])
    same_array(o0.state_vecs(), o1.state_vecs(), f"{tag} state_vecs")
    if predictions:
        same_array(o0.predictions(), o1.predictions(), f"{tag} prediction bits")
    a0, a1 = o0.argmin_data(), o1.argmin_data()
    assert a0.eval.tobytes() == a1.eval.tobytes() and (a0.agent, a0.node) == (a1.agent, a1.node) and a0.cost == a1.cost, tag
    if getattr(o0.space, "COST", None) == "ah":
        assert o0.space.ah_cost(a0.state["adj"])["cost"] == a0.cost["cost"], tag


# ---------------------------------------------------------------- reference engines
def words(bits, kw):
    out = np.zeros(kw, np.uint64)
    for b in bits:
        out[b >> 6] |= np.uint64(1 << (b & 63))
    return out


class OracleRef:
    """an oracle.orc.Engine -- c21, dense or Ramsey by how it was created -- behind the interface run_lockstep drives"""

    def __init__(self, engine):
        self.e, self.KW = engine, engine.KW

    @classmethod
    def c21(cls, orc, n, B, threads=8):
        return cls(orc.Engine(n, B, threads=threads))

    @classmethod
    def dense(cls, orc, n, B, p, threads=8):
        return cls(orc.Engine(n, B, threads=threads, dense=True, dense_p=p))

    def new(self, roots, h):
        self.e.new_begin(*roots)
        self.e.new_end(h)

    def step(self, tol, h):
        self.e.rollout_begin(*tol)
        return self.e.rollout_end(h)

    state_vecs = lambda self: self.e.state_vecs()
    tree = lambda self, i: self.e.export_tree(i)
    agent_state = lambda self, i: self.e.agent_state(i)
    observe = lambda self, t: self.e.observe(t)
    counters = lambda self: self.e.counters()
    argmin = lambda self: self.e.argmin()

    def modify_roots(self, seed, epoch, first_agent, kmin, kmax):
        return self.e.modify_roots(seed, epoch, first_agent, kmin, kmax)

    def reset(self, roots, h):
        self.e.reset_begin(*roots)
        self.e.reset_end(h)


class CppRef(OracleRef):
    """the C++ oracle's Ramsey engine (N <= 32); argmin() -> (colours, permitted words, eval, totals)"""

    def __init__(self, orc, n, sizes, weights, B, threads=16):
        super().__init__(orc.Engine(n, B, threads=threads, ramsey=(sizes, weights)))
        self.C = len(sizes)

    counts = lambda self, i: self.e.agent_counts(i)

    def argmin(self):
        a = self.e.argmin()
        return a["parents"], a["permitted"], a["eval"], self.e.argmin_totals()[:self.C].tolist()


class PyRef:
    """tests/ramsey64_ref.py's engine (any N) behind the same interface; it keeps no counters"""

    def __init__(self, n, sizes, weights, B):
        self.e = R.Ramsey64RefEngine(n, sizes, weights, B)
        self.E, self.C = self.e.E, len(sizes)
        self.KW = (self.e.A + 63) // 64

    def new(self, roots, h):
        self.e.new_begin(R.unpack_roots(roots[0], roots[1], self.E))
        self.e.new_end(h)

    def step(self, tol, h):
        self.e.rollout_begin(*tol)
        return self.e.rollout_end(h)

    state_vecs = lambda self: self.e.vecs
    tree = lambda self, i: self.e.export_tree(i, self.KW)
    counts = lambda self, i: np.array(self.e.states[i].counts, np.int32)
    observe = lambda self, t: self.e.observe(t)
    counters = lambda self: None

    def agent_state(self, i):
        st = self.e.states[i]
        return dict(parents=np.array(st.colors, np.uint8), permitted=words(st.permitted, self.KW), path=words(self.e.paths[i], self.KW),
                    state_pos=self.e.posn[i])

    def argmin(self):
        st = self.e.argmin["state"]
        return np.array(st.colors, np.uint8), words(st.permitted, self.KW), np.float32(self.e.argmin["eval"]), list(st.totals)

    def modify_roots(self, seed, epoch, first_agent, kmin, kmax):
        return R.pack_roots(self.e.modify_roots(seed, epoch, first_agent, kmin, kmax), self.E, self.KW)

    def reset(self, roots, h):
        self.e.reset_begin(R.unpack_roots(roots[0], roots[1], self.E))
        self.e.reset_end(h)


class PyDenseRef(OracleRef):
    """dense_ah_ref.PyDenseEngine or dense_ah_wide_ref.PyDenseWideEngine (the oracle's method names; the argmin is an attribute
    there): argmin() -> the cost record with adj and permitted as the engine's arrays"""

    def __init__(self, engine):
        self.e, self.KW = engine, engine.KW

    def argmin(self):
        a = self.e.argmin
        return dict(a, adj=np.array(a["state"].adj, np.uint64), permitted=np.array(self.e.mask(a["state"].slots), np.uint64))


# ---------------------------------------------------------------- the families' comparisons: compare(opt, ref, agents, tag)
def compare_c21(opt, ref, agents, tag, counters=MAIN_CTRS):
    """c21 and the dense-graph space with the c21 cost: state vectors, trees, every key of the reference's agent state (lambda_1 as
    an f64: a bit-identical procedure), argmin state, eval, lambda_1 and matching size, `counters` (see C21_CTRS)"""
    same_array(opt.state_vecs(), ref.state_vecs(), f"{tag} state_vecs")
    for i in agents:
        assert_tree_equal(opt.get_tree(i), ref.tree(i), f"{tag} agent {i}")
        sg, so = opt.agent_state(i), ref.agent_state(i)
        for k in so:
            assert np.array_equal(sg[k], so[k]), (tag, i, k, sg[k], so[k])
    ag, ao = opt.argmin_data(), ref.argmin()
    root = ag.state["adj"].view(np.uint8) if "adj" in ag.state else ag.state["parents"]
    assert np.array_equal(root, ao["parents"]) and np.array_equal(ag.state["permitted"], ao["permitted"]), tag
    assert ag.eval == ao["eval"] and ag.cost["lambda_1"] == ao["lambda1"] and len(ag.cost["matching"]) == ao["matching"], tag
    same_counters(opt.counters(), ref.counters(), tag, counters)


def compare_ramsey(space, taken=None, argmin_any=False):
    """the Ramsey spaces: compare_c21's items over the four agent-state keys, plus live clique counts and the argmin's totals.  The
    argmin's permitted words are compared over the (E + 63) // 64 that hold edges; both sides' words beyond them are zero.
    taken: a set that collects the action ids on the compared agents' paths.  argmin_any: the device's record has exactly
    those words (argmin_data() went through azd_engine_ramsey_argmin_any)."""
    pw = (space.E + 63) // 64

    def compare(opt, ref, agents, tag):
        same_array(opt.state_vecs(), ref.state_vecs(), f"{tag} state_vecs")
        for i in agents:
            assert_tree_equal(opt.get_tree(i), ref.tree(i), f"{tag} agent {i}")
            sg, so = opt.agent_state(i), ref.agent_state(i)
            for k in AGENT_KEYS:
                assert np.array_equal(sg[k], so[k]), (tag, i, k, sg[k], so[k])
            if taken is not None:
                taken.update(64 * w + b for w, x in enumerate(sg["path"]) for b in range(64) if (int(x) >> b) & 1)
            cg, tg = opt.ramsey_agent_counts(i)
            assert np.array_equal(cg, ref.counts(i)), (tag, i)
        ag = opt.argmin_data()
        colors_o, perm_o, eval_o, totals_o = ref.argmin()
        perm_g = ag.state["permitted"]
        assert np.array_equal(ag.state["colors"], colors_o), tag
        assert np.array_equal(perm_g[:pw], perm_o[:pw]) and not perm_g[pw:].any() and not perm_o[pw:].any(), tag
        if argmin_any:
            assert len(perm_g) == pw, tag
        assert ag.eval.tobytes() == np.float32(eval_o).tobytes(), (tag, ag.eval, eval_o)
        assert ag.cost["clique_counts"] == totals_o, tag
        co = ref.counters()
        if co is not None:
            same_counters(opt.counters(), co, tag)

    return compare


def f64_bits(x):
    return np.float64(x).view(np.uint64)


def compare_ah(opt, ref, agents, tag):
    """the dense-graph space with the Aouchiche-Hansen cost against PyDenseRef: the cost fields bit for bit, the counters the
    reference keeps, and the argmin's graph re-evaluated through the host function"""
    same_array(opt.state_vecs(), ref.state_vecs(), f"{tag} state_vecs")
    for i in agents:
        assert_tree_equal(opt.get_tree(i), ref.tree(i), f"{tag} agent {i}")
        sg, sp = opt.agent_state(i), ref.agent_state(i)
        for k in sp:  # (the cost fields are absent while the reference's agent stands on its root)
            if k in ("proximity", "eigenvalue"):
                assert f64_bits(sg[k]) == f64_bits(sp[k]), (tag, i, k, sg[k], sp[k])
            elif k == "cost":
                assert np.float32(sg[k]).view(np.uint32) == np.float32(sp[k]).view(np.uint32), (tag, i, k)
            else:
                assert np.array_equal(sg[k], sp[k]), (tag, i, k, sg[k], sp[k])
    cp = ref.counters()
    same_counters(opt.counters(), cp, tag, names=cp)
    ag, ap = opt.argmin_data(), ref.argmin()
    assert ag.eval.view(np.uint32) == np.float32(ap["eval"]).view(np.uint32), tag
    assert f64_bits(ag.cost["proximity"]) == f64_bits(ap["proximity"]) and f64_bits(ag.cost["eigenvalue"]) == f64_bits(ap["eigenvalue"]), tag
    assert (ag.cost["diameter"], ag.cost["k"]) == (ap["diameter"], ap["k"]) and ag.cost["cost"] == ap["cost"], tag
    assert np.array_equal(ag.state["adj"], ap["adj"]) and np.array_equal(ag.state["permitted"], ap["permitted"]), tag
    again = opt.space.ah_cost(ag.state["adj"])
    assert again["cost"] == ag.cost["cost"] and again["eval"] == ag.eval and f64_bits(again["eigenvalue"]) == f64_bits(ag.cost["eigenvalue"]), tag


# ---------------------------------------------------------------- the lock-step driver
def assert_form(opt, form):
    """what ran after a chunk of calls.  None: not asserted; "per_call": the form's name starts with it; "pool": the pool step with no
    reason to report; "dense_per_call" / "dense_pool": the dense spaces' forms -- one launch per phase with the space's reason, or the
    pool step with every expanded row through the evaluator's launches"""
    if form is None:
        return
    ran = opt.step_form()
    if form == "per_call":
        assert ran[0].startswith("per_call"), ran
    elif form == "dense_per_call":
        assert ran[0] == "per_call" and "dense-graph space" in ran[1], ran
    else:
        assert form in ("pool", "dense_pool"), form
        assert ran == ("pool", ""), ran
        if form == "dense_pool":
            c = opt.counters()
            assert c["EVAL_ROWS"] == c["EXPANSIONS"] > 0, (c["EVAL_ROWS"], c["EXPANSIONS"])


def run_lockstep(opt, ref, roots, orc, compare, *, seed, tol, steps, epochs=None, kmin, kmax, n_obs_tol, first_agent=0, check_every=1,
                 sample=None, boundary="alternate", host_policy=False, last_boundary=True, form=None, nan_payloads=False,
                 clean_end=True):
    """Drives `opt` (created by par_new on `roots` with a HashStreamModel(seed, first_agent)) and the reference engine `ref` through
    the same predictions -- orc.hash_predictions(seed, first_agent, B, ACTION_DIM, call), call counted here -- and compares them with
    compare(opt, ref, agents, tag) after par_new, after every chunk of `check_every` calls and after every reset.
    steps: calls per epoch, one number (with `epochs`) or one per epoch.  sample: the agents compared (default all).
    boundary, after an epoch's calls and the observe check: "alternate" -- the device policy's roots equal the reference's, then
    par_reset_trees_policy in even epochs and par_reset_trees(reference's roots) in odd ones; "policy" -- the same with
    par_reset_trees_policy every time; "fresh" -- fresh seeded roots from the host, no policy.  host_policy: the host restatement
    of the policy (c21_modify_roots(device=False)) is held to the reference's roots too.  last_boundary=False: the run ends with
    the last epoch's calls.  form: see assert_form.  nan_payloads: observations equal bit for bit, NaNs included (default: equal NaN
    positions, every other value bit for bit -- a NaN's payload is not part of the Ramsey spaces' contract).  clean_end: FAILED == 0
    and EXPANSIONS > 0 when the run is over."""
    space, B = opt.space, opt.batch
    steps = [steps] * epochs if epochs is not None else list(steps)
    agents = range(B) if sample is None else sample
    call = 0
    h = lambda: orc.hash_predictions(seed, first_agent, B, space.ACTION_DIM, call)
    ref.new(roots, h())
    compare(opt, ref, agents, "par_new")
    for epoch, n_steps in enumerate(steps):
        s = 0
        while s < n_steps:
            k = min(check_every, n_steps - s)
            improved_g = opt.par_roll_out_episodes(tol, n_calls=k)
            assert_form(opt, form)
            improved_o = 0
            for _ in range(k):
                call += 1
                improved_o += ref.step(tol, h())
            assert improved_g == improved_o, (epoch, s, improved_g, improved_o)
            s += k
            compare(opt, ref, agents, f"epoch {epoch} step {s}")
        if epoch + 1 == len(steps) and not last_boundary:
            break
        sv, obs, w = opt.observe(n_obs_tol)
        oo, ow = ref.observe(n_obs_tol)
        nan = np.isnan(oo)
        assert np.array_equal(np.isnan(obs), nan), (epoch, "observation NaNs")
        same_array(obs if nan_payloads else obs[~nan], oo if nan_payloads else oo[~nan], f"epoch {epoch} observations")
        assert np.array_equal(w, ow), (epoch, "observation weights")
        same_array(sv, ref.state_vecs(), f"epoch {epoch} observe rows")
        if boundary == "fresh":
            new_roots = space.generate_roots(seed, B, epoch=epoch + 1, kmin=kmin, kmax=kmax)  # `modify_root`: fresh seeded roots from the host
            opt.par_reset_trees(new_roots)
        else:
            assert boundary in ("alternate", "policy"), boundary
            new_roots = ref.modify_roots(seed, epoch, first_agent, kmin, kmax)  # the drivers' modify_root policy (02-r44.rs:196-228)
            for device in (True, False) if host_policy else (True,):
                got = opt.modify_roots(seed, epoch, kmin, kmax, **({} if device else dict(device=False)))
                assert np.array_equal(got[0], new_roots[0]) and np.array_equal(got[1], new_roots[1]), (epoch, device)
            if boundary == "policy" or epoch % 2 == 0:
                opt.par_reset_trees_policy(seed, epoch, kmin, kmax)  # policy + reset without a host round trip
            else:
                opt.par_reset_trees(new_roots)
        call += 1
        ref.reset(new_roots, h())
        compare(opt, ref, agents, f"epoch {epoch} reset")
    if clean_end:
        c = opt.counters()
        assert c["FAILED"] == 0 and c["EXPANSIONS"] > 0, (c["FAILED"], c["EXPANSIONS"])
