"""tests/gpu_parity.py's lock-step driver and Ramsey comparison on the CPU: a facade presents the optimizer methods they call over
the C++ oracle's engine, at the smallest shape at which the narrow GPU test reports terminals and transpositions (the Ramsey space
at N = 6, [3, 3]; 6 agents; 12 calls per epoch, 2 epochs, compared every 4 calls).
  a) the facade passes against tests/ramsey64_ref.py's engine (PyRef: another implementation) and against the oracle itself (CppRef);
  b) with one element of one compared item wrong -- one bit of an f32 -- the driver raises, item by item.
Every colouring of K6 has a monochromatic triangle, so no observation of this shape is NaN (h_sa = 1 - c*/c needs c = 0): the NaN
case plants a NaN in the facade's observations instead of taking one away, and no case is skipped."""
import types

import numpy as np
import pytest

from gpu_parity import CppRef, PyRef, compare_ramsey, run_lockstep

N, SIZES, WEIGHTS, B, KMIN, KMAX, SEED = 6, [3, 3], [1.0, 1.0], 6, 3, 7, 1
TOL_SMALL, STEPS, EPOCHS, EVERY = ([6, 3, 2], 1), 12, 2, 4
TREE_FIELDS = ("c", "c_star", "n_t", "exhausted", "act_begin", "act_end", "keys", "e_src", "e_dst", "e_pp", "p_aid", "p_g", "p_edge")
ITEMS = (["state_vecs"] + ["tree." + f for f in TREE_FIELDS] + ["agent." + k for k in ("parents", "permitted", "path", "state_pos")] +
         ["counts", "argmin.colors", "argmin.permitted", "argmin.eval", "argmin.totals", "counter", "improved", "obs", "weights", "nan",
          "roots.colors", "roots.masks"])


def flipped(x):
    """x with its first element changed: one bit of a float, the lowest bit of an integer"""
    if isinstance(x, (int, np.integer)):
        return x ^ 1
    if isinstance(x, np.floating):
        return (np.array([x]).view(np.uint32) ^ np.uint32(1)).view(np.float32)[0]
    y = np.array(x)
    if not y.size:
        raise ValueError("nothing to corrupt")
    flat = y.reshape(-1)
    if y.dtype.kind == "f":
        flat.view(np.uint32)[0] ^= np.uint32(1)
    else:
        flat[0] ^= 1
    return y


class Facade:
    """the optimizer methods run_lockstep and compare_ramsey call, over orc.Engine fed the hash stream; `corrupt` names the one item
    it reports wrongly (agent 0's, where the item is per agent) once the first chunk of calls is through"""

    def __init__(self, orc, roots, corrupt=None):
        self.orc, self.corrupt, self.call, self.batch, self.seen = orc, corrupt, 0, B, {}
        self.e = e = orc.Engine(N, B, threads=1, ramsey=(SIZES, WEIGHTS))
        self.space = types.SimpleNamespace(E=N * (N - 1) // 2, C=len(SIZES), STATE_DIM=e.S, ACTION_DIM=e.A, KEY_WORDS=e.KW)
        e.new_begin(*roots)
        e.new_end(self.h())

    def h(self):
        return self.orc.hash_predictions(SEED, 0, B, self.space.ACTION_DIM, self.call)

    def wrong(self, item, value, agent=0):
        return flipped(value) if item == self.corrupt and agent == 0 and self.call > EVERY else value

    def par_roll_out_episodes(self, tol, n_calls=1):
        improved = 0
        for _ in range(n_calls):
            self.e.rollout_begin(*tol)
            self.call += 1
            improved += self.e.rollout_end(self.h())
        return self.wrong("improved", improved)

    def step_form(self):
        return "per_call", "the oracle"

    def state_vecs(self):
        return self.wrong("state_vecs", self.e.state_vecs())

    def get_tree(self, i):
        t = self.e.export_tree(i)
        if i == 0 and self.call == 2 * EVERY:  # where a corrupted run is first compared
            self.seen["tree"] = {f: getattr(t, f).size for f in t.FIELDS}
        for f in t.FIELDS:
            setattr(t, f, self.wrong("tree." + f, getattr(t, f), i))
        return t

    def agent_state(self, i):
        return {k: self.wrong("agent." + k, v, i) for k, v in self.e.agent_state(i).items()}

    def ramsey_agent_counts(self, i):
        return self.wrong("counts", self.e.agent_counts(i), i), self.e.agent_totals(i)[:self.space.C]

    def argmin_data(self):
        a = self.e.argmin()
        totals = self.e.argmin_totals()[:self.space.C]
        return types.SimpleNamespace(state=dict(colors=self.wrong("argmin.colors", a["parents"]), permitted=self.wrong("argmin.permitted", a["permitted"])),
                                     eval=self.wrong("argmin.eval", a["eval"]), cost=dict(clique_counts=self.wrong("argmin.totals", totals).tolist()))

    def counters(self):
        c = self.e.counters()
        c["TERMINALS"] = self.wrong("counter", c["TERMINALS"])
        return c

    def observe(self, n_obs_tol):
        obs, w = self.e.observe(n_obs_tol)
        assert not np.isnan(obs).any()  # (see the module's docstring)
        self.seen["weights"] = self.seen.get("weights", 0) + int(w.sum())
        if self.corrupt == "nan":
            obs[0, 0] = np.nan
        return self.e.state_vecs(), self.wrong("obs", obs), self.wrong("weights", w)

    def modify_roots(self, seed, epoch, kmin, kmax):
        colors, masks = self.e.modify_roots(seed, epoch, 0, kmin, kmax)
        return self.wrong("roots.colors", colors), self.wrong("roots.masks", masks)

    def par_reset_trees(self, roots):
        self.e.reset_begin(*roots)
        self.call += 1
        self.e.reset_end(self.h())

    def par_reset_trees_policy(self, seed, epoch, kmin, kmax):
        self.par_reset_trees(self.e.modify_roots(seed, epoch, 0, kmin, kmax))


def drive(orc, ref, corrupt=None):
    roots = orc.gen_ramsey_roots(SEED, 0, 0, B, N, len(SIZES), KMIN, KMAX)
    opt = Facade(orc, roots, corrupt)
    run_lockstep(opt, ref, roots, orc, compare_ramsey(opt.space), seed=SEED, tol=TOL_SMALL, steps=STEPS, epochs=EPOCHS, kmin=KMIN, kmax=KMAX,
                 n_obs_tol=2, check_every=EVERY, form="per_call")
    return opt


@pytest.mark.parametrize("ref", ["py", "cpp"])
def test_the_facade_passes_against_both_references(orc, ref):
    opt = drive(orc, PyRef(N, SIZES, WEIGHTS, B) if ref == "py" else CppRef(orc, N, SIZES, WEIGHTS, B, threads=1))
    assert opt.call == EPOCHS * (STEPS + 1)


@pytest.fixture(scope="module")
def clean(orc):
    return drive(orc, CppRef(orc, N, SIZES, WEIGHTS, B, threads=1))


@pytest.mark.parametrize("item", ITEMS)
def test_one_wrong_element_fails_the_run(orc, clean, item):
    # the uncorrupted run is not vacuous: terminals, transpositions, observations with weight, and something in every field of
    # agent 0's tree where a corrupted run is first compared
    c = clean.counters()
    assert c["TERMINALS"] > 0 and c["TRANSPOSITIONS"] > 0 and clean.seen["weights"] > 0, (c, clean.seen)
    assert all(clean.seen["tree"][f] > 0 for f in TREE_FIELDS), clean.seen
    with pytest.raises(AssertionError):
        drive(orc, CppRef(orc, N, SIZES, WEIGHTS, B, threads=1), corrupt=item)
