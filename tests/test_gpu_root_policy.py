"""GPU checks of the root policy's options (azd_root_policy): the best-cost rule and the weighted colours of a fresh Ramsey root on
every tier and space, against tests/root_policy_ref.py (pinned on the CPU by tests/test_root_policy_abi.py) -- roots, the
per-tree report, and the trees and state vectors after par_reset_trees_policy -- bit for bit; the dense-graph spaces by a
property of the engine alone; the defaults against the C++ oracle; the r45 / r3333 drivers."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import ramsey64_ref as R64
import root_policy_ref as RP
from gpu_parity import R45_W, TOL, assert_tree_equal, az, same_array  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R45_P = [0.4685, 0.5315]


def caps_per_node(calls, per_node):
    return dict(node_capacity=2 * calls + 256, arc_capacity=min(65535, 8 * calls + 256), prediction_capacity=(calls + 2) * per_node + 256)


def bits_of(row, universe):
    return {b for b in range(universe) if (int(row[b >> 6]) >> (b & 63)) & 1}


class RamseyCase:
    """a Ramsey engine and tests/root_policy_ref.py's engine on the same roots and prediction stream"""

    def __init__(self, az, orc, n, sizes, weights, B, kmin, kmax, seed, **space_kw):
        self.az, self.orc, self.B, self.kmin, self.kmax, self.seed = az, orc, B, kmin, kmax, seed
        self.space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, **space_kw)
        sp = self.space
        colors, permitted = sp.generate_roots(seed, B, kmin=kmin, kmax=kmax)
        self.opt = az.NablaOptimizer.par_new(sp, (colors, permitted), az.HashStreamModel(sp.STATE_DIM, sp.ACTION_DIM, seed), B,
                                             **caps_per_node(40, kmax * (sp.C - 1)))
        self.ref = RP.Ramsey64PolicyEngine(n, sizes, weights, B)
        self.call = 0
        self.ref.new_begin(R64.unpack_roots(colors, permitted, sp.E))
        self.ref.new_end(self.h())

    def h(self):
        h = self.orc.hash_predictions(self.seed, 0, self.B, self.space.ACTION_DIM, self.call)
        self.call += 1
        return h

    def roll(self, calls):
        improved = self.opt.par_roll_out_episodes(TOL, n_calls=calls)
        ref = 0
        for _ in range(calls):
            self.ref.rollout_begin(*TOL)
            ref += self.ref.rollout_end(self.h())
        assert improved == ref

    def pack(self, roots):
        return R64.pack_roots(roots, self.space.E, self.space.KEY_WORDS)

    def unpack(self, roots):
        return R64.unpack_roots(roots[0], roots[1], self.space.E)

    def ref_tree(self, i):
        return self.ref.export_tree(i, self.space.KEY_WORDS)


class C21Case(RamseyCase):
    def __init__(self, az, orc, n, B, kmin, kmax, seed, path):
        self.az, self.orc, self.B, self.kmin, self.kmax, self.seed = az, orc, B, kmin, kmax, seed
        self.space = sp = az.ROTModifyParentsOnce(n)
        parents, permitted = sp.generate_roots(seed, B, kmin=kmin, kmax=kmax)
        self.opt = az.NablaOptimizer.par_new(sp, (parents, permitted), az.HashStreamModel(sp.STATE_DIM, sp.ACTION_DIM, seed), B, path=path)
        self.ref = RP.C21PolicyEngine(n, B, seq=path.PATH_KIND == 1)
        self.call = 0
        self.ref.new_begin(self.unpack((parents, permitted)))
        self.ref.new_end(self.h())

    def pack(self, roots):
        sp = self.space
        parents = np.zeros((self.B, sp.n), np.uint8)
        permitted = np.zeros((self.B, sp.KEY_WORDS), np.uint64)
        for i, (p, m) in enumerate(roots):
            parents[i] = p
            for a in m:
                permitted[i, a >> 6] |= np.uint64(1 << (a & 63))
        return parents, permitted

    def unpack(self, roots):
        return [([int(x) for x in roots[0][i]], bits_of(roots[1][i], self.space.ACTION_DIM)) for i in range(self.B)]


def check_policy(case, epoch, rule, color_weights, sample, want_branches=()):
    """the device policy == the helper's: roots, report; then par_reset_trees_policy == the helper's reset (state vectors, sampled
    trees).  Returns (device roots, report)."""
    opt, ref = case.opt, case.ref
    opt.set_root_policy(rule, color_weights)
    want = case.pack(ref.modify_roots(case.seed, epoch, 0, case.kmin, case.kmax, rule=rule, color_weights=color_weights))
    got = opt.modify_roots(case.seed, epoch, case.kmin, case.kmax)
    rep = opt.root_policy_report()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (epoch, rule)
    want_rep = np.array(ref.report, np.int64)
    for k, col in enumerate(("branch", "node", "kept")):
        assert np.array_equal(rep[col].astype(np.int64), want_rep[:, k]), (epoch, col, rep[col], want_rep[:, k])
    print("epoch %d rule %s: branches fresh / stagnant / improved = %s" % (epoch, rule, np.bincount(rep["branch"], minlength=3).tolist()))
    for b in want_branches:
        assert (rep["branch"] == b).any(), (b, rep["branch"])
    opt.par_reset_trees_policy(case.seed, epoch, case.kmin, case.kmax)
    again = opt.root_policy_report()
    assert all(np.array_equal(again[k], rep[k]) for k in rep)
    ref.reset_begin(case.unpack(want))
    ref.reset_end(case.h())
    same_array(opt.state_vecs(), ref.vecs, (epoch, "state_vecs after the reset"))
    for i in sample:
        assert_tree_equal(opt.get_tree(i), case.ref_tree(i), "epoch %d agent %d" % (epoch, i))
    return got, rep


# ---------------------------------------------------------------- 1. narrow Ramsey against the helper
def test_narrow_ramsey_best_rule_and_weights_against_the_helper(az, orc):
    """N = 10, [3,3,3], colour weights [3,1,2], 32 agents, 5..=12 permitted edges, two epochs of 30 calls under BEST.  Every branch
    of the policy is met (asserted from the report), and BEST installs other roots than THRESHOLD from the same trees."""
    case = RamseyCase(az, orc, 10, [3, 3, 3], [1.0] * 3, 32, 5, 12, seed=3)
    w = [3, 1, 2]
    assert case.space.tier == "narrow"
    seen, differing = set(), 0
    for epoch in (0, 1):
        case.roll(30)
        case.opt.set_root_policy("threshold", w)
        thr = case.opt.modify_roots(case.seed, epoch, case.kmin, case.kmax)
        thr_ref = case.pack(case.ref.modify_roots(case.seed, epoch, 0, case.kmin, case.kmax, rule="threshold", color_weights=w))
        assert np.array_equal(thr[0], thr_ref[0]) and np.array_equal(thr[1], thr_ref[1])
        best, rep = check_policy(case, epoch, "best", w, range(0, 32, 4))
        seen |= set(rep["branch"].tolist())
        imp = rep["branch"] == RP.BRANCH_IMPROVED
        d = int(((best[0] != thr[0]).any(axis=1) & imp).sum())
        assert not ((best[0] != thr[0]).any(axis=1) & ~imp).any()  # the rule changes nothing outside the improved branch
        assert np.array_equal(best[1], thr[1])                     # ... and no draw: the permitted sets are the same
        print("epoch %d: roots under BEST differ from THRESHOLD in %d of %d improved trees" % (epoch, d, int(imp.sum())))
        differing += d
    assert {RP.BRANCH_STAGNANT, RP.BRANCH_IMPROVED} <= seen, seen
    assert differing >= 1
    assert case.opt.counters()["FAILED"] == 0


# ---------------------------------------------------------------- 2. the fresh branch with weights
def test_fresh_roots_take_the_colour_weights(az, orc):
    """kmin = kmax = 8, the policy straight after par_new: every tree has c_root == c_root* at kmax, so every root is fresh"""
    case = RamseyCase(az, orc, 10, [3, 3, 3], [1.0] * 3, 32, 8, 8, seed=3)
    w = [3, 1, 2]
    got, rep = check_policy(case, 0, "best", w, range(0, 32, 8))
    assert (rep["branch"] == RP.BRANCH_FRESH).all() and (rep["node"] == RP.NO_NODE).all() and (rep["kept"] == 0).all()
    domain = RP.po.D_RESET
    for i in range(32):
        assert got[0][i].tolist() == RP.edge_colors(case.seed, domain, i, case.space.E, 3, w), i
    share = [float((got[0] == c).mean()) for c in range(3)]
    print("shares of the colours under [3, 1, 2]:", share)
    assert share[0] > share[2] > share[1]  # 1/2, 1/3, 1/6 over 1440 edges: 13 standard deviations apart at the least
    case.opt.set_root_policy("best", None)
    uniform = case.opt.modify_roots(case.seed, 1, 8, 8)
    want = case.pack(case.ref.modify_roots(case.seed, 1, 0, 8, 8, rule="best"))
    assert np.array_equal(uniform[0], want[0]) and np.array_equal(uniform[1], want[1])
    case.opt.set_root_policy("best", [1, 1, 1])  # equal weights: the uniform draw
    equal = case.opt.modify_roots(case.seed, 1, 8, 8)
    assert np.array_equal(equal[0], uniform[0]) and np.array_equal(equal[1], uniform[1])


# ---------------------------------------------------------------- 3. the other tiers and spaces
def test_wide_tier_at_the_r45_shape(az, orc):
    """RamseyWideSpace<10>: N = 24, [4, 5], max_slots = 276, the driver's colour probabilities.  The roots bring 4..=16 permitted
    edges: c_root* moves only when a cascade reaches the root, after a terminal state or a transposition, and with the driver's
    10..=276 no path of 20 calls ends -- every tree would be stagnant and the rule never asked (seen with the reference on the CPU:
    32 stagnant of 32; at 4..=16 and this seed 1 fresh, 8 stagnant, 23 improved, 16 of them re-rooted elsewhere than by THRESHOLD)."""
    case = RamseyCase(az, orc, 24, [4, 5], R45_W, 32, 4, 16, seed=4, max_slots=276)
    assert case.space.tier == "wide"
    case.roll(20)
    check_policy(case, 0, "best", R45_P, range(0, 32, 8), want_branches=(RP.BRANCH_IMPROVED,))


def test_u64_tier_at_the_r3333_shape(az, orc):
    """RamseyU64Space: N = 34, [3,3,3,3], 10..=30 permitted edges, 12 calls: only the trees whose roots brought 10 .. 12 edges can
    have ended a path and improved.  Seed 2 (chosen with the reference on the CPU): 1 fresh, 13 stagnant, 2 improved."""
    case = RamseyCase(az, orc, 34, [3, 3, 3, 3], [1.0] * 4, 16, 10, 30, seed=2)
    assert case.space.tier == "u64"
    case.roll(12)
    check_policy(case, 0, "best", None, range(0, 16, 4), want_branches=(RP.BRANCH_IMPROVED,))


@pytest.mark.parametrize("path_name", ["ActionSet", "ActionSequence"])
def test_c21_set_and_sequence_keys(az, orc, path_name):
    """c21, N = 13: the radix select over set keys, and the subtree-count walk over sequence keys (AZD_PATH_SEQUENCE)"""
    case = C21Case(az, orc, 13, 32, 5, 20, seed=2, path=getattr(az, path_name))
    case.roll(30)
    with pytest.raises(az.AzdError, match="color_weights"):
        case.opt.set_root_policy("best", [1.0, 1.0])
    assert case.opt.root_policy() == dict(rule="threshold", color_weights=None)  # a refused policy leaves the one in force
    thr = case.opt.modify_roots(case.seed, 0, case.kmin, case.kmax)
    best, rep = check_policy(case, 0, "best", None, range(0, 32, 4), want_branches=(RP.BRANCH_IMPROVED,))
    assert case.opt.root_policy() == dict(rule="best", color_weights=None)
    imp = rep["branch"] == RP.BRANCH_IMPROVED
    print("c21 %s: roots under BEST differ from THRESHOLD in %d of %d improved trees" % (
        path_name, int(((best[0] != thr[0]).any(axis=1) & imp).sum()), int(imp.sum())))


@pytest.mark.parametrize("cost", ["c21", "ah"])
def test_dense_spaces_jump_to_the_best_cost(az, cost):
    """The dense-graph spaces have no Python reference of the policy; what holds for every space: a tree the report puts in the
    improved branch is re-rooted, under BEST, at a node whose cost is c_root* -- the new tree's root cost has that bit pattern --
    and under THRESHOLD, from the same trees, at least one of them is re-rooted elsewhere."""
    n, B, seed, kmin, kmax, calls = 8, 32, 5, 5, 14, 20
    space = az.DenseGraphSpace(n, 0.4, max_slots=28, cost=cost)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    after = {}
    for rule in ("best", "threshold"):
        opt = az.NablaOptimizer.par_new(space, roots, az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B)
        opt.par_roll_out_episodes(TOL, n_calls=calls)
        before = [opt.get_tree(i) for i in range(B)]
        c_star = np.array([t.c_star[0] for t in before], np.float32)
        opt.set_root_policy(rule)
        opt.par_reset_trees_policy(seed, 0, kmin, kmax)
        rep = opt.root_policy_report()
        c_new = np.array([opt.get_tree(i).c[0] for i in range(B)], np.float32)
        imp = rep["branch"] == RP.BRANCH_IMPROVED
        for i in np.nonzero(imp)[0]:
            t = before[i]
            assert rep["kept"][i] >= 1 and rep["node"][i] < len(t.c), i
            assert c_new[i].tobytes() == t.c[rep["node"][i]].tobytes(), (rule, i)  # the new root IS the reported node's state
            want_kept = int((t.c == t.c_star[0]).sum()) if rule == "best" else int((t.c <= (t.c[0] + np.float32(3.0) * t.c_star[0]) / np.float32(4.0)).sum())
            assert rep["kept"][i] == want_kept, (rule, i)
        after[rule] = (imp, c_new, c_star)
        assert opt.counters()["FAILED"] == 0
    imp, c_best, c_star = after["best"]
    assert np.array_equal(imp, after["threshold"][0]) and np.array_equal(c_star.view(np.uint32), after["threshold"][2].view(np.uint32))
    assert imp.any()
    assert np.array_equal(c_best[imp].view(np.uint32), c_star[imp].view(np.uint32))
    d = int((after["threshold"][1][imp].view(np.uint32) != c_best[imp].view(np.uint32)).sum())
    print("dense %s: %d improved trees, THRESHOLD re-roots %d of them at another cost" % (cost, int(imp.sum()), d))
    assert d >= 1


# ---------------------------------------------------------------- 4. defaults unchanged
def test_defaults_equal_the_cpp_oracle(az, orc):
    """no set_root_policy call, and again after set_root_policy(NULL): the device policy == the C++ oracle's modify_roots at the
    shape of case 1"""
    n, sizes, B, kmin, kmax, seed = 10, [3, 3, 3], 32, 5, 12, 3
    space = az.RamseySpaceNoEdgeRecolor(n, sizes)
    roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    opt = az.NablaOptimizer.par_new(space, roots, az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B, **caps_per_node(40, kmax * 2))
    oe = orc.Engine(n, B, threads=8, ramsey=(sizes, [1.0] * 3))
    oe.new_begin(*roots)
    oe.new_end(orc.hash_predictions(seed, 0, B, space.ACTION_DIM, 0))
    with pytest.raises(az.AzdError):
        opt.root_policy_report()  # nothing to report yet
    assert opt.root_policy() == dict(rule="threshold", color_weights=None)
    opt.par_roll_out_episodes(TOL, n_calls=30)
    for call in range(1, 31):
        oe.rollout_begin(*TOL)
        oe.rollout_end(orc.hash_predictions(seed, 0, B, space.ACTION_DIM, call))
    ro = oe.modify_roots(seed, 0, 0, kmin, kmax)
    rg = opt.modify_roots(seed, 0, kmin, kmax)
    assert np.array_equal(rg[0], ro[0]) and np.array_equal(rg[1], ro[1])
    opt.set_root_policy("best", [3, 1, 2])
    assert opt.root_policy() == dict(rule="best", color_weights=[3.0, 1.0, 2.0])
    assert not np.array_equal(opt.modify_roots(seed, 0, kmin, kmax)[0], ro[0])
    assert opt._L.azd_engine_set_root_policy(opt._h, None) == 0
    assert opt.root_policy() == dict(rule="threshold", color_weights=None)
    rg = opt.modify_roots(seed, 0, kmin, kmax)
    assert np.array_equal(rg[0], ro[0]) and np.array_equal(rg[1], ro[1])
    for bad, name in ((dict(rule=2), "rule"), (dict(n=2, w=[1, 1]), "n_color_weights"), (dict(n=3, w=[1, 0, 1]), "color_weights")):
        from azdopt_amd import _lib
        p = _lib.RootPolicy(bad.get("rule", 0), bad.get("n", 0))
        for i, x in enumerate(bad.get("w", [])):
            p.color_weights[i] = x
        assert opt._L.azd_engine_set_root_policy(opt._h, C.byref(p)) == 1
        assert opt._L.azd_last_error().decode().startswith(name + ":"), (bad, opt._L.azd_last_error())


# ---------------------------------------------------------------- 5. the drivers
def test_r45_driver_runs_the_reference_policy(tmp_path):
    from azdopt_amd import sinks
    out = tmp_path / "ev"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ramsey.py"), "r45", "--epochs", "2", "--episodes", "40", "--batch",
                        "32", "--hidden", "64", "--stride", "10", "--out", str(out)], cwd=tmp_path, check=True, timeout=600,
                       capture_output=True, text=True)
    assert "TotalCounts([" in r.stdout and "==== EPOCH: 2 ====" in r.stdout, r.stdout
    ev = sinks.read_events(out / "tfevents-losses")
    tags = [t for e in ev for t, _ in e[3]]
    assert tags.count("loss") == 2 and {"clique_counts/0", "clique_counts/1"} <= set(tags)


def test_driver_presets_set_the_policy(az):
    """the engines as examples/ramsey.py builds them: r45 under BEST with the driver's colour probabilities and a ReLU head, r3333
    under BEST, r44 on the defaults"""
    spec = importlib.util.spec_from_file_location("ramsey_example", os.path.join(ROOT, "examples", "ramsey.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    assert ex.DRIVERS["r45"]["final_act"] == az.ACT_RELU == ex.DRIVERS["r3333"]["final_act"]
    opt, model, kmin, kmax, episodes = ex.build_optimizer("r45", batch=32, episodes=40, hidden=[64])
    assert opt.root_policy() == dict(rule="best", color_weights=[0.4685, 1.0 - 0.4685]) and (kmin, kmax, episodes) == (10, 276, 40)
    opt.par_roll_out_episodes(ex.DRIVERS["r45"]["tol"], n_calls=10)
    opt.par_reset_trees_policy(0, 1, kmin, kmax)
    assert opt.counters()["FAILED"] == 0 and len(opt.root_policy_report()["branch"]) == 32
    opt, _, _, _, _ = ex.build_optimizer("r3333", batch=16, episodes=20, hidden=[64])
    assert opt.root_policy() == dict(rule="best", color_weights=None)
    opt, _, _, _, _ = ex.build_optimizer("r44", batch=16, episodes=20, hidden=[64])
    assert opt.root_policy() == dict(rule="threshold", color_weights=None)
