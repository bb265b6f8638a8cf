#!/usr/bin/env python3
"""Measurements of the dense-graph space with the weighted-invariant cost (profiles/r17_dense_inv.txt) on one MI355X.

    python tools/bench_dense_inv.py [--reps 100] [--graphs 512] [--epochs 2] [--episodes 200] [--agents 512] [--wide]

  * microseconds per cost from the probe (azd_debug_probe_inv_cost, `reps` repetitions per wave) at n = 31 on G(31, 0.4) graphs under
    the recipes AH, INT, ADJ and BOTH of tests/dense_inv_ref.py, beside azd_debug_probe_ah_cost on the same graphs in the same
    process;
  * expansions/s of the examples' loop -- examples/ah.py and examples/invariants.py: one call per launch, the fp32 model
    1396-256-128-930, par_update_model and the device root policy at the epoch boundary; the first epoch is warm-up and not counted
    -- at N = 31 for an AZD_ENGINE_DENSE_AH engine, an AZD_ENGINE_DENSE_INV engine under the AH recipe, and one under INT (which
    runs no eigen-solve).
--wide (profiles/r18_dense_inv_wide.txt): the cost's 64-row form -- the wide probe (azd_debug_probe_inv_cost_wide) at n = 50 and
n = 64 on G(n, 0.4) graphs under AH, INT and BOTH beside azd_debug_probe_ah_cost_wide on the same graphs, which is run twice (the
difference of the two is the box's run-to-run spread); at n = 32 the wide probe beside the narrow one; and the examples' loop at
N = 50 for an ah_wide=True engine, an inv_wide=True engine under the AH recipe, and one under INT.
One line per figure; nothing here asserts."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import azdopt_amd as az  # noqa: E402
from azdopt_amd import _lib  # noqa: E402
import dense_ah_ref as A  # noqa: E402
import dense_inv_ref as R  # noqa: E402

N, P, TOL = 31, 0.4, ([200, 50, 50], 25)


def cost_of(recipe):
    return az.InvariantCost(recipe.weights(), **recipe.kwargs())


def probes(graphs, reps):
    L = az.lib()
    a = np.array(graphs, dtype=np.uint64)
    ms = C.c_float(0)
    for rnd in range(2):  # the second round's figures are printed (the first loads the code objects)
        out = (_lib.DenseAhCost * len(graphs))()
        _lib.check(L.azd_debug_probe_ah_cost(0, _lib.ptr(a), N, len(graphs), reps, out, C.byref(ms)), "probe_ah_cost")
        ah = ms.value
        if rnd:
            print("probe n=%d graphs=%d reps=%d  azd_debug_probe_ah_cost       %8.3f ms  %7.3f us/cost/wave" % (N, len(graphs), reps, ah, 1e3 * ah / reps))
        for name in ("AH", "INT", "ADJ", "BOTH"):
            rc = cost_of(R.RECIPES[name](N)).recipe()
            dev = (_lib.DenseInvCost * len(graphs))()
            _lib.check(L.azd_debug_probe_inv_cost(0, _lib.ptr(a), N, len(graphs), reps, C.byref(rc), dev, C.byref(ms)), "probe_inv_cost")
            if rnd:
                print("probe n=%d graphs=%d reps=%d  azd_debug_probe_inv_cost %-4s  %8.3f ms  %7.3f us/cost/wave  %.3f x the AH probe"
                      % (N, len(graphs), reps, name, ms.value, 1e3 * ms.value / reps, ms.value / ah))


def probes_wide(n, count, reps):
    L = az.lib()
    rng = np.random.default_rng(n)
    a = np.array([A.gnp_connected(rng, n, P) for _ in range(count)], dtype=np.uint64)
    ms = C.c_float(0)
    tag = "probe n=%d graphs=%d reps=%d " % (n, count, reps)
    for rnd in range(2):  # the second round's figures are printed (the first loads the code objects)
        ah = []
        for _ in range(2):
            out = (_lib.DenseAhCost * count)()
            _lib.check(L.azd_debug_probe_ah_cost_wide(0, _lib.ptr(a), n, count, reps, out, C.byref(ms)), "probe_ah_cost_wide")
            ah.append(ms.value)
        if rnd:
            print(tag + " azd_debug_probe_ah_cost_wide        %9.3f ms  %8.3f us/cost/wave; again %9.3f ms  %8.3f us/cost/wave  (spread %.3f %%)"
                  % (ah[0], 1e3 * ah[0] / reps, ah[1], 1e3 * ah[1] / reps, 100.0 * abs(ah[0] - ah[1]) / min(ah)))
        for name in ("AH", "INT", "BOTH"):
            rc = cost_of(R.RECIPES[name](n)).recipe()
            dev = (_lib.DenseInvCost * count)()
            _lib.check(L.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), n, count, reps, C.byref(rc), dev, C.byref(ms)), "probe_inv_cost_wide")
            if rnd:
                print(tag + " azd_debug_probe_inv_cost_wide %-4s  %9.3f ms  %8.3f us/cost/wave  %.3f x the AH-wide probe (its smaller run)"
                      % (name, ms.value, 1e3 * ms.value / reps, ms.value / min(ah)))
            if n <= 32:
                _lib.check(L.azd_debug_probe_inv_cost(0, _lib.ptr(a), n, count, reps, C.byref(rc), dev, C.byref(ms)), "probe_inv_cost")
                if rnd:
                    print(tag + " azd_debug_probe_inv_cost      %-4s  %9.3f ms  %8.3f us/cost/wave  (the 32-row kernel)" % (name, ms.value, 1e3 * ms.value / reps))


def loop_rate(cost, agents, epochs, episodes, seed=0, n=N, **wide):
    space = az.DenseGraphSpace(n, P, max_slots=128, cost=cost, **wide)
    model = az.ActionModel(agents, space.STATE_DIM, space.ACTION_DIM, hidden=(256, 128), lr=1e-4, l2=1e-6, seed=seed)
    kmin, kmax = space.default_permitted_range()
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(seed, agents, kmin=kmin, kmax=kmax), model, agents, **az.tree_capacities(episodes, kmax))
    rates = []
    for epoch in range(epochs + 1):
        e0 = opt.counters()["EXPANSIONS"]
        t0 = time.perf_counter()
        for _ in range(episodes):
            if opt.par_roll_out_episodes(TOL, n_calls=1):
                opt.argmin_data()
        opt.par_update_model(200)
        opt.par_reset_trees_policy(seed, epoch, kmin, kmax)
        e1 = opt.counters()["EXPANSIONS"]
        if epoch:
            rates.append((e1 - e0) / (time.perf_counter() - t0))
    return float(np.mean(rates)), opt.step_form()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    if args.wide:
        for n in (50, 64, 32):
            probes_wide(n, args.graphs, args.reps)
        for tag, cost, kw in (("cost=\"ah\", ah_wide=True (AZD_ENGINE_DENSE_AH_WIDE)", "ah", dict(ah_wide=True)),
                              ("InvariantCost AH recipe, inv_wide=True", cost_of(R.recipe_ah(50)), dict(inv_wide=True)),
                              ("InvariantCost INT recipe, inv_wide=True", cost_of(R.recipe_int(50)), dict(inv_wide=True))):
            rate, form = loop_rate(cost, args.agents, args.epochs, args.episodes, n=50, **kw)
            print("loop  n=50 agents=%d episodes=%d fp32 256-128, one call per launch  %-48s %8.3f M expansions/s  form %s"
                  % (args.agents, args.episodes, tag, rate / 1e6, form[0]), flush=True)
        return
    rng = np.random.default_rng(31)
    probes([A.gnp_connected(rng, N, P) for _ in range(args.graphs)], args.reps)
    for tag, cost in (("cost=\"ah\" (AZD_ENGINE_DENSE_AH)", "ah"), ("InvariantCost AH recipe", cost_of(R.recipe_ah(N))),
                      ("InvariantCost INT recipe", cost_of(R.recipe_int(N)))):
        rate, form = loop_rate(cost, args.agents, args.epochs, args.episodes)
        print("loop  n=%d agents=%d episodes=%d fp32 256-128, one call per launch  %-34s %8.3f M expansions/s  form %s" % (N, args.agents, args.episodes, tag, rate / 1e6, form[0]))


if __name__ == "__main__":
    main()
