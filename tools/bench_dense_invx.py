#!/usr/bin/env python3
"""Measurements of the dense-graph space with the extended invariant cost (profiles/r19_dense_invx.txt) on one MI355X.

    python tools/bench_dense_invx.py [--reps 100] [--graphs 512] [--epochs 2] [--episodes 200] [--agents 512] [--no-loop] [--wide]

  * microseconds per cost from the probe (azd_debug_probe_invx_cost, `reps` repetitions per wave) at n = 31 on G(31, 0.4) graphs
    under the recipes AH and INT of tests/dense_inv_ref.py, converted, beside azd_debug_probe_inv_cost under the same recipes on the
    same graphs in the same process, alternating (INV, INVX, INV, INVX, INV); the largest difference among the INV probe's three
    runs is the run-to-run spread;
  * the same under LAP, SLAP, ALL4, DEG and RATIO of tests/dense_invx_ref.py (no INV counterpart);
  * expansions/s of examples/invariants.py's loop -- one call per launch, the fp32 model 1396-256-128-930, par_update_model and the
    device root policy at the epoch boundary; the first epoch is warm-up and not counted -- at N = 31 for an AZD_ENGINE_DENSE_INV
    engine and an AZD_ENGINE_DENSE_INVX engine under the AH recipe, and an AZD_ENGINE_DENSE_INVX engine under LAP.
--wide (profiles/r21_dense_invx_wide.txt): the cost's 64-row form -- the wide probe (azd_debug_probe_invx_cost_wide) at n = 50 and
n = 64 on G(n, 0.4) graphs under AH and INT beside azd_debug_probe_inv_cost_wide under the same recipes, alternating as above; under
LAP, ALL4 and DEG alone; at n = 32 the wide probe beside the narrow one under ALL4; and the examples' loop at N = 50 for an
inv_wide=True engine under the AH recipe (twice: the difference is the run-to-run spread), an invx_wide=True engine under the AH
recipe, and one under LAP (algebraic connectivity).
One line per figure; nothing here asserts."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import azdopt_amd as az  # noqa: E402
from azdopt_amd import _lib  # noqa: E402
import dense_ah_ref as A  # noqa: E402
import dense_inv_ref as I  # noqa: E402
import dense_invx_ref as R  # noqa: E402
from bench_dense_inv import loop_rate  # noqa: E402

N, P = 31, 0.4


def cost_of(recipe):
    return az.InvariantCostX(recipe.weights(), **recipe.kwargs())


def probes(graphs, reps):
    L = az.lib()
    a = np.array(graphs, dtype=np.uint64)
    ms = C.c_float(0)
    tag = "probe n=%d graphs=%d reps=%d  " % (N, len(graphs), reps)
    for rnd in range(2):  # the second round's figures are printed (the first loads the code objects)
        for name in ("AH", "INT"):
            ri, rx = R.c_inv_recipe(I.RECIPES[name](N)), R.c_recipe(R.RECIPES[name](N))
            k = reps if name == "AH" else 20 * reps  # (the integer recipe runs no eigen-solve: twenty times the repetitions for a window of some length)
            inv, invx = [], []
            for run in range(5):  # alternating: INV, INVX, INV, INVX, INV
                if run % 2 == 0:
                    dev = (_lib.DenseInvCost * len(graphs))()
                    _lib.check(L.azd_debug_probe_inv_cost(0, _lib.ptr(a), N, len(graphs), k, C.byref(ri), dev, C.byref(ms)), "probe_inv_cost")
                    inv.append(ms.value)
                else:
                    devx = (_lib.DenseInvxCost * len(graphs))()
                    _lib.check(L.azd_debug_probe_invx_cost(0, _lib.ptr(a), N, len(graphs), k, C.byref(rx), devx, C.byref(ms)), "probe_invx_cost")
                    invx.append(ms.value)
            if rnd:
                print(tag + "azd_debug_probe_inv_cost  %-5s x%-5d %s us/cost/wave  (spread %.3f %%)"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in inv), 100.0 * (max(inv) - min(inv)) / min(inv)))
                print(tag + "azd_debug_probe_invx_cost %-5s x%-5d %s us/cost/wave  mean %.4f x the INV probe's mean"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in invx), np.mean(invx) / np.mean(inv)))
        for name in R.NEW_RECIPES:
            rx = R.c_recipe(R.RECIPES[name](N))
            devx = (_lib.DenseInvxCost * len(graphs))()
            _lib.check(L.azd_debug_probe_invx_cost(0, _lib.ptr(a), N, len(graphs), reps, C.byref(rx), devx, C.byref(ms)), "probe_invx_cost")
            if rnd:
                print(tag + "azd_debug_probe_invx_cost %-5s %8.3f us/cost/wave" % (name, 1e3 * ms.value / reps))


def probes_wide(n, count, reps):
    L = az.lib()
    rng = np.random.default_rng(n)
    a = np.array([A.gnp_connected(rng, n, P) for _ in range(count)], dtype=np.uint64)
    ms = C.c_float(0)
    tag = "probe n=%d graphs=%d reps=%d  " % (n, count, reps)
    for rnd in range(2):  # the second round's figures are printed (the first loads the code objects)
        for name in ("AH", "INT"):
            ri, rx = R.c_inv_recipe(I.RECIPES[name](n)), R.c_recipe(R.RECIPES[name](n))
            k = reps if name == "AH" else 20 * reps
            inv, invx = [], []
            for run in range(5):  # alternating: INV-wide, INVX-wide, INV-wide, INVX-wide, INV-wide
                if run % 2 == 0:
                    dev = (_lib.DenseInvCost * count)()
                    _lib.check(L.azd_debug_probe_inv_cost_wide(0, _lib.ptr(a), n, count, k, C.byref(ri), dev, C.byref(ms)), "probe_inv_cost_wide")
                    inv.append(ms.value)
                else:
                    devx = (_lib.DenseInvxCost * count)()
                    _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, count, k, C.byref(rx), devx, C.byref(ms)), "probe_invx_cost_wide")
                    invx.append(ms.value)
            if rnd:
                print(tag + "azd_debug_probe_inv_cost_wide  %-5s x%-5d %s us/cost/wave  (spread %.3f %%)"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in inv), 100.0 * (max(inv) - min(inv)) / min(inv)))
                print(tag + "azd_debug_probe_invx_cost_wide %-5s x%-5d %s us/cost/wave  mean %.4f x the INV-wide probe's mean"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in invx), np.mean(invx) / np.mean(inv)), flush=True)
        for name in ("LAP", "ALL4", "DEG"):
            rx = R.c_recipe(R.RECIPES[name](n))
            k = 20 * reps if name == "DEG" else reps  # (DEG runs no eigen-solve)
            devx = (_lib.DenseInvxCost * count)()
            _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, count, k, C.byref(rx), devx, C.byref(ms)), "probe_invx_cost_wide")
            if rnd:
                print(tag + "azd_debug_probe_invx_cost_wide %-5s x%-5d %8.3f us/cost/wave" % (name, k, 1e3 * ms.value / k), flush=True)
            if n <= 32 and name == "ALL4":
                _lib.check(L.azd_debug_probe_invx_cost(0, _lib.ptr(a), n, count, k, C.byref(rx), devx, C.byref(ms)), "probe_invx_cost")
                if rnd:
                    print(tag + "azd_debug_probe_invx_cost      %-5s x%-5d %8.3f us/cost/wave  (the 32-row kernel)" % (name, k, 1e3 * ms.value / k), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    if args.wide:
        for n in (50, 64, 32):
            probes_wide(n, args.graphs, args.reps)
        if args.no_loop:
            return
        ah = I.recipe_ah(50)
        inv_ah = az.InvariantCost(ah.weights(), **ah.kwargs())
        for tag, cost, kw in (("InvariantCost AH recipe, inv_wide=True", inv_ah, dict(inv_wide=True)),
                              ("InvariantCost AH recipe, inv_wide=True (again)", inv_ah, dict(inv_wide=True)),
                              ("InvariantCostX AH recipe, invx_wide=True", cost_of(R.RECIPES["AH"](50)), dict(invx_wide=True)),
                              ("InvariantCostX LAP recipe, invx_wide=True", cost_of(R.recipe_lap(50)), dict(invx_wide=True))):
            rate, form = loop_rate(cost, args.agents, args.epochs, args.episodes, n=50, **kw)
            print("loop  n=50 agents=%d episodes=%d fp32 256-128, one call per launch  %-50s %8.3f M expansions/s  form %s"
                  % (args.agents, args.episodes, tag, rate / 1e6, form[0]), flush=True)
        return
    rng = np.random.default_rng(31)
    probes([A.gnp_connected(rng, N, P) for _ in range(args.graphs)], args.reps)
    if args.no_loop:
        return
    ah = I.recipe_ah(N)
    for tag, cost in (("InvariantCost AH recipe (AZD_ENGINE_DENSE_INV)", az.InvariantCost(ah.weights(), **ah.kwargs())),
                      ("InvariantCostX AH recipe (AZD_ENGINE_DENSE_INVX)", cost_of(R.RECIPES["AH"](N))),
                      ("InvariantCostX LAP recipe (AZD_ENGINE_DENSE_INVX)", cost_of(R.recipe_lap(N)))):
        rate, form = loop_rate(cost, args.agents, args.epochs, args.episodes)
        print("loop  n=%d agents=%d episodes=%d fp32 256-128, one call per launch  %-50s %8.3f M expansions/s  form %s"
              % (N, args.agents, args.episodes, tag, rate / 1e6, form[0]), flush=True)


if __name__ == "__main__":
    main()
