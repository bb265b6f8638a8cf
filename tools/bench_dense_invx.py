#!/usr/bin/env python3
"""Measurements of the dense-graph space with the extended invariant cost (profiles/r19_dense_invx.txt) on one MI355X.

    python tools/bench_dense_invx.py [--reps 100] [--graphs 512] [--epochs 2] [--episodes 200] [--agents 512] [--no-loop]

  * microseconds per cost from the probe (azd_debug_probe_invx_cost, `reps` repetitions per wave) at n = 31 on G(31, 0.4) graphs
    under the recipes AH and INT of tests/dense_inv_ref.py, converted, beside azd_debug_probe_inv_cost under the same recipes on the
    same graphs in the same process, alternating (INV, INVX, INV, INVX, INV); the largest difference among the INV probe's three
    runs is the run-to-run spread;
  * the same under LAP, SLAP, ALL4, DEG and RATIO of tests/dense_invx_ref.py (no INV counterpart);
  * expansions/s of examples/invariants.py's loop -- one call per launch, the fp32 model 1396-256-128-930, par_update_model and the
    device root policy at the epoch boundary; the first epoch is warm-up and not counted -- at N = 31 for an AZD_ENGINE_DENSE_INV
    engine and an AZD_ENGINE_DENSE_INVX engine under the AH recipe, and an AZD_ENGINE_DENSE_INVX engine under LAP.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--no-loop", action="store_true")
    args = ap.parse_args()
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
