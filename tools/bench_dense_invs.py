#!/usr/bin/env python3
"""Measurements of the dense-graph space with the spectrum invariant cost (profiles/r22_dense_invs.txt) on one MI355X.

    python tools/bench_dense_invs.py [--reps 200] [--graphs 512] [--epochs 2] [--episodes 200] [--agents 512] [--no-loop]

  * the equivalence cost: microseconds per cost from the probe (azd_debug_probe_invs_cost, `reps` repetitions per wave) at n = 31 on
    G(31, 0.4) graphs under the recipes AH and INT of tests/dense_inv_ref.py, converted, beside azd_debug_probe_invx_cost under the
    same recipes on the same graphs in the same process, alternating (INVX, INVS, INVX, INVS, INVX); the largest difference among
    the INVX probe's three runs is the run-to-run spread;
  * the whole-spectrum finisher: the INVS probe under ENERGY, LAPE, SPREAD, ERATIO and ALLE of tests/dense_invs_ref.py beside the
    one-eigenvalue recipe ADJ (adjacency reduction + multisection) and ALL4 (four reductions + four multisections);
  * expansions/s of examples/invariants.py's loop -- one call per launch, the fp32 model 1396-256-128-930, par_update_model and the
    device root policy at the epoch boundary; the first epoch is warm-up and not counted -- at N = 31 for an AZD_ENGINE_DENSE_INVX
    engine under ADJ (twice: the difference is the run-to-run spread), an AZD_ENGINE_DENSE_INVS engine under ADJ and one under ENERGY.
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
import dense_invs_ref as R  # noqa: E402
import dense_invx_ref as X  # noqa: E402
from bench_dense_inv import loop_rate  # noqa: E402

N, P = 31, 0.4


def probes(graphs, reps):
    L = az.lib()
    a = np.array(graphs, dtype=np.uint64)
    ms = C.c_float(0)
    tag = "probe n=%d graphs=%d reps=%d  " % (N, len(graphs), reps)
    for rnd in range(2):  # the second round's figures are printed (the first loads the code objects)
        for name in ("AH", "INT"):
            rx, rs = X.c_recipe(X.RECIPES[name](N)), R.c_recipe(R.RECIPES[name](N))
            k = reps if name == "AH" else 20 * reps  # (the integer recipe runs no eigen-solve: twenty times the repetitions for a window of some length)
            invx, invs = [], []
            for run in range(5):  # alternating: INVX, INVS, INVX, INVS, INVX
                if run % 2 == 0:
                    dev = (_lib.DenseInvxCost * len(graphs))()
                    _lib.check(L.azd_debug_probe_invx_cost(0, _lib.ptr(a), N, len(graphs), k, C.byref(rx), dev, C.byref(ms)), "probe_invx_cost")
                    invx.append(ms.value)
                else:
                    devs = (_lib.DenseInvsCost * len(graphs))()
                    _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), N, len(graphs), k, C.byref(rs), devs, C.byref(ms)), "probe_invs_cost")
                    invs.append(ms.value)
            if rnd:
                print(tag + "azd_debug_probe_invx_cost %-6s x%-5d %s us/cost/wave  (spread %.3f %%)"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in invx), 100.0 * (max(invx) - min(invx)) / min(invx)))
                print(tag + "azd_debug_probe_invs_cost %-6s x%-5d %s us/cost/wave  mean %.4f x the INVX probe's mean"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in invs), np.mean(invs) / np.mean(invx)), flush=True)
        for name in ("ADJ", "ALL4") + R.NEW_RECIPES:
            rs = R.c_recipe(R.RECIPES[name](N))
            devs = (_lib.DenseInvsCost * len(graphs))()
            _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), N, len(graphs), reps, C.byref(rs), devs, C.byref(ms)), "probe_invs_cost")
            if rnd:
                print(tag + "azd_debug_probe_invs_cost %-6s %8.3f us/cost/wave" % (name, 1e3 * ms.value / reps), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
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
    adj_x, adj_s, energy = X.RECIPES["ADJ"](N), R.RECIPES["ADJ"](N), R.RECIPES["ENERGY"](N)
    for tag, cost in (("InvariantCostX ADJ recipe (AZD_ENGINE_DENSE_INVX)", az.InvariantCostX(adj_x.weights(), **adj_x.kwargs())),
                      ("InvariantCostX ADJ recipe (AZD_ENGINE_DENSE_INVX) (again)", az.InvariantCostX(adj_x.weights(), **adj_x.kwargs())),
                      ("InvariantCostS ADJ recipe (AZD_ENGINE_DENSE_INVS)", az.InvariantCostS(adj_s.weights(), **adj_s.kwargs())),
                      ("InvariantCostS ENERGY recipe (AZD_ENGINE_DENSE_INVS)", az.InvariantCostS(energy.weights(), **energy.kwargs()))):
        rate, form = loop_rate(cost, args.agents, args.epochs, args.episodes)
        print("loop  n=%d agents=%d episodes=%d fp32 256-128, one call per launch  %-58s %8.3f M expansions/s  form %s"
              % (N, args.agents, args.episodes, tag, rate / 1e6, form[0]), flush=True)


if __name__ == "__main__":
    main()
