#!/usr/bin/env python3
"""Measurements of the dense-graph space with the spectrum invariant cost (profiles/r22_dense_invs.txt) on one MI355X.

    python tools/bench_dense_invs.py [--reps 200] [--graphs 512] [--epochs 2] [--episodes 200] [--agents 512] [--no-loop] [--wide] [--beside LIB]

  * the equivalence cost: microseconds per cost from the probe (azd_debug_probe_invs_cost, `reps` repetitions per wave) at n = 31 on
    G(31, 0.4) graphs under the recipes AH and INT of tests/dense_inv_ref.py, converted, beside azd_debug_probe_invx_cost under the
    same recipes on the same graphs in the same process, alternating (INVX, INVS, INVX, INVS, INVX); the largest difference among
    the INVX probe's three runs is the run-to-run spread;
  * the whole-spectrum finisher: the INVS probe under ENERGY, LAPE, SPREAD, ERATIO and ALLE of tests/dense_invs_ref.py beside the
    one-eigenvalue recipe ADJ (adjacency reduction + multisection) and ALL4 (four reductions + four multisections);
  * expansions/s of examples/invariants.py's loop -- one call per launch, the fp32 model 1396-256-128-930, par_update_model and the
    device root policy at the epoch boundary; the first epoch is warm-up and not counted -- at N = 31 for an AZD_ENGINE_DENSE_INVX
    engine under ADJ (twice: the difference is the run-to-run spread), an AZD_ENGINE_DENSE_INVS engine under ADJ and one under ENERGY.
--wide (profiles/r24_dense_invs_wide.txt): the cost's 64-row form -- the wide probe (azd_debug_probe_invs_cost_wide) at n = 50 and
n = 64 on G(n, 0.4) graphs under AH and INT beside azd_debug_probe_invx_cost_wide under the same recipes, alternating as above; under
ADJ, ALL4, ENERGY, LAPE, SPREAD, ERATIO and ALLE alone; and the examples' loop at N = 50 for an invx_wide=True engine under ADJ
(twice: the difference is the run-to-run spread), an invs_wide=True engine under ADJ and one under ENERGY.
--beside LIB: the narrow probe at n = 31 under AH, ENERGY and INT from this build's library beside the same probe from another build
of the library (a path to its libazdopt_amd.so), alternating in this process (other, this, other, this, other); nothing else runs.
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


def probes_wide(n, count, reps):
    L = az.lib()
    rng = np.random.default_rng(n)
    a = np.array([A.gnp_connected(rng, n, P) for _ in range(count)], dtype=np.uint64)
    ms = C.c_float(0)
    tag = "probe n=%d graphs=%d reps=%d  " % (n, count, reps)
    for rnd in range(2):  # the second round's figures are printed (the first loads the code objects)
        for name in ("AH", "INT"):
            rx, rs = X.c_recipe(X.RECIPES[name](n)), R.c_recipe(R.RECIPES[name](n))
            k = reps if name == "AH" else 20 * reps
            invx, invs = [], []
            for run in range(5):  # alternating: INVX-wide, INVS-wide, INVX-wide, INVS-wide, INVX-wide
                if run % 2 == 0:
                    dev = (_lib.DenseInvxCost * count)()
                    _lib.check(L.azd_debug_probe_invx_cost_wide(0, _lib.ptr(a), n, count, k, C.byref(rx), dev, C.byref(ms)), "probe_invx_cost_wide")
                    invx.append(ms.value)
                else:
                    devs = (_lib.DenseInvsCost * count)()
                    _lib.check(L.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), n, count, k, C.byref(rs), devs, C.byref(ms)), "probe_invs_cost_wide")
                    invs.append(ms.value)
            if rnd:
                print(tag + "azd_debug_probe_invx_cost_wide %-6s x%-5d %s us/cost/wave  (spread %.3f %%)"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in invx), 100.0 * (max(invx) - min(invx)) / min(invx)))
                print(tag + "azd_debug_probe_invs_cost_wide %-6s x%-5d %s us/cost/wave  mean %.4f x the INVX-wide probe's mean"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in invs), np.mean(invs) / np.mean(invx)), flush=True)
        for name in ("ADJ", "ALL4") + R.NEW_RECIPES:
            rs = R.c_recipe(R.RECIPES[name](n))
            devs = (_lib.DenseInvsCost * count)()
            _lib.check(L.azd_debug_probe_invs_cost_wide(0, _lib.ptr(a), n, count, reps, C.byref(rs), devs, C.byref(ms)), "probe_invs_cost_wide")
            if rnd:
                print(tag + "azd_debug_probe_invs_cost_wide %-6s %8.3f us/cost/wave" % (name, 1e3 * ms.value / reps), flush=True)


def probes_beside(path, graphs, reps):
    """the narrow probe of this build beside the same probe of the library at `path`"""
    mine, other = az.lib(), C.CDLL(path)
    sig = mine.azd_debug_probe_invs_cost
    other.azd_debug_probe_invs_cost.restype, other.azd_debug_probe_invs_cost.argtypes = sig.restype, sig.argtypes
    a = np.array(graphs, dtype=np.uint64)
    ms = C.c_float(0)
    tag = "probe n=%d graphs=%d reps=%d  " % (N, len(graphs), reps)
    for rnd in range(2):
        for name in ("AH", "ENERGY", "INT"):
            rs = R.c_recipe(R.RECIPES[name](N))
            k = 20 * reps if name == "INT" else reps
            t = {0: [], 1: []}
            out = {}
            for run in range(5):  # alternating: other, this, other, this, other
                L = mine if run % 2 else other
                devs = (_lib.DenseInvsCost * len(graphs))()
                _lib.check(L.azd_debug_probe_invs_cost(0, _lib.ptr(a), N, len(graphs), k, C.byref(rs), devs, C.byref(ms)), "probe_invs_cost")
                t[run % 2].append(ms.value)
                out[run % 2] = bytes(devs)
            if rnd:
                print(tag + "azd_debug_probe_invs_cost %-6s x%-5d other build %s us/cost/wave  (spread %.3f %%)"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in t[0]), 100.0 * (max(t[0]) - min(t[0])) / min(t[0])))
                print(tag + "azd_debug_probe_invs_cost %-6s x%-5d this build  %s us/cost/wave  mean %.4f x the other build's mean, records %s"
                      % (name, k, " ".join("%8.3f" % (1e3 * x / k) for x in t[1]), np.mean(t[1]) / np.mean(t[0]), "equal" if out[0] == out[1] else "DIFFER"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--agents", type=int, default=512)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--wide", action="store_true")
    ap.add_argument("--beside", metavar="LIB")
    args = ap.parse_args()
    if args.beside:
        rng = np.random.default_rng(31)
        probes_beside(args.beside, [A.gnp_connected(rng, N, P) for _ in range(args.graphs)], args.reps)
        return
    if args.wide:
        for n in (50, 64):
            probes_wide(n, args.graphs, args.reps)
        if args.no_loop:
            return
        adj_x, adj_s, energy = X.RECIPES["ADJ"](50), R.RECIPES["ADJ"](50), R.RECIPES["ENERGY"](50)
        for tag, cost, kw in (("InvariantCostX ADJ recipe, invx_wide=True", az.InvariantCostX(adj_x.weights(), **adj_x.kwargs()), dict(invx_wide=True)),
                              ("InvariantCostX ADJ recipe, invx_wide=True (again)", az.InvariantCostX(adj_x.weights(), **adj_x.kwargs()), dict(invx_wide=True)),
                              ("InvariantCostS ADJ recipe, invs_wide=True", az.InvariantCostS(adj_s.weights(), **adj_s.kwargs()), dict(invs_wide=True)),
                              ("InvariantCostS ENERGY recipe, invs_wide=True", az.InvariantCostS(energy.weights(), **energy.kwargs()), dict(invs_wide=True))):
            rate, form = loop_rate(cost, args.agents, args.epochs, args.episodes, n=50, **kw)
            print("loop  n=50 agents=%d episodes=%d fp32 256-128, one call per launch  %-52s %8.3f M expansions/s  form %s"
                  % (args.agents, args.episodes, tag, rate / 1e6, form[0]), flush=True)
        return
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
