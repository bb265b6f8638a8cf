#!/usr/bin/env python3
"""Measurements of the dense-graph space with the Aouchiche-Hansen cost (profiles/r08_dense_ah.txt) on one MI355X.

    python tools/bench_dense_ah.py [--epochs 3] [--episodes 200] [--agents 512 4096] [--reps 20] [--wide]

  * expansions/s of an AH engine at N = 31 with the model 1396-256-128-930 over whole epochs (par_roll_out_episodes x episodes,
    par_update_model, par_reset_trees with the device root policy; the first epoch is warm-up and not counted), per population and
    per storage: bf16 runs the pool step, fp32 one launch per phase (the dense pool step serves gathered bf16 rows only);
  * beside it the same shape with cost="c21", for scale;
  * microseconds per AH cost from the probe (azd_debug_probe_ah_cost with `reps` repetitions per wave), per n.
--wide (profiles/r11_dense_ah_wide.txt): the cost's 64-row form -- the probe at n = 32 in both kernels and at n = 50 and 64 in
the wide one, the pool plan per key width, and the engines at N = 50 (BASELINE configs[4]'s shape) with ah_wide=True beside
cost="c21", bf16 storage.
One line per figure; nothing here asserts."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import azdopt_amd as az  # noqa: E402
from azdopt_amd import _lib  # noqa: E402

N, P, TOL = 31, 0.4, ([200, 50, 50], 25)


def epochs_rate(cost, agents, dtype, epochs, episodes, seed=0, n=N, wide=False):
    space = az.DenseGraphSpace(n, P, max_slots=128, cost=cost, ah_wide=wide and cost == "ah")
    model = az.ActionModel(agents, space.STATE_DIM, space.ACTION_DIM, hidden=(256, 128), seed=seed, dtype=dtype)
    kmin, kmax = space.default_permitted_range()
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(seed, agents, kmin=kmin, kmax=kmax), model, agents,
                                    **az.tree_capacities(episodes, kmax))
    rates = []
    for epoch in range(epochs + 1):
        e0 = opt.counters()["EXPANSIONS"]
        t0 = time.perf_counter()
        opt.par_roll_out_episodes(TOL, n_calls=episodes)
        opt.par_update_model(200)
        opt.par_reset_trees_policy(seed, epoch, kmin, kmax)
        opt.counters()  # (a read-back: the epoch's work is through)
        dt = time.perf_counter() - t0
        if epoch:
            rates.append((opt.counters()["EXPANSIONS"] - e0) / dt)
    form, why = opt.step_form()
    best = opt.argmin_data()
    print("n=%d cost=%-3s%s agents=%5d %-4s form=%-14s expansions/s median %.3f M (min %.3f, max %.3f; %d epochs of %d calls)  best eval %.6f%s"
          % (n, cost, " wide" if wide and cost == "ah" else "", agents, dtype, form, np.median(rates) / 1e6, min(rates) / 1e6, max(rates) / 1e6, epochs, episodes, best.eval,
             ("  [" + why + "]") if why else ""), flush=True)


def probe(n, count, reps, seed=0, wide=False):
    rng = np.random.default_rng(seed)
    graphs = []
    while len(graphs) < count:
        adj = [0] * n
        for v in range(1, n):
            for u in range(v):
                if rng.random() < P:
                    adj[v] |= 1 << u
                    adj[u] |= 1 << v
        seen = frontier = 1
        while frontier:
            nxt = 0
            for w in range(n):
                if (frontier >> w) & 1:
                    nxt |= adj[w]
            frontier = nxt & ~seen
            seen |= nxt
        if seen == (1 << n) - 1:
            graphs.append(adj)
    a = np.array(graphs, dtype=np.uint64)
    out = (_lib.DenseAhCost * count)()
    ms = C.c_float(0)
    fn = az.lib().azd_debug_probe_ah_cost_wide if wide else az.lib().azd_debug_probe_ah_cost
    _lib.check(fn(0, _lib.ptr(a), n, count, reps, out, C.byref(ms)), "probe_ah_cost")
    # `count` waves run at once (one per workgroup): the time of one wave's `reps` costs, all waves in flight
    print("probe%s n=%2d: %d graphs x %d reps in %.3f ms -> %.2f us per cost per wave (%.1f M costs/s over the device)"
          % (" (64-row kernel)" if wide else " (32-row kernel)", n, count, reps, ms.value, 1e3 * ms.value / reps, count * reps / ms.value / 1e3), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--agents", type=int, nargs="*", default=[512, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-epochs", action="store_true")
    ap.add_argument("--wide", action="store_true")
    args = ap.parse_args()
    if args.wide:
        probe(32, 2048, args.reps)
        for n in (32, 50, 64):
            probe(n, 2048, args.reps, wide=True)
        for ms in (128, 256, 640):  # key widths 2, 4, 10
            cfg = _lib.EngineConfig(_lib.SPACE_DENSE, 50, 512, 0, 0, 0, 0, 0, _lib.ENGINE_DENSE_AH | _lib.ENGINE_DENSE_AH_WIDE)
            cfg.max_slots, cfg.dense_p = ms, P
            waves, lds = C.c_int(0), C.c_size_t(0)
            _lib.check(az.lib().azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)), "ext_pool_plan")
            print("pool plan n=50 max_slots=%d: %d waves per searcher workgroup, %d bytes of LDS" % (ms, waves.value, lds.value), flush=True)
        if args.no_epochs:
            return
        for agents in args.agents:
            for cost in ("ah", "c21"):
                epochs_rate(cost, agents, "bf16", args.epochs, args.episodes, n=50, wide=True)
        return
    for n in (8, 16, 24, 31, 32):
        probe(n, 2048, args.reps)
    if args.no_epochs:
        return
    for agents in args.agents:
        for dtype in ("bf16", "f32"):
            for cost in ("ah", "c21"):
                epochs_rate(cost, agents, dtype, args.epochs, args.episodes)


if __name__ == "__main__":
    main()
