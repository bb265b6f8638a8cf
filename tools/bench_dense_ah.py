#!/usr/bin/env python3
"""Measurements of the dense-graph space with the Aouchiche-Hansen cost (profiles/r08_dense_ah.txt) on one MI355X.

    python tools/bench_dense_ah.py [--epochs 3] [--episodes 200] [--agents 512 4096] [--reps 20] [--wide]
                                   [--cost ah|c21] [--dtypes bf16 f32] [--f32-form per_call|pool|both] [--streams 1 2]

  * expansions/s of an AH engine at N = 31 with the model 1396-256-128-930 over whole epochs (par_roll_out_episodes x episodes,
    par_update_model, par_reset_trees with the device root policy; the first epoch is warm-up and not counted), per population and
    per storage: bf16 runs the pool step; fp32 runs what --f32-form names -- per_call: one launch per phase (an engine without
    AZD_ENGINE_EXT_POOL_F32), pool: the pool step with the gathered fp32 GEMMs (ext_pool_f32=True), both: one after the other;
    --streams: the evaluator streams of the fp32 pool arm (AZD_DENSE_POOL_STREAMS), one run per count; without it, and for bf16, the
    engine's default.
    A pool arm's line ends with the busy shares of the evaluator's stream and of the searcher waves (azd_engine_pool_utilisation);
  * beside it the same shape with cost="c21", for scale;
  * microseconds per AH cost from the probe (azd_debug_probe_ah_cost with `reps` repetitions per wave), per n.
--wide (profiles/r11_dense_ah_wide.txt): the cost's 64-row form -- the probe at n = 32 in both kernels and at n = 50 and 64 in
the wide one, the pool plan per key width, and the engines at N = 50 (BASELINE configs[4]'s shape) with ah_wide=True beside
cost="c21", bf16 storage; with --f32-form / --dtypes the AH-wide engine's arms alone (profiles/r16_dense_ext_f32.txt).
--cost c21 (profiles/r16_dense_ext_f32.txt): BASELINE configs[4]'s engine itself -- N = 50, G(50, 0.1), 512-512-512 -- with roots of
at most 128 and of at most 612 slots, the same arms; no probes.
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


def epochs_rate(cost, agents, dtype, epochs, episodes, seed=0, n=N, wide=False, f32_pool=False, streams=0, p=P, max_slots=128, hidden=(256, 128)):
    """f32_pool: ask the pool step for its fp32 evaluator (an fp32 model otherwise runs one launch per phase); streams: its evaluator
    streams (0: the engine's default)"""
    if streams:
        os.environ["AZD_DENSE_POOL_STREAMS"] = str(streams)
    else:
        os.environ.pop("AZD_DENSE_POOL_STREAMS", None)
    space = az.DenseGraphSpace(n, p, max_slots=max_slots, cost=cost, ah_wide=wide and cost == "ah")
    model = az.ActionModel(agents, space.STATE_DIM, space.ACTION_DIM, hidden=hidden, seed=seed, dtype=dtype)
    kmin, kmax = space.default_permitted_range()
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(seed, agents, kmin=kmin, kmax=kmax), model, agents,
                                    ext_pool_f32=f32_pool, **az.tree_capacities(episodes, kmax))
    rates, util = [], None
    for epoch in range(epochs + 1):
        e0 = opt.counters()["EXPANSIONS"]
        t0 = time.perf_counter()
        opt.par_roll_out_episodes(TOL, n_calls=episodes)
        if opt.step_form()[0] == "pool":
            util = opt.pool_utilisation()
        opt.par_update_model(200)
        opt.par_reset_trees_policy(seed, epoch, kmin, kmax)
        opt.counters()  # (a read-back: the epoch's work is through)
        dt = time.perf_counter() - t0
        if epoch:
            rates.append((opt.counters()["EXPANSIONS"] - e0) / dt)
    form, why = opt.step_form()
    best = opt.argmin_data()
    print("n=%d cost=%-3s%s slots<=%d %s agents=%5d %-4s form=%-14s%s expansions/s median %.3f M (min %.3f, max %.3f; %d epochs of %d calls)  best eval %.6f%s%s"
          % (n, cost, " wide" if wide and cost == "ah" else "", max_slots, "-".join(str(h) for h in hidden), agents, dtype, form,
             (" streams=%s" % (streams or "default")) if form == "pool" else "", np.median(rates) / 1e6, min(rates) / 1e6, max(rates) / 1e6, epochs,
             episodes, best.eval, ("  busy: evaluator stream %.2f, searcher waves %.2f" % util) if util and form == "pool" else "",
             ("  [" + why + "]") if why else ""), flush=True)
    os.environ.pop("AZD_DENSE_POOL_STREAMS", None)


def arms(dtypes, f32_form, streams):
    """(dtype, f32_pool, streams) of every run of one shape: bf16 on the pool step, fp32 in the forms asked for"""
    out = []
    for dtype in dtypes:
        forms = [False] if dtype == "bf16" else {"per_call": [False], "pool": [True], "both": [False, True]}[f32_form]
        for f32_pool in forms:
            out += [(dtype, f32_pool, s) for s in (streams if f32_pool and streams else [0])]  # (bf16 is there for scale: the default)
    return out


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
    ap.add_argument("--cost", choices=["ah", "c21"], default="ah", help="c21: config E's engine (N = 50, 512-512-512), roots of <= 128 and <= 612 slots")
    ap.add_argument("--dtypes", nargs="+", choices=["bf16", "f32"], default=None)
    ap.add_argument("--f32-form", choices=["per_call", "pool", "both"], default=None,
                    help="what an fp32 model runs: one launch per phase, or the pool step with its fp32 evaluator (ext_pool_f32=True)")
    ap.add_argument("--streams", type=int, nargs="*", default=[], help="evaluator streams of the fp32 pool arm (AZD_DENSE_POOL_STREAMS), one run per count")
    args = ap.parse_args()
    forms_asked = args.f32_form is not None or args.dtypes is not None
    runs = arms(args.dtypes or ["bf16", "f32"], args.f32_form or "per_call", args.streams)
    if args.cost == "c21":
        for agents in args.agents:
            for ms in (128, 612):
                for dtype, f32_pool, streams in runs:
                    epochs_rate("c21", agents, dtype, args.epochs, args.episodes, n=50, f32_pool=f32_pool, streams=streams, p=0.1, max_slots=ms,
                                hidden=(512, 512, 512))
        return
    if args.wide and forms_asked:
        for agents in args.agents:
            for dtype, f32_pool, streams in runs:
                epochs_rate("ah", agents, dtype, args.epochs, args.episodes, n=50, wide=True, f32_pool=f32_pool, streams=streams)
        return
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
    if not forms_asked:
        for n in (8, 16, 24, 31, 32):
            probe(n, 2048, args.reps)
    if args.no_epochs:
        return
    for agents in args.agents:
        for dtype, f32_pool, streams in runs:
            for cost in ("ah",) if forms_asked else ("ah", "c21"):
                epochs_rate(cost, agents, dtype, args.epochs, args.episodes, f32_pool=f32_pool, streams=streams)


if __name__ == "__main__":
    main()
