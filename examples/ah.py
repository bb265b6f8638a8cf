#!/usr/bin/env python3
"""What the reference's graph-state/examples/05-ah.rs set out to be (its driver is a todo!() stub; its objective,
ConnectedBitsetGraph::ah_cost, is live code), written as the live drivers' loop over the MI355X engine: a search for counterexamples
to the Aouchiche-Hansen conjecture on connected graphs with N = 31 vertices.

    python examples/ah.py [--epochs 250] [--episodes 800] [--batch 512] [--dtype f32|bf16] [--f32-form per_call|pool] [--n N --wide]

Roots are G(31, 0.4) redrawn until connected (05-ah.rs:93); the model is 1396-256-128-930 (the stub's widths under the live
ActionModel head).  The loop is par_roll_out_episodes x episodes, par_update_model, par_reset_trees with the device root policy.
A cost below 0 would be a counterexample: the run stops there.  (The complete graph's cost is 0 up to the eigen-solve's rounding,
a few 1e-16 either way, so "below 0" is taken as below -1e-4.)  With --dtype bf16 and 256 agents or more the engine runs its pool
step.  An fp32 model runs one launch per phase, or with --f32-form pool the pool step too (ext_pool_f32=True: the evaluator's gathered
fp32 GEMMs; same predictions bit for bit, so the printed lines and the event file are the same).  That option is off by default
because this loop asks for ONE call per launch, as the reference's drivers do, and a pool launch of one call pays its start-up 800
times an epoch: 0.49 M expansions/s against 0.57 M with one launch per phase on an MI355X at the default shape, where a whole epoch
in one launch (par_roll_out_episodes(n_calls=800), tools/bench_dense_ah.py) runs 2.6 M against 0.82 M
(profiles/r16_dense_ext_f32.txt).  --n N sets another number of vertices; beyond 32 it needs --wide, the cost's 64-row
form (AZD_ENGINE_DENSE_AH_WIDE, N <= 64), which is asked for by name and never chosen from N."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import azdopt_amd as az  # noqa: E402
from azdopt_amd import sinks  # noqa: E402

N, P = 31, 0.4                  # 05-ah.rs:30,93
TOL = ([200, 50, 50], 25)       # the live drivers' n_as_tol (04-c21-tree.rs:136-138)
COUNTEREXAMPLE_BELOW = -1e-4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=250)
    ap.add_argument("--episodes", type=int, default=800)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--hidden", type=int, nargs="*", default=[256, 128])
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--f32-form", choices=["per_call", "pool"], default="per_call",
                    help="--dtype f32: the pool step with its fp32 evaluator (ext_pool_f32=True), or one launch per phase")
    ap.add_argument("--max-slots", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=N, help="vertices (default 31, the reference's; more than 32 needs --wide)")
    ap.add_argument("--wide", action="store_true", help="the cost's 64-row form: n <= 64")
    args = ap.parse_args()

    space = az.DenseGraphSpace(args.n, P, max_slots=args.max_slots, cost="ah", ah_wide=args.wide)
    model = az.ActionModel(args.batch, space.STATE_DIM, space.ACTION_DIM, hidden=args.hidden, lr=1e-4, l2=1e-6, seed=args.seed,
                           dtype=args.dtype)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        writer = sinks.TensorboardWriter(open(os.path.join(args.out, "tfevents-losses"), "wb"))
        writer.write_file_version()
    else:
        writer = sinks.TensorboardWriter.create("05-ah")
    kmin, kmax = space.default_permitted_range()
    caps = az.tree_capacities(args.episodes, kmax)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(args.seed, args.batch, kmin=kmin, kmax=kmax), model, args.batch,
                                    ext_pool_f32=args.dtype == "f32" and args.f32_form == "pool", **caps)

    def process_argmin(argmin, step):
        c = argmin.cost
        print("%s\tAhCost { cost: %s, proximity: %s, eigenvalue: %s, diameter: %d, k: %d }"
              % (argmin.eval, c["cost"], c["proximity"], c["eigenvalue"], c["diameter"], c["k"]))
        writer.write_summary(None, step, sinks.ah_cost_summary(c))
        writer.flush()
        if c["cost"] < COUNTEREXAMPLE_BELOW:
            raise SystemExit("counterexample to the Aouchiche-Hansen conjecture (cost %s):\n%s" % (c["cost"], argmin.state["adj"]))

    process_argmin(opt.argmin_data(), 0)
    for epoch in range(1, args.epochs + 1):
        print("==== EPOCH: %d ====" % epoch)
        for done in range(1, args.episodes + 1):
            if opt.par_roll_out_episodes(TOL, n_calls=1):
                process_argmin(opt.argmin_data(), args.episodes * (epoch - 1) + done)
        print("==== EPISODE: %d ====" % args.episodes)
        print("sizes:", sinks.sizes(opt.get_tree(0)))
        loss = opt.par_update_model(200)
        writer.write_summary(None, args.episodes * epoch, sinks.loss_summary(loss))
        writer.write_summary(None, args.episodes * epoch, sinks.ah_cost_summary(opt.argmin_data().cost))
        writer.flush()
        opt.par_reset_trees_policy(args.seed, epoch, kmin, kmax)


if __name__ == "__main__":
    main()
