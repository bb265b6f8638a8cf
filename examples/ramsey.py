#!/usr/bin/env python3
"""The reference's Ramsey drivers (graph-state/examples/01-r333.rs, 02-r44.rs, 03-r3333.rs, 05-r45.rs) over the MI355X engine.

    python examples/ramsey.py r333|r44|r3333|r45|r46 [--epochs 250] [--episodes N] [--batch B]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import azdopt_amd as az  # noqa: E402
from azdopt_amd import sinks  # noqa: E402

DRIVERS = {  # N, SIZES, BATCH, episodes, n_as_tol, num_permitted_edges_range.start
    "r333": dict(n=16, sizes=[3, 3, 3], batch=256, episodes=6400, kmin=10,
                 tol=([200, 200, 200, 100, 100, 100, 50, 50, 50, 25, 25, 25], 10), tag="01-r333-grad"),   # 01-r333.rs:35-38,61,83,126-130
    "r44": dict(n=17, sizes=[4, 4], batch=512, episodes=3200, kmin=12,
                tol=([200, 200, 100, 100, 50, 50, 25, 25], 10), tag="01-r333-grad"),                      # 02-r44.rs:35-38,61,83,126-130
    # 05-r45.rs:35-46,58,61,83,101-103,129: N 24, [4, 5], every edge may be permitted (10..=E: a wide engine, max_slots = E),
    # weights [1, P_RED / P_BLUE] with P_RED = 0.4685, a ReLU head (:58), lr 3e-4.  Roots are coloured by
    # WeightedIndex([P_RED, P_BLUE]) (:84-90): generate_roots(color_weights=...) at the start, the root policy's color_weights for
    # the fresh roots of an epoch boundary.  modify_root keeps c == c_root_star (:201): rule="best".  The driver's roll-out takes a
    # decay (:134) this engine does not have: r44's tolerances stand in.
    "r45": dict(n=24, sizes=[4, 5], batch=128, episodes=3200, kmin=10, kmax="E", weights=[1.0, 0.4685 / (1.0 - 0.4685)], lr=3e-4,
                final_act=az._lib.ACT_RELU, rule="best", color_weights=[0.4685, 1.0 - 0.4685],
                tol=([200, 200, 100, 100, 50, 50, 25, 25], 10), tag="01-r333-grad"),
    # 03-r3333.rs:34-63,83-84,98,121-124: N 34, [3,3,3,3], unit weights, uniform root colours, 10..=30 permitted edges, a ReLU head
    # (:57), lr 3e-4, 800 episodes: the engine's 64-bit tier (64-bit neighbourhood words, as the driver's B64).  Its roll-out takes a
    # decay (:124) this engine does not have: r44's tolerances stand in, as for r45.  modify_root keeps c == c_root_star (:191):
    # rule="best".
    "r3333": dict(n=34, sizes=[3, 3, 3, 3], batch=512, episodes=800, kmin=10, kmax=30, lr=3e-4, final_act=az._lib.ACT_RELU, rule="best",
                  tol=([200, 200, 100, 100, 50, 50, 25, 25], 10), tag="01-r333-grad"),
    # BUILD-DEFINED: the reference has no R(4,6) driver (its space takes any clique sizes, its examples stop at K5).  N 35 -- the
    # open R(4,6) is in [36, 40] -- with [4, 6] on the 64-bit tier with big cliques (the size asks for it), and every
    # hyper-parameter of the r45 entry above; "every edge may be permitted" ends at what a node of that tier holds (512 actions).
    "r46": dict(n=35, sizes=[4, 6], batch=128, episodes=3200, kmin=10, kmax="E", weights=[1.0, 0.4685 / (1.0 - 0.4685)], lr=3e-4,
                final_act=az._lib.ACT_RELU, rule="best", color_weights=[0.4685, 1.0 - 0.4685],
                tol=([200, 200, 100, 100, 50, 50, 25, 25], 10), tag="01-r333-grad"),
}


def build_optimizer(driver, batch=0, episodes=0, hidden=(512, 1024, 512), seed=0, ext_pool_step=False):
    """the space, model and optimizer of a driver as its reference sets them up: (opt, model, kmin, kmax, episodes)"""
    d = DRIVERS[driver]
    batch = batch or d["batch"]
    episodes = episodes or d["episodes"]
    space = az.RamseySpaceNoEdgeRecolor(d["n"], d["sizes"], d.get("weights", [1.0] * len(d["sizes"])))
    model = az.ActionModel(batch, space.STATE_DIM, space.ACTION_DIM, hidden=list(hidden), lr=d.get("lr", 1e-4), l2=1e-6, seed=seed,
                           final_act=d.get("final_act", az._lib.ACT_SIGMOID), **(dict(dtype="bf16") if ext_pool_step else {}))
    kmin, kmax = d["kmin"], space.default_permitted_range()[1]   # ..=(E / 2), capped by what a node holds
    if d.get("kmax") == "E":
        kmax = min(space.E, space.MAX_SLOTS) if space.wide else space.E
    elif d.get("kmax"):
        kmax = d["kmax"]
    C = len(d["sizes"])
    caps = az.tree_capacities(episodes, kmax * (C - 1))  # (limits of the packed records: 65536 nodes, 65535 arcs, 2^20 predictions)
    roots = space.generate_roots(seed, batch, kmin=kmin, kmax=kmax, color_weights=d.get("color_weights"))
    opt = az.NablaOptimizer.par_new(space, roots, model, batch, **caps, **(dict(ext_pool_step=True) if ext_pool_step else {}))
    opt.set_root_policy(rule=d.get("rule", "threshold"), color_weights=d.get("color_weights"))  # r333 / r44: the engine's defaults
    return opt, model, kmin, kmax, episodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("driver", choices=sorted(DRIVERS))
    ap.add_argument("--epochs", type=int, default=250)
    ap.add_argument("--episodes", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--hidden", type=int, nargs="*", default=[512, 1024, 512])
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ext-pool-step", action="store_true",
                    help="r45 / r3333 / r46 with bf16 weight storage: the searcher-only pool step with the model's batched GEMMs beside it "
                         "(NablaOptimizer.par_new(..., ext_pool_step=True)); the default stays the engine's own choice of form")
    args = ap.parse_args()
    d = DRIVERS[args.driver]
    opt, model, kmin, kmax, episodes = build_optimizer(args.driver, args.batch, args.episodes, args.hidden, args.seed, args.ext_pool_step)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        writer = sinks.TensorboardWriter(open(os.path.join(args.out, "tfevents-losses"), "wb"))
        writer.write_file_version()
    else:
        writer = sinks.TensorboardWriter.create(d["tag"])

    def process_argmin(argmin, step):
        print("%s\tTotalCounts(%s)" % (argmin.eval, argmin.cost["clique_counts"]))
        writer.write_summary(None, step, sinks.clique_counts_summary(argmin.cost["clique_counts"]))
        writer.flush()
        if argmin.eval == 0:
            raise SystemExit("state is optimal:\n%s" % (argmin.state["colors"],))

    process_argmin(opt.argmin_data(), 0)
    for epoch in range(1, args.epochs + 1):
        print("==== EPOCH: %d ====" % epoch)
        done = 0
        if args.stride < episodes:  # the epoch's calls in one launch, handed out call by call (NablaOptimizer.run_ahead)
            opt.run_ahead(d["tol"], episodes)
        while done < episodes:
            k = min(args.stride, episodes - done)
            if opt.par_roll_out_episodes(d["tol"], n_calls=k):
                process_argmin(opt.argmin_data(), episodes * (epoch - 1) + done + k)
            done += k
        print("==== EPISODE: %d ====" % episodes)
        print("sizes:", sinks.sizes(opt.get_tree(0)))
        loss = opt.par_update_model(200)
        writer.write_summary(None, episodes * epoch, sinks.loss_summary(loss))
        writer.write_summary(None, episodes * epoch, sinks.clique_counts_summary(opt.argmin_data().cost["clique_counts"]))
        writer.flush()
        opt.par_reset_trees_policy(args.seed, epoch, kmin, kmax)


if __name__ == "__main__":
    main()
