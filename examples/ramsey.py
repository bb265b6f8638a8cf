#!/usr/bin/env python3
"""The reference's Ramsey drivers (graph-state/examples/01-r333.rs, 02-r44.rs, 03-r3333.rs, 05-r45.rs) over the MI355X engine.

    python examples/ramsey.py r333|r44|r3333|r45 [--epochs 250] [--episodes N] [--batch B]"""
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
    # 05-r45.rs:35-46,61,83,101-103,129: N 24, [4, 5], every edge may be permitted (10..=E: a wide engine, max_slots = E),
    # weights [1, P_RED / P_BLUE] with P_RED = 0.4685, lr 3e-4.  The seeded root generator draws colours uniformly: the driver's
    # P_RED colouring probability (WeightedIndex, :84-90) is NOT reproduced -- it would change the generator's spec, which the
    # oracle shares.  The driver's roll-out takes a decay (:134) this engine does not have: r44's tolerances stand in.
    "r45": dict(n=24, sizes=[4, 5], batch=128, episodes=3200, kmin=10, kmax="E", weights=[1.0, 0.4685 / (1.0 - 0.4685)], lr=3e-4,
                tol=([200, 200, 100, 100, 50, 50, 25, 25], 10), tag="01-r333-grad"),
    # 03-r3333.rs:34-63,83-84,98,121-124: N 34, [3,3,3,3], unit weights, uniform root colours, 10..=30 permitted edges, a ReLU head
    # (:57), lr 3e-4, 800 episodes: the engine's 64-bit tier (64-bit neighbourhood words, as the driver's B64).  Its roll-out takes a
    # decay (:124) this engine does not have: r44's tolerances stand in, as for r45.  The driver's modify_root keeps
    # c == c_root_star; the engine's root policy is 02-r44's threshold rule.
    "r3333": dict(n=34, sizes=[3, 3, 3, 3], batch=512, episodes=800, kmin=10, kmax=30, lr=3e-4, final_act=az._lib.ACT_RELU,
                  tol=([200, 200, 100, 100, 50, 50, 25, 25], 10), tag="01-r333-grad"),
}


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
                    help="r45 / r3333 with bf16 weight storage: the searcher-only pool step with the model's batched GEMMs beside it "
                         "(NablaOptimizer.par_new(..., ext_pool_step=True)); the default stays the engine's own choice of form")
    args = ap.parse_args()
    d = DRIVERS[args.driver]
    batch = args.batch or d["batch"]
    episodes = args.episodes or d["episodes"]

    space = az.RamseySpaceNoEdgeRecolor(d["n"], d["sizes"], d.get("weights", [1.0] * len(d["sizes"])))
    model = az.ActionModel(batch, space.STATE_DIM, space.ACTION_DIM, hidden=args.hidden, lr=d.get("lr", 1e-4), l2=1e-6, seed=args.seed,
                           final_act=d.get("final_act", az._lib.ACT_SIGMOID), **(dict(dtype="bf16") if args.ext_pool_step else {}))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        writer = sinks.TensorboardWriter(open(os.path.join(args.out, "tfevents-losses"), "wb"))
        writer.write_file_version()
    else:
        writer = sinks.TensorboardWriter.create(d["tag"])
    kmin, kmax = d["kmin"], space.default_permitted_range()[1]   # ..=(E / 2), capped by what a node holds
    if d.get("kmax") == "E":
        kmax = space.E
    elif d.get("kmax"):
        kmax = d["kmax"]
    C = len(d["sizes"])
    caps = az.tree_capacities(episodes, kmax * (C - 1))  # (limits of the packed records: 65536 nodes, 65535 arcs, 2^20 predictions)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(args.seed, batch, kmin=kmin, kmax=kmax), model, batch, **caps,
                                    **(dict(ext_pool_step=True) if args.ext_pool_step else {}))

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
