#!/usr/bin/env python3
"""examples/ah.py's loop with the objective taken from the command line: a search over connected graphs on N vertices for a graph
that minimises a linear combination of graph invariants -- the shape of an AutoGraphiX conjecture, "a combination of invariants is
bounded below by ..." -- on the MI355X engine's weighted-invariant cost (AZD_ENGINE_DENSE_INV, N <= 32; with --wide its 64-row
form, AZD_ENGINE_DENSE_INV_WIDE, N <= 64, which is asked for by name and never chosen from N; with --extended the extended
invariant cost, AZD_ENGINE_DENSE_INVX, N <= 32: sixteen invariants and products or quotients of two of them; with both flags that
cost's 64-row form, AZD_ENGINE_DENSE_INVX_WIDE, N <= 64; with --spectrum the spectrum invariant cost, AZD_ENGINE_DENSE_INVS, N <= 32:
twenty-one invariants, the graph energies and the adjacency spread among them; with --spectrum --wide that cost's 64-row form,
AZD_ENGINE_DENSE_INVS_WIDE, N <= 64).

    python examples/invariants.py --recipe '{"weights": {"remoteness": 1, "proximity": -1}, "eval_offset": 2, "eval_scale": 0.02}'
                                  [--n 31] [--extended | --spectrum] [--wide] [--epochs 250] [--episodes 800] [--batch 512] [--dtype f32|bf16]

--recipe is a JSON object: "weights" (name -> weight over edges, max_degree, min_degree, diameter, radius, proximity, remoteness,
avg_distance, adj_eig, dist_eig), and optionally "bias", "adj_index", "dist_index" (a descending index or "ah"), "eval_offset",
"eval_scale" (the evaluator is trained on eval = eval_scale * (cost + eval_offset): choose them so that evals lie in (0, 1)).
--recipe ah is the Aouchiche-Hansen cost as a recipe: the trees examples/ah.py grows, bit for bit.  A spectral invariant whose
weight is zero is not computed, so a recipe over the integer invariants and the transmissions alone runs no eigen-solve.
--extended: "weights" may also name lap_eig, slap_eig, randic, zagreb1, zagreb2, triangles; "lap_index" and "slap_index" are
descending indices into the Laplacian and signless-Laplacian spectra (n - 2 is the algebraic connectivity); "terms" is a list of up
to four [coef, "a", "*" or "/", "b"], e.g. [[1, "remoteness", "/", "radius"]] (a divisor is one of the first eight invariants, randic,
zagreb1 or zagreb2).  Without the flag the driver is what it was: the new names are unknown to it.
--spectrum: everything --extended takes, and "weights" and "terms" may also name adj_energy (the graph energy), dist_energy,
lap_energy, slap_energy and adj_spread, each a function of a matrix's whole spectrum, e.g.
'{"weights": {"adj_energy": 1}, "eval_scale": 0.01}'; all five may divide.  With --wide beside it: N <= 64 (neither form has a pool step).
The loop is par_roll_out_episodes x episodes, par_update_model, par_reset_trees with the device root policy; every improvement of
the argmin and every epoch print the argmin's invariants."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import azdopt_amd as az  # noqa: E402
from azdopt_amd import sinks  # noqa: E402

P = 0.4
TOL = ([200, 50, 50], 25)       # the live drivers' n_as_tol (04-c21-tree.rs:136-138)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recipe", required=True, help='a JSON object (see above), or "ah"')
    ap.add_argument("--n", type=int, default=31)
    ap.add_argument("--wide", action="store_true", help="the cost's 64-row form (N <= 64)")
    ap.add_argument("--extended", action="store_true", help="the extended invariant cost: sixteen invariants, pair terms (N <= 32; N <= 64 with --wide)")
    ap.add_argument("--spectrum", action="store_true", help="the spectrum invariant cost: twenty-one invariants, energies and spread (N <= 32; N <= 64 with --wide)")
    ap.add_argument("--epochs", type=int, default=250)
    ap.add_argument("--episodes", type=int, default=800)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--hidden", type=int, nargs="*", default=[256, 128])
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--max-slots", type=int, default=128)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    if args.spectrum and args.extended:
        ap.error("--spectrum and --extended exclude each other: the spectrum invariant cost takes --extended's recipes as they are")
    cost = az.InvariantCost.aouchiche_hansen(args.n) if args.recipe == "ah" else None
    if args.spectrum:
        cost = az.InvariantCostS.from_invariant_cost(cost) if cost is not None else az.InvariantCostS.from_dict(json.loads(args.recipe))
    elif args.extended:
        cost = az.InvariantCostX.from_invariant_cost(cost) if cost is not None else az.InvariantCostX.from_dict(json.loads(args.recipe))
    elif cost is None:
        cost = az.InvariantCost.from_dict(json.loads(args.recipe))
    wide = dict(invs_wide=True) if args.wide and args.spectrum else dict(invx_wide=True) if args.wide and args.extended else dict(inv_wide=args.wide)
    space = az.DenseGraphSpace(args.n, P, max_slots=args.max_slots, cost=cost, **wide)
    model = az.ActionModel(args.batch, space.STATE_DIM, space.ACTION_DIM, hidden=args.hidden, lr=1e-4, l2=1e-6, seed=args.seed,
                           dtype=args.dtype)
    kmin, kmax = space.default_permitted_range()
    caps = az.tree_capacities(args.episodes, kmax)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(args.seed, args.batch, kmin=kmin, kmax=kmax), model, args.batch, **caps)

    def show(argmin, tag):
        c = argmin.cost
        parts = ", ".join("%s: %s" % (name, c[name]) for i, name in enumerate(cost.NAMES) if (c["computed"] >> i) & 1)
        print("%s\t%s\t%s { cost: %s, %s, dist_k: %d }" % (tag, argmin.eval, type(cost).__name__, c["cost"], parts, c["dist_k"]))

    show(opt.argmin_data(), "argmin")
    for epoch in range(1, args.epochs + 1):
        print("==== EPOCH: %d ====" % epoch)
        for _ in range(args.episodes):
            if opt.par_roll_out_episodes(TOL, n_calls=1):
                show(opt.argmin_data(), "argmin")
        print("sizes:", sinks.sizes(opt.get_tree(0)))
        loss = opt.par_update_model(200)
        print("loss:", loss)
        show(opt.argmin_data(), "epoch %d" % epoch)
        opt.par_reset_trees_policy(args.seed, epoch, kmin, kmax)


if __name__ == "__main__":
    main()
