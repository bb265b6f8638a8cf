#!/usr/bin/env python3
"""Expansions/s of wide Ramsey engines (azd_engine_config::max_slots > 0) in every step form, at the reference's R(4,5) shape
(05-r45.rs: N 24, [4, 5], 10..=E permitted edges, 512-1024-512 model; fp32 and bf16 weights) and at N = 32, C = 2.  Each form is
asked for with the engine's flags; the line says which form ran and, when another one did, why (azd_engine_step_form).
--preset u64: the 64-bit tier (AZD_ENGINE_RAMSEY_U64) at the reference's R(3,3,3,3) shape (03-r3333.rs: N 34, four colours, 10..=30
permitted edges, 512-1024-512 model with a ReLU head, 512 agents) and r45 under the flag beside r45 on the 32-bit tier (what the
wider word costs); and, by tag (--shapes r46 r37), the tier with clique sizes above 5 (AZD_ENGINE_RAMSEY_BIG_CLIQUES): r46 (N 35, [4, 6]) and
r37 (N 22, [3, 7]) at 512 agents.
The form 'ext' is the searcher-only pool step (par_new(..., ext_pool_step=True): bf16 storage only; with fp32 the line shows what ran
instead; 'ext_f32' is the same form with its fp32 evaluator, ext_pool_f32=True beside it: run it with --dtypes f32); its line ends with the busy shares of the evaluator's stream and of the searching waves (azd_engine_pool_utilisation).
--forms picks the forms to time (a library built before 'ext' existed, chosen with AZD_LIB, is timed with --forms per_call pool).

    python tools/time_ramsey_wide.py [--preset wide|u64] [--batch 256] [--calls 60] [--warmup 10] [--forms ext per_call] [--shapes r45]"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import azdopt_amd as az  # noqa: E402
from gpu_parity import TOL  # noqa: E402

FORMS = {"pool": dict(pool_step=True), "async": dict(async_step=True, pool_step=False),
         "barrier": dict(async_step=False, pool_step=False), "per_call": dict(persistent=False), "ext": dict(ext_pool_step=True),
         "ext_f32": dict(ext_pool_step=True, ext_pool_f32=True)}
SHAPES = [("r45", 24, [4, 5], [1.0, 0.4685 / 0.5315], "f32"), ("r45", 24, [4, 5], [1.0, 0.4685 / 0.5315], "bf16"),
          ("n32c2", 32, [4, 4], [1.0, 1.0], "f32")]
# (tag, n, sizes, weights, dtype, options: u64 = the tier, kmax, batch, relu head)
U64_SHAPES = [("r3333", 34, [3, 3, 3, 3], [1.0] * 4, "f32", dict(u64=True, kmax=30, batch=512, relu=True)),
              ("r3333", 34, [3, 3, 3, 3], [1.0] * 4, "bf16", dict(u64=True, kmax=30, batch=512, relu=True)),
              ("r45", 24, [4, 5], [1.0, 0.4685 / 0.5315], "bf16", dict(u64=False)),
              ("r45u64", 24, [4, 5], [1.0, 0.4685 / 0.5315], "bf16", dict(u64=True)),
              ("r45", 24, [4, 5], [1.0, 0.4685 / 0.5315], "f32", dict(u64=False, forms=["per_call"])),
              ("r45u64", 24, [4, 5], [1.0, 0.4685 / 0.5315], "f32", dict(u64=True, forms=["per_call"]))]
# the 64-bit tier with clique sizes above 5 (AZD_ENGINE_RAMSEY_BIG_CLIQUES): r46 = examples/ramsey.py's entry (N 35, [4, 6], r45's weights, as many
# permitted edges as a node of 512 actions holds), r37 = N 22, [3, 7]; 512 agents.  Run them by tag: --preset u64 --shapes r46 r37 r45u64 --batch 512
U64_SHAPES += [(tag, n, sizes, w, dtype, dict(batch=512, forms=["per_call"]))
               for tag, n, sizes, w in (("r46", 35, [4, 6], [1.0, 0.4685 / 0.5315]), ("r37", 22, [3, 7], [1.0, 1.0])) for dtype in ("f32", "bf16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", choices=["wide", "u64"], default="wide")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--hidden", type=int, nargs="*", default=[512, 1024, 512])
    ap.add_argument("--forms", nargs="*", default=list(FORMS), choices=list(FORMS))
    ap.add_argument("--shapes", nargs="*", default=None, help="tags of the preset's shapes to run (default: all)")
    ap.add_argument("--dtypes", nargs="*", default=["f32", "bf16"])
    args = ap.parse_args()
    B, calls = args.batch, args.calls
    print("# wide Ramsey engines (tools/time_ramsey_wide.py): batch %d, %d timed calls after %d, hidden %s; r45 = N 24, [4, 5], 10..=276 "
          "permitted edges; n32c2 = N 32, [4, 4], 10..=496; 'ran' = azd_engine_step_form's form, 'why' its reasons (each once)"
          % (B, calls, args.warmup, args.hidden))
    if args.preset == "u64":
        print("# --preset u64: r3333 = N 34, [3,3,3,3], 10..=30 permitted edges, ReLU head, batch 512, the 64-bit tier; r45u64 = r45 on the 64-bit "
              "tier (AZD_ENGINE_RAMSEY_U64) beside r45 on the 32-bit wide tier; r46 = N 35, [4, 6], 10..=512 permitted edges, r37 = N 22, [3, 7], "
              "10..=231, both with AZD_ENGINE_RAMSEY_BIG_CLIQUES (the size asks for it), batch 512")
    print("# shape  dtype  asked     ran       expansions/s  s/call     why")
    for tag, n, sizes, weights, dtype, *rest in (U64_SHAPES if args.preset == "u64" else SHAPES):
        o = rest[0] if rest else {}
        if (args.shapes and tag not in args.shapes) or dtype not in args.dtypes:
            continue
        B = o.get("batch", args.batch)
        space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, u64=o.get("u64"))
        kmax = o.get("kmax", min(space.E, space.MAX_SLOTS))  # (every edge, or as many as a node of the 64-bit tier holds)
        roots = space.generate_roots(0, B, kmin=10, kmax=kmax)
        for form, kw in FORMS.items():
            if form not in list(o.get("forms", FORMS)) + ["ext", "ext_f32"] or form not in args.forms:
                continue
            model = az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=args.hidden, seed=1, dtype=dtype,
                                   **(dict(final_act=az._lib.ACT_RELU) if o.get("relu") else {}))
            caps = az.tree_capacities(args.warmup + calls + 8, kmax * (space.C - 1))
            opt = az.NablaOptimizer.par_new(space, roots, model, B, **kw, **caps)
            opt.par_roll_out_episodes(TOL, n_calls=args.warmup)
            e0 = opt.counters()["EXPANSIONS"]
            t0 = time.perf_counter()
            opt.par_roll_out_episodes(TOL, n_calls=calls)
            dt = time.perf_counter() - t0
            exp = opt.counters()["EXPANSIONS"] - e0
            ran, why = opt.step_form()
            # (the engine's reason string names a plan's refusal once per form it fell through, run together: each once, "; " between)
            parts = [p.strip(" ;") for p in re.split(r"(?=(?:pool|asynchronous|barrier) step:|AZD_ENGINE_)", why) if p.strip(" ;")]
            why = "; ".join(dict.fromkeys(parts))
            if form in ("ext", "ext_f32") and ran == "pool":
                why = "evaluator stream busy %.2f, searcher waves busy %.2f; workgroups (evaluator, searcher) %s" % (*opt.pool_utilisation(), opt.pool_split())
            print("%-7s %-6s %-9s %-9s %12.0f  %.2e   %s" % (tag, dtype, form, ran, exp / dt, dt / calls, why), flush=True)
            del opt, model


if __name__ == "__main__":
    main()
