#!/usr/bin/env python3
"""Differential fuzz of the step forms on the GPU (tests/test_gpu_fuzz.py runs a 40-case slice; more cases: minutes of GPU time): random spaces, populations,
models, call counts and pool-step knobs; every case runs the same seeded search in two forms -- pool step (in one launch, in
random chunks, or call by call through a run-ahead window) against the asynchronous step for c21 / Ramsey, pool searchers
against the launch-per-phase form for the dense-graph space -- and compares trees, counters, argmin, improvement counts and state vectors.
Ramsey shapes whose STATE_DIM is no multiple of 4 (12 [3,4,3]: key width 4 at three colours; 14 [3,3,3,3]: four colours, E*C = 364;
20 [4,4]: the narrow tier's ceiling) take neither the pool step nor a model in the kernel: there the two forms are the asynchronous
step and the launch-per-phase form, both on the hash-stream model.
    python tools/fuzz_forms.py [cases 40] [seed 0] [dense_f32]
dense_f32 (run(..., dense_f32=True); tests/test_gpu_fuzz_dense_f32.py runs a 12-case slice): dense-graph cases only, on all three
tiers, with an fp32 model in the pool step (ext_pool_f32=True: the evaluator's gathered fp32 GEMMs) against the launch-per-phase
form; prediction bits are compared too, and a case whose pool step did not run fails.  Without it the cases drawn are what they were."""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import azdopt_amd as az  # noqa: E402
from gpu_parity import C21_CTRS, assert_tree_equal  # noqa: E402


KNOBS = {"AZD_POOL_EARLY_POST": ["0", "1", "2"], "AZD_POOL_EXPRESS_WGS": ["0", "8", "16"], "AZD_POOL_EVAL_WGS": ["24", "64", "100"],
         "AZD_POOL_READY_LANES": ["0", "1"], "AZD_DENSE_POOL_SEARCH_WGS": ["32", "96", "128"], "AZD_DENSE_POOL_ROUNDS": ["1", "4"],
         "AZD_DENSE_POOL_STREAMS": ["1", "2"]}
RAMSEY_SHAPES = [(16, [4, 4]), (17, [4, 4]), (16, [3, 3, 3]), (16, [3, 3, 3]), (12, [3, 4, 3]), (14, [3, 3, 3, 3]), (20, [4, 4])]


def run(cases=40, seed=0, dense_f32=False):
    saved = {k: os.environ.get(k) for k in list(KNOBS) + ["AZD_DENSE_NO_POOL"]}
    try:
        _run(cases, seed, dense_f32)
    finally:  # whatever happens, the process's environment is what it was
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(cases, seed, dense_f32=False):
    rng = random.Random(seed)

    def same(o1, i1, o2, i2, B, tag):
        assert i1 == i2, (tag, i1, i2)
        c1, c2 = o1.counters(), o2.counters()
        for k in C21_CTRS:
            assert c1[k] == c2[k], (tag, k, c1[k], c2[k])
        for t in rng.sample(range(B), min(B, 24)):
            assert_tree_equal(o1.get_tree(t), o2.get_tree(t), f"{tag} agent {t}")
        a1, a2 = o1.argmin_data(), o2.argmin_data()
        assert a1.eval == a2.eval and a1.agent == a2.agent and a1.node == a2.node, tag
        assert np.array_equal(o1.state_vecs(), o2.state_vecs()), tag
        if dense_f32:  # the gathered fp32 GEMMs' sums are forward's: every agent's current row, bit for bit
            assert np.array_equal(o1.predictions().view(np.uint32), o2.predictions().view(np.uint32)), tag

    for case in range(cases):
        kind = "dense" if dense_f32 else rng.choice(["c21", "c21", "ramsey", "dense", "dense"])
        seed = rng.randrange(1 << 30)
        env = {k: rng.choice(v) for k, v in KNOBS.items() if rng.random() < 0.4}
        calls = rng.choice([20, 60, 150, 400])
        hashed = False
        if kind == "c21":
            n = rng.choice([8, 13, 19, 22])
            B = rng.choice([256, 300, 1024, 3000])
            space = az.ROTModifyParentsOnce(n)
            hidden = rng.choice([(64, 64), (256, 256, 256), (128,)])
            dtype = rng.choice(["f32", "bf16"])
            tol = ([200, 50, 50], 25)
            kw = {}
        elif kind == "ramsey":
            B = rng.choice([256, 512, 2048])
            n, sizes = rng.choice(RAMSEY_SHAPES)
            space = az.RamseySpaceNoEdgeRecolor(n, sizes, [1.0] * len(sizes))
            hashed = space.STATE_DIM % 4 != 0  # (rows travel as 16-byte stores: no pool step, no model in the kernel)
            hidden = rng.choice([(64, 64), (256, 256)])
            dtype = rng.choice(["f32", "bf16"])
            tol = ([200, 200, 100, 100, 50, 50, 25, 25], 10)
            kw = dict(prediction_capacity=131072)
            calls = min(calls, 150)
        elif dense_f32:
            cost, wide = rng.choice([("c21", False), ("c21", False), ("ah", False), ("ah", True)])
            n = rng.choice([33, 40] if wide else [12, 20, 31] if cost == "ah" else [12, 20, 50])
            slots = rng.choice([128, 128, 256, 612])
            if cost == "ah":
                slots = min(slots, n * (n - 1) // 2)
            B = rng.choice([256, 300, 512])
            space = az.DenseGraphSpace(n, rng.choice([0.2, 0.4]), max_slots=slots, cost=cost, ah_wide=wide)
            hidden = rng.choice([(64,), (256, 128), (512, 512, 512)])
            dtype = "f32"
            tol = ([200, 50, 50], 25)
            kw = dict(prediction_capacity=262144)
            calls = rng.choice([20, 60, 100])
        else:
            n = rng.choice([12, 20, 50])
            slots = rng.choice([128, 128, 256, 612])
            B = rng.choice([256, 512, 1500])
            space = az.DenseGraphSpace(n, rng.choice([0.1, 0.3]), max_slots=slots)
            hidden = rng.choice([(64,), (512, 512, 512)])
            dtype = "bf16"
            tol = ([200, 50, 50], 25)
            kw = dict(prediction_capacity=262144)
            calls = min(calls, 150)
        lo, hi = space.default_permitted_range()
        kmin = rng.randint(lo, max(lo, hi // 2))
        roots = space.generate_roots(seed, B, kmin=kmin, kmax=hi)
        mode = rng.choice(["one", "chunks", "window"]) if kind != "dense" and not hashed else rng.choice(["one", "chunks"])
        tag = f"case {case}: {kind}{f' n={space.n} {space.sizes}' if kind == 'ramsey' else ''}{' ' + space.COST + (' wide' if space.AH_WIDE else '') + f' n={n} slots={slots}' if dense_f32 else ''} B={B} calls={calls} hidden={hidden} {dtype} mode={mode} env={env} seed={seed}"
        print(tag, flush=True)
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)

        def mk(**more):
            m = (az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed) if hashed else
                 az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=hidden, seed=seed, dtype=dtype))
            return az.NablaOptimizer.par_new(space, roots, m, B, **kw, **more)

        o1 = mk(pool_step=False) if hashed else mk(pool_step=True, **(dict(ext_pool_f32=True) if dense_f32 else {}))
        if mode == "one":
            i1 = o1.par_roll_out_episodes(tol, n_calls=calls)
        elif mode == "chunks":
            i1, left = 0, calls
            while left:
                k = min(left, rng.choice([1, 3, 17, 64]))
                i1 += o1.par_roll_out_episodes(tol, n_calls=k)
                left -= k
        else:
            if not o1.run_ahead(tol, calls):  # (the engine is not on the pool step: the calls run as they are asked for)
                print("   window refused")
            i1, left = 0, calls
            while left:
                k = min(left, rng.choice([1, 1, 2, 9]))
                i1 += o1.par_roll_out_episodes(tol, n_calls=k)
                if rng.random() < 0.1:
                    o1.argmin_data()
                left -= k
        assert not dense_f32 or o1.step_form() == ("pool", ""), (tag, o1.step_form())
        assert not hashed or o1.step_form() == ("async", ""), (tag, o1.step_form())
        if o1.step_form()[0] != "pool" and not hashed:  # (a width the in-kernel evaluator does not take: nothing to compare)
            print("   skipped:", o1.step_form())
            for k in KNOBS:  # (the case's knobs must not outlive it: they once leaked into the rest of the test session)
                os.environ.pop(k, None)
            continue
        for k in KNOBS:
            os.environ.pop(k, None)
        if kind == "dense":
            os.environ["AZD_DENSE_NO_POOL"] = "1"
            o2 = mk()
            i2 = o2.par_roll_out_episodes(tol, n_calls=calls)
            os.environ.pop("AZD_DENSE_NO_POOL")
            assert o2.step_form()[0].startswith("per_call"), o2.step_form()
        elif hashed:
            o2 = mk(persistent=False)
            i2 = o2.par_roll_out_episodes(tol, n_calls=calls)
            assert o2.step_form()[0].startswith("per_call"), o2.step_form()
        else:
            o2 = mk(pool_step=False)
            i2 = o2.par_roll_out_episodes(tol, n_calls=calls)
            assert o2.step_form()[0] == "async", o2.step_form()
        same(o1, i1, o2, i2, B, tag)
        # an epoch boundary on both, and a few more calls
        l1, l2 = o1.par_update_model(3), o2.par_update_model(3)
        assert l1 == l2 or (np.isnan(l1) and np.isnan(l2)), (tag, l1, l2)
        o1.par_reset_trees_policy(seed, 1, kmin, hi)
        o2.par_reset_trees_policy(seed, 1, kmin, hi)
        os.environ.update(env)
        j1 = o1.par_roll_out_episodes(tol, n_calls=15)
        for k in KNOBS:
            os.environ.pop(k, None)
        if kind == "dense":
            os.environ["AZD_DENSE_NO_POOL"] = "1"
        j2 = o2.par_roll_out_episodes(tol, n_calls=15)
        os.environ.pop("AZD_DENSE_NO_POOL", None)
        same(o1, j1, o2, j2, B, tag + " (second epoch)")
        del o1, o2
    print("all", cases, "cases agree")



if __name__ == "__main__":
    run(int(sys.argv[1]) if len(sys.argv) > 1 else 40, int(sys.argv[2]) if len(sys.argv) > 2 else 0, "dense_f32" in sys.argv[3:])
