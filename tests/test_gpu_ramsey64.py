"""GPU parity of the 64-bit Ramsey tier (AZD_ENGINE_RAMSEY_U64: N <= 64 over 64-bit neighbourhood words, E*C <= 2304, keys of 36
words) bit for bit through the C ABI with the hash-stream model: exported trees, state vectors, live clique counts, agent state,
observations, the argmin through azd_engine_ramsey_argmin_any and the counters.
  * the R(4,5) shape (N = 24) under the flag against the C++ oracle and against a 32-bit wide engine on the same roots -- two checks
    of the 64-bit kernels that do not rest on the Python reference;
  * past 32 vertices against tests/ramsey64_ref.py (pinned on the CPU by tests/test_ramsey64_reference.py): the reference's
    R(3,3,3,3) shape (N = 34), N = 33 [3,4], N = 39 [3,3,4], N = 48 [4,5];
  * the step forms, the reference's own model (5049-512-1024-512-2244, ReLU head) in fp32 and bf16, the argmin call on the 32-bit
    tiers, the r3333 driver."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mlp_f64 as M
from gpu_parity import (MAIN_CTRS, R3333, R3333_DIMS, R45_W, TOL, CppRef, PyRef, assert_tree_equal, az, caps,  # noqa: F401
                        compare_ramsey, run_lockstep, same_array)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_parity(az, orc, ref, n, sizes, weights, B, kmin, kmax, steps, epochs, seed, n_obs_tol=4, check_every=10, sample=None, **kw):
    """run_wide_parity of tests/test_gpu_ramsey_wide.py for an engine of the 64-bit tier against `ref` (CppRef or PyRef)"""
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, u64=True)
    assert space.tier == "u64"
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
    colors, permitted = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
    co, mo = orc.gen_ramsey_roots(seed, 0, 0, B, n, len(sizes), kmin, kmax)
    assert np.array_equal(colors, co) and np.array_equal(permitted, mo)
    opt = az.NablaOptimizer.par_new(space, (colors, permitted), model, B, **kw, **caps(steps + 8, space, kmax))
    assert ref.KW == space.KEY_WORDS
    opt.taken = set()  # action ids on the agents' paths at the compared moments
    run_lockstep(opt, ref, (colors, permitted), orc, compare_ramsey(space, taken=opt.taken, argmin_any=True), seed=seed, tol=TOL,
                 steps=steps, epochs=epochs, kmin=kmin, kmax=kmax, n_obs_tol=n_obs_tol, check_every=check_every, sample=sample,
                 form="per_call")
    return opt, ref


def test_r45_under_the_flag_against_the_cpp_oracle(az, orc):
    """N 24, [4, 5], 48 agents, 10..=276 permitted edges, two epochs with the device root policy between them: the 64-bit kernels
    at a shape the C++ oracle takes"""
    opt, ref = run_parity(az, orc, CppRef(orc, 24, [4, 5], R45_W, 48), 24, [4, 5], R45_W, B=48, kmin=10, kmax=276, steps=30, epochs=2,
                          seed=4, sample=range(0, 48, 3))
    assert max(ref.tree(i).act_end[0] - ref.tree(i).act_begin[0] for i in range(48)) > 128  # nodes beyond two chunks


@pytest.mark.parametrize("n,sizes,weights,kmin,kmax", [(24, [4, 5], R45_W, 10, 276), (20, [3, 3, 3, 3], [1.0] * 4, 20, 170),
                                                      (32, [5, 3], [1.0, 1.0], 100, 496)])
def test_u64_engine_equals_the_32_bit_wide_engine_on_the_same_roots(az, n, sizes, weights, kmin, kmax):
    """the same roots through RamseyU64Space and RamseyWideSpace<10/16>: trees, rows, counts, counters, argmin, root policy"""
    B, seed = 32, 9
    runs = []
    for u64 in (True, False):
        space = az.RamseySpaceNoEdgeRecolor(n, sizes, weights, max_slots=kmax, u64=u64)
        assert space.tier == ("u64" if u64 else "wide")
        roots = space.generate_roots(seed, B, kmin=kmin, kmax=kmax)
        model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed)
        opt = az.NablaOptimizer.par_new(space, roots, model, B, persistent=False, **caps(70, space, kmax))
        opt.par_roll_out_episodes(TOL, n_calls=40)
        mid = opt.modify_roots(seed, 0, kmin, kmax)
        opt.par_reset_trees_policy(seed, 0, kmin, kmax)
        opt.par_roll_out_episodes(TOL, n_calls=20)
        runs.append((opt, mid))
    (a, ma), (b, mb) = runs
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    same_array(a.state_vecs(), b.state_vecs(), "state_vecs")
    ca, cb = a.counters(), b.counters()
    for k in MAIN_CTRS:
        assert ca[k] == cb[k], k
    for i in range(B):
        assert_tree_equal(a.get_tree(i), b.get_tree(i), f"agent {i}")
        assert np.array_equal(a.ramsey_agent_counts(i)[0], b.ramsey_agent_counts(i)[0])
        sa, sb = a.agent_state(i), b.agent_state(i)
        assert all(np.array_equal(sa[k], sb[k]) for k in ("parents", "permitted", "path", "state_pos")), i
    x, y = a.argmin_data(), b.argmin_data()
    pw = (a.space.E + 63) // 64
    assert x.eval.tobytes() == y.eval.tobytes() and np.array_equal(x.state["colors"], y.state["colors"])
    assert np.array_equal(x.state["permitted"][:pw], y.state["permitted"][:pw]) and x.cost == y.cost and (x.agent, x.node) == (y.agent, y.node)


def test_r3333_shape_against_the_reference(az, orc):
    """03-r3333.rs's shape: N 34, [3,3,3,3], permitted 10..=30, two epochs of 20 calls with the device root policy between them,
    16 agents, every agent compared after every 10 calls (the Python reference takes well under a minute for them)"""
    n, sizes, w = R3333
    run_parity(az, orc, PyRef(n, sizes, w, 16), n, sizes, w, B=16, kmin=10, kmax=30, steps=20, epochs=2, seed=3)


def test_n33_first_shape_past_the_32_bit_word(az, orc):
    """N = 33, [3, 4], up to 264 permitted edges: vertex 32 (edge positions 496..527) must take part in recoloured edges, so the
    case cannot pass on the low word of a neighbourhood alone"""
    opt, ref = run_parity(az, orc, PyRef(33, [3, 4], [1.0, 1.0], 12), 33, [3, 4], [1.0, 1.0], B=12, kmin=100, kmax=264, steps=20, epochs=2,
                          seed=5)
    E = 33 * 32 // 2
    hit = sum(1 for a in opt.taken if a % E >= 496)
    print("N = 33: %d of %d recoloured edges on the compared paths are at vertex 32" % (hit, len(opt.taken)))
    assert hit >= 4


@pytest.mark.parametrize("n,sizes,B,kmin,kmax,steps", [(39, [3, 3, 4], 8, 20, 120, 15), (48, [4, 5], 6, 40, 200, 12)])
def test_three_colours_at_n39_and_five_cliques_at_n48(az, orc, n, sizes, B, kmin, kmax, steps):
    """N = 39 at three colours (E*C = 2223) and N = 48 at [4, 5] (E*C = 2256: five-cliques over 64-bit words)"""
    run_parity(az, orc, PyRef(n, sizes, [1.0] * len(sizes), B), n, sizes, [1.0] * len(sizes), B=B, kmin=kmin, kmax=kmax, steps=steps,
               epochs=2, seed=6, check_every=5)


FORMS = {"per_call": dict(persistent=False), "async": dict(async_step=True, pool_step=False),
         "barrier": dict(async_step=False, pool_step=False), "pool": dict(pool_step=True), "default": dict()}


def test_every_step_form_at_r3333_runs_or_falls_back_with_a_reason(az):
    """the 64-bit tier runs the launch-per-phase form; every CU-resident form asked for falls back to it and says why (16 waves'
    clique counts alone are 144 KB of a CU's 160 at this shape) -- and what ran equals the launch-per-phase run array by array"""
    n, sizes, w = R3333
    B, seed = 32, 2
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, w)
    roots = space.generate_roots(seed, B, kmin=10, kmax=30)
    runs = {}
    for form, kw in FORMS.items():
        for hashed in (True, False):
            model = (az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed) if hashed else
                     az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=(64, 64), seed=seed))
            opt = az.NablaOptimizer.par_new(space, roots, model, B, **kw, **caps(30, space, 30))
            opt.par_roll_out_episodes(TOL, n_calls=20)
            ran, why = opt.step_form()
            print("r3333 step form: asked", form, "hash" if hashed else "mlp", "ran", ran, "--", why)
            assert ran.startswith("per_call"), (form, ran, why)
            if form != "per_call":  # (the 64-64 model's own reason comes first: 5049 inputs are no multiple of 4, no in-kernel evaluator)
                assert ("not built for the 64-bit Ramsey tier" in why) if hashed else ("cannot run inside the kernel" in why), (form, hashed, why)
            runs[(form, hashed)] = opt
    for hashed in (True, False):
        base = runs[("per_call", hashed)]
        for form in FORMS:
            o = runs[(form, hashed)]
            same_array(o.state_vecs(), base.state_vecs(), form)
            assert o.counters()["EXPANSIONS"] == base.counters()["EXPANSIONS"]
            for i in range(B):
                assert_tree_equal(o.get_tree(i), base.get_tree(i), f"{form} agent {i}")


def bf16_forward_bound(params, dims, x, act):
    """(f64 predictions, allowed |error| of the bf16-storage forward per output).  The device multiplies bf16(W) by bf16(a) in f32
    sums.  u_b = 2^-9 is bf16's relative half-ulp; a rounding's error is taken uniform within it (variance u_b^2 / 3 of the value)
    and independent from product to product, as tests/mlp_f64.py takes the f32 roundings: on top of its f32 terms
        var(z_l) += u_b^2 / 3 sum_k (W_lk a_k)^2 (1 + [a_k is not exact in bf16]) + var(a_{l-1}) W_l^2,
    the inputs of this space (0 / 1 and clique counts below 256) being exact.  Allowance: M.C_SIGMA standard deviations."""
    import torch
    ub2 = (2.0 ** -9) ** 2 / 3.0
    t, var = M._t(x), None
    layers = M.unpack(params, dims)
    for l, (W, b) in enumerate(layers):
        z = t @ W.T + b
        v = M._sum_var(dims[l] + 1, t.abs() @ W.abs().T + b.abs()) + ub2 * (1.0 if l == 0 else 2.0) * ((t * t) @ (W * W).T)
        if var is not None:
            v = v + var @ (W * W).T
        amb = z.abs() <= M.C_SIGMA * torch.sqrt(v)
        var = torch.where((z > 0) | amb, v, torch.zeros_like(v))
        t = torch.relu(z) if l < len(layers) - 1 else M.head(z, act)
    return t, M.C_SIGMA * torch.sqrt(v + (2 * M.U * t) ** 2)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_r3333_reference_model_trains_an_epoch(az, dtype):
    """03-r3333.rs's own model (5049-512-1024-512-2244, ReLU head; lr 3e-4, L2 1e-6) at its shape: an epoch of calls and the
    update run; the predictions of the last call and the gradient of the epoch's training rows are within tests/mlp_f64.py's bounds,
    which follow from the layer widths and these rows (clique counts up to 32 in 5049 inputs), not from a fixed tolerance.  bf16
    weight storage trains on the f32 master weights: its gradient is the fp32 one's bit for bit and is held to the same bounds;
    its predictions are held to bf16_forward_bound, the same derivation with bf16's rounding of weights and activations added.
    Measured on an MI355X at these seeds, error over allowance: forward 0.0066 (fp32), 0.82 (bf16); gradient 0.0088 (both)."""
    n, sizes, w = R3333
    B, seed, calls = 64, 7, 12
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, w)
    assert (space.STATE_DIM, space.ACTION_DIM) == (R3333_DIMS[0], R3333_DIMS[-1])
    model = az.ActionModel(B, R3333_DIMS[0], R3333_DIMS[-1], hidden=R3333_DIMS[1:-1], final_act=M.ACT_RELU, seed=seed, dtype=dtype,
                           lr=3e-4, l2=1e-6)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(seed, B, kmin=10, kmax=30), model, B, **caps(calls + 4, space, 30))
    opt.par_roll_out_episodes(TOL, n_calls=calls)
    assert opt.step_form()[0].startswith("per_call") and opt.counters()["FAILED"] == 0 and opt.counters()["EXPANSIONS"] > 0
    p0 = model.get_params()
    s, h = opt.state_vecs(), opt.predictions()
    fresh = [i for i in range(B) if opt.agent_state(i)["path"].any()]  # rows the last call evaluated
    assert s.max() < 256 and np.array_equal(s, np.round(s))  # (exact in bf16: bf16_forward_bound)
    p64, bound = (M.forward_bound if dtype == "f32" else bf16_forward_bound)(p0, R3333_DIMS, s[fresh], M.ACT_RELU)
    err = np.abs(h[fresh] - p64.numpy()) / bound.numpy().clip(min=1e-300)
    print("r3333 forward %s: max err/bound %.3g over %d rows, max |err| %.3g" % (dtype, err.max(), len(fresh), np.abs(h[fresh] - p64.numpy()).max()))
    assert err.max() <= 1.0, err.max()
    assert (h[fresh] > 0).any()
    sv, obs, wts = opt.observe(4)
    obs = np.nan_to_num(obs)  # (weight 0 there)
    assert wts.sum() > 0
    g, loss = model.debug_gradients(sv, obs, wts)
    ref = M.Reference(p0, R3333_DIMS, sv, obs, wts, M.ACT_RELU)
    rep = ref.check_gradients(g, loss, what="r3333 " + dtype)
    print("r3333 gradient %s: max err/(tol+A) %.3g" % (dtype, max(v[0] for k, v in rep.items() if k != "loss")))
    if dtype == "bf16":
        m32 = az.ActionModel(B, R3333_DIMS[0], R3333_DIMS[-1], hidden=R3333_DIMS[1:-1], final_act=M.ACT_RELU, seed=seed, lr=3e-4, l2=1e-6)
        assert np.array_equal(m32.get_params().view(np.uint32), p0.view(np.uint32))
        g32, loss32 = m32.debug_gradients(sv, obs, wts)
        assert np.array_equal(g32.view(np.uint32), g.view(np.uint32)) and loss32 == loss
    loss_u = opt.par_update_model(4)
    assert np.isfinite(loss_u) and not np.array_equal(model.get_params(), p0)
    opt.par_reset_trees_policy(seed, 0, 10, 30)
    opt.par_roll_out_episodes(TOL, n_calls=2)
    assert opt.counters()["FAILED"] == 0


def test_argmin_any_equals_the_fixed_size_calls_on_the_32_bit_tiers(az):
    """azd_engine_ramsey_argmin_any on a narrow (r44) and on a 32-bit wide (r45) engine == the existing calls; the wide call on an
    engine with E > 496 refuses and names the new one"""
    from azdopt_amd import _lib
    for n, sizes, rec_t, call in ((17, [4, 4], _lib.RamseyArgmin, "azd_engine_ramsey_argmin_data"),
                                  (24, [4, 5], _lib.RamseyWideArgmin, "azd_engine_ramsey_wide_argmin_data")):
        space = az.RamseySpaceNoEdgeRecolor(n, sizes)
        assert space.tier != "u64"
        B, seed = 32, 3
        opt = az.NablaOptimizer.par_new(space, space.generate_roots(seed, B), az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, seed), B)
        opt.par_roll_out_episodes(TOL, n_calls=30)
        rec = rec_t()
        assert getattr(opt._L, call)(opt._h, C.byref(rec)) == 0
        a = opt.ramsey_argmin_any()
        pw = (space.E + 63) // 64
        assert bytes(rec.colors[:space.E]) == a.colors.tobytes() and list(rec.permitted[:pw]) == a.permitted.tolist()
        assert list(rec.totals) == a.totals.tolist() and np.float32(rec.eval).tobytes() == np.float32(a.eval).tobytes()
        assert (rec.agent, rec.node) == (a.agent, a.node)
        short = np.zeros(space.E - 1, np.uint8)
        assert opt._L.azd_engine_ramsey_argmin_any(opt._h, _lib.ptr(short), space.E - 1, None, 0, None, None, None, None) == 1
    n, sizes, w = R3333
    space = az.RamseySpaceNoEdgeRecolor(n, sizes, w)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(1, 8, kmin=10, kmax=30), az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, 1), 8)
    wide = _lib.RamseyWideArgmin()
    assert opt._L.azd_engine_ramsey_wide_argmin_data(opt._h, C.byref(wide)) == 1
    assert "azd_engine_ramsey_argmin_any" in opt._L.azd_last_error().decode()


def test_r3333_driver_writes_the_reference_scalars(tmp_path):
    from azdopt_amd import sinks
    out = tmp_path / "ev"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ramsey.py"), "r3333", "--epochs", "1", "--episodes", "20", "--batch",
                        "16", "--hidden", "64", "--stride", "10", "--out", str(out)], cwd=tmp_path, check=True, timeout=600,
                       capture_output=True, text=True)
    assert "TotalCounts([" in r.stdout and "==== EPOCH: 1 ====" in r.stdout and "==== EPISODE: 20 ====" in r.stdout, r.stdout
    ev = sinks.read_events(out / "tfevents-losses")
    tags = [t for e in ev for t, _ in e[3]]
    assert tags.count("loss") == 1 and {"clique_counts/%d" % c for c in range(4)} <= set(tags)
