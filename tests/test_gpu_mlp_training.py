"""The evaluator's training step against the float64 reference of tests/mlp_f64.py, with bounds derived from the f32
computation (see there): the gradient and loss of azd_debug_mlp_gradients -- the product's own launches up to the optimiser
step -- at the shapes, batches, heads and action weights the project trains with or where the kernels change path; Adam
replayed in f64 on the recorded device gradients; the forward of non-sigmoid heads on the f32, bf16 and in-kernel paths.

Adam divides a per-tensor gradient scale out, so a parameter comparison after the step cannot see one: the gradient itself is
compared here, per tensor, including its least-squares scale against the reference."""
import numpy as np
import pytest

import mlp_f64 as R
from test_gpu_bf16 import bf16_round
from gpu_parity import az  # noqa: F401

pytestmark = pytest.mark.gpu

SMALL = (304, 256, 256, 256, 152)
REF_SHAPE = (304, 512, 1024, 512, 152)     # 04-c21-tree.rs:33-54
CONFIG_E = (3676, 512, 512, 512, 2450)     # bench.py config E: ragged on every side of the 64 x 64 k_gemm tile
RAGGED = [(88, 48, 32, 44), (10, 24, 5), (13, 7, 33, 3)]   # the last: no width a multiple of 4 (scalar loads in k_gemm)
RAGGED_B = {(88, 48, 32, 44): 100, (10, 24, 5): 37, (13, 7, 33, 3): 70}
HEADS = {"none": R.ACT_NONE, "relu": R.ACT_RELU, "sigmoid": R.ACT_SIGMOID}
VISIBLE = dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-3, l2=1e-1)
REFERENCE = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, l2=1e-6)  # 04-c21-tree.rs:87-92
TOL_REF = ([200, 50, 50], 25)


def report(tag, ref, rep):
    worst = max(v[0] for k, v in rep.items() if k != "loss")
    scale = max(abs(v[1] - 1) for k, v in rep.items() if k != "loss")
    resid = max(v[2] / v[3] if v[3] else 0.0 for k, v in rep.items() if k != "loss")
    print("MLP-GRAD %s: max err/(tol+A) %.3g, max |scale-1| %.3g (allowed %.0e), max residual/bound %.3g, loss err/tol %.3g, "
          "ambiguous ReLU units per layer %s" % (tag, worst, scale, R.SCALE_TOL, resid, rep.get("loss", 0.0), ref.ambiguous))


def gradient_case(az, dims, B, act=R.ACT_SIGMOID, wkind="sparse", seed=1, dtype="f32", model_batch=None):
    m = az.ActionModel(model_batch or B, dims[0], dims[-1], hidden=dims[1:-1], final_act=act, seed=seed, dtype=dtype, **REFERENCE)
    rng = np.random.default_rng(seed + B)
    x, obs, w = R.batch(dims, B, rng, wkind)
    p0 = m.get_params()
    g, loss = m.debug_gradients(x, obs, w)
    assert np.array_equal(m.get_params().view(np.uint32), p0.view(np.uint32))  # the read-out leaves the parameters alone
    ref = R.Reference(p0, dims, x, obs, w, act)
    tag = "%s B=%d act=%d w=%s %s" % ("-".join(map(str, dims)), B, act, wkind, dtype)
    report(tag, ref, ref.check_gradients(g, loss, what=tag))
    return m, g, loss, (x, obs, w)


@pytest.mark.parametrize("B", [1, 63, 513, 4096, 32768, 65536])
def test_gradient_small_model_over_batches(az, B):
    """below one tile, one batch-split part and two, the shards' gathered batches of configs D (32768) and C (65536) where the
    weight gradient's split reaches its cap of 64 parts (1024 rows each)"""
    gradient_case(az, SMALL, B)


def test_gradient_reference_shape(az):
    gradient_case(az, REF_SHAPE, 512)


@pytest.mark.parametrize("name", ["r333", "r44"])
def test_gradient_ramsey_models(az, name):
    space = az.RamseySpaceNoEdgeRecolor(16, [3, 3, 3]) if name == "r333" else az.RamseySpaceNoEdgeRecolor(17, [4, 4])
    gradient_case(az, (space.STATE_DIM, 256, 256, 256, space.ACTION_DIM), 2048)


def test_gradient_config_e_and_bf16_storage_trains_on_the_master_weights(az):
    _, g32, l32, _ = gradient_case(az, CONFIG_E, 1024, seed=2)
    _, g16, l16, _ = gradient_case(az, CONFIG_E, 1024, seed=2, dtype="bf16")
    assert np.array_equal(g32.view(np.uint32), g16.view(np.uint32)) and l32 == l16


@pytest.mark.parametrize("head", sorted(HEADS))
@pytest.mark.parametrize("dims", RAGGED + [SMALL])
def test_gradient_ragged_widths_and_heads(az, dims, head):
    gradient_case(az, dims, RAGGED_B.get(dims, 130), act=HEADS[head])


@pytest.mark.parametrize("wkind", ["sparse", "dense", "single", "zero_row"])
@pytest.mark.parametrize("dims,B", [(SMALL, 513), ((13, 7, 33, 3), 70)])
def test_gradient_action_weights(az, dims, B, wkind):
    gradient_case(az, dims, B, wkind=wkind)


def test_gradient_after_the_batch_grows(az):
    """created for 64 rows, trained on 1300: ensure_batch reallocates the activation and delta buffers"""
    gradient_case(az, SMALL, 1300, model_batch=64)
    gradient_case(az, (13, 7, 33, 3), 1300, act=R.ACT_RELU, model_batch=64)


@pytest.mark.parametrize("cfg", ["visible", "reference"])
@pytest.mark.parametrize("dims,B,act", [(SMALL, 513, R.ACT_SIGMOID), ((13, 7, 33, 3), 70, R.ACT_RELU)])
def test_adam_against_the_f64_replay(az, dims, B, act, cfg):
    """three steps of update_model, each after a debug_gradients on the same rows (the update recomputes the same gradient:
    test_mlp_update_is_deterministic); the f64 Adam on the recorded gradients, from zero moments, gives the parameters"""
    c = VISIBLE if cfg == "visible" else REFERENCE
    m = az.ActionModel(B, dims[0], dims[-1], hidden=dims[1:-1], final_act=act, seed=4, **c)
    rng = np.random.default_rng(4)
    p0 = m.get_params()
    grads, params = [], []
    for t in range(3):
        x, obs, w = R.batch(dims, B, rng)
        g, loss = m.debug_gradients(x, obs, w)
        assert m.update_model(x, obs, w) == loss
        grads.append(g)
        params.append(m.get_params())
    steps = R.adam_replay(p0, grads, **c)
    worst = [R.check_adam(p, *s, what=(cfg, t)) for t, (p, s) in enumerate(zip(params, steps), 1)]
    print("MLP-ADAM %s %s: max err/bound per step %s" % (cfg, "-".join(map(str, dims)), ["%.3g" % v for v in worst]))
    # the step is not hidden inside the bound: the parameters moved by many bounds
    assert np.max(np.abs(params[-1] - p0)) > 100 * np.max(steps[-1][1])


def bf16_forward(params, dims, x, act):
    """test_gpu_bf16.reference_forward with the head as a parameter: bf16(x) . bf16(W)^T in f64, + b in f32, hidden
    activations rounded to bf16 by the next layer's input rounding"""
    off, t = 0, np.asarray(x, np.float32)
    for l in range(len(dims) - 1):
        W = params[off:off + dims[l] * dims[l + 1]].reshape(dims[l + 1], dims[l]); off += W.size
        b = params[off:off + dims[l + 1]]; off += b.size
        t = (bf16_round(t).astype(np.float64) @ bf16_round(W).astype(np.float64).T + b).astype(np.float32)
        if l < len(dims) - 2 or act == R.ACT_RELU:
            t = np.maximum(t, 0)
        elif act == R.ACT_SIGMOID:
            t = (1.0 / (1.0 + np.exp(-t.astype(np.float64)))).astype(np.float32)
    return t


@pytest.mark.parametrize("head", sorted(HEADS))
@pytest.mark.parametrize("dims,B", [(SMALL, 300), ((13, 7, 33, 3), 70), ((88, 48, 32, 44), 100)])
def test_forward_heads(az, dims, B, head):
    act = HEADS[head]
    rng = np.random.default_rng(5)
    x = (rng.random((B, dims[0])) < 0.3).astype(np.float32)
    m = az.ActionModel(B, dims[0], dims[-1], hidden=dims[1:-1], final_act=act, seed=6)
    y = np.zeros((B, dims[-1]), np.float32)
    m.write_predictions(x, y)
    p64, bound = R.forward_bound(m.get_params(), dims, x, act)
    err = np.abs(y - p64.numpy()) / bound.numpy().clip(min=1e-300)
    assert err.max() <= 1.0, (head, err.max())
    if act == R.ACT_RELU:
        assert (y == 0).any() and (y > 0).any()
    # the bf16 storage path (the LDS-DMA GEMM where its shapes allow, else the bf16 MFMA GEMM)
    m16 = az.ActionModel(B, dims[0], dims[-1], hidden=dims[1:-1], final_act=act, seed=6, dtype="bf16")
    y16 = np.zeros_like(y)
    m16.write_predictions(x, y16)
    assert np.max(np.abs(y16 - bf16_forward(m16.get_params(), dims, x, act))) < 1e-3
    print("MLP-FWD %s %s: max err/bound %.3g" % ("-".join(map(str, dims)), head, err.max()))


@pytest.mark.parametrize("form", ["pool", "async", "per_phase"])
def test_in_kernel_evaluators_with_a_relu_head(az, form):
    """predictions() after one call of the c21 search (N = 19, 256 agents) with a ReLU head, in each step form, against the
    f64 forward of the state rows the call evaluated"""
    n, B, seed = 19, 256, 8
    space = az.ROTModifyParentsOnce(n)
    dims = (space.STATE_DIM, 256, 256, 256, space.ACTION_DIM)
    kw = {"pool": dict(pool_step=True), "async": dict(pool_step=False), "per_phase": dict(persistent=False)}[form]
    model = az.ActionModel(B, dims[0], dims[-1], hidden=dims[1:-1], final_act=R.ACT_RELU, seed=seed)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(seed, B), model, B, **kw)
    opt.par_roll_out_episodes(TOL_REF, n_calls=1)
    assert opt.step_form()[0] == {"per_phase": "per_call"}.get(form, form), opt.step_form()
    if form != "per_phase":
        assert opt.counters()["EVAL_ROWS"] > 0  # the in-kernel evaluator ran
    s, h = opt.state_vecs(), opt.predictions()
    p64, bound = R.forward_bound(model.get_params(), dims, s, R.ACT_RELU)
    err = np.abs(h - p64.numpy()) / bound.numpy().clip(min=1e-300)
    assert err.max() <= 1.0, (form, err.max(), np.unravel_index(np.argmax(err), err.shape))
    assert (h == 0).any() and (h > 0).any()
