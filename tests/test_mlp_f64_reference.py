"""The float64 reference of the training step (tests/mlp_f64.py) and its derived bounds, on the CPU: a float32 restatement of
the device's step (mlp_kernels.hip: k_gemm forward, k_loss_delta, the batch-split weight and bias gradients, k_adam) passes
them at the shapes the GPU module checks, and each of a set of small mutations of that restatement fails them.  The last test
records which of those mutations the older check -- parameters after Adam within 0.05 lr -- lets through."""
import numpy as np
import pytest
import torch

import mlp_f64 as R

F32 = torch.float32
MUTATIONS = ("grad_scale_1e-3", "dp_without_2", "bias_doubled", "split_part_twice", "l2_sign", "eps_in_sqrt", "bc_swapped")
GRADIENT_MUTATIONS = MUTATIONS[:4]
VISIBLE = dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-3, l2=1e-1)   # every term of the Adam step visible
REFERENCE = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, l2=1e-6)  # 04-c21-tree.rs:87-92


def f32_gradients(params, dims, x, obs, w, act, mut=None):
    """(flat gradient, loss) in f32 the way the device computes them; `mut` names one mutation"""
    x, obs, w = (torch.as_tensor(np.asarray(t), dtype=F32) for t in (x, obs, w))
    P = torch.as_tensor(np.asarray(params), dtype=F32)
    layers = [(P[wo:bo].reshape(dims[l + 1], dims[l]), P[bo:bo + dims[l + 1]]) for l, (wo, bo) in enumerate(R.layout(dims))]
    a = [x]
    for l, (W, b) in enumerate(layers):
        z = a[-1] @ W.T + b
        a.append(torch.relu(z) if l < len(layers) - 1 else R.head(z, act))
    p = a.pop()
    ws = w.sum()
    wt = w / ws
    d = p - obs
    loss = (wt * d * d).sum()
    if mut in ("loss_half", "loss_double"):
        loss = loss * (0.5 if mut == "loss_half" else 2.0)
    dp = (wt * d) if mut == "dp_without_2" else (2.0 * wt * d)
    if act == R.ACT_SIGMOID:
        dp = dp * (p * (1.0 - p))
    elif act == R.ACT_RELU:
        dp = torch.where(p > 0, dp, torch.zeros_like(dp))
    B = x.shape[0]
    k, parts = R.batch_splits(B)
    g = torch.zeros(P.shape[0], dtype=F32)
    dz = dp
    for l in range(len(layers) - 1, -1, -1):
        wo, bo = R.layout(dims)[l]
        xin = a[l]
        dW = torch.zeros(dims[l + 1], dims[l], dtype=F32)
        db = torch.zeros(dims[l + 1], dtype=F32)
        for i in range(parts):   # the parts of the batch sum, added in order (k_sum_splits)
            dW = dW + dz[i * k:(i + 1) * k].T @ xin[i * k:(i + 1) * k]
            db = db + dz[i * k:(i + 1) * k].sum(0)
        if mut == "split_part_twice" and l == 0:
            dW = dW + dz[:k].T @ xin[:k]
        if mut == "bias_doubled" and l == len(layers) - 1:
            db = 2.0 * db
        if mut == "tile_tail" and l == len(layers) - 1:
            # the ragged last 64-row tile of the head's weight gradient without the batch's last 16-row k block
            r0 = dims[l + 1] // 64 * 64
            dW[r0:] = dW[r0:] - dz[B - 16:, r0:].T @ xin[B - 16:]
        if mut == "grad_scale_1e-3" and l == 1:
            dW = dW * np.float32(1 + 1e-3)
        g[wo:bo] = dW.reshape(-1)
        g[bo:bo + dims[l + 1]] = db
        if l > 0:
            dz = torch.where(xin > 0, dz @ layers[l][0], torch.zeros_like(xin))
    return g.numpy(), float(loss)


def f32_adam(p, g, m, v, t, cfg, mut=None):
    """k_adam on f32 tensors (in place), step t >= 1"""
    b1, b2 = np.float32(cfg["betas"][0]), np.float32(cfg["betas"][1])
    lr, eps, l2 = np.float32(cfg["lr"]), np.float32(cfg["eps"]), np.float32(cfg["l2"])
    bc1, bc2 = np.float32(1) - b1 ** np.float32(t), np.float32(1) - b2 ** np.float32(t)
    if mut == "bc_swapped":
        bc1, bc2 = bc2, bc1
    gi = g - l2 * p if mut == "l2_sign" else g + l2 * p
    m[:] = b1 * m + (np.float32(1) - b1) * gi
    v[:] = b2 * v + (np.float32(1) - b2) * gi * gi
    mh, vh = m / bc1, v / bc2
    den = np.sqrt(vh + eps) if mut == "eps_in_sqrt" else np.sqrt(vh) + eps
    p -= lr * mh / den


def run_steps(params, dims, batches, act, cfg, mut=None):
    """three f32 steps: [(gradient, loss)], final f32 parameters"""
    p = np.array(params, np.float32)
    m, v = np.zeros_like(p), np.zeros_like(p)
    rec = []
    for t, (x, obs, w) in enumerate(batches, 1):
        g, loss = f32_gradients(p, dims, x, obs, w, act, mut)
        rec.append((g, loss, p.copy()))
        f32_adam(p, g, m, v, t, cfg, mut)
    return rec, p


def gradient_check(dims, act, B, wkind, seed, mut=None):
    rng = np.random.default_rng(seed)
    params = R.init_params(dims, seed)
    x, obs, w = R.batch(dims, B, rng, wkind)
    g, loss = f32_gradients(params, dims, x, obs, w, act, mut)
    ref = R.Reference(params, dims, x, obs, w, act)
    return ref, ref.check_gradients(g, loss, what=(dims, B, act, wkind, mut))


SMALL = (304, 256, 256, 256, 152)
CONFIG_E = (3676, 512, 512, 512, 2450)
# the GPU module's matrix (tests/test_gpu_mlp_training.py): a batch below a tile, one batch-split part and two, the 64-part cap,
# the reference shape, the Ramsey models of bench.py, config E, widths that are no multiple of 4, every head and kind of weights
CASES = [(SMALL, 1, R.ACT_SIGMOID, "sparse"), (SMALL, 63, R.ACT_SIGMOID, "sparse"), (SMALL, 513, R.ACT_SIGMOID, "sparse"),
         (SMALL, 4096, R.ACT_SIGMOID, "sparse"), (SMALL, 65536, R.ACT_SIGMOID, "sparse"),
         ((304, 512, 1024, 512, 152), 512, R.ACT_SIGMOID, "sparse"), ((840, 256, 256, 256, 360), 2048, R.ACT_SIGMOID, "sparse"),
         ((680, 256, 256, 256, 272), 2048, R.ACT_SIGMOID, "sparse"), (CONFIG_E, 1024, R.ACT_SIGMOID, "sparse"),
         (SMALL, 130, R.ACT_RELU, "sparse"), (SMALL, 130, R.ACT_NONE, "sparse"), (SMALL, 513, R.ACT_SIGMOID, "dense"),
         (SMALL, 513, R.ACT_SIGMOID, "single"), (SMALL, 513, R.ACT_SIGMOID, "zero_row"),
         ((88, 48, 32, 44), 100, R.ACT_SIGMOID, "sparse"), ((88, 48, 32, 44), 100, R.ACT_RELU, "sparse"),
         ((10, 24, 5), 37, R.ACT_NONE, "zero_row"), ((13, 7, 33, 3), 70, R.ACT_RELU, "dense"),
         ((13, 7, 33, 3), 70, R.ACT_NONE, "single"), ((13, 7, 33, 3), 1300, R.ACT_RELU, "sparse")]
SHARE_FLOOR = 1e-2


@pytest.mark.parametrize("dims,B,act,wkind", CASES)
def test_f32_restatement_is_within_the_derived_bounds(dims, B, act, wkind):
    ref, rep = gradient_check(dims, act, B, wkind, seed=B)
    # the bounds are not vacuous: the restatement's own f32 error uses a visible share of its allowance
    share = max(v[0] for k, v in rep.items() if k != "loss")
    assert share > SHARE_FLOOR, rep
    if B == 65536:
        assert R.batch_splits(B) == (1024, 64)  # the 64-part cap of the weight gradient's batch sum


@pytest.mark.parametrize("mut", ["tile_tail", "loss_half", "loss_double"])
def test_localised_and_loss_mutations_fail_at_config_e(mut):
    """an error in one ragged output tile (18 rows of the head's dW missing 16 of 1024 batch rows) is far below a per-tensor
    scale: the elementwise bound catches it; a loss off by a factor 2 either way is caught by the loss bound"""
    with pytest.raises(AssertionError) as ei:
        gradient_check(CONFIG_E, R.ACT_SIGMOID, 1024, "sparse", seed=1024, mut=mut)
    assert ("W3" in str(ei.value) and "elementwise" in str(ei.value)) if mut == "tile_tail" else "loss" in str(ei.value)


def test_adam_replay_bounds_the_f32_step():
    dims, B = (88, 48, 32, 44), 100
    rng = np.random.default_rng(3)
    params = R.init_params(dims, 3)
    batches = [R.batch(dims, B, rng)] * 3
    for cfg in (VISIBLE, REFERENCE):
        rec, p = run_steps(params, dims, batches, R.ACT_SIGMOID, cfg)
        steps = R.adam_replay(params, [g for g, _, _ in rec], **cfg)
        for t in range(1, 3):
            R.check_adam(rec[t][2], *steps[t - 1], what=t)
        worst = R.check_adam(p, *steps[-1])
        assert worst > 1e-3  # f32 rounding is visible against the bound


def mutation_outcome(mut, dims=(88, 48, 32, 44), B=1100, cfg=VISIBLE):
    """(caught by the gradient check, caught by the Adam check) of one mutation"""
    rng = np.random.default_rng(7)
    params = R.init_params(dims, 7)
    x, obs, w = R.batch(dims, B, rng, "dense")
    ref = R.Reference(params, dims, x, obs, w, R.ACT_SIGMOID)
    rec, p = run_steps(params, dims, [(x, obs, w)] * 3, R.ACT_SIGMOID, cfg, mut)
    try:
        ref.check_gradients(rec[0][0], rec[0][1], what=mut)
        grad_caught = False
    except AssertionError:
        grad_caught = True
    steps = R.adam_replay(params, [g for g, _, _ in rec], **cfg)
    try:
        for t in range(1, 3):
            R.check_adam(rec[t][2], *steps[t - 1])
        R.check_adam(p, *steps[-1])
        adam_caught = False
    except AssertionError:
        adam_caught = True
    return grad_caught, adam_caught


@pytest.mark.parametrize("mut", MUTATIONS)
def test_each_mutation_fails_the_new_checks(mut):
    grad_caught, adam_caught = mutation_outcome(mut)
    if mut in GRADIENT_MUTATIONS:
        assert grad_caught, mut
    else:
        assert adam_caught and not grad_caught, mut


def test_the_parameter_comparison_lets_the_gradient_scale_mutations_through():
    """What the older check sees: three steps of the (mutated) f32 restatement against the f64 step on the f64 gradients, at
    the reference Adam configuration, parameters within 0.05 lr.  Adam divides a per-tensor gradient scale out, so the scale
    mutations pass it; that is what the gradient check above is for."""
    dims, B, cfg = (88, 48, 32, 44), 1100, REFERENCE
    rng = np.random.default_rng(7)
    params = R.init_params(dims, 7)
    x, obs, w = R.batch(dims, B, rng, "dense")
    p64, g64s = np.array(params, np.float64), []
    for t in range(3):  # the f64 step on the f64 gradient of the f64 parameters
        g64s.append(R.gradients(p64, dims, x, obs, w, R.ACT_SIGMOID)[1])
        p64 = R.adam_replay(params, g64s, **cfg)[-1][0]
    through = set()
    for mut in (None,) + MUTATIONS:
        _, p = run_steps(params, dims, [(x, obs, w)] * 3, R.ACT_SIGMOID, cfg, mut)
        if np.max(np.abs(p - p64)) < 0.05 * cfg["lr"]:
            through.add(mut)
    # the unmutated step passes it, and so do the scale errors of one tensor.  Dropping the factor 2 of every gradient does not:
    # on parameters whose gradient is as small as l2 p (dead units among them) the halved gradient moves the step's sign
    assert through == {None, "grad_scale_1e-3", "bias_doubled"}, through
