"""Float64 reference of the MLP evaluator's training step (model/dfdx.rs:86-131 with Adam and L2, 04-c21-tree.rs:87-92),
with error bounds derived from the f32 computation it checks rather than tuned to it.  A test helper, not a conftest: torch on
the CPU in float64, no oracle.

Layout: the flat parameter vector of get_params, per layer W[out][in] then b[out].  Hidden layers are ReLU, the head is
`act` (NONE / RELU / SIGMOID).  Loss: w~ = w / sum(w), L = sum w~ (p - o)^2.

Bounds.  u = 2^-24.  The f32 error of a sum of n exact products (FMA chains, MFMA) is sum_k delta_k S_k over its partial sums
S_k with |delta_k| <= u; with the roundings independent its standard deviation is at most u sqrt(n / 3) sum |terms|.  Errors
are carried from layer to layer in variance (through W^2, not |W|: a worst case through |W| grows geometrically with depth and
says nothing at the trained shapes), and the allowance of every element is C_SIGMA standard deviations.
  forward     var(z_l) = u^2 (K_l + 1) / 3 (|W_l| |a_{l-1}| + |b_l|)^2 + var(a_{l-1}) W_l^2.
  magnitude   M(dW_l) = |delta_l|^T |a_{l-1}|, M(db_l) = the column sums of |delta_l|.
  gradient    var = u^2 n / 3 M^2 (n: the batch sum's longest serial length as the device splits it) + the head delta's, the
              backward's and the forward's errors carried in variance, row by row.
  ambiguity   a pre-activation with |z64| <= C_SIGMA sigma can take either ReLU mask in f32.  Such units are counted, and their
              full backward contribution, carried in absolute value to the lower layers, is a separate term A: the elementwise
              check allows tol + A, never a looser tol.
  scale       per tensor, <g, g64> / <g64, g64> within 1 +- SCALE_TOL (Adam divides a per-tensor scale out, so nothing after
              the gradient sees one); what the scale fit leaves, less A, within RESID_SIGMAS ||sigma|| in norm.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_SIGMA = 8.0      # allowance per element, in standard deviations
RESID_SIGMAS = 4.0  # allowance of the residual's norm, in ||sigma||
SCALE_TOL = 2e-4
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
# the weight gradient's batch split (mlp_kernels.hip gemm_dw): only the length of the longest f32 sum is taken from it
SPLIT_K, MAX_SPLITS, BK = 512, 64, 16


def layout(dims):
    """[(w_off, b_off)] of the flat parameter vector"""
    out, off = [], 0
    for l in range(len(dims) - 1):
        out.append((off, off + dims[l] * dims[l + 1]))
        off += dims[l] * dims[l + 1] + dims[l + 1]
    return out


def n_params(dims):
    return sum(dims[l] * dims[l + 1] + dims[l + 1] for l in range(len(dims) - 1))


def tensors(dims):
    """(name, slice) of every tensor of the flat vector"""
    out = []
    for l, (wo, bo) in enumerate(layout(dims)):
        out += [("W%d" % l, slice(wo, bo)), ("b%d" % l, slice(bo, bo + dims[l + 1]))]
    return out


def batch_splits(B):
    """(rows per part, parts) of the weight gradient's batch sum"""
    splits = min(-(-B // SPLIT_K), MAX_SPLITS)
    if splits <= 1:
        return B, 1
    k = -(-B // splits)
    k = -(-k // BK) * BK
    return k, -(-B // k)


def batch_sum_length(B):
    k, parts = batch_splits(B)
    return k + parts - 1


def reduce_length(n):
    """the device's two-stage sums (256 blocks x 256 threads strided, then trees): the weight sum and the loss"""
    return -(-n // 65536) + 8 + 8 + 8


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def unpack(flat, dims):
    p = flat if isinstance(flat, torch.Tensor) else _t(flat)
    return [(p[wo:bo].reshape(dims[l + 1], dims[l]), p[bo:bo + dims[l + 1]]) for l, (wo, bo) in enumerate(layout(dims))]


def head(z, act):
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == ACT_RELU:
        return torch.relu(z)
    return z


def forward(params, dims, x, act):
    """f64 predictions [B, A]"""
    t = _t(x)
    layers = unpack(params, dims)
    for l, (W, b) in enumerate(layers):
        t = t @ W.T + b
        t = head(t, act) if l == len(layers) - 1 else torch.relu(t)
    return t


def forward_bound(params, dims, x, act):
    """(f64 predictions, allowed |error| of the f32 forward per output) -- the bound the forward tests use"""
    p, _, _, var, _ = _forward_terms(unpack(params, dims), dims, _t(x), act)
    return p, C_SIGMA * _head_sigma(p, var[-1], act)


def _head_slope(p, act):
    if act == ACT_SIGMOID:
        return p * (1 - p)
    return torch.ones_like(p)


def _head_sigma(p, var_z, act):
    """sigma of the f32 head output: the pre-activation's, through the head's slope, and the head's own few roundings"""
    return torch.sqrt(_head_slope(p, act) ** 2 * var_z + (2 * U * p) ** 2)


def _sum_var(n, abs_sum):
    """variance scale of an f32 sum of n exact products whose absolute values add up to abs_sum: (u^2 n / 3) abs_sum^2"""
    return (U * U * n / 3.0) * abs_sum * abs_sum


def _forward_terms(layers, dims, x, act):
    """activations a_0..a_{L-1}, pre-activations z_1..z_L, the head output, the variance scale var_l of z_l's f32 error,
    ambiguity masks"""
    a, zs, var, amb = [x], [], [], []
    v_prev = None
    for l, (W, b) in enumerate(layers):
        z = a[-1] @ W.T + b
        v = _sum_var(dims[l] + 1, a[-1].abs() @ W.abs().T + b.abs())
        if v_prev is not None:
            v = v + v_prev @ (W * W).T
        zs.append(z)
        var.append(v)
        last = l == len(layers) - 1
        if not last or act == ACT_RELU:
            amb.append(z.abs() <= C_SIGMA * torch.sqrt(v))
            # the next layer's input error: the activation's own (ReLU passes it where either mask may hold)
            v_prev = torch.where((z > 0) | amb[-1], v, torch.zeros_like(v))
        else:
            amb.append(torch.zeros_like(z, dtype=torch.bool))
        if not last:
            a.append(torch.relu(z))
    return head(zs[-1], act), a, zs, var, amb


class Reference:
    """Gradient (autograd), loss, and the bounds of a device gradient at one batch.  Attributes (numpy f64 unless noted):
    loss, grad, M (|delta|^T |a|: the magnitude behind each element), sigma (the f32 error's scale per element), tol =
    C_SIGMA sigma, A (ambiguous ReLU units), loss_tol, ambiguous (ReLU units per layer that can take either mask)."""

    def __init__(self, params, dims, x, obs, w, act):
        dims = tuple(int(d) for d in dims)
        self.dims, self.act = dims, act
        x, obs, w = _t(x).reshape(-1, dims[0]), _t(obs).reshape(-1, dims[-1]), _t(w).reshape(-1, dims[-1])
        B, L = x.shape[0], len(dims) - 1
        flat = _t(params).clone().requires_grad_(True)
        layers = unpack(flat, dims)
        p, a, zs, var, amb = _forward_terms(layers, dims, x, act)
        ws = w.sum()
        wt = w / ws
        loss = (wt * (p - obs) ** 2).sum()
        (g,) = torch.autograd.grad(loss, flat)
        self.loss, self.grad = float(loss.detach()), g.numpy().copy()
        with torch.no_grad():
            Ws = [W.detach() for W, _ in layers]
            p, a = p.detach(), [t.detach() for t in a]
            zs, var = [t.detach() for t in zs], [t.detach() for t in var]
            d = p - obs
            hp = _head_slope(p, act)
            delta = 2 * wt * d * hp
            if act == ACT_RELU:
                delta = torch.where(p > 0, delta, torch.zeros_like(delta))
            n_red = reduce_length(B * dims[-1])
            # the head delta's error: the prediction's (through the slope and the factor p - o, both move with p), the weight
            # sum's (n_red) and the few elementwise roundings of k_loss_delta
            sp = _head_sigma(p, var[-1], act)
            pmask = (p > 0) | amb[-1] if act == ACT_RELU else torch.ones_like(p, dtype=torch.bool)
            vd = torch.where(pmask, (2 * wt * (hp + d.abs()) * sp) ** 2, torch.zeros_like(p)) + _sum_var(n_red + 8, delta.abs())
            # ambiguous head units (ReLU head): the delta the other mask would give
            E = torch.where(amb[-1], (2 * wt * d).abs(), torch.zeros_like(p))
            nb = batch_sum_length(B)
            self.M = np.zeros_like(self.grad)
            self.sigma = np.zeros_like(self.grad)
            self.A = np.zeros_like(self.grad)
            self.ambiguous = [int(t.sum()) for t in amb[:-1]] + ([int(amb[-1].sum())] if act == ACT_RELU else [])
            for l in range(L - 1, -1, -1):
                wo, bo = layout(dims)[l]
                xin = a[l]
                # the input activation's own error (the forward's), where either mask may hold
                va = torch.where((zs[l - 1] > 0) | amb[l - 1], var[l - 1], torch.zeros_like(xin)) if l > 0 else torch.zeros_like(xin)
                D = delta.abs()
                MW, Mb = D.T @ xin.abs(), D.sum(0)
                self.M[wo:bo] = MW.reshape(-1).numpy()
                self.M[bo:bo + dims[l + 1]] = Mb.numpy()
                # the batch sum's own rounding (length nb), the delta's error and the input's, each row independent
                vW = _sum_var(nb, MW) + vd.T @ (xin * xin) + (delta * delta).T @ va
                vb = _sum_var(nb, Mb) + vd.sum(0)
                self.sigma[wo:bo] = torch.sqrt(vW).reshape(-1).numpy()
                self.sigma[bo:bo + dims[l + 1]] = torch.sqrt(vb).numpy()
                self.A[wo:bo] = (E.T @ xin.abs()).reshape(-1).numpy()
                self.A[bo:bo + dims[l + 1]] = E.sum(0).numpy()
                if l == 0:
                    break
                W = Ws[l]
                G = delta @ W                       # the backward before layer l's ReLU mask
                on = zs[l - 1] > 0
                either = on | amb[l - 1]
                delta = torch.where(on, G, torch.zeros_like(G))
                vd = torch.where(either, vd @ (W * W) + _sum_var(dims[l + 1], D @ W.abs()), torch.zeros_like(G))
                E = torch.where(either, E @ W.abs(), torch.zeros_like(G)) + torch.where(amb[l - 1], G.abs(), torch.zeros_like(G))
            self.tol = C_SIGMA * self.sigma
            # the loss: its sum's and the weight sum's rounding (all terms >= 0: their absolute sum is the loss), and the
            # predictions' errors through 2 w~ (p - o)
            vl = 2 * _sum_var(n_red + 8, loss.detach()) + ((2 * wt * d) ** 2 * sp * sp).sum()
            self.loss_tol = float(C_SIGMA * torch.sqrt(vl) + (wt * (C_SIGMA * sp) ** 2).sum())

    def check_gradients(self, g, loss=None, what=""):
        """raises AssertionError naming the first tensor out of bounds; returns {tensor: (max |err| / (tol + A), scale,
        residual after the scale fit, its bound)} and 'loss': |err| / loss_tol"""
        g = np.asarray(g, np.float64)
        assert g.shape == self.grad.shape, (what, g.shape, self.grad.shape)
        assert np.all(np.isfinite(g)), what
        rep = {}
        for name, sl in tensors(self.dims):
            ref, dev, tol, A = self.grad[sl], g[sl], self.tol[sl], self.A[sl]
            err = np.abs(dev - ref)
            worst = float(np.max(err / (tol + A + 1e-300)))
            assert worst <= 1.0, (what, name, "elementwise", worst, int(np.argmax(err / (tol + A + 1e-300))))
            nref = float(np.linalg.norm(ref))
            if nref == 0.0:
                rep[name] = (worst, 1.0, 0.0, 0.0)
                continue
            s = float(np.dot(dev, ref) / (nref * nref))
            # what the scale fit leaves and A does not explain, against RESID_SIGMAS x the norm of the per-element sigmas
            # (independent errors add in norm to about ||sigma||: far below the elementwise allowance summed)
            resid = float(np.linalg.norm(np.maximum(np.abs(dev - s * ref) - A, 0.0)) / nref)
            rbound = float(RESID_SIGMAS * np.linalg.norm(self.sigma[sl]) / nref)
            assert abs(s - 1.0) <= SCALE_TOL, (what, name, "scale", s)
            assert resid <= rbound, (what, name, "residual", resid, rbound)
            rep[name] = (worst, s, resid, rbound)
        if loss is not None:
            r = abs(float(loss) - self.loss) / self.loss_tol if self.loss_tol > 0 else float(abs(float(loss) - self.loss) > 0)
            assert r <= 1.0, (what, "loss", float(loss), self.loss, self.loss_tol)
            rep["loss"] = r
        return rep


def gradients(params, dims, x, obs, w, act):
    """(loss, flat gradient) in f64 by autograd"""
    flat = _t(params).clone().requires_grad_(True)
    ws = _t(w).sum()
    loss = (_t(w) / ws * (forward(flat, dims, x, act) - _t(obs).reshape(-1, dims[-1])) ** 2).sum()
    (g,) = torch.autograd.grad(loss, flat)
    return float(loss.detach()), g.numpy().copy()


def adam_replay(p0, grads, lr, betas, eps, l2):
    """f64 Adam with coupled L2 (g += l2 p), bias correction 1 - beta^t, eps outside the sqrt, from zero moments, on the
    given per-step gradients.  Returns [(p_t, bound_t)]: bound_t is the allowed |p_dev - p_t| after step t when p_dev is
    the f32 step on the same gradients -- per step 2 ulp(p) for the update's rounding, and lr |m^ / (sqrt(v^) + eps)| times the
    relative error of that ratio in f32: (4 + 4 t) u for the moments and the division, and u beta^t / (1 - beta^t) for each bias
    correction (1 - beta^t rounded after beta^t: 500 u at t = 2 for beta = 0.999) -- summed over the steps so far.  The
    hyperparameters are taken at f32 precision, as the device receives them."""
    lr, eps, l2 = (float(np.float32(c)) for c in (lr, eps, l2))
    b1, b2 = (float(np.float32(c)) for c in betas)
    p = np.asarray(p0, np.float64).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    out, acc = [], np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        gi = np.asarray(g, np.float64) + l2 * p
        m = b1 * m + (1 - b1) * gi
        v = b2 * v + (1 - b2) * gi * gi
        r = (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
        p = p - lr * r
        rel = (4 + 4 * t + b1 ** t / (1 - b1 ** t) + 0.5 * b2 ** t / (1 - b2 ** t)) * U
        acc = acc + 2 * np.spacing(np.abs(p).astype(np.float32)).astype(np.float64) + rel * lr * np.abs(r)
        out.append((p.copy(), acc.copy()))
    return out


def check_adam(p_dev, p_ref, bound, what=""):
    """max |p_dev - p_ref| / bound (asserted <= 1)"""
    err = np.abs(np.asarray(p_dev, np.float64) - p_ref)
    worst = float(np.max(err / bound))
    assert worst <= 1.0, (what, "adam", worst, int(np.argmax(err / bound)))
    return worst


def weights(kind, B, A, rng):
    """action weights of the test matrix: 'sparse' 0/1, 'dense' spread over 1e-3..1, 'single' one nonzero in the batch,
    'zero_row' sparse with one row all zeros"""
    if kind == "sparse":
        w = (rng.random((B, A)) < 0.05).astype(np.float32)
        w[0, 0] = 1.0
    elif kind == "dense":
        w = (10.0 ** rng.uniform(-3, 0, (B, A))).astype(np.float32)
    elif kind == "single":
        w = np.zeros((B, A), np.float32)
        w[B // 2, A // 3] = 1.0
    elif kind == "zero_row":
        w = (rng.random((B, A)) < 0.2).astype(np.float32)
        w[0, 0] = 1.0
        w[B - 1] = 0.0
    else:
        raise ValueError(kind)
    return w


def batch(dims, B, rng, wkind="sparse"):
    """(states, observations, action weights) like the search's: 0/1 state rows, observations in [0, 1)"""
    x = (rng.random((B, dims[0])) < 0.3).astype(np.float32)
    obs = rng.random((B, dims[-1]), dtype=np.float32)
    return x, obs, weights(wkind, B, dims[-1], rng)


def init_params(dims, seed):
    """dfdx's Linear init in distribution (U(-1/sqrt(in), 1/sqrt(in))) -- for CPU tests; GPU tests use the device's own"""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(len(dims) - 1):
        bound = 1.0 / math.sqrt(dims[l])
        out.append(rng.uniform(-bound, bound, dims[l] * dims[l + 1]))
        out.append(rng.uniform(-bound, bound, dims[l + 1]))
    return np.concatenate(out).astype(np.float32)
