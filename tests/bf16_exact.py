"""Exact reference of the bf16 evaluator forward on integer-valued models.  A test helper, not a conftest: numpy on the CPU.

The argument.  A product of two bf16 values is exact in f32 (8 + 8 significant bits).  If every operand of a layer is an integer
multiple of a power of two (its quantum), every product and the bias are multiples of one quantum q; if, for an output element,
sum |a w| + |b| stays below 2^24 q, then every partial sum of those terms -- in ANY order, tile form, k split or MFMA schedule --
is a multiple of q below 2^24 q in magnitude, hence an f32 value, hence computed without rounding.  The device's result must then
equal the integer result word for word; the only roundings left are the stated ones (RNE to bf16 of the input rows and of every
hidden activation), and the reference below performs them with the same formula as csrc/bf16.h.  `assert_exact` checks the
condition on the inputs (it is no tolerance), the GPU tests compare words.

Layout: the flat parameter vector of get_params, per layer W[out][in] then b[out].  Hidden layers are ReLU, the head is `act`.
The tables at the end name every shape tests/test_gpu_gemm_bf16_exact.py runs; tests/test_bf16_exact_reference.py checks the
condition and the sensitivity of the data at each of them on the CPU."""
import functools

import numpy as np

F = np.float32
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
LIMIT = float(1 << 24)


# ---- bf16 (RNE), bit for bit csrc/bf16.h
def bf16_bits(x):
    """uint16 bit patterns of RNE(x), x float32 (finite)"""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).reshape(np.shape(x))


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(F).reshape(np.shape(bits))


def bf16_round(x):
    return bf16_to_f32(bf16_bits(x))


def bf16_round_ties_away(x):
    """the WRONG rounding a test mutates the reference with: ties away from zero"""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    return ((((u + 0x8000) >> 16) << 16) & 0xFFFFFFFF).astype(np.uint32).view(F).reshape(np.shape(x))


def is_bf16(x):
    return (np.ascontiguousarray(x, F).view(np.uint32) & 0xFFFF) == 0


def quantum(x):
    """the largest power of two every element of x is an integer multiple of (1.0 for an all-zero array)"""
    v = np.abs(np.asarray(x, np.float64)).ravel()
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    m, e = np.frexp(v)
    mi = np.round(np.ldexp(m, 53)).astype(np.int64)
    low = mi & -mi  # the lowest set bit of the 53-bit mantissa
    return float(2.0 ** int((e - 53 + np.round(np.log2(low.astype(np.float64))).astype(np.int64)).min()))


# ---- integer-valued operands from a seed
def int_array(rng, shape, density, lo, hi):
    """float64 integers in [lo, hi], zero outside a random mask of the given density"""
    return (rng.integers(lo, hi + 1, shape) * (rng.random(shape) < density)).astype(np.float64)


def layout(dims):
    out, off = [], 0
    for l in range(len(dims) - 1):
        out.append((off, off + dims[l] * dims[l + 1]))
        off += dims[l] * dims[l + 1] + dims[l + 1]
    return out


def unpack(params, dims):
    p = np.asarray(params, np.float64)
    return [(p[wo:bo].reshape(dims[l + 1], dims[l]), p[bo:bo + dims[l + 1]]) for l, (wo, bo) in enumerate(layout(dims))]


def make_params(seed, dims, density=3 / 16, w_range=(-1, 1), b_range=(-3, 3), scales=None):
    """flat float32 parameters: W_l = integers of w_range at `density` (a number or one per layer) times 2^scales[l], b_l = integers of
    b_range times the layer's output quantum 2^(scales[0] + .. + scales[l]); the last bias of every layer is not zero"""
    rng = np.random.default_rng([seed, 1])
    L = len(dims) - 1
    dens = [density] * L if np.isscalar(density) else list(density)
    parts, cum = [], 0
    for l in range(L):
        s = scales[l] if scales else 0
        cum += s
        W = int_array(rng, (dims[l + 1], dims[l]), dens[l], *w_range) * 2.0 ** s
        b = rng.integers(b_range[0], b_range[1] + 1, dims[l + 1]).astype(np.float64)
        if b[-1] == 0:
            b[-1] = 1.0
        parts += [W.ravel(), b * 2.0 ** cum]
    p = np.concatenate(parts)
    assert np.array_equal(p.astype(F).astype(np.float64), p)
    return p.astype(F)


def make_states(seed, rows, width, density=0.3, hi=2):
    """float32 rows of integers 0 .. hi at the given density"""
    return int_array(np.random.default_rng([seed, 2]), (rows, width), density, 0, hi).astype(F)


# integers bf16 cannot hold: 8 significant bits, so spacing 2 from 256, 4 from 512, 8 from 1024.  Ties (to even): 257 -> 256,
# 259 -> 260, 261 -> 260, 514 -> 512, 518 -> 520, 1028 -> 1024, 1036 -> 1040; not ties: 513 -> 512, 515 -> 516, 1030 -> 1032
ROUNDING_VALUES = (257, 259, 261, 513, 514, 515, 518, 1028, 1030, 1036)


def with_rounding_columns(x, seed, n_cols=6, density=0.3):
    """a copy of x in which n_cols columns (the first and the last among them) hold, at `density`, integers that are not
    bf16-representable, exact ties included, of both signs -- so that the f32 -> bf16 conversion of the input rows rounds; row r
    holds the r-th of the values for certain (row 0: a tie)"""
    x = np.array(x, F)
    rows, width = x.shape
    rng = np.random.default_rng([seed, 3])
    cols = np.unique(np.linspace(0, width - 1, n_cols).astype(int))
    vals = np.array(ROUNDING_VALUES + tuple(-v for v in ROUNDING_VALUES), F)
    for c in cols:
        pick = rng.choice(vals, rows)
        mask = rng.random(rows) < density
        x[:, c] = np.where(mask, pick, x[:, c])
    for r in range(min(rows, len(vals))):
        x[r, cols[r % len(cols)]] = vals[r]
    return x


# ---- the reference
def layer_inputs(params, dims, x, bf16=True, round_fn=None, skip_round=()):
    """[(a, W, b, z)] per layer, float64: a = the layer's input as the kernel takes it (rounded to bf16 under bf16 storage),
    z = a W^T + b.  round_fn / skip_round: mutations for the sensitivity tests."""
    rnd = round_fn or bf16_round
    t = np.asarray(x, np.float64)
    out = []
    layers = unpack(params, dims)
    for l, (W, b) in enumerate(layers):
        if bf16 and l not in skip_round:
            t = rnd(t.astype(F)).astype(np.float64)
        z = t @ W.T + b
        out.append((t, W, b, z))
        t = np.maximum(z, 0.0)
    return out


def head(z, act):
    """the head's output: float32 (exact) for NONE / RELU, float64 for SIGMOID"""
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-z))
    return (np.maximum(z, 0.0) if act == ACT_RELU else z).astype(F)


def exact_forward(params, dims, x, head_act, bf16=True, round_fn=None, skip_round=()):
    """(output, head pre-activation (float64)): per layer round the input to bf16 (RNE), multiply, add the bias, ReLU -- the
    project's stated rounding points (tests/test_gpu_bf16.py reference_forward), in exact integer arithmetic (float64 holds
    every value: assert_exact).  bf16=False: fp32 storage, no rounding anywhere."""
    z = layer_inputs(params, dims, x, bf16, round_fn, skip_round)[-1][3]
    return head(z, head_act), z


def assert_exact(layers, operands_bf16=True):
    """The condition under which the device's f32 sums are exact, on [(a, W, b, ...)]: per layer every operand a multiple of a
    power of two, sum |a w| + |b| of every output element below 2^24 quanta; under bf16 storage a and W bf16-representable, b an
    f32 value.  Returns the largest bound per layer, in quanta."""
    worst = []
    for l, (a, W, b, *_) in enumerate(layers):
        a, W, b = (np.asarray(v, np.float64) for v in (a, W, b))
        assert np.isfinite(a).all() and np.isfinite(W).all() and np.isfinite(b).all()
        for name, v in (("a", a), ("W", W), ("b", b)):
            assert np.array_equal(v.astype(F).astype(np.float64), v), (l, name, "not an f32 value")
        if operands_bf16:
            assert is_bf16(a.astype(F)).all(), (l, "input not bf16-representable")
            assert is_bf16(W.astype(F)).all(), (l, "weight not bf16-representable")
        q = min(quantum(a) * quantum(W), quantum(b))
        bound = (np.abs(a) @ np.abs(W).T + np.abs(b)) / q
        assert bound.max() < LIMIT, (l, float(bound.max()))
        worst.append(float(bound.max()))
    return worst


def gemm_words(A, W, b, act, out_bf16):
    """the words of Y = act(A W^T + b): uint32 of the f32 output or uint16 of its RNE bf16"""
    y = head(np.asarray(A, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64), act)
    return bf16_bits(y) if out_bf16 else y.view(np.uint32)


def lattice(y):
    """rint(8 logit(y)): the multiple of 1/8 a sigmoid output came from"""
    y = np.asarray(y, np.float64)
    return np.rint(8.0 * np.log(y / (1.0 - y))).astype(np.int64)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the cases of tests/test_gpu_gemm_bf16_exact.py
# (a) k_gemm16 alone: (M, N, Kp).  Every M edge of the 128-row panel with one N and Kp, every N edge of the 64 / 128-wide tiles
# with one M and Kp, 1 / 2 / 3 / 5 k tiles (nt == 1, the two-buffer loop's even and odd exits), and 11 row panels x 130 columns:
# the last group of the 8-panel walk has 3 panels, 22 or 33 blocks are no multiple of the 8 XCDs.  K = Kp - 7: the last 16-wide
# k step holds 9 columns and 7 of padding.
GEMM_SHAPES = ((1, 65, 128), (127, 65, 128), (128, 65, 128), (129, 65, 128), (129, 1, 128), (129, 63, 128), (129, 64, 128),
               (129, 130, 128), (129, 65, 64), (129, 65, 192), (129, 65, 320), (1403, 130, 192))
K_PAD = 7


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, Kp, kind):
    """(A [M, Kp], W [N, Kp], b [N]) float32, zero from K = Kp - 7 on.  kind "wide": A 0 .. 7 at 50 %, W -96 .. 96 at 50 %,
    b -300 .. 300 -- sums in the thousands, so the bf16 epilogue rounds, ties included; "lattice": A 0 .. 2 at 30 %,
    W {-1, 0, 1} / 8 at 3 / 16, b {-3 .. 3} / 8 -- pre-activations on the 1 / 8 lattice for the sigmoid decode"""
    rng = np.random.default_rng([M, N, Kp, 0 if kind == "wide" else 1])
    K = Kp - K_PAD
    A, W = np.zeros((M, Kp)), np.zeros((N, Kp))
    if kind == "wide":
        A[:, :K] = int_array(rng, (M, K), 0.5, 0, 7)
        W[:, :K] = int_array(rng, (N, K), 0.5, -96, 96)
        b = rng.integers(-300, 301, N).astype(np.float64)
    else:
        A[:, :K] = int_array(rng, (M, K), 0.3, 0, 2)
        W[:, :K] = int_array(rng, (N, K), 3 / 16, -1, 1) / 8.0
        b = rng.integers(-3, 4, N) / 8.0
    if b[-1] == 0:
        b[-1] = 1.0 if kind == "wide" else 0.125
    return frozen(A.astype(F), W.astype(F), b.astype(F))


# (b), (c), (d): whole forwards.  name -> (dims, rows, head, bf16 storage, scales, input rows with rounding columns)
MODELS = {
    "37-40-33": ((37, 40, 33), 80, ACT_RELU, True, None, True),
    "133-96-70-45": ((133, 96, 70, 45), 80, ACT_RELU, True, None, True),
    "300-512-512-512-70": ((300, 512, 512, 512, 70), 77, ACT_RELU, True, None, True),
    "1100-96-45": ((1100, 96, 45), 77, ACT_RELU, True, None, True),
    "132-96-68-44": ((132, 96, 68, 44), 80, ACT_RELU, True, None, True),
    "37-40-33 sigmoid": ((37, 40, 33), 80, ACT_SIGMOID, True, (0, -3), False),
    "1100-512-512-512-70": ((1100, 512, 512, 512, 70), 80, ACT_RELU, True, None, True),
    "304-256-256-256-152": ((304, 256, 256, 256, 152), 100, ACT_RELU, True, None, True),
    "88-48-32-44": ((88, 48, 32, 44), 100, ACT_RELU, True, None, True),
    "304-256-256-256-152 f32": ((304, 256, 256, 256, 152), 100, ACT_RELU, False, None, True),
    "88-48-32-44 f32": ((88, 48, 32, 44), 100, ACT_RELU, False, None, True),
}


@functools.lru_cache(maxsize=None)
def model_case(name):
    """(dims, head, bf16, params, x, output, head pre-activation): the recipe of the issue -- input rows of integers 0 .. 2 at
    30 % (plus the rounding columns), weights {-1, 0, 1} at 3 / 16, biases -3 .. 3 -- and its exact forward, computed once"""
    dims, rows, act, bf16, scales, rounding = MODELS[name]
    seed = sum(dims) + rows
    params = make_params(seed, dims, scales=scales)
    x = make_states(seed, rows, dims[0])
    if rounding:
        x = with_rounding_columns(x, seed)
    y, z = exact_forward(params, dims, x, act, bf16)
    frozen(params, x, y, z)
    return dims, act, bf16, params, x, y, z
