"""The exact reference of the bf16 forward (tests/bf16_exact.py) checked on the CPU: its rounding is torch's, bit for bit; an
f32 accumulation of the test operands gives the integer result in every order; the 2^24 condition holds at every shape
tests/test_gpu_gemm_bf16_exact.py runs; and the data is sensitive -- each of a handful of plausible kernel errors, applied to the
reference, changes at least one output word at every one of those shapes, so a device result that equals the reference word for
word rules them out."""
import numpy as np
import pytest
import torch

import bf16_exact as X

F = np.float32


def torch_round(x):
    return torch.from_numpy(np.ascontiguousarray(x, F)).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_round_is_torchs_on_random_words_and_constructed_ties():
    rng = np.random.default_rng(0)
    words = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    # ties (low half 0x8000) and their neighbours, under an even and an odd kept mantissa, both signs, many exponents
    hi = rng.integers(0, 1 << 15, 4096, dtype=np.uint64).astype(np.uint32) << 16
    low = np.array([0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF], np.uint32)
    made = (hi[:, None] | low[None, :]).ravel()
    made = np.concatenate([made, made ^ np.uint32(0x00010000), made | np.uint32(0x80000000)])
    ints = np.array(X.ROUNDING_VALUES + tuple(-v for v in X.ROUNDING_VALUES), F).view(np.uint32)
    w = np.concatenate([words, made, ints])
    x = w.view(F)
    x = x[np.isfinite(x)]
    got, want = X.bf16_round(x), torch_round(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(X.bf16_bits(x), want.view(np.uint32) >> 16)
    assert X.is_bf16(got).all()
    # the documented ties and non-ties
    v = np.array([257, 259, 261, 513, 514, 515, 518, 1028, 1030, 1036, -257, -259, -518], F)
    assert X.bf16_round(v).tolist() == [256, 260, 260, 512, 512, 516, 520, 1024, 1032, 1040, -256, -260, -520]
    away = X.bf16_round_ties_away(v)
    assert away.tolist() == [258, 260, 262, 512, 516, 516, 520, 1032, 1032, 1040, -258, -260, -520]
    # ... and away from zero differs from RNE on ties alone
    d = X.bf16_round_ties_away(x).view(np.uint32) != got.view(np.uint32)
    assert d.any() and ((x.view(np.uint32)[d] & 0xFFFF) == 0x8000).all()


def test_quantum():
    assert X.quantum([0.0, 0.0]) == 1.0
    assert X.quantum([3.0, -6.0, 12.0]) == 1.0
    assert X.quantum([6.0, 12.0, 0.0]) == 2.0
    assert X.quantum([0.375, 2.0]) == 0.125
    assert X.quantum([1024.0, 2024.0]) == 8.0


def f32_sum(A, W, order, parts=1):
    """sum_k A[:, k] W[:, k] accumulated in float32, k in the given order, dealt to `parts` partial sums that are added in turn"""
    acc = []
    for chunk in np.array_split(np.asarray(order), parts):
        s = np.zeros((A.shape[0], W.shape[0]), F)
        for k in chunk:
            s = (s + np.outer(A[:, k], W[:, k]).astype(F)).astype(F)
        acc.append(s)
    total = acc[0]
    for s in acc[1:]:
        total = (total + s).astype(F)
    return total


@pytest.mark.parametrize("kind", ["wide", "lattice"])
def test_an_f32_accumulation_gives_the_integer_result_in_every_order(kind):
    A, W, b = X.gemm_case(129, 65, 320, kind)
    X.assert_exact([(A, W, b)])
    want = A.astype(np.float64) @ W.astype(np.float64).T
    K = A.shape[1]
    rng = np.random.default_rng(3)
    orders = [("ascending", np.arange(K), 1), ("descending", np.arange(K)[::-1], 1), ("permuted", rng.permutation(K), 1),
              ("permuted again", rng.permutation(K), 1), ("2-way", np.arange(K), 2), ("4-way", np.arange(K), 4),
              ("8-way", np.arange(K), 8), ("8-way permuted", rng.permutation(K), 8)]
    for name, order, parts in orders:
        got = f32_sum(A, W, order, parts)
        assert np.array_equal(got.astype(np.float64), want), name
        # the bias last or first
        assert np.array_equal((got + b).astype(F).astype(np.float64), want + b), name
    # a float32 that does NOT satisfy the condition is order dependent: the check means something
    big = (A * F(1 << 20)).astype(F)
    with pytest.raises(AssertionError):
        X.assert_exact([(big, W * F(4097), b)], operands_bf16=False)


def test_assert_exact_refuses_what_it_should():
    A, W, b = (np.array(v) for v in X.gemm_case(129, 65, 64, "wide"))
    X.assert_exact([(A, W, b)])
    W2 = W.copy()
    W2[0, 0] = 257.0  # not a bf16 value
    with pytest.raises(AssertionError):
        X.assert_exact([(A, W2, b)])
    X.assert_exact([(A, W2, b)], operands_bf16=False)
    A2 = A.copy()
    A2[0, 0] = 0.3
    with pytest.raises(AssertionError):
        X.assert_exact([(A2, W, b)])
    b2 = b.astype(np.float64)
    b2[0] = 2.0 ** 25 + 1  # no f32 value
    with pytest.raises(AssertionError):
        X.assert_exact([(A, W, b2)])


# ---- the isolated GEMM's shapes
def drop_k(A, lo, hi):
    A = np.array(A)
    A[:, lo:hi] = 0
    return A


@pytest.mark.parametrize("shape", X.GEMM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_gemm_shapes_satisfy_the_condition_and_the_data_is_sensitive(shape):
    M, N, Kp = shape
    K = Kp - X.K_PAD
    A, W, b = X.gemm_case(M, N, Kp, "wide")
    assert not A[:, K:].any() and not W[:, K:].any() and A[:, K - 1].any() + W[:, K - 1].any() > 0
    worst = X.assert_exact([(A, W, b)])
    print("%s: sum |a w| + |b| <= %d quanta" % (shape, worst[0]))
    words = {(act, o): X.gemm_words(A, W, b, act, o) for act in (X.ACT_NONE, X.ACT_RELU) for o in (0, 1)}
    plain = words[(X.ACT_NONE, 0)]
    z = plain.view(F)
    # the data exercises the epilogues: both signs, values bf16 cannot hold, exact ties among them
    assert (z > 0).any() and (z < 0).any()
    assert (~X.is_bf16(z)).any()
    ties = X.bf16_round_ties_away(z).view(np.uint32) != X.bf16_round(z).view(np.uint32)
    assert ties.any(), "no tie among the outputs"
    print("%s: %d of %d outputs are not bf16 values, %d exact ties" % (shape, int((~X.is_bf16(z)).sum()), z.size, int(ties.sum())))

    def changed(A2=A, W2=W, b2=b):
        return (X.gemm_words(A2, W2, b2, X.ACT_NONE, 0) != plain).any()

    s_last = (K - 1) // 16
    assert changed(A2=drop_k(A, 16 * s_last, 16 * s_last + 16)), "the last 16-wide k step"
    mid = (Kp // 64) // 2
    assert changed(A2=drop_k(A, 64 * mid, 64 * mid + 64)), "a k tile in the middle"
    if M >= 2:  # the clamped row of a ragged panel: the last valid row taken from its neighbour (with one row there is none)
        A2 = np.array(A)
        A2[M - 1] = A2[M - 2]
        assert (X.gemm_words(A2, W, b, X.ACT_NONE, 0)[M - 1] != plain[M - 1]).any(), "the last valid row"
    b2 = np.array(b)
    b2[-1] = 0
    assert changed(b2=b2), "the last column's bias"
    assert (X.bf16_bits(X.bf16_round_ties_away(z)) != words[(X.ACT_NONE, 1)]).any(), "ties away from zero"
    # ReLU epilogues differ from the plain ones (negatives exist), bf16 from f32 ones
    assert (words[(X.ACT_RELU, 0)] != plain).any()
    assert (words[(X.ACT_RELU, 1)] != words[(X.ACT_NONE, 1)]).any()
    # the lattice operands of the sigmoid case: pre-activations multiples of 1/8 in [-6, 6], decoded without ambiguity
    A, W, b = X.gemm_case(M, N, Kp, "lattice")
    X.assert_exact([(A, W, b)])
    zl = A.astype(np.float64) @ W.astype(np.float64).T + b
    assert np.abs(zl).max() <= 6.0 and np.array_equal(np.rint(zl * 8), zl * 8)
    y = X.head(zl, X.ACT_SIGMOID)
    assert np.array_equal(X.lattice(y), (zl * 8).astype(np.int64))
    assert np.array_equal(X.lattice(y.astype(F)), (zl * 8).astype(np.int64))  # ... also after the output's rounding to f32
    if M * N > 1000:
        assert len(np.unique(zl)) > 16


# ---- the whole forwards
def forward_words(name, params=None, x=None, **kw):
    dims, act, bf16, p0, x0, _, _ = X.model_case(name)
    y, z = X.exact_forward(p0 if params is None else params, dims, x0 if x is None else x, act, bf16, **kw)
    return (y.view(np.uint32) if act != X.ACT_SIGMOID else X.lattice(y)), z


@pytest.mark.parametrize("name", list(X.MODELS))
def test_model_cases_satisfy_the_condition_and_the_data_is_sensitive(name):
    dims, act, bf16, params, x, y, z = X.model_case(name)
    L = len(dims) - 1
    layers = X.layer_inputs(params, dims, x, bf16)
    worst = X.assert_exact(layers, operands_bf16=bf16)
    print("%s: sum |a w| + |b| per layer, in quanta: %s" % (name, [int(w) for w in worst]))
    assert max(worst) < X.LIMIT
    # about half of the ReLU outputs are positive; hidden activations bf16 cannot hold, ties among them
    for l in range(L - 1):
        zl = layers[l][3]
        assert 0.2 < (zl > 0).mean() < 0.8, (l, float((zl > 0).mean()))
    base, _ = forward_words(name)
    rows = x.shape[0]
    if act == X.ACT_SIGMOID:
        assert np.abs(z).max() <= 6.0 and np.array_equal(np.rint(z * 8), z * 8) and np.array_equal(base, (z * 8).astype(np.int64))
        assert np.array_equal(X.lattice(y.astype(F)), base)
        assert len(np.unique(base)) > 16
    else:
        assert np.array_equal(y.astype(np.float64), np.maximum(z, 0.0))
    row_sets = {"300-512-512-512-70": (1, 33, 77)}.get(name, (rows,))  # the batches the GPU test runs
    for B in row_sets:
        want = base[:B]

        def changed(params=None, x2=None, **kw):
            got, _ = forward_words(name, params, (x if x2 is None else x2)[:B], **kw)
            return (got != want).any()

        K = dims[0]
        s_last = (K - 1) // 16
        assert changed(x2=drop_k(x, 16 * s_last, 16 * s_last + 16)), (B, "the first layer's last 16-wide k step")
        mid = ((K + 63) // 64) // 2
        assert changed(x2=drop_k(x, 64 * mid, 64 * mid + 64)), (B, "a k tile in the middle of the first layer")
        if B >= 2:
            x2 = np.array(x)
            x2[B - 1] = x2[B - 2]
            assert changed(x2=x2), (B, "the last valid row")
        p2 = np.array(params)
        p2[-1] = 0
        assert params[-1] != 0 and changed(params=p2), (B, "the head's last bias")
        if bf16 and act != X.ACT_SIGMOID:  # (the sigmoid model's values are small: its epilogue is what it is for)
            assert changed(round_fn=X.bf16_round_ties_away), (B, "ties away from zero")
            for l in range(1, L):
                assert changed(skip_round=(l,)), (B, "no rounding of hidden layer %d" % l)
            assert changed(skip_round=(0,)), (B, "no rounding of the input rows")
    if bf16 and act != X.ACT_SIGMOID:
        for l in range(L):
            a = layers[l][0] if l == 0 else np.maximum(layers[l - 1][3], 0.0)
            raw = np.asarray(x if l == 0 else a, F)
            n_off = int((~X.is_bf16(raw)).sum())
            n_tie = int((X.bf16_round_ties_away(raw).view(np.uint32) != X.bf16_round(raw).view(np.uint32)).sum())
            print("%s: layer %d input: max %d, %d values bf16 cannot hold, %d exact ties" % (name, l, int(np.abs(raw).max()), n_off, n_tie))
            assert n_off > 0 and n_tie > 0, l


def test_fp32_storage_cases_differ_from_their_bf16_twins():
    for name in ("304-256-256-256-152", "88-48-32-44"):
        a, b = X.model_case(name), X.model_case(name + " f32")
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        assert (a[5].view(np.uint32) != b[5].view(np.uint32)).any()
