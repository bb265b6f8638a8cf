"""Every implementation of the bf16 evaluator forward against the exact integer reference (tests/bf16_exact.py), word for word:
with integer-valued operands whose sums stay below 2^24 quanta every f32 partial sum is exact in every accumulation order, so a
word that differs is a kernel or staging error, never noise.  No tolerance anywhere; the sigmoid cases decode the 1/8 lattice
their pre-activations lie on.

  a  k_gemm16 alone (azd_debug_gemm_bf16): the four tile forms (AZD_GEMM16_BN 64 / 128 two LDS buffers, 1064 / 1128 one; unset:
     the shape rule's one-buffer 64-wide form), M, N and k-tile edges, the XCD swizzle with a short last group, five epilogues
  b  the whole forward of a bf16 ActionModel: forward16 (k_rows_to_bf16, k_gemm16, k_hidden2_fused or one launch per layer),
     split-k (k_gemm16 partial sums + k_splitk_finish) under each long-k form, AZD_GEMM_OLD (k_gemm_bf16<1>, <2>, the generic
     k_gemm with k_round_bf16)
  c  the gathered forward (k_gemm16<.., EXT>, k_hidden2_fused<EXT>, split-k with the row count in device memory)
  d  the in-kernel tile task of the pool / asynchronous step (debug_tile_forward), bf16 and fp32 storage"""
import ctypes as C

import numpy as np
import pytest
import torch  # (before the package loads its library: one HIP runtime in the process, torch's)

import bf16_exact as X
from gpu_parity import az  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
SENT32 = np.uint32(0x7FC0ABCD)  # a quiet NaN with a payload: an untouched f32 word
SENT16 = np.uint16(0x7FC1)      # ... an untouched bf16 word
TOL = ([200, 50, 50], 25)


def diff_report(got, want, what):
    """the words that differ, by index: which row panel, column tile"""
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return ""
    r, c = bad[0]
    return "%s: %d of %d words differ; first at row %d col %d: got %#x want %#x; rows %d..%d cols %d..%d" % (
        what, len(bad), want.size, r, c, int(got[r, c]), int(want[r, c]), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())


# ---- a. k_gemm16 in isolation
def device_gemm(az, A16, W16, bias, M, N, Kp, act, out_bf16, ldy):
    """Y [M + 1][ldy] as words: the GEMM's output in the first M rows and N columns, the sentinel elsewhere"""
    from azdopt_amd import _lib
    if out_bf16:
        y = torch.from_numpy(np.full((M + 1, ldy), SENT16, np.uint16).view(np.int16)).view(torch.bfloat16).cuda()
    else:
        y = torch.from_numpy(np.full((M + 1, ldy), SENT32, np.uint32).view(F)).cuda()
    ms = C.c_float()
    _lib.check(_lib.lib().azd_debug_gemm_bf16(0, M, N, Kp, C.c_void_p(A16.data_ptr()), C.c_void_p(W16.data_ptr()), C.c_void_p(bias.data_ptr()),
                                              C.c_void_p(y.data_ptr()), ldy, int(out_bf16), act, 1, C.byref(ms)), "azd_debug_gemm_bf16")
    torch.cuda.synchronize()
    if out_bf16:
        return y.cpu().view(torch.int16).numpy().view(np.uint16)
    return y.cpu().numpy().view(np.uint32)


def to_device_bf16(a):
    assert X.is_bf16(a).all()
    return torch.from_numpy(X.bf16_bits(a).view(np.int16)).view(torch.bfloat16).cuda()


@pytest.mark.parametrize("shape", X.GEMM_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("form", [None, "64", "128", "1064", "1128"])
def test_gemm16_alone_gives_the_exact_words(az, monkeypatch, form, shape):
    M, N, Kp = shape
    if form is not None:
        monkeypatch.setenv("AZD_GEMM16_BN", form)
    ldy = N + 3
    A, W, b = X.gemm_case(M, N, Kp, "wide")
    X.assert_exact([(A, W, b)])
    A16, W16, bias = to_device_bf16(A), to_device_bf16(W), torch.from_numpy(np.array(b)).cuda()
    for act, out_bf16 in ((X.ACT_NONE, 0), (X.ACT_RELU, 0), (X.ACT_NONE, 1), (X.ACT_RELU, 1)):
        got = device_gemm(az, A16, W16, bias, M, N, Kp, act, out_bf16, ldy)
        want = X.gemm_words(A, W, b, act, out_bf16)
        what = "form %s, %s, act %d, %s out" % (form, shape, act, "bf16" if out_bf16 else "f32")
        assert np.array_equal(got[:M, :N], want), diff_report(got[:M, :N], want, what)
        sent = SENT16 if out_bf16 else SENT32
        assert (got[:M, N:] == sent).all(), what + ": a column at or beyond N was written"
        assert (got[M] == sent).all(), what + ": the row after M was written"
    # the sigmoid head: pre-activations on the 1/8 lattice in [-6, 6]; neighbouring lattice values are >= 0.125 sigma'(6) = 3.1e-4
    # apart in y and g16_sigmoid is good to ~3e-7 relative, so the decode is unambiguous and needs no tolerance
    A, W, b = X.gemm_case(M, N, Kp, "lattice")
    X.assert_exact([(A, W, b)])
    z = A.astype(np.float64) @ W.astype(np.float64).T + b
    assert np.abs(z).max() <= 6.0
    got = device_gemm(az, to_device_bf16(A), to_device_bf16(W), torch.from_numpy(np.array(b)).cuda(), M, N, Kp, X.ACT_SIGMOID, 0, ldy)
    y = got[:M, :N].view(F)
    assert np.isfinite(y).all() and (y > 0).all() and (y < 1).all()
    print("form %s, %s: sigmoid head, largest |y - sigma_64| = %.3g" % (form, shape, np.abs(y - X.head(z, X.ACT_SIGMOID)).max()))
    want = np.rint(z * 8).astype(np.int64)
    assert np.array_equal(X.lattice(y), want), diff_report(X.lattice(y), want, "form %s, %s, sigmoid" % (form, shape))
    assert (got[:M, N:] == SENT32).all() and (got[M] == SENT32).all()


# ---- b. the whole forward of a bf16 ActionModel
def model_of(az, name, rows=None):
    dims, act, bf16, params, x, y, z = X.model_case(name)
    X.assert_exact(X.layer_inputs(params, dims, x, bf16), operands_bf16=bf16)
    B = x.shape[0] if rows is None else rows
    m = az.ActionModel(B, dims[0], dims[-1], hidden=dims[1:-1], final_act=act, seed=1, dtype="bf16" if bf16 else "f32")
    m.set_params(np.array(params))
    return m, dims, act, np.array(x[:B]), y[:B], z[:B]


def check_forward(az, name, rows=None, what=""):
    m, dims, act, x, y, z = model_of(az, name, rows)
    got = np.full((x.shape[0], dims[-1]), SENT32, np.uint32).view(F)
    m.write_predictions(x, got)
    want = y.view(np.uint32)
    assert np.array_equal(got.view(np.uint32), want), diff_report(got.view(np.uint32), want, "%s %s" % (name, what))
    return got


@pytest.mark.parametrize("name", ["37-40-33", "133-96-70-45"])
def test_forward16_gives_the_exact_words(az, name):
    check_forward(az, name)


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("B", [1, 33, 77])
def test_fused_hidden_pair_and_layer_by_layer_each_give_the_exact_words(az, monkeypatch, B, fuse):
    """k_hidden2_fused (AZD_MLP_FUSE_HIDDEN unset or 1) and one k_gemm16 launch per 512-wide layer (0): each equals the reference,
    not merely the other; batches of one row, one panel and a row, two panels and a ragged third"""
    monkeypatch.setenv("AZD_MLP_FUSE_HIDDEN", fuse)
    check_forward(az, "300-512-512-512-70", B, "fuse " + fuse)


@pytest.mark.parametrize("form", [None, "128", "1064"])
@pytest.mark.parametrize("slices", ["2", "4", "8"])
def test_split_k_gives_the_exact_words(az, monkeypatch, slices, form):
    """Kp = 1152 = 18 k tiles dealt to 2 / 4 / 8 blocks per output tile (9 + 9; 4 + 5 + 4 + 5; 2 and 3), partial sums added by
    k_splitk_finish; under the shape rule's two-buffer 64-wide form, the two-buffer 128-wide one and the one-buffer 64-wide one"""
    monkeypatch.setenv("AZD_GEMM16_KSPLIT", slices)  # (before the model is created: it sizes the partial-sum buffer)
    if form:
        monkeypatch.setenv("AZD_GEMM16_LONGK_FORM", form)
    check_forward(az, "1100-96-45", None, "ksplit %s form %s" % (slices, form))


@pytest.mark.parametrize("name,small_below", [("132-96-68-44", None), ("132-96-68-44", "0"), ("37-40-33", None)])
def test_the_older_gemm_paths_give_the_same_exact_words(az, monkeypatch, name, small_below):
    """AZD_GEMM_OLD=1: all widths multiples of 4 -> k_gemm_bf16<1> (64 x 128 tiles), with AZD_GEMM_SMALL_BELOW=0 (read when the
    model is created) k_gemm_bf16<2> (128 x 128); other widths -> the generic k_gemm over k_round_bf16's rows.  'The same sums,
    bit for bit' as k_gemm16: all equal the one reference."""
    if small_below is not None:
        monkeypatch.setenv("AZD_GEMM_SMALL_BELOW", small_below)
    new = check_forward(az, name, None, "default path")
    monkeypatch.setenv("AZD_GEMM_OLD", "1")
    old = check_forward(az, name, None, "AZD_GEMM_OLD small_below %s" % small_below)
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))


def test_forward16_sigmoid_head_decodes_to_the_exact_lattice(az):
    m, dims, act, x, y, z = model_of(az, "37-40-33 sigmoid")
    assert act == X.ACT_SIGMOID and np.abs(z).max() <= 6.0
    got = np.zeros((x.shape[0], dims[-1]), F)
    m.write_predictions(x, got)
    assert (got > 0).all() and (got < 1).all()
    print("37-40-33 sigmoid: largest |y - sigma_64| = %.3g" % np.abs(got - y).max())
    want = np.rint(z * 8).astype(np.int64)
    assert np.array_equal(X.lattice(got), want), diff_report(X.lattice(got), want, "sigmoid head")


# ---- c. the gathered bf16 forward
ROWS = 80


def row_lists():
    perm = np.random.default_rng(11).permutation(ROWS).astype(np.uint32)
    return {"empty": np.zeros(0, np.uint32), "one": np.array([57], np.uint32), "31": np.arange(31, dtype=np.uint32) + 3,
            "32": np.arange(32, dtype=np.uint32) + 40, "33 permuted": perm[:33].copy(), "80 permuted": perm,
            "20 with gaps": np.arange(79, -1, -4, dtype=np.uint32)}


GATHERED = [("133-96-70-45", None, None), ("1100-512-512-512-70", None, None), ("1100-512-512-512-70", "64", None),
            ("1100-512-512-512-70", "128", None), ("1100-512-512-512-70", "1064", None), ("1100-512-512-512-70", "1128", None),
            ("1100-512-512-512-70", None, "4")]


@pytest.mark.parametrize("name,form,slices", GATHERED)
def test_gathered_forward_writes_the_exact_words_into_the_named_rows_only(az, monkeypatch, name, form, slices):
    """debug_write_predictions_gathered on a bf16 model: k_gemm16<.., EXT> with rows_in on the first layer, rows_out on the head and
    the count in device memory; the second model adds k_hidden2_fused<EXT> and a long-k first layer whose form the knob picks (the
    launcher sizes the form for a quarter of max_rows on half the chip: at 80 rows the 128-wide EXT instantiations are reached
    only so), and the split-k EXT partial sums with k_splitk_finish reading the count"""
    if form:
        monkeypatch.setenv("AZD_GEMM16_LONGK_FORM", form)
    if slices:
        monkeypatch.setenv("AZD_GEMM16_KSPLIT", slices)
    m, dims, act, x, y, z = model_of(az, name)
    assert x.shape[0] == ROWS
    want = y.view(np.uint32)
    for tag, rows in row_lists().items():
        p = np.full((ROWS, dims[-1]), SENT32, np.uint32).view(F)
        m.debug_write_predictions_gathered(rows, x, p, max_rows=ROWS)
        got = p.view(np.uint32)
        named = np.zeros(ROWS, bool)
        named[rows] = True
        assert named.sum() == len(rows)
        what = "%s form %s ksplit %s, list %s" % (name, form, slices, tag)
        assert np.array_equal(got[named], want[named]), diff_report(got[named], want[named], what)
        assert (got[~named] == SENT32).all(), what + ": a row no list names was written"


# ---- d. the in-kernel tile task
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("name,n", [("304-256-256-256-152", 19), ("88-48-32-44", 11), ("304-256-256-256-152 f32", 19), ("88-48-32-44 f32", 11)])
def test_tile_task_gives_the_exact_words(az, name, n, pool):
    """mlp_tile_task through debug_tile_forward on 100 integer-valued rows that are no state vectors (k_tile_forward's staging, the
    fragment-major weights, 16-wide ragged fragments at N = 11): bf16 storage against the reference with its roundings, fp32 storage
    (an fmaf chain in k order: exact inputs give exact sums) against the same integers without them.  The engine is built after
    set_params and then runs a call of its own step form: the in-kernel evaluator exists for this model and served it."""
    space = az.ROTModifyParentsOnce(n)
    B = 72
    model, dims, act, x, y, z = model_of(az, name, B)
    x, y = X.model_case(name)[4], X.model_case(name)[5]  # (all 100 rows: the tile forward takes any number)
    assert (space.STATE_DIM, space.ACTION_DIM) == (dims[0], dims[-1]) and x.shape[0] == 100
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(3, B), model, B, pool_step=pool)
    got = opt.debug_tile_forward(x).view(np.uint32)
    want = y.view(np.uint32)
    assert np.array_equal(got, want), diff_report(got, want, "%s pool_step=%s" % (name, pool))
    opt.par_roll_out_episodes(TOL, n_calls=2)
    assert opt.step_form()[0] == ("pool" if pool else "async"), opt.step_form()
    assert opt.counters()["EVAL_ROWS"] > 0
