"""The gathered fp32 GEMM (k_gemm_f32_gathered, gemm_f32_gathered.inc: the evaluator of the searcher-only pool step under
AZD_ENGINE_EXT_POOL_F32) in isolation, through azd_debug_write_predictions_gathered on an fp32 ActionModel: the rows a list names
receive the BITS write_predictions gives them in a whole-batch forward (the same f32 FMA chain in k order, the same epilogue), every
other row of the prediction array keeps its bits, whichever rows share a tile.  Models with K and N that are no multiples of the k
tile or of 32, an odd pitch (rows that are not 16-byte aligned), both head activations; lists that are empty, one row, cross a
32-row tile, permute all rows, or leave gaps."""
import numpy as np
import pytest

import mlp_f64 as M
from gpu_parity import az  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = 80
SENTINEL = np.uint32(0x7FC0ABCD)  # a quiet NaN with a payload: an untouched prediction word
MODELS = {"37-40-33 sigmoid": ((37, 40, 33), M.ACT_SIGMOID), "64-64-64 relu": ((64, 64, 64), M.ACT_RELU),
          "133-96-70-45 sigmoid": ((133, 96, 70, 45), M.ACT_SIGMOID)}


def row_lists():
    perm = np.random.default_rng(11).permutation(ROWS).astype(np.uint32)
    return {"empty": np.zeros(0, np.uint32), "one": np.array([57], np.uint32), "31": np.arange(31, dtype=np.uint32) + 3,
            "32": np.arange(32, dtype=np.uint32) + 40, "33": perm[:33].copy(), "80 permuted": perm,
            "20 with gaps": np.arange(79, -1, -4, dtype=np.uint32)}


@pytest.fixture(scope="module")
def cases(az):
    """per model: the model, its 80 state rows and the whole-batch forward (computed once, never written again)"""
    out = {}
    for i, (tag, (dims, act)) in enumerate(MODELS.items()):
        model = az.ActionModel(ROWS, dims[0], dims[-1], hidden=dims[1:-1], final_act=act, seed=20 + i)
        x = np.random.default_rng(5 + i).standard_normal((ROWS, dims[0])).astype(np.float32)
        full = np.zeros((ROWS, dims[-1]), np.float32)
        model.write_predictions(x, full)
        assert np.isfinite(full).all()
        full.setflags(write=False)
        out[tag] = (model, dims, act, x, full)
    return out


def gathered(model, dims, x, rows):
    p = np.full((ROWS, dims[-1]), SENTINEL, np.uint32).view(np.float32)
    model.debug_write_predictions_gathered(rows, x, p, max_rows=ROWS)
    return p.view(np.uint32)


@pytest.mark.parametrize("rows_tag", list(row_lists()))
@pytest.mark.parametrize("tag", list(MODELS))
def test_named_rows_get_the_whole_batch_bits_and_the_others_are_left(cases, tag, rows_tag):
    model, dims, act, x, full = cases[tag]
    rows = row_lists()[rows_tag]
    got = gathered(model, dims, x, rows)
    want = full.view(np.uint32)
    named = np.zeros(ROWS, bool)
    named[rows] = True
    assert named.sum() == len(rows)
    diff = got[named] != want[named]
    print("%s, %s: %d of %d words of the named rows differ" % (tag, rows_tag, int(diff.sum()), diff.size))
    assert not diff.any()
    assert (got[~named] == SENTINEL).all()


@pytest.mark.parametrize("tag", list(MODELS))
def test_a_row_has_the_same_bits_whichever_rows_share_its_tile(cases, tag):
    model, dims, act, x, full = cases[tag]
    lists = row_lists()
    rows = lists["33"]
    alone, among = gathered(model, dims, x, rows), gathered(model, dims, x, lists["80 permuted"])
    assert np.array_equal(alone[rows], among[rows])


def test_outputs_against_the_float64_forward(cases):
    """37-40-33 against tests/mlp_f64.py within the project's fp32 tolerance on sigmoid outputs, 2e-5 absolute"""
    model, dims, act, x, full = cases["37-40-33 sigmoid"]
    got = gathered(model, dims, x, row_lists()["80 permuted"]).view(np.float32)
    p64 = M.forward(model.get_params(), dims, x, act).numpy()
    err = np.abs(got.astype(np.float64) - p64).max()
    print("gathered fp32 forward 37-40-33 against float64: max |err| %.3g" % err)
    assert err <= 2e-5, err
