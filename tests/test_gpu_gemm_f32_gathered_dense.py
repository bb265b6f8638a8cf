"""The gathered fp32 GEMM (k_gemm_f32_gathered, gemm_f32_gathered.inc) at the dense-graph space's shapes, in isolation through
azd_debug_write_predictions_gathered on an fp32 ActionModel -- the evaluator of the space's pool step under AZD_ENGINE_EXT_POOL_F32.
tests/test_gpu_gemm_f32_gathered.py holds the kernel to its contract at the Ramsey tiers' shapes and on normal rows; the dense space
brings
  * S = 3 E + 1, a multiple of 4 only when E = 1 (mod 4): N = 31 (1396) and N = 50 (3676) take the 16-byte loads, N = 8 (85), N = 20
    (571) and N = 33 (1585) one float per lane and load;
  * rows of zeros and ones -- about a fifth set, as G(n, 0.2) gives them -- with a last entry k / E;
  * heads from 56 columns (less than half a block's 128) to 2450 (twenty column tiles, the last one 18 wide).
Every row a list names receives the BITS write_predictions gives it in a whole-batch forward, every other row keeps its bits: lists
of 1, 31, 32, 33 and 200 rows in shuffled order, in a launch sized for 256."""
import numpy as np
import pytest

from gpu_parity import az  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = 256  # state rows and max_rows: more than any list
SENTINEL = np.uint32(0x7FC0ABCD)  # a quiet NaN with a payload: an untouched prediction word
# (state_dim, action_dim) of N = 8, 20, 31, 33, 50 and the hidden widths the tests and drivers run them with
SHAPES = {(85, 56): (64, 32), (571, 380): (256, 128), (1396, 930): (256, 128), (1585, 1056): (256, 128), (3676, 2450): (512, 512, 512)}
LENGTHS = (1, 31, 32, 33, 200)


def dense_rows(rng, state_dim):
    """rows as DenseSpace::write_rows_direct writes them: E edge bits, 2 E more 0/1 entries, then k / E"""
    E = (state_dim - 1) // 3
    assert 3 * E + 1 == state_dim
    x = (rng.random((ROWS, state_dim)) < 0.2).astype(np.float32)
    x[:, -1] = (rng.integers(0, E + 1, ROWS).astype(np.float32) / np.float32(E))
    return x


def row_list(length):
    return np.random.default_rng(100 + length).permutation(ROWS)[:length].astype(np.uint32)


@pytest.fixture(scope="module")
def cases(az):
    """per shape: the model, its 256 state rows and the whole-batch forward (computed once, never written again)"""
    out = {}
    for i, ((sd, ad), hidden) in enumerate(SHAPES.items()):
        model = az.ActionModel(ROWS, sd, ad, hidden=hidden, seed=40 + i)
        x = dense_rows(np.random.default_rng(9 + i), sd)
        full = np.zeros((ROWS, ad), np.float32)
        model.write_predictions(x, full)
        assert np.isfinite(full).all() and len(np.unique(full[:, 0])) > ROWS // 2  # (rows that tell each other apart)
        full.setflags(write=False)
        x.setflags(write=False)
        out[(sd, ad)] = (model, x, full)
    return out


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=["%d-%d" % s for s in SHAPES])
def test_named_rows_get_the_whole_batch_bits_and_the_others_are_left(cases, shape, length):
    model, x, full = cases[shape]
    rows = row_list(length)
    p = np.full((ROWS, shape[1]), SENTINEL, np.uint32).view(np.float32)
    model.debug_write_predictions_gathered(rows, x, p, max_rows=ROWS)
    got, want = p.view(np.uint32), full.view(np.uint32)
    named = np.zeros(ROWS, bool)
    named[rows] = True
    assert named.sum() == length
    diff = got[named] != want[named]
    print("%s, %d rows: %d of %d words of the named rows differ" % (shape, length, int(diff.sum()), diff.size))
    assert not diff.any()
    assert (got[~named] == SENTINEL).all()
