"""The paths on which the host side lets go of device resources and takes new ones: an evaluator's buffers regrown for a larger
batch, in fp32 and in bf16 storage (whose own buffers come with the first switch), and engines of every tier created, run and
destroyed one after another in one process.  A resource released too early or twice shows as a HIP error status of a later call."""
import ctypes as C

import numpy as np
import pytest

from gpu_parity import az  # noqa: F401
from test_gpu_engine_tiers import TIERS, TOL, make_space

pytestmark = pytest.mark.gpu

N, HIDDEN, SEED, SMALL, LARGE = 8, (32, 32), 0, 16, 64
F32, BF16 = 0, 1  # AZD_STORAGE_*


def model(az, batch, dtype="f32"):
    space = az.ROTModifyParentsOnce(N)
    return az.ActionModel(batch, space.STATE_DIM, space.ACTION_DIM, hidden=HIDDEN, seed=SEED, dtype=dtype)


def predictions(m, rows=LARGE):
    x = np.random.default_rng(7).random((rows, m.state_dim), dtype=np.float32)
    p = np.zeros((rows, m.action_dim), np.float32)
    m.write_predictions(x, p)
    assert np.isfinite(p).all() and p.any()
    return p.view(np.uint32)


def set_storage(az, m, dtype):
    from azdopt_amd import _lib
    _lib.check(_lib.lib().azd_evaluator_set_weight_storage(m._h, dtype), "azd_evaluator_set_weight_storage")


def test_fp32_model_regrown_for_a_larger_batch_equals_one_built_for_it(az):
    """built for 16 rows, asked for 64 (azd_evaluator_write_predictions: ensure_batch above the constructor's batch)"""
    grown, whole = model(az, SMALL), model(az, LARGE)
    assert np.array_equal(predictions(grown, SMALL), predictions(whole, SMALL))
    assert np.array_equal(predictions(grown), predictions(whole))
    assert np.array_equal(predictions(grown, SMALL), predictions(whole, SMALL))  # (and the regrown buffers serve a smaller batch)


def test_bf16_buffers_of_the_first_switch_then_regrown_equal_a_fresh_bf16_model(az):
    """fp32 -> bf16 -> fp32 -> bf16 on one model built for 16 rows (the bf16 buffers come with the first switch and stay), then
    64 rows in bf16: bit-equal to a model created in bf16 for 64 rows"""
    m = model(az, SMALL)
    f32_rows = predictions(m, SMALL)
    for dtype in (F32, BF16, F32):
        set_storage(az, m, dtype)
    assert np.array_equal(predictions(m, SMALL), f32_rows)
    set_storage(az, m, BF16)
    fresh = model(az, LARGE, dtype="bf16")
    assert np.array_equal(predictions(m, SMALL), predictions(fresh, SMALL))
    got = predictions(m)
    assert np.array_equal(got, predictions(fresh))
    assert not np.array_equal(got, predictions(model(az, LARGE)))  # (bf16 storage is in force: not the fp32 model's bits)


def run_engine(az, tier):
    """one engine of a tier at the smallest shapes, two calls: what it found, then its destruction (status checked)"""
    if tier == "ramsey_u64_big":
        space = az.RamseySpaceNoEdgeRecolor(6, [3, 3], max_slots=15, u64=True, big_cliques=True)
    else:
        space = make_space(az, tier)
    B = 16
    hidden = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, 1)
    opt = az.NablaOptimizer.par_new(space, space.generate_roots(1, B), hidden, B, node_capacity=256)
    for _ in range(2):
        opt.par_roll_out_episodes(TOL, n_calls=1)
    ctr = opt.counters()
    assert ctr["FAILED"] == 0
    trees = [opt.get_tree(i) for i in (0, B - 1)]
    out = (sorted(ctr.items()), [[getattr(t, f).tobytes() for f in t.FIELDS] for t in trees])
    assert opt._L.azd_engine_destroy(opt._h) == 0
    opt._h = C.c_void_p()
    return out


@pytest.mark.parametrize("tier", TIERS + ("ramsey_u64_big",))
def test_three_engines_of_a_tier_one_after_another_find_the_same(az, tier):
    first = run_engine(az, tier)
    for _ in range(2):
        assert run_engine(az, tier) == first, tier
