"""AZD_ENGINE_EXT_POOL_F32 on the dense-graph space, on the host side.  The space's pool step is the searcher-only form and needs no
flag of its own, so there the flag stands alone, on all three tiers (default cost, AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE):
which configurations azd_engine_create takes and refuses with it, the LDS plan it leaves as it was, and the Python option.
No GPU needed.

The plan without the flag is read from azd_debug_ext_pool_plan only where that entry gives one: on the wide tier.  For the other two
tiers the entry refuses a configuration without the flag (tests/test_dense_ah_wide_abi.py pins that), so there the flagged plan is
held to the waves the tiers are built for and to the flagged plan of the same shape at another batch and with AZD_ENGINE_POOL_STEP
set -- the plan reads the shape alone."""
import ctypes as C

import pytest

from test_ramsey_ext_pool_abi import INVALID, OK, R45, config, create

NO_PERSISTENT, POOL, AH, EXT, F32, WIDE = 1, 8, 32, 64, 128, 256
DENSE = 3  # AZD_SPACE_DENSE
TIERS = [dict(space_id=DENSE, n=20, max_slots=64, flags=F32),
         dict(space_id=DENSE, n=31, max_slots=128, flags=F32 | AH),
         dict(space_id=DENSE, n=50, max_slots=128, flags=F32 | AH | WIDE)]


def plan(**kw):
    import azdopt_amd as az
    L = az.lib()
    cfg = config(**kw)
    waves, lds = C.c_int32(), C.c_size_t()
    st = L.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds))
    return st, (waves.value, lds.value), L.azd_last_error().decode()


def test_the_flag_alone_is_accepted_on_the_three_dense_tiers():
    from azdopt_amd import _lib
    assert (_lib.SPACE_DENSE, _lib.ENGINE_EXT_POOL_F32, _lib.ENGINE_DENSE_AH, _lib.ENGINE_DENSE_AH_WIDE) == (DENSE, F32, AH, WIDE)
    for kw in TIERS:
        st, err = create(**kw)
        assert st in OK, (kw, st, err)
        st, err = create(**dict(kw, flags=kw["flags"] | POOL))  # ... and beside the flag that forces the pool step below 256 agents
        assert st in OK, (kw, st, err)


def test_what_was_refused_is_still_refused_and_named():
    from azdopt_amd import _lib
    # alone on c21 and on r45 (both of its tiers): both flags named, as before
    for kw in (dict(flags=F32, space_id=_lib.SPACE_C21, n=19), dict(flags=F32, **R45), dict(flags=F32 | 16, **R45)):
        st, err = create(**kw)
        assert st == INVALID, (kw, st, err)
        assert "AZD_ENGINE_EXT_POOL_F32" in err and "AZD_ENGINE_EXT_POOL_STEP" in err, (kw, err)
    # the Ramsey form's flag on the dense space, with and without the fp32 flag beside it
    for kw in TIERS:
        for flags in (kw["flags"] | EXT, (kw["flags"] | EXT) & ~F32):
            st, err = create(**dict(kw, flags=flags))
            assert st == INVALID and "AZD_ENGINE_EXT_POOL_STEP" in err, (kw, flags, st, err)
    # beside the flag that rules every CU-resident form out: refused, both flags named
    for kw in TIERS:
        st, err = create(**dict(kw, flags=kw["flags"] | NO_PERSISTENT))
        assert st == INVALID, (kw, st, err)
        assert "AZD_ENGINE_EXT_POOL_F32" in err and "AZD_ENGINE_NO_PERSISTENT_STEP" in err, (kw, err)
        st, _, err = plan(**dict(kw, flags=kw["flags"] | NO_PERSISTENT))
        assert st == INVALID and "AZD_ENGINE_NO_PERSISTENT_STEP" in err, (kw, st, err)


def test_the_lds_plan_does_not_know_the_flag():
    plans = []
    for kw in TIERS:
        st, p, err = plan(**kw)
        assert st == 0, (kw, st, err)
        assert 0 < p[1] <= 160 * 1024, (kw, p)
        # the shape alone decides: another population, the pool step forced
        st, q, err = plan(**dict(kw, batch=4096, flags=kw["flags"] | POOL))
        assert st == 0 and q == p, (kw, p, q, err)
        plans.append(p)
    assert [p[0] for p in plans] == [16, 10, 6], plans  # the waves the three tiers' searcher workgroups have at these shapes
    # the wide tier's plan can be read without the flag: identical
    st, p, err = plan(**dict(TIERS[2], flags=AH | WIDE))
    assert st == 0 and p == plans[2], (p, plans[2], err)
    # the narrower waves of the AH tier at its wider keys: 9 and 7, with the flag as the bf16 engines run them
    assert [plan(**dict(TIERS[1], max_slots=ms))[1][0] for ms in (128, 256, 465)] == [10, 9, 7]


def test_par_new_takes_ext_pool_f32_on_the_dense_space():
    import azdopt_amd as az
    space = az.DenseGraphSpace(20, max_slots=64)
    roots = space.generate_roots(0, 4)
    if az.device_count() > 0:
        az.NablaOptimizer.par_new(space, roots, az.TrivialModel(space.STATE_DIM, space.ACTION_DIM), 4, ext_pool_f32=True)
        return
    with pytest.raises(az._lib.AzdError) as ei:  # past check_engine_config: no device is the first thing in the way
        az.NablaOptimizer.par_new(space, roots, None, 4, ext_pool_f32=True)
    assert ei.value.status == 2, str(ei.value)
    with pytest.raises(az._lib.AzdError) as ei:
        az.NablaOptimizer.par_new(space, roots, None, 4, ext_pool_f32=True, persistent=False)
    assert ei.value.status == INVALID and "AZD_ENGINE_NO_PERSISTENT_STEP" in str(ei.value)
