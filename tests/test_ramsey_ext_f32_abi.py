"""AZD_ENGINE_EXT_POOL_F32 (the searcher-only pool step of the Ramsey tiers with an fp32 model) on the host side: the flag in the
header and the binding, the debug entry of the gathered forward, which configurations azd_engine_create and azd_debug_ext_pool_plan
take and refuse with it, the unchanged LDS plan, and the Python option.  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

from test_ramsey_ext_pool_abi import INVALID, OK, R45, config, create

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, EXT, F32 = 16, 64, 128
R3333 = dict(n=34, n_colors=4, clique_sizes=[3, 3, 3, 3], max_slots=30)
BOTH = [dict(flags=EXT | F32, **R45), dict(flags=EXT | F32 | U64, **R45), dict(flags=EXT | F32 | U64, **R3333)]
ALONE = [dict(flags=F32, **R45), dict(flags=F32 | U64, **R45), dict(flags=F32 | U64, **R3333)]


def test_the_flag_and_the_debug_entry_are_declared_and_bound():
    import azdopt_amd as az
    from azdopt_amd import _lib
    text = open(os.path.join(ROOT, "include", "azdopt_amd.h")).read()
    assert re.search(r"#define AZD_ENGINE_EXT_POOL_F32 128u", text)
    assert "azd_debug_write_predictions_gathered" in text
    assert _lib.ENGINE_EXT_POOL_F32 == 128
    assert C.sizeof(_lib.EngineConfig) == 96  # the flag changes nothing in the struct's layout
    assert hasattr(C.CDLL(az._lib.LIB_PATH), "azd_debug_write_predictions_gathered")
    assert hasattr(az.ActionModel, "debug_write_predictions_gathered")


def test_both_flags_are_accepted_on_both_tiers():
    for kw in BOTH:
        st, err = create(**kw)
        assert st in OK, (kw, err)


def test_the_flag_alone_is_refused_and_both_flags_are_named():
    import azdopt_amd as az
    L = az.lib()
    for kw in ALONE:
        st, err = create(**kw)
        assert st == INVALID, (kw, st, err)
        assert "AZD_ENGINE_EXT_POOL_F32" in err and "AZD_ENGINE_EXT_POOL_STEP" in err, (kw, err)
        cfg = config(**kw)
        assert L.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(C.c_int32()), C.byref(C.c_size_t())) == INVALID, kw
        err = L.azd_last_error().decode()
        assert "AZD_ENGINE_EXT_POOL_F32" in err and "AZD_ENGINE_EXT_POOL_STEP" in err, (kw, err)


def test_the_lds_plan_is_that_of_the_first_flag_alone():
    import azdopt_amd as az
    L = az.lib()
    for kw in BOTH:
        plans = []
        for flags in (kw["flags"], kw["flags"] & ~F32):
            cfg = config(**dict(kw, flags=flags))
            waves, lds = C.c_int32(), C.c_size_t()
            assert L.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0, (kw, flags, L.azd_last_error().decode())
            plans.append((waves.value, lds.value))
        assert plans[0] == plans[1] and plans[0][0] >= 8, (kw, plans)  # the searchers are the same: same waves, same bytes


def test_par_new_takes_ext_pool_f32():
    import azdopt_amd as az
    assert "ext_pool_f32" in inspect.signature(az.NablaOptimizer.__init__).parameters
    space = az.ROTModifyParentsOnce(19)
    # (both options reach azd_engine_create, which refuses them on c21 before any device is touched)
    with pytest.raises(az._lib.AzdError) as ei:
        az.NablaOptimizer.par_new(space, space.generate_roots(0, 4), None, 4, ext_pool_step=True, ext_pool_f32=True)
    assert ei.value.status == INVALID and "AZD_ENGINE_EXT_POOL_STEP" in str(ei.value)
    # alone it reaches the engine too, whose refusal names both flags
    with pytest.raises(az._lib.AzdError) as ei:
        az.NablaOptimizer.par_new(space, space.generate_roots(0, 4), None, 4, ext_pool_f32=True)
    assert ei.value.status == INVALID and "AZD_ENGINE_EXT_POOL_F32" in str(ei.value) and "AZD_ENGINE_EXT_POOL_STEP" in str(ei.value)
