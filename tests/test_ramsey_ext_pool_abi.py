"""The searcher-only pool step of the Ramsey tiers with max_slots > 0 (AZD_ENGINE_EXT_POOL_STEP) on the host side: the flag in the
header and the binding, which configurations azd_engine_create takes and refuses with it, the Python option, and the LDS plan of a
searcher workgroup (azd_debug_ext_pool_plan: arithmetic, no device).  No GPU needed."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OK = (0, 2)  # created, or "no gfx950 device" on a CPU-only box
NO_PERSISTENT, U64, EXT = 1, 16, 64

R45 = dict(n=24, n_colors=2, clique_sizes=[4, 5], max_slots=276)
ACCEPTED = [dict(flags=EXT, **R45),                                                          # r45, 32-bit wide tier
            dict(flags=EXT | U64, **R45),                                                    # the same on the 64-bit tier
            dict(flags=EXT | U64, n=34, n_colors=4, clique_sizes=[3, 3, 3, 3], max_slots=30),  # r3333
            dict(flags=EXT | U64, n=48, n_colors=2, clique_sizes=[4, 5], max_slots=512)]
PLANNED = ACCEPTED + [dict(flags=EXT, n=32, n_colors=2, clique_sizes=[4, 4], max_slots=496),          # the wide tier's largest rows
                      dict(flags=EXT | U64, n=39, n_colors=3, clique_sizes=[3, 3, 4], max_slots=100),
                      dict(flags=EXT | U64, n=33, n_colors=2, clique_sizes=[3, 4], max_slots=264)]


def config(**kw):
    from azdopt_amd import _lib
    cfg = _lib.EngineConfig()
    cfg.space_id, cfg.batch = _lib.SPACE_RAMSEY, 8
    for i in range(4):
        cfg.color_weights[i] = 1.0
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            arr = getattr(cfg, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(cfg, k, v)
    return cfg


def refused_configs():
    from azdopt_amd import _lib
    return [("c21", dict(flags=EXT, space_id=_lib.SPACE_C21, n=19)),
            ("dense", dict(flags=EXT, space_id=_lib.SPACE_DENSE, n=20, max_slots=64)),
            ("narrow Ramsey", dict(flags=EXT, n=17, n_colors=2, clique_sizes=[4, 4], max_slots=0)),
            ("with NO_PERSISTENT_STEP", dict(flags=EXT | U64 | NO_PERSISTENT, n=34, n_colors=4, clique_sizes=[3, 3, 3, 3], max_slots=30))]


def create(**kw):
    import azdopt_amd as az
    L = az.lib()
    cfg = config(**kw)
    h = C.c_void_p()
    st = L.azd_engine_create(C.byref(h), C.byref(cfg), None)
    if st == 0:
        L.azd_engine_destroy(h)
    return st, L.azd_last_error().decode()


def test_the_flag_is_declared_and_bound():
    import azdopt_amd as az
    from azdopt_amd import _lib
    text = open(os.path.join(ROOT, "include", "azdopt_amd.h")).read()
    assert re.search(r"#define AZD_ENGINE_EXT_POOL_STEP 64u", text)
    assert "azd_debug_ext_pool_plan" in text
    assert _lib.ENGINE_EXT_POOL_STEP == 64
    assert hasattr(C.CDLL(az._lib.LIB_PATH), "azd_debug_ext_pool_plan")
    assert C.sizeof(_lib.EngineConfig) == 96  # the flag changes nothing in the struct's layout


def test_the_flag_is_accepted_on_both_ramsey_tiers_with_max_slots():
    for kw in ACCEPTED:
        st, err = create(**kw)
        assert st in OK, (kw, err)


def test_the_flag_is_refused_elsewhere_and_named():
    for tag, kw in refused_configs():
        st, err = create(**kw)
        assert st == INVALID, (tag, st, err)
        assert "AZD_ENGINE_EXT_POOL_STEP" in err, (tag, err)
    # what it needs is said: the space and max_slots, or the flag it cannot be combined with
    assert "max_slots > 0" in create(**refused_configs()[2][1])[1]
    assert "AZD_ENGINE_NO_PERSISTENT_STEP" in create(**refused_configs()[3][1])[1]
    # without the flag these configurations are what they were
    for tag, kw in refused_configs()[:3]:
        assert create(**dict(kw, flags=0))[0] in OK, tag


def test_par_new_takes_ext_pool_step():
    import azdopt_amd as az
    assert "ext_pool_step" in inspect.signature(az.NablaOptimizer.__init__).parameters
    space = az.ROTModifyParentsOnce(19)
    # (the option reaches azd_engine_create, which refuses it on c21 before any device is touched)
    with pytest.raises(az._lib.AzdError) as ei:
        az.NablaOptimizer.par_new(space, space.generate_roots(0, 4), None, 4, ext_pool_step=True)
    assert ei.value.status == INVALID and "AZD_ENGINE_EXT_POOL_STEP" in str(ei.value)


def test_the_lds_plan_gives_eight_waves_within_the_cu_at_every_accepted_shape():
    """per wave: the block (RamseyWideLds 2144 B, RamseyU64Lds 4944 B), the search scratch (max(512 CH, CORE_DYN_BYTES): 5120 B, 8192 B
    for a wide engine with 16-word keys) and the clique counts (4 E C B); eight of them and the workgroup's 16 B must fit 160 KB"""
    import azdopt_amd as az
    L = az.lib()
    for kw in PLANNED:
        cfg = config(**kw)
        waves, lds = C.c_int32(), C.c_size_t()
        assert L.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == 0, (kw, L.azd_last_error().decode())
        E = kw["n"] * (kw["n"] - 1) // 2
        counts = 4 * E * kw["n_colors"]
        if kw["flags"] & U64:
            per_wave = 4944 + 5120 + counts
        else:
            per_wave = 2144 + (5120 if E * kw["n_colors"] <= 640 else 8192) + counts
        print("ext pool plan", kw, "->", waves.value, "waves,", lds.value, "B of LDS")
        assert waves.value >= 8, (kw, waves.value)
        assert lds.value <= 160 * 1024, (kw, lds.value)
        # the plan's own numbers against the struct sizes (each wave's region is rounded up to 16 B)
        assert 8 * per_wave <= lds.value <= 8 * (per_wave + 16) + 32, (kw, lds.value, per_wave)
    for tag, kw in refused_configs():
        cfg = config(**kw)
        waves, lds = C.c_int32(), C.c_size_t()
        assert L.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(waves), C.byref(lds)) == INVALID, tag
    cfg = config(**dict(R45, flags=0))  # a configuration without the flag has no such plan
    assert L.azd_debug_ext_pool_plan(C.byref(cfg), C.byref(C.c_int32()), C.byref(C.c_size_t())) == INVALID
