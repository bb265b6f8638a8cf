"""The 64-bit Ramsey tier (AZD_ENGINE_RAMSEY_U64 beside max_slots > 0) on the host side: 3 <= n <= 64 over 64-bit neighbourhood
words, E*C <= 2304 (keys of 36 words), nodes of up to 512 actions -- the reference's R(3,3,3,3) shape (03-r3333.rs: N = 34, four
colours, 10..=30 permitted edges).  Config validation with and without the flag, dimensions, the seeded root generator against
the oracle, the new entry points; no GPU needed."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OK = (0, 2)  # created, or "no gfx950 device" on a CPU-only box
U64 = 16     # AZD_ENGINE_RAMSEY_U64

R3333 = dict(n=34, n_colors=4, clique_sizes=[3, 3, 3, 3], max_slots=30)
ACCEPTED = [R3333,
            dict(n=39, n_colors=3, clique_sizes=[3, 3, 4], max_slots=100),  # E*C = 2223
            dict(n=48, n_colors=2, clique_sizes=[4, 5], max_slots=512),     # E*C = 2256
            dict(n=33, n_colors=2, clique_sizes=[3, 4], max_slots=264),
            dict(n=24, n_colors=2, clique_sizes=[4, 5], max_slots=276),     # r45: a 32-bit wide engine takes it too
            dict(n=3, n_colors=2, clique_sizes=[3, 3], max_slots=3)]


def create(**kw):
    import azdopt_amd as az
    from azdopt_amd import _lib
    L = az.lib()
    cfg = _lib.EngineConfig()
    cfg.space_id, cfg.batch = _lib.SPACE_RAMSEY, 8
    cfg.n, cfg.n_colors = 34, 4
    for i in range(4):
        cfg.clique_sizes[i], cfg.color_weights[i] = 3, 1.0
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            arr = getattr(cfg, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(cfg, k, v)
    h = C.c_void_p()
    st = L.azd_engine_create(C.byref(h), C.byref(cfg), None)
    if st == 0:
        L.azd_engine_destroy(h)
    return st, L.azd_last_error().decode()


def test_u64_configs_are_accepted_with_the_flag():
    for kw in ACCEPTED:
        st, err = create(flags=U64, **kw)
        assert st in OK, (kw, err)


def test_the_same_configs_without_the_flag_meet_todays_limits():
    for kw in ACCEPTED[:4]:
        st, err = create(flags=0, **kw)
        assert st == INVALID, kw
        assert ("n <= 32" in err and "E*C <= 1024" in err) and "64" not in err, (kw, err)
    assert create(flags=0, **ACCEPTED[4])[0] in OK  # r45 stays a 32-bit wide engine
    st, err = create(flags=0, n=34, n_colors=4, max_slots=0)
    assert st == INVALID and "E <= 256" in err


def test_u64_dimensions_and_key_words(orc):
    import azdopt_amd as az
    sp = az.RamseySpaceNoEdgeRecolor(34, [3, 3, 3, 3])
    assert (sp.STATE_DIM, sp.ACTION_DIM, sp.KEY_WORDS, sp.E) == (5049, 2244, 36, 561)
    assert sp.tier == "u64" and sp.U64 and sp.MAX_SLOTS == 170 and sp.default_permitted_range() == (12, 170)
    for n, sizes in ((34, [3, 3, 3, 3]), (39, [3, 3, 4]), (48, [4, 5]), (33, [3, 4])):
        sp = az.RamseySpaceNoEdgeRecolor(n, sizes)
        e = orc.Engine(n if n <= 32 else 32, 1, ramsey=(sizes, [1.0] * len(sizes)))  # (the C++ oracle stops at 32 vertices: formulas below)
        E, c = n * (n - 1) // 2, len(sizes)
        assert (sp.STATE_DIM, sp.ACTION_DIM, sp.KEY_WORDS) == (E * (2 * c + 1), E * c, (E * c + 63) // 64)
        assert e.S == 496 * (2 * c + 1)
        assert sp.tier == "u64" and sp.MAX_SLOTS == min(E, 512 // (c - 1))
        assert orc.gen_ramsey_roots(0, 0, 0, 1, n, c, 1, 2)[1].shape[1] == sp.KEY_WORDS
    # the 32-bit tiers are chosen as before; the 64-bit one can be forced or forbidden
    assert az.RamseySpaceNoEdgeRecolor(24, [4, 5]).tier == "wide" and az.RamseySpaceNoEdgeRecolor(17, [4, 4]).tier == "narrow"
    sp = az.RamseySpaceNoEdgeRecolor(24, [4, 5], u64=True)
    e = orc.Engine(24, 1, ramsey=([4, 5], [1.0, 1.0]))
    assert sp.tier == "u64" and sp.MAX_SLOTS == 276 and (sp.STATE_DIM, sp.ACTION_DIM, sp.KEY_WORDS) == (e.S, e.A, e.KW)
    assert az.RamseySpaceNoEdgeRecolor(34, [3, 3, 3, 3], u64=False).tier == "wide"  # (the engine will refuse it: n <= 32)


def test_u64_configs_beyond_the_limits_are_refused_and_named():
    cases = [(dict(n=65, n_colors=2, max_slots=10), "n <= 64"),
             (dict(n=35, n_colors=4, max_slots=30), "E*C <= 2304"),                       # 595 * 4 = 2380
             (dict(n=40, n_colors=3, clique_sizes=[3, 3, 3], max_slots=30), "E*C <= 2304"),  # 780 * 3 = 2340
             (dict(n=49, n_colors=2, max_slots=30), "E*C <= 2304"),                       # 1176 * 2 = 2352
             (dict(n=34, max_slots=171), "max_slots * (C - 1) <= 512"),                   # 171 * 3 = 513: the node capacity
             (dict(n=48, n_colors=2, max_slots=513), "max_slots * (C - 1) <= 512"),
             (dict(n=34, max_slots=562), "max_slots <= E"),
             (dict(n=34, max_slots=-1), "max_slots <= E"),
             (dict(n=34, max_slots=30, layers=2), "Layered"),
             (dict(n=34, max_slots=30, path_kind=1), "AZD_PATH_SET"),
             (dict(n=34, max_slots=30, clique_sizes=[3, 3, 3, 6]), "clique sizes 2..5"),
             (dict(n=34, max_slots=30, n_colors=5), "2..4 colours"),
             (dict(n=34, max_slots=0), "max_slots > 0"),                                  # the flag on a narrow config
             (dict(n=17, n_colors=2, clique_sizes=[4, 4], max_slots=0), "max_slots > 0")]
    for kw, named in cases:
        st, err = create(flags=U64, **kw)
        assert st == INVALID, kw
        assert named in err and ("AZD_ENGINE_RAMSEY_U64" in err or "64-bit" in err), (kw, err)
    from azdopt_amd import _lib
    st, err = create(flags=U64, space_id=_lib.SPACE_C21, n=19, n_colors=0, max_slots=0)  # the flag on c21
    assert st == INVALID and "AZD_ENGINE_RAMSEY_U64" in err and "Ramsey" in err


def test_u64_seeded_root_generator_matches_the_oracle(orc):
    import azdopt_amd as az
    for n, sizes, kmin, kmax in ((34, [3, 3, 3, 3], 10, 30), (48, [4, 5], 1, 512), (39, [3, 3, 4], 5, 256)):
        sp = az.RamseySpaceNoEdgeRecolor(n, sizes)
        for seed, epoch, first in ((0, 0, 0), (5, 1, 77)):
            c, m = sp.generate_roots(seed, 9, first_agent=first, epoch=epoch, kmin=kmin, kmax=kmax)
            co, mo = orc.gen_ramsey_roots(seed, epoch, first, 9, n, len(sizes), kmin, kmax)
            assert c.tobytes() == co.tobytes() and m.tobytes() == mo.tobytes()
            assert all(kmin <= sum(bin(int(w)).count("1") for w in row) <= kmax for row in m)
    c = np.zeros((1, 65 * 32), np.uint8)
    m = np.zeros((1, 80), np.uint64)
    from azdopt_amd import _lib
    assert az.lib().azd_ramsey_generate_roots(0, 0, 0, 1, 65, 2, 1, 2, _lib.ptr(c), _lib.ptr(m)) == INVALID


def test_u64_entry_points_are_declared_and_bound():
    import azdopt_amd as az
    from azdopt_amd import _lib
    text = open(os.path.join(ROOT, "include", "azdopt_amd.h")).read()
    assert re.search(r"#define AZD_RAMSEY_U64_MAX_N 64\b", text) and re.search(r"#define AZD_ENGINE_RAMSEY_U64 16u", text)
    assert re.search(r"#define AZD_RAMSEY_U64_NODE_ACTIONS 512\b", text)
    assert "azd_engine_ramsey_argmin_any" in text
    L = C.CDLL(az._lib.LIB_PATH)
    assert hasattr(L, "azd_engine_ramsey_argmin_any")
    assert (_lib.RAMSEY_U64_MAX_N, _lib.ENGINE_RAMSEY_U64, _lib.RAMSEY_U64_NODE_ACTIONS) == (64, 16, 512)
    assert az.lib().azd_engine_ramsey_argmin_any(None, None, 0, None, 0, None, None, None, None) == INVALID
    assert C.sizeof(_lib.EngineConfig) == 96  # the flag changes nothing in the struct's layout
