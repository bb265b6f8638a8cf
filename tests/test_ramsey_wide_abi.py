"""Wide Ramsey engines (azd_engine_config::max_slots > 0) on the host side: N <= 32, E*C <= 1024 and up to max_slots
permitted edges per root -- the reference's R(4,5) shape (05-r45.rs: N = 24, [4, 5], every edge may be permitted).
Config validation, dimensions and the seeded root generator against the oracle; no GPU needed."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
OK = (0, 2)  # created, or "no gfx950 device" on a CPU-only box


def create(**kw):
    import azdopt_amd as az
    from azdopt_amd import _lib
    L = az.lib()
    cfg = _lib.EngineConfig()
    cfg.space_id, cfg.batch = _lib.SPACE_RAMSEY, 8
    cfg.n, cfg.n_colors = 24, 2
    for i, (s, w) in enumerate(zip([4, 5, 3, 3], [1.0, 1.0, 1.0, 1.0])):
        cfg.clique_sizes[i], cfg.color_weights[i] = s, w
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


def test_wide_configs_are_accepted():
    for kw in (dict(n=24, clique_sizes=[4, 5], max_slots=276),
               dict(n=32, clique_sizes=[3, 3], max_slots=496),
               dict(n=26, n_colors=3, clique_sizes=[3, 3, 3], max_slots=325),
               dict(n=20, n_colors=4, clique_sizes=[3, 3, 3, 3], max_slots=190),
               dict(n=17, clique_sizes=[4, 4], max_slots=1),
               dict(n=3, clique_sizes=[3, 3], max_slots=3)):
        st, err = create(**kw)
        assert st in OK, (kw, err)


def test_wide_configs_beyond_the_limits_are_refused_and_named():
    cases = [(dict(n=33, max_slots=100), "n <= 32"),
             (dict(n=27, n_colors=3, clique_sizes=[3, 3, 3], max_slots=100), "E*C <= 1024"),  # E*C = 1053
             (dict(n=24, max_slots=277), "max_slots <= E"),
             (dict(n=24, max_slots=-1), "max_slots <= E"),
             (dict(n=24, max_slots=276, layers=2), "Layered"),
             (dict(n=24, max_slots=276, path_kind=1), "AZD_PATH_SET"),
             (dict(n=24, max_slots=276, clique_sizes=[4, 6]), "clique sizes 2..5"),
             (dict(n=24, max_slots=276, n_colors=5), "2..4 colours")]
    for kw, named in cases:
        st, err = create(**kw)
        assert st == INVALID, kw
        assert named in err, (kw, err)


def test_narrow_limits_stand_without_max_slots():
    st, err = create(n=24, clique_sizes=[4, 5], max_slots=0)
    assert st == INVALID and "E <= 256" in err
    assert create(n=17, clique_sizes=[4, 4], max_slots=0)[0] in OK


def test_r45_space_dimensions_match_the_oracle(orc):
    import azdopt_amd as az
    sp = az.RamseySpaceNoEdgeRecolor(24, [4, 5])
    e = orc.Engine(24, 1, ramsey=([4, 5], [1.0, 1.0]))
    assert (sp.STATE_DIM, sp.ACTION_DIM, sp.KEY_WORDS) == (1380, 552, 9) == (e.S, e.A, e.KW)
    assert sp.MAX_SLOTS == sp.E == 276 and sp.wide
    assert sp.default_permitted_range() == (12, 138)
    for n, c in ((32, 2), (26, 3), (20, 4)):
        sp = az.RamseySpaceNoEdgeRecolor(n, [3] * c)
        e = orc.Engine(n, 1, ramsey=([3] * c, [1.0] * c))
        assert (sp.STATE_DIM, sp.ACTION_DIM, sp.KEY_WORDS) == (e.S, e.A, e.KW)
        assert sp.MAX_SLOTS == sp.E
    # narrow shapes keep max_slots = 0 (today's engine) unless asked
    assert az.RamseySpaceNoEdgeRecolor(17, [4, 4]).MAX_SLOTS == 0
    assert az.RamseySpaceNoEdgeRecolor(17, [4, 4], max_slots=136).MAX_SLOTS == 136
    assert az.RamseySpaceNoEdgeRecolor(17, [4, 4], max_slots=20).default_permitted_range() == (12, 20)


def test_wide_seeded_root_generator_matches_the_oracle(orc):
    import azdopt_amd as az
    for n, sizes, kmin, kmax in ((24, [4, 5], 10, 276), (32, [3, 3], 10, 496), (26, [3, 3, 3], 1, 325)):
        sp = az.RamseySpaceNoEdgeRecolor(n, sizes)
        for seed, epoch, first in ((0, 0, 0), (5, 1, 77)):
            c, m = sp.generate_roots(seed, 9, first_agent=first, epoch=epoch, kmin=kmin, kmax=kmax)
            co, mo = orc.gen_ramsey_roots(seed, epoch, first, 9, n, len(sizes), kmin, kmax)
            assert c.tobytes() == co.tobytes() and m.tobytes() == mo.tobytes()
            assert all(kmin <= sum(bin(int(w)).count("1") for w in row) <= kmax for row in m)
    # every edge permitted at kmin = kmax = E
    c, m = az.RamseySpaceNoEdgeRecolor(24, [4, 5]).generate_roots(3, 2, kmin=276, kmax=276)
    assert all(sum(bin(int(w)).count("1") for w in row) == 276 for row in m)
    L = az.lib()
    assert L.azd_ramsey_generate_roots(0, 0, 0, 1, 33, 2, 1, 2, None, None) == INVALID


def test_wide_entry_points_are_declared_and_bound():
    import azdopt_amd as az
    from azdopt_amd import _lib
    text = open(os.path.join(ROOT, "include", "azdopt_amd.h")).read()
    assert re.search(r"#define AZD_RAMSEY_WIDE_MAX_N 32\b", text)
    assert "azd_engine_ramsey_wide_argmin_data" in text and "azd_ramsey_wide_argmin" in text
    L = C.CDLL(az._lib.LIB_PATH)
    assert hasattr(L, "azd_engine_ramsey_wide_argmin_data")
    assert _lib.RAMSEY_WIDE_MAX_N == 32
    assert C.sizeof(_lib.RamseyWideArgmin) == 496 + 64 + 16 + 12 + 4  # (8-byte aligned)
    assert az.lib().azd_engine_ramsey_wide_argmin_data(None, None) == INVALID
