"""Clique sizes up to 8 on the 64-bit Ramsey tier (AZD_ENGINE_RAMSEY_BIG_CLIQUES beside AZD_ENGINE_RAMSEY_U64) on the host side: the
names, config validation with and without the flag -- the flag's company, the sizes, the reference's i32 bound C(s,2) * C(n,s)
<= 2^31 - 1 per colour, the tier's other limits -- and the Python space's option; no GPU needed."""
import ctypes as C
import os
import re
from math import comb

import pytest

from test_ramsey64_abi import INVALID, OK, U64, create

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 512  # AZD_ENGINE_RAMSEY_BIG_CLIQUES
OVERFLOW = "C(s,2) * C(n,s)"


def test_the_names_are_declared_and_bound():
    from azdopt_amd import _lib
    text = open(os.path.join(ROOT, "include", "azdopt_amd.h")).read()
    assert re.search(r"#define AZD_ENGINE_RAMSEY_BIG_CLIQUES 512u", text) and re.search(r"#define AZD_RAMSEY_BIG_CLIQUE_MAX 8\b", text)
    assert (_lib.ENGINE_RAMSEY_BIG_CLIQUES, _lib.RAMSEY_BIG_CLIQUE_MAX) == (512, 8)
    assert C.sizeof(_lib.EngineConfig) == 96  # the flag changes nothing in the struct's layout
    flags = [int(v) for v in re.findall(r"#define AZD_ENGINE_[A-Z0-9_]+ (\d+)u", text)]
    assert len(flags) == len(set(flags)) and all(f & (f - 1) == 0 for f in flags)  # one bit each, none shared


def test_the_flag_needs_the_64_bit_tier_beside_it():
    from azdopt_amd import _lib
    cases = [dict(flags=BIG, n=20, n_colors=2, clique_sizes=[3, 6], max_slots=30),          # without AZD_ENGINE_RAMSEY_U64: a wide config
             dict(flags=BIG, n=17, n_colors=2, clique_sizes=[4, 4], max_slots=0),           # ... a narrow one
             dict(flags=BIG, space_id=_lib.SPACE_C21, n=19, n_colors=0, max_slots=0),       # on c21
             dict(flags=BIG | U64, space_id=_lib.SPACE_C21, n=19, n_colors=0, max_slots=0),
             dict(flags=BIG, space_id=_lib.SPACE_DENSE, n=20, n_colors=0, max_slots=0),     # on the dense-graph space
             dict(flags=BIG | U64, space_id=_lib.SPACE_DENSE, n=20, n_colors=0, max_slots=0)]
    for kw in cases:
        st, err = create(**kw)
        assert st == INVALID, kw
        assert "AZD_ENGINE_RAMSEY_BIG_CLIQUES" in err and "AZD_ENGINE_RAMSEY_U64" in err, (kw, err)


def test_flagged_configs_are_accepted():
    for kw in (dict(n=35, n_colors=2, clique_sizes=[4, 6], max_slots=276),   # r46
               dict(n=22, n_colors=2, clique_sizes=[3, 7], max_slots=100),
               dict(n=27, n_colors=2, clique_sizes=[3, 8], max_slots=100),
               dict(n=48, n_colors=2, clique_sizes=[4, 7], max_slots=512),   # E*C = 2256
               dict(n=16, n_colors=3, clique_sizes=[3, 3, 6], max_slots=40),
               dict(n=12, n_colors=2, clique_sizes=[2, 8], max_slots=10),
               dict(n=24, n_colors=2, clique_sizes=[4, 5], max_slots=276),   # a shape the tier takes without the flag
               dict(n=34, n_colors=4, clique_sizes=[3, 3, 3, 3], max_slots=30)):
        st, err = create(flags=U64 | BIG, **kw)
        assert st in OK, (kw, err)


def test_sizes_beyond_8_are_refused_with_the_flagged_text():
    for sizes in ([3, 9], [9, 3], [1, 6], [3, 100]):
        st, err = create(flags=U64 | BIG, n=20, n_colors=2, clique_sizes=sizes, max_slots=30)
        assert st == INVALID and "clique sizes 2..8" in err and "AZD_ENGINE_RAMSEY_BIG_CLIQUES" in err, (sizes, err)


def test_the_references_i32_bound_per_colour():
    """RamseyCounts::new adds C(s,2) * C(n,s) into an i32 on a monochromatic root: size 8 stops at n = 39, size 7 at n = 50 (where
    two colours no longer fit E*C <= 2304: the bound is met first and named), size 6 never within n <= 64"""
    assert comb(8, 2) * comb(39, 8) <= 2 ** 31 - 1 < comb(8, 2) * comb(40, 8)
    assert comb(7, 2) * comb(50, 7) <= 2 ** 31 - 1 < comb(7, 2) * comb(51, 7)
    assert comb(6, 2) * comb(64, 6) <= 2 ** 31 - 1
    st, err = create(flags=U64 | BIG, n=40, n_colors=2, clique_sizes=[8, 3], max_slots=30)
    assert st == INVALID and OVERFLOW in err and "AZD_ENGINE_RAMSEY_BIG_CLIQUES" in err and "colour 0" in err, err
    st, err = create(flags=U64 | BIG, n=40, n_colors=2, clique_sizes=[3, 8], max_slots=30)
    assert st == INVALID and OVERFLOW in err and "colour 1" in err, err
    st, err = create(flags=U64 | BIG, n=39, n_colors=2, clique_sizes=[8, 3], max_slots=30)
    assert st in OK, err
    st, err = create(flags=U64 | BIG, n=51, n_colors=2, clique_sizes=[3, 7], max_slots=30)
    assert st == INVALID and OVERFLOW in err and "AZD_ENGINE_RAMSEY_BIG_CLIQUES" in err and "colour 1" in err, err
    st, err = create(flags=U64 | BIG, n=50, n_colors=2, clique_sizes=[3, 7], max_slots=30)  # passes the bound; two colours at n = 50 are E*C = 2450
    assert st == INVALID and OVERFLOW not in err and "E*C <= 2304" in err, err
    st, err = create(flags=U64 | BIG, n=48, n_colors=2, clique_sizes=[3, 7], max_slots=30)
    assert st in OK, err
    st, err = create(flags=U64 | BIG, n=64, n_colors=2, clique_sizes=[6, 6], max_slots=30)  # refused for E*C only
    assert st == INVALID and OVERFLOW not in err and "E*C <= 2304" in err and "clique sizes 2..8" in err, err


def test_the_tiers_other_limits_hold_under_the_flag():
    cases = [(dict(n=65, n_colors=2, clique_sizes=[3, 6], max_slots=10), "n <= 64"),
             (dict(n=35, n_colors=4, clique_sizes=[3, 3, 3, 6], max_slots=30), "E*C <= 2304"),
             (dict(n=35, n_colors=2, clique_sizes=[4, 6], max_slots=513), "max_slots * (C - 1) <= 512"),
             (dict(n=35, n_colors=2, clique_sizes=[4, 6], max_slots=596), "max_slots <= E"),
             (dict(n=35, n_colors=2, clique_sizes=[4, 6], max_slots=0), "max_slots > 0"),
             (dict(n=35, n_colors=2, clique_sizes=[4, 6], max_slots=30, layers=2), "Layered"),
             (dict(n=35, n_colors=2, clique_sizes=[4, 6], max_slots=30, path_kind=1), "AZD_PATH_SET"),
             (dict(n=35, n_colors=5, clique_sizes=[4, 6], max_slots=30), "2..4 colours")]
    for kw, named in cases:
        st, err = create(flags=U64 | BIG, **kw)
        assert st == INVALID, kw
        assert named in err and ("AZD_ENGINE_RAMSEY_U64" in err or "64-bit" in err), (kw, err)


def test_without_the_flag_a_size_6_meets_todays_text_in_all_three_tiers():
    for kw in (dict(flags=U64, n=35, n_colors=2, clique_sizes=[4, 6], max_slots=276),
               dict(flags=0, n=24, n_colors=2, clique_sizes=[4, 6], max_slots=276),
               dict(flags=0, n=17, n_colors=2, clique_sizes=[4, 6], max_slots=0)):
        st, err = create(**kw)
        assert st == INVALID and "clique sizes 2..5" in err and "BIG_CLIQUES" not in err, (kw, err)


def test_python_space_option():
    import azdopt_amd as az
    sp = az.RamseySpaceNoEdgeRecolor(35, [4, 6])
    E = 35 * 34 // 2
    assert sp.tier == "u64" and sp.U64 and sp.BIG_CLIQUES
    assert (sp.E, sp.STATE_DIM, sp.ACTION_DIM, sp.KEY_WORDS) == (E, E * 5, E * 2, (E * 2 + 63) // 64)
    assert sp.MAX_SLOTS == min(E, 512)
    sp = az.RamseySpaceNoEdgeRecolor(12, [3, 6])  # a shape the narrow tier would take: the size forces the 64-bit tier
    assert sp.tier == "u64" and sp.BIG_CLIQUES and sp.MAX_SLOTS == 66
    for kw in (dict(u64=False), dict(big_cliques=False), dict(u64=True, big_cliques=False)):
        with pytest.raises(ValueError):
            az.RamseySpaceNoEdgeRecolor(35, [4, 6], **kw)
    with pytest.raises(ValueError):
        az.RamseySpaceNoEdgeRecolor(24, [4, 5], u64=False, big_cliques=True)
    with pytest.raises(ValueError, match="colour 0"):
        az.RamseySpaceNoEdgeRecolor(40, [8, 3])
    with pytest.raises(ValueError, match="colour 1"):
        az.RamseySpaceNoEdgeRecolor(51, [3, 7])
    assert az.RamseySpaceNoEdgeRecolor(39, [8, 3]).BIG_CLIQUES
    sp = az.RamseySpaceNoEdgeRecolor(24, [4, 5])  # unchanged: wide, no flag
    assert sp.tier == "wide" and not sp.U64 and not sp.BIG_CLIQUES and sp.MAX_SLOTS == 276
    sp = az.RamseySpaceNoEdgeRecolor(24, [4, 5], u64=True)
    assert sp.tier == "u64" and not sp.BIG_CLIQUES
    sp = az.RamseySpaceNoEdgeRecolor(24, [4, 5], big_cliques=True)  # the flag by name on a K5 shape: the 64-bit tier with it
    assert sp.tier == "u64" and sp.BIG_CLIQUES
    assert not az.RamseySpaceNoEdgeRecolor(34, [3, 3, 3, 3]).BIG_CLIQUES and not az.RamseySpaceNoEdgeRecolor(17, [4, 4]).BIG_CLIQUES
