"""Every row of tests/domain_cases.py -- the minima, the ceilings and the switches of the domain check_engine_config accepts -- on
the device against its reference engine, bit for bit through gpu_parity.run_lockstep: once with one launch per phase and once in
the engine's default form, whose name and reason are asserted through step_form().  Refusal rows assert status and message.
(tests/test_domain_cases.py shows on the CPU that the reference side of every row is non-vacuous.)"""
import functools

import pytest

import domain_cases as D
from gpu_parity import C21_CTRS, az, caps, compare_ah, compare_c21, compare_ramsey, run_lockstep  # noqa: F401

pytestmark = pytest.mark.gpu


def comparison(c, space):
    if c.family == "ramsey":
        return compare_ramsey(space, argmin_any=space.tier == "u64")
    if c.ctor.get("cost") == "ah":
        return compare_ah
    return functools.partial(compare_c21, counters=C21_CTRS)


def engine_arguments(c, space, form):
    kw = dict(first_agent=c.first_agent)
    if form == "per_call":
        kw["persistent"] = False
    if c.family == "ramsey" and space.wide:  # nodes of up to max_slots * (C - 1) actions: arenas for the row's calls
        kw.update(caps(c.calls + 8, space, c.k[1]))
    return kw


@pytest.mark.parametrize("form", ["per_call", "default"])
@pytest.mark.parametrize("c", [c for c in D.CASES if not c.refuse], ids=lambda c: c.id)
def test_row_against_the_oracle(az, orc, c, form):
    space = D.make_space(az, c)
    roots = D.oracle_roots(orc, c)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, c.seed, c.first_agent)
    opt = az.NablaOptimizer.par_new(space, roots, model, c.B, **engine_arguments(c, space, form))
    dense = c.family == "dense"
    asked = ("dense_per_call" if dense else "per_call") if form == "per_call" or c.default[0] == "per_call" else None
    run_lockstep(opt, D.make_ref(orc, c), roots, orc, comparison(c, space), seed=c.seed, tol=c.tol, steps=c.calls, epochs=c.epochs,
                 kmin=c.k[0], kmax=c.k[1], n_obs_tol=c.n_obs_tol, first_agent=c.first_agent, check_every=c.check_every,
                 boundary="policy" if dense else "alternate", host_policy=c.family == "c21", nan_payloads=c.family != "ramsey",
                 form=asked, clean_end=False)  # (c21 at N = 4 expands nothing: every new node is terminal)
    ran, why = opt.step_form()
    print("%s: asked %s, ran %s -- %s" % (c.id, form, ran, why))
    if form == "per_call":
        assert ran.startswith("per_call") and ("dense-graph space" if dense else "AZD_ENGINE_NO_PERSISTENT_STEP") in why, (ran, why)
    else:
        assert ran.startswith(c.default[0]) and (c.default[1] in why if c.default[1] else why == ""), (c.id, ran, why)
    got = opt.counters()
    assert got["FAILED"] == 0, c.id
    for name in c.conditions:  # the conditions that read counters hold on the device's own counters too
        if name in ("terminals", "transpositions", "root_exhausted"):
            assert D.CONDITIONS[name](c, dict(counters=got)), (c.id, name)


@pytest.mark.parametrize("c", [D.BY_ID["w_n25"], D.BY_ID["w_n26"]], ids=lambda c: c.id)
def test_wide_row_on_the_searcher_only_pool_step(az, orc, c):
    """both sides of the wide tier's key-width switch under AZD_ENGINE_EXT_POOL_STEP too: at 16 words it is the tier's only CU-resident
    form (k_pool_search<RamseyExtSpace<RamseyWideSpace<16>>>), and no other test selects it there.  The hash stream is served like a
    model's rows, as in tests/test_gpu_ramsey_ext_pool.py"""
    space = D.make_space(az, c)
    roots = D.oracle_roots(orc, c)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, c.seed, c.first_agent).serve_from_pool_evaluators()
    opt = az.NablaOptimizer.par_new(space, roots, model, c.B, ext_pool_step=True, **engine_arguments(c, space, "default"))
    run_lockstep(opt, D.make_ref(orc, c), roots, orc, comparison(c, space), seed=c.seed, tol=c.tol, steps=c.calls, epochs=c.epochs,
                 kmin=c.k[0], kmax=c.k[1], n_obs_tol=c.n_obs_tol, check_every=c.check_every, form="pool")
    ev_wgs, search_wgs = opt.pool_split()
    assert ev_wgs == 0 and search_wgs >= 1, (ev_wgs, search_wgs)  # searchers only


@pytest.mark.parametrize("c", [c for c in D.CASES if c.refuse], ids=lambda c: c.id)
def test_refusal_row(az, orc, c):
    space = D.make_space(az, c)
    model = az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, c.seed, c.first_agent)
    with pytest.raises(az.AzdError) as ei:
        az.NablaOptimizer.par_new(space, D.oracle_roots(orc, c), model, c.B)
    assert ei.value.status == c.refuse[0] and c.refuse[1] in str(ei.value), str(ei.value)
