"""The pool step's split of the chip, pinned to a recording.

tests/golden/pool_split_mi355x.json holds, per case, the evaluator / searcher workgroups and the evaluator groups that the FIRST
roll-out of a fresh engine launched (azd_engine_pool_split, azd_engine_pool_groups), recorded once on an MI355X from the library
as it stood before the split arithmetic became a function of its own (engine_rollout.hip: pool_split).  Trees do not depend on the
split, so no parity test sees a slip in that arithmetic; this module does.  Every case sets AZD_POOL_MAX_RESIDENT, so that the
co-resident capacity is an input and not what the runtime of the day reports; the first roll-out of an engine runs before the
feedback controller has acted.

Of the values the split also decides -- express workgroups, ready lanes, early post -- the library has no accessor; they are
covered by review of pool_split against its parent, not by this module."""
import json
import os

import pytest

from gpu_parity import az  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_split_mi355x.json")
KNOBS = ("AZD_POOL_MAX_RESIDENT", "AZD_POOL_EVAL_WGS", "AZD_POOL_SEARCH_WGS", "AZD_POOL_EVAL_GROUP", "AZD_POOL_READY_LANES",
         "AZD_POOL_EXPRESS_WGS", "AZD_POOL_EXPRESS_WAVES", "AZD_POOL_EXPRESS_SHIFT", "AZD_POOL_EARLY_POST", "AZD_POOL_FEEDBACK")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _replayed(rows):
    """every row at B <= 1024, plus the first row at 4096 agents of each space's in-kernel or searcher-only form"""
    out, big = [], set()
    for r in rows:
        kind = r["case"]["space"]["kind"]
        if r["case"]["B"] <= 1024:
            out.append(r)
        elif r["case"]["B"] == 4096 and not r["case"]["kw"].get("ext_pool_step") and kind not in big:
            big.add(kind)
            out.append(r)
    return out


def make_space(az, s):
    if s["kind"] == "c21":
        return az.ROTModifyParentsOnce(s["n"])
    if s["kind"] == "ramsey":
        return az.RamseySpaceNoEdgeRecolor(s["n"], s["sizes"], s.get("weights"), u64=s.get("u64"))
    return az.DenseGraphSpace(s["n"], s["p"], max_slots=s["max_slots"])


def make_model(az, space, m, B):
    if m["kind"] == "trivial":
        return az.TrivialModel(space.STATE_DIM, space.ACTION_DIM)
    if m["kind"] == "hash_pool":
        return az.HashStreamModel(space.STATE_DIM, space.ACTION_DIM, 3).serve_from_pool_evaluators()
    return az.ActionModel(B, space.STATE_DIM, space.ACTION_DIM, hidden=tuple(m["hidden"]), seed=3, dtype=m["dtype"])


def first_roll_out(az, case, setenv, delenv):
    """a fresh engine of `case`, its first roll-out: -> (step_form, pool_split, pool_groups)"""
    for k in KNOBS:
        delenv(k)
    for k, v in case["env"].items():
        setenv(k, v)
    space = make_space(az, case["space"])
    B = case["B"]
    roots = space.generate_roots(3, B, **case["roots"])
    opt = az.NablaOptimizer.par_new(space, roots, make_model(az, space, case["model"], B), B, **case["kw"])
    opt.par_roll_out_episodes((case["tol"][0], case["tol"][1]), n_calls=case["n_calls"])
    return opt.step_form(), opt.pool_split(), opt.pool_groups()


def test_the_device_is_the_one_the_table_was_recorded_on(az):
    import torch
    g = _golden()
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cus == g["n_cus"], f"the table was recorded on a device of {g['n_cus']} CUs, this one has {n_cus}: the split depends on the count"


def test_the_recording_agrees_with_the_values_worked_out_by_hand():
    """c21 N = 19, 256 x 3 fp32, on 256 CUs; worked out from the arithmetic on paper before it moved (capacity 256 unless said)"""
    rows = {r["case"]["id"]: r for r in _golden()["rows"]}
    for cid, want in (("c21-f32-B4096-c200", (103, 153)), ("c21-f32-B4096-c20", (117, 139)), ("c21-f32-B512-c40", (117, 64)),
                      ("c21-f32-B512-c40-cap40", (20, 20)), ("c21-f32-B512-c40-cap24-ev200", (12, 12))):
        assert (rows[cid]["eval_wgs"], rows[cid]["search_wgs"]) == want, cid


@pytest.mark.parametrize("row", _replayed(_golden()["rows"]), ids=lambda r: r["case"]["id"])
def test_first_launch_has_the_recorded_split(az, monkeypatch, row):
    form, split, groups = first_roll_out(az, row["case"], monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    print(row["case"]["id"], form, split, groups)
    assert form == ("pool", "")
    assert split == (row["eval_wgs"], row["search_wgs"])
    assert list(groups) == row["groups"]
