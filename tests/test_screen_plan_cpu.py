"""The launch plan of the two-stage MATCH (csrc/match_screen.hip, screen_plan) against a recorded table.

tests/golden/screen_plans.json holds, for calls that straddle every branch of the policy -- the 256 / 512 / 1024 query
widths, the switch to the 16x16x32 passes at 12 blocks of 1024 queries, the sampling rule for fewer than 256 tiles, the
cap of the identity bits --, what the launches were given when the policy was still written out per kernel family.
mh_screen_plan has to state every field of it, and mh_screen_launch_plan's eight values are the 16x16x32 view of the same
plan (zeros for the other launches).  Host arithmetic: no context, no GPU."""
import json
import os

from moped_amd import capi

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "screen_plans.json")
# mh_screen_launch_plan's values by the plan's field names
_VIEW = {"onesweep": "onesweep", "tile_first": "a_tile_first", "tile_stride": "a_stride", "sampled_tiles": "a_tiles",
         "splits_a": "a_splits", "pack_bits": "pack_bits", "splits_b": "b_splits", "tiles_b": "b_tiles"}


def _table():
    with open(_GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_policy():
    t = _table()
    assert tuple(t["plan_keys"]) == capi.SCREEN_PLAN_KEYS and set(t["launch_plan_keys"]) == set(_VIEW)
    assert len(t["rows"]) == 13 * 2 * 9
    plans = [dict(zip(t["plan_keys"], r["plan"])) for r in t["rows"]]
    assert {(p["family"], p["nqb"]) for p in plans} == {(32, 1), (32, 2), (32, 4), (16, 4)}
    assert {p["a_stride"] for p in plans} == {4, 8}
    # (7 M rows: pass A takes more splits than its workgroup target asks for, so that a lane slot's blocks still count in 10 bits)
    assert max(p["pack_bits"] for p in plans) == 10 and max(p["a_splits"] for p in plans if p["family"] == 16) > 21


def test_plan_is_the_recorded_one():
    t = _table()
    for r in t["rows"]:
        want = dict(zip(t["plan_keys"], r["plan"]))
        got = capi.screen_plan(r["Q"], r["N"], r["q_expected"])
        assert got == want, (r["Q"], r["q_expected"], r["N"])


def test_launch_plan_is_a_view_of_the_plan():
    t = _table()
    for r in t["rows"]:
        plan = capi.screen_plan(r["Q"], r["N"], r["q_expected"])
        view = capi.screen_launch_plan(r["Q"], r["N"], r["q_expected"])
        want = {k: (plan[f] if plan["family"] == 16 else 0) for k, f in _VIEW.items()}
        assert view == want, (r["Q"], r["q_expected"], r["N"])
        assert [view[k] for k in t["launch_plan_keys"]] == r["launch_plan"], (r["Q"], r["q_expected"], r["N"])
