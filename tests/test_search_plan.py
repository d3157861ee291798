"""The launch planner (csrc/search_plan.hpp) against the record of what the engine decided before the planner was split out of it
(tests/golden/plans/search_plans.json, written by scripts/record_search_plans.py on an MI355X): every recorded search is planned again
from its recorded shape facts and the recorded number of queries per rung of the retry ladder, through the test hook — pure integer
arithmetic, no GPU in the loop — and must report the same statistics, or refuse with the same message."""
import os

import pytest

from tests import search_plan_cases as plans

RECORDS = plans.load_golden()
DECIDED = [name for name in plans.STAT_FIELDS if not name.startswith("sketch_")]  # (the sketch's two counters are measured)
# `read_search_knobs` with nothing set (hash_load_pct: 50 for rows of 8 lanes, 75 below)
NO_KNOBS = dict(lds_budget=160 * 1024, hash_cap=0, hash_load_pct=None, next_cap=0, mode=0, top_in_memory=0, no_two_cells=0, frontier=0, variant=0,
                no_team=0, no_plain=0, waves_per_cu=32, no_small_batch_lds=0, early_rows=1, aside_cells=0,
                plain_whatever_the_room=0, seen_cells=2 ** 64 - 1)


def planned(record, knobs=None):
    from usearch_amd.index import test_plan_search
    case, facts, stats = record["case"], record["facts"], record.get("stats", {})
    shape = dict(size=facts["size"], count=record["count"], wanted=record["wanted"], expansion=case["expansion"], metric=facts["metric"],
                 dtype=facts["dtype"], lanes=facts["lanes"], chunks=facts["chunks"], m0=facts["m0"], compute_units=facts["compute_units"],
                 has_tombstones=int(facts["tombstones"]), nbr0=1, nbr0_rows=int(facts["inline_rows"]), sketch=int(facts["sketch"]),
                 allow_bits=int(case["filter"]))
    pending = [record["count"]] + [stats[name] for name in ("retried_lds", "retried_global") if stats.get(name)]
    try:
        plan, rungs = test_plan_search(shape, case["tuning"], pending, knobs)
    except RuntimeError as refusal:
        return dict(refused=str(refusal).split(": ", 1)[1])
    return dict(stats={name: plan["stats"][name] for name in DECIDED})


def expected(record):
    return dict(refused=record["refused"]) if "refused" in record else dict(stats={name: record["stats"][name] for name in DECIDED})


def test_the_record_covers_the_case_list():
    assert [record["case"] for record in RECORDS] == plans.cases(), "rerun scripts/record_search_plans.py from the commit before the change"
    assert {record["case"]["shape"] for record in RECORDS} == set(plans.SHAPES)


@pytest.mark.parametrize("shape", list(plans.SHAPES))
def test_planner_reproduces_the_record(shape, monkeypatch):
    for name in list(os.environ):
        if name.startswith("USEARCH_AMD_"):
            monkeypatch.delenv(name)
    wrong, records = [], [record for record in RECORDS if record["case"]["shape"] == shape]
    assert records
    for record in records:
        with monkeypatch.context() as patch:  # the overrides arrive the way they reach the engine: through the environment
            for name, value in record["case"]["env"].items():
                patch.setenv("USEARCH_AMD_" + name, value)
            got = planned(record)
        if got != expected(record):
            wrong.append((record["case"], record["count"], got, expected(record)))
    assert not wrong, f"{len(wrong)} of {len(records)} plans differ from the record; first: {wrong[0]}"


def test_knob_struct_and_environment_agree(monkeypatch):
    """The hook's explicit knob struct is the same input as the environment `read_search_knobs` reads."""
    overridden = [record for record in RECORDS if record["case"]["env"]]
    assert overridden
    for record in overridden:
        knobs = dict(NO_KNOBS, hash_load_pct=50 if record["facts"]["lanes"] >= 8 else 75)
        knobs.update({name.lower(): int(value) for name, value in record["case"]["env"].items()})
        assert planned(record, knobs) == expected(record), record["case"]
