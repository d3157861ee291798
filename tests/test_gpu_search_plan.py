"""The live engine against the record of tests/golden/plans/search_plans.json: every recorded search runs again, on indexes built the
same way, and must report the same statistics (the sketch's counters included) or refuse with the same message. Together with
tests/test_search_plan.py — the planner alone against the same record — this shows that the engine runs the planner and nothing else."""
import pytest

from tests import search_plan_cases as plans

pytestmark = pytest.mark.gpu
RECORDS = plans.load_golden()


@pytest.fixture(scope="module")
def runner(reference):
    return plans.Runner()


@pytest.mark.parametrize("shape", list(plans.SHAPES))
def test_engine_reproduces_the_record(runner, shape):
    wrong, records = [], [record for record in RECORDS if record["case"]["shape"] == shape]
    assert records
    for record in records:  # in the recorded order: a large batch in auto mode may retire the index's sketch for the cases after it
        got = runner.run(record["case"])
        if got != record:
            wrong.append((got, record))
    assert not wrong, f"{len(wrong)} of {len(records)} searches differ from the record; first (got, recorded): {wrong[0]}"
