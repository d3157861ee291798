"""Records what the engine decides for every search of tests/search_plan_cases.py → tests/golden/plans/search_plans.json.

The record is the yardstick of csrc/search_plan.hpp: it was written by the engine as it stood BEFORE the planner was split out of
`search_begin` / `run_ladder` / `search_finish`, through nothing but `Index.restore`, `Index.search` and filters. Run it on an MI355X;
rerun it only when a decision is meant to change, from the commit before that change.

    python scripts/record_search_plans.py
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import search_plan_cases as plans  # noqa: E402


def main() -> None:
    # no timed scratch-placement draws: with them off (FIXED_ENV, applied by the runner to every case) a scratch block of any size is
    # simply allocated, so the 8-MB threshold of the draws never decides anything in the record
    assert plans.FIXED_ENV.get("SCRATCH_DRAWS") == "1"
    started = time.time()
    runner = plans.Runner()
    records = [runner.run(case) for case in plans.cases()]
    for record in records:
        assert record["facts"]["size"] <= 3000 and ("refused" in record) != ("stats" in record)
    plans.save_golden(records)
    refused = sum("refused" in record for record in records)
    climbed = sum(record.get("stats", {}).get("passes", 0) > 1 for record in records)
    print(f"{len(records)} cases ({refused} refused, {climbed} climbed the ladder) in {time.time() - started:.1f} s → {plans.GOLDEN}")


if __name__ == "__main__":
    main()
