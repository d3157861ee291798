"""The searches whose launch plans are pinned: shared by scripts/record_search_plans.py (which ran them on the engine as it was before
`csrc/search_plan.hpp` existed and wrote tests/golden/plans/search_plans.json), tests/test_search_plan.py (the planner alone, no GPU)
and tests/test_gpu_search_plan.py (the live engine).

A case is a plain dict: `shape` (a key of SHAPES), `count` (a number, or "2cu" / "2cu+1": twice the compute units, the team boundary),
`expansion`, `tuning` (keywords of `Tuning`), `env` (USEARCH_AMD_* overrides, without the prefix) and `filter` (every third key).
Sizes are the smallest at which a branch of the planner can still differ from its neighbour; one index per shape serves all its cases,
in list order (a batch of 1 024 queries or more in auto mode may retire the sketch: each record says whether it was there)."""
from __future__ import annotations

import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans", "search_plans.json")
WANTED = 10
# the timed draws of scratch placements (engine.hip, `draw_scratch`) run the launch's first queries a few more times and change no
# decision; they stay out of the record and of the replay
FIXED_ENV = {"SCRATCH_DRAWS": "1"}

SHAPES = {
    "b1x128": dict(n=3000, ndim=128, metric="tanimoto", dtype="b1", seed=41),   # one lane, rows inline: `seen`, plain without `aside`
    "i8x96": dict(n=3000, ndim=96, metric="l2sq", dtype="i8", seed=42),         # two lanes: early rows, `aside`, two cells per lane
    "f16x768": dict(n=2500, ndim=768, metric="cos", dtype="f16", seed=43),      # 12 chunks per lane: every variant, team, sketch
    "f32x256": dict(n=2500, ndim=256, metric="cos", dtype="f32", seed=44),      # 8 chunks per lane: u8_w3
    "f32x24": dict(n=500, ndim=24, metric="l2sq", dtype="f32", seed=45),        # outside the common set: 4-deep only, no team
    "i8x1024": dict(n=2500, ndim=1024, metric="l2sq", dtype="i8", seed=46),     # integer pair on long rows: heap only
    "f16x768_40": dict(n=40, ndim=768, metric="cos", dtype="f16", seed=47),     # the size clamps of hash_cap and next_cap bind
    "f16x768_removed": dict(n=2500, ndim=768, metric="cos", dtype="f16", seed=43, removed=25),  # tombstones
}
SHORT = ("b1x128", "i8x96")
SMALL = ("f16x768_40", "f16x768_removed")  # variations of f16x768: the default grid at two counts and a few tunings
BOUNDARIES = (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025)
COUNTS = (1, "2cu", "2cu+1", 3000)
# every shape: the scratch modes, the frontiers, fewer waves, the refusals, and caps small enough to climb the ladder
TUNINGS = ([dict(mode=m) for m in (1, 2, 3)] + [dict(frontier=f) for f in (1, 2)] +
           [dict(waves_per_cu=2), dict(frontier=2, mode=3), dict(mode=4), dict(hash_cap=256, next_cap=96, mode=1),
            dict(hash_cap=64, next_cap=40, mode=2), dict(mode=2, waves_per_cu=1)])
# rows of eight lanes with every kernel build (and a sketch): the builds, the sketch modes, and what is refused among them
LONG_ROW_TUNINGS = ([dict(variant=v) for v in (1, 2, 3, 4)] + [dict(variant=4, frontier=1), dict(variant=2, frontier=2)] +
                    [dict(sketch=s) for s in (1, 2, 3)])


def expansions(shape: str):
    return BOUNDARIES[:4] if shape in SHORT else BOUNDARIES


def cases():
    out = []

    def add(shape, count, expansion, tuning=None, env=None, filter=False):
        out.append(dict(shape=shape, count=count, expansion=expansion, tuning=dict(tuning or {}), env=dict(env or {}), filter=filter))

    for shape in SHAPES:
        for expansion in expansions(shape):  # both sides of every boundary of the expansion, at every boundary of the batch size
            for count in ((1, 3000) if shape in SMALL else COUNTS):
                add(shape, count, expansion)
        # the rest at one small and one large register-`top` size, alone and in a batch that fills the chip
        points = [(count, expansion) for expansion in ((64, 129) if shape in SHORT else (64, 513)) for count in (1, 3000)]
        for count, expansion in points:
            for tuning in (TUNINGS[:5] if shape in SMALL else TUNINGS):
                add(shape, count, expansion, tuning)
            for tuning in (LONG_ROW_TUNINGS if shape in ("f16x768", "f32x256") else [dict(variant=2), dict(sketch=3)] if shape == "i8x1024" else []):
                add(shape, count, expansion, tuning)
            if shape not in SMALL:
                for env in (dict(LDS_BUDGET="65536"), dict(HASH_LOAD_PCT="75"), dict(NO_SMALL_BATCH_LDS="1"),
                            dict(TOP_IN_MEMORY="1")):  # (`search_tuning_t::top_in_memory` has no Python keyword)
                    add(shape, count, expansion, env=env)
        add(shape, 1, 64, filter=True)
        add(shape, 3000, 257, filter=True)
        add(shape, 3000, 64, dict(frontier=2), filter=True)
    add("f16x768", 40000, 608)  # the `count >= 40000` variant switch; the walk over 2 500 members is short
    add("f16x768", "2cu", 608, env=dict(NO_SMALL_BATCH_LDS="1"))  # the tighter visited set of a small batch, and without it
    add("f16x768", "2cu", 608)
    for shape in ("f16x768", "i8x1024"):  # `top` in scratch memory
        for tuning in (dict(frontier=2), dict(mode=1), dict(mode=2)):
            add(shape, 1, 1025, tuning)
            add(shape, 3000, 1025, tuning)
    for shape in ("f16x768", "f32x256"):
        for expansion in (64, 513, 1025):
            for count in (1, "2cu", "2cu+1"):
                add(shape, count, expansion, env=dict(NO_TEAM="1"))
    for shape in SHORT:
        for env in (dict(NO_PLAIN="1"), dict(NO_TWO_CELLS="1"), dict(SEEN_CELLS="0"), dict(SEEN_CELLS="300")):
            for expansion in expansions(shape):
                for count in (1, 3000):
                    add(shape, count, expansion, env=env)
            add(shape, 3000, 64, dict(mode=2), env=env)
            add(shape, 3000, 129, dict(mode=2), env=env)
    for expansion in (64, 80, 128):  # a table that is sure to fill up: this climbs the ladder (tests/test_gpu_search_parity.py)
        for count in (200, 3000):
            add("i8x96", count, expansion, dict(mode=2), env=dict(ASIDE_CELLS="64", PLAIN_WHATEVER_THE_ROOM="1"))
    return out


def case_name(case: dict) -> str:
    """The case in one string, as the record keeps it: shape/count/expansion[/tuning][/environment][/filtered]."""
    parts = [case["shape"], str(case["count"]), str(case["expansion"])]
    parts += [",".join(f"{name}={value}" for name, value in group.items()) for group in (case["tuning"], case["env"]) if group]
    return "/".join(parts + (["filtered"] if case["filter"] else []))


def resolve_count(count, compute_units: int) -> int:
    return {"2cu": 2 * compute_units, "2cu+1": 2 * compute_units + 1}.get(count, count)


def load_golden():
    """→ the records, one per case of `cases()` in its order: {case, count, wanted, facts, stats | refused}. The file keeps the facts
    once per shape (only the sketch's presence changes from case to case), the refusals' messages once, and a record as
    [case_name, count, sketch, the stats in the order of STAT_FIELDS | the number of the refusal], several to a line."""
    with open(GOLDEN) as file:
        stored = json.load(file)
    assert stored["stat_fields"] == list(STAT_FIELDS)
    named = {case_name(case): case for case in cases()}
    records = []
    for name, count, sketch, outcome in stored["records"]:
        record = dict(case=named[name], count=count, wanted=stored["wanted"], facts=dict(stored["facts"][named[name]["shape"]], sketch=bool(sketch)))
        if isinstance(outcome, int):
            record["refused"] = stored["refusals"][outcome]
        else:
            record["stats"] = dict(zip(STAT_FIELDS, outcome))
        records.append(record)
    return records


def save_golden(records) -> None:
    facts, refusals, rows = {}, [], []
    for record in records:
        shape_facts = {name: value for name, value in record["facts"].items() if name != "sketch"}
        assert facts.setdefault(record["case"]["shape"], shape_facts) == shape_facts
        if "refused" in record and record["refused"] not in refusals:
            refusals.append(record["refused"])
        outcome = refusals.index(record["refused"]) if "refused" in record else [record["stats"][name] for name in STAT_FIELDS]
        rows.append(json.dumps([case_name(record["case"]), record["count"], int(record["facts"]["sketch"]), outcome], separators=(",", ":")))
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as file:
        file.write('{"wanted": %d, "stat_fields": %s,\n "facts": {\n' % (WANTED, json.dumps(list(STAT_FIELDS))))
        file.write(",\n".join("  %s: %s" % (json.dumps(shape), json.dumps(value)) for shape, value in facts.items()))
        file.write('},\n "refusals": %s,\n "records": [\n' % json.dumps(refusals, indent=1))
        file.write(",\n".join(", ".join(rows[i:i + 8]) for i in range(0, len(rows), 8)))
        file.write("\n]}\n")


# ---- running a case on the live engine (the recorder and the GPU replay): only what `Index` offered before the planner moved

STAT_FIELDS = ("passes", "retried_lds", "retried_global", "mode", "grid", "lds_bytes", "frontier", "variant", "top_cells", "probe_mode",
               "seen_cells", "claim_bits", "early_rows", "plain", "aside_cells", "sketch_tested", "sketch_pruned")


class Runner:
    """Builds each shape's index once and runs cases on it → what the record holds for one case."""

    def __init__(self):
        import torch
        self.compute_units = int(torch.cuda.get_device_properties(0).multi_processor_count)
        self.indexes = {}

    def index(self, shape: str):
        if shape not in self.indexes:
            from tests import util
            from usearch_amd import Index
            s = SHAPES[shape]
            removed = tuple(range(1000, 1000 + s.get("removed", 0)))  # the first keys of `build_image`
            image, _, _ = util.build_image(s["n"], s["ndim"], s["metric"], s["dtype"], seed=s["seed"], remove=removed)
            index = Index.restore(image)
            queries = util.make_vectors(40000 if shape == "f16x768" else 3000, s["ndim"], s["dtype"], seed=s["seed"] + 100)
            every_third = index.filter_keys(np.arange(1000, 1000 + s["n"], 3, dtype=np.uint64))
            self.indexes[shape] = (index, queries, every_third)
        return self.indexes[shape]

    def run(self, case: dict) -> dict:
        from usearch_amd import Tuning
        index, queries, every_third = self.index(case["shape"])
        s = SHAPES[case["shape"]]
        count = resolve_count(case["count"], self.compute_units)
        arrays = index.arrays
        lanes = int(index.lanes_per_row)
        chunks = -(-int(index.bytes_per_vector) // (16 * lanes)) * lanes  # whole 16-byte chunks, a multiple of the lanes (the pitch may be wider)
        facts = dict(metric=s["metric"], dtype=s["dtype"], lanes=lanes, chunks=chunks,
                     size=int(arrays.size), m0=int(arrays.level0_cells), inline_rows=bool(index.inline_rows),
                     sketch=bool(arrays.sketch), tombstones=bool(s.get("removed")), compute_units=self.compute_units)
        names = ["USEARCH_AMD_" + name for name in list(FIXED_ENV) + list(case["env"])]
        saved = {name: os.environ.get(name) for name in names}
        try:
            for name, value in {**FIXED_ENV, **case["env"]}.items():
                os.environ["USEARCH_AMD_" + name] = value
            got = index.search(queries[:count], WANTED, expansion=case["expansion"], dtype=s["dtype"], tuning=Tuning(**case["tuning"]),
                               filter=every_third if case["filter"] else None)
            outcome = dict(stats={name: int(getattr(got.stats, name)) for name in STAT_FIELDS})
        except RuntimeError as refusal:  # "<entry point>: <the engine's message>"
            outcome = dict(refused=str(refusal).split(": ", 1)[1])
        finally:
            for name, value in saved.items():
                if value is None:
                    os.environ.pop(name, None)
                else:
                    os.environ[name] = value
        return dict(case=case, count=count, wanted=WANTED, facts=facts, **outcome)
