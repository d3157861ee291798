"""The f64 truth of the sketch (tests/sketch_truth.py) against the host twins (usearch_amd/csrc/sketch.hpp), and the model of the walk's
prune decision. CPU only.

  · on the data sets of tests/test_sketch_bound.py the twins' records must pass every assertion the device's records are held to in
    tests/test_gpu_sketch_records.py (sound, tight, coefficients, never-pruned rows, the gram defect);
  · the prune model on a hand-made trace of three hops;
  · TEETH: on the data of every case of tests/test_gpu_sketch_counts.py the model's pruned total must change when every bound moves
    by +1e-3 and by −1e-3 and when two coefficient columns of the records change places — a counter test that could not tell these
    apart would pass a ρ that is 1e-3 too small or a coefficient read from the wrong lane."""
from __future__ import annotations

import numpy as np
import pytest

import usearch_amd.index as ua_index
from oracle import oraclebind
from tests import sketch_cases, sketch_truth
from tests import test_sketch_bound as bound_data


@pytest.mark.parametrize("kind", ["lowrank", "gaussian"])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("ndim", [768, 100, 24])
def test_twin_records_hold_against_the_truth(ndim, dtype, kind):
    rows, _, never_rows, _ = bound_data._dataset(kind, ndim, dtype)
    directions, rank, defect = ua_index.test_sketch_directions(rows, dtype)
    assert rank == sketch_truth.rank_of(directions) and 0 < rank <= min(62, ndim)
    records = ua_index.test_sketch_twin_records(rows, dtype, directions, defect)
    duplicates = bound_data.DUPLICATES if kind == "lowrank" else ()
    sketch_truth.check_records(sketch_truth.widen(rows, dtype), directions, defect, records, never_rows, duplicates, f"twin, {kind} {ndim} {dtype}")


def test_true_distance_is_above_the_twin_bound():
    """The truth's own cos distance against the twins' bound (which allows for the kernel's f32 error on top): a cross-check of
    `cos_distance`, `widen` and the binding of the split twins."""
    rows, queries, _, _ = bound_data._dataset("lowrank", 100, "bf16")
    directions, _, defect = ua_index.test_sketch_directions(rows, "bf16")
    records = ua_index.test_sketch_twin_records(rows, "bf16", directions, defect)
    rows64, queries64 = sketch_truth.widen(rows, "bf16"), sketch_truth.widen(queries, "bf16")
    # Σa² as the one-piece hook sums it: one fused f32 chain in element order (the oracle's layout of one lane)
    sums = np.array([oraclebind.sum_of_squares(q, "bf16", 100, lanes=1) for q in queries], dtype=np.float32)
    bounds, used = ua_index.test_sketch_twin_bounds(queries, sums, "bf16", directions, records)
    whole, _ = ua_index.test_sketch_bounds(rows, queries, "bf16")
    assert np.array_equal(bounds, whole), "the split twins and the hook that runs them in one piece disagree"
    assert [q for q in range(len(queries)) if not used[q]] == sorted(bound_data._dataset("lowrank", 100, "bf16")[3])
    ordinary = sketch_truth.ordinary_rows(rows64)
    for q in np.flatnonzero(used)[:16]:
        distances = sketch_truth.cos_distance(queries64[q], rows64[ordinary])
        assert np.all(bounds[q, ordinary] <= distances)


def test_prune_model_on_three_hops():
    bounds = np.full(10, -np.inf, dtype=np.float32)
    bounds[[1, 2, 3, 4, 5, 6, 7]] = [0.5, 0.25, 0.75, np.nan, 0.5, 0.125, 0.375]
    trace = [
        (False, 0.9, True, np.array([1, 2], dtype=np.uint32)),  # `top` not full yet: nothing is tested, whatever the bounds
        (True, 0.5, True, np.array([3, 1, 4, 0], dtype=np.uint32)),  # 0.75 and 0.5 reach the radius (>=), NaN and −inf prove nothing
        (True, 0.5, True, np.array([], dtype=np.uint32)),  # a hop that found nothing fresh
        (True, 0.375, True, np.array([5], dtype=np.uint32)),  # first tile of a long list …
        (True, 0.25, False, np.array([6, 7], dtype=np.uint32)),  # … its second tile against the radius the first one's commit left
    ]
    assert sketch_truth.prune_counts(trace, bounds) == (7, 4)
    assert sketch_truth.prune_counts(trace, None) == (0, 0), "a query that walks without the sketch"
    assert sketch_truth.prune_counts(trace, bounds + np.float32(0.25)) == (7, 5)  # 0.125 + 0.25 reaches 0.25
    assert sketch_truth.prune_counts(trace[:1], bounds) == (0, 0)


def test_record_decoder():
    record = np.zeros((1, 128), dtype=np.uint8)
    record[0, :124] = np.arange(1, 63, dtype=np.float16).view(np.uint8)
    record[0, 124:] = np.array([0.25], dtype=np.float32).view(np.uint8)
    halves, rho = sketch_truth.decode_records(record)
    assert np.array_equal(halves[0], np.arange(1, 63)) and rho[0] == 0.25
    other = record.copy()
    other[0, 2:4] = np.array([2.002], dtype=np.float16).view(np.uint8)
    other[0, 124:] = np.array([np.nextafter(np.float32(0.25), np.float32(1))], dtype=np.float32).view(np.uint8)
    assert sketch_truth.differences(record, other) == {"records": 1, "halves": 1, "largest_half_step": 1, "rho": 1, "largest_rho_step": 1}


@pytest.mark.parametrize("name", list(sketch_cases.CASES))
def test_prune_model_has_teeth(name):
    c = sketch_cases.case(name)
    count = sketch_cases.SINGLES
    queries, sums = c["queries"][:count], c["sums"][:count]
    bounds, used = sketch_cases.bounds_of(c, queries, sums, c["directions"], c["records"])
    assert used.all()
    swapped = c["records"].copy()
    swapped[:, 0:2], swapped[:, 2:4] = c["records"][:, 2:4], c["records"][:, 0:2]
    bounds_swapped, _ = sketch_cases.bounds_of(c, queries, sums, c["directions"], swapped)
    for expansion in (16, 64):
        for frontier in (1, 2):
            _, traces = sketch_cases.traced(name, expansion, frontier, count)
            tested, pruned = sketch_cases.model_counts(traces, bounds, used).sum(axis=0)
            totals = {label: int(sketch_cases.model_counts(traces, b, used)[:, 1].sum())
                      for label, b in (("+1e-3", bounds + np.float32(1e-3)), ("-1e-3", bounds - np.float32(1e-3)), ("columns 0 and 1 swapped", bounds_swapped))}
            print(f"{name}, expansion {expansion}, frontier {frontier}: tested {tested}, pruned {pruned}; pruned with the bounds moved: {totals}")
            assert 0 < pruned < tested, "a case that prunes nothing, or everything, tells nothing"
            assert totals["+1e-3"] > pruned and totals["-1e-3"] < pruned and totals["columns 0 and 1 swapped"] != pruned
