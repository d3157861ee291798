"""The device's sketch records (usearch_amd/csrc/sketch.hip `sketch_records_kernel`) against a float64 truth (tests/sketch_truth.py) and
against their host twin (sketch.hpp `sketch_record_host`), bit for bit.

The shapes are the smallest that cross every edge of the kernel: 600 rows = two full tiles of 256 and a ragged one of 88; `first` = 0
and 344 (no multiple of 256: the first block starts inside a tile of the run from 0 and nothing below row 344 may be written);
f16 / bf16 rows of 768 and 777 elements (777: a ragged last step of 16, row bytes no multiple of 16), f32 rows of 384 (1 536 bytes, the
shortest eligible) and 389; low-rank rows with noise, EXACTLY rank-10 rows (the residual is what f16 leaves of the coefficients and
the 1e-9 under the root carries the proof), i.i.d. Gaussian rows; the edge rows of tests/test_sketch_bound.py; directions drawn by the
twin from the same rows, and once from 40 rows only, so that fewer than 62 directions exist and the columns behind them are zero.

Every set of records is held to `sketch_truth.check_records`: sound (ρ ≥ the true residual, no tolerance), tight (ρ no more than the
closing arithmetic can make of it), every coefficient an f16 neighbour of the true one, the never-pruned rows, equal records for
equal rows. Then the snapshots: the sketch read back from an index as built, after `extend` (the records move to a larger array and are
appended at a `first` that is no tile boundary), after a second `extend` (into spare room) and after `update` (made anew) must equal
what the kernel gives for the snapshot's current rows under the snapshot's own directions, and pass the truth."""
from __future__ import annotations

import numpy as np
import pytest

import usearch_amd.index as ua_index
from tests import sketch_truth, util

pytestmark = pytest.mark.gpu

ROWS, FIRST, PATTERN = 600, 344, 0xA5
F16_LARGEST, F16_SMALLEST_NORMAL = 65504.0, 2.0 ** -14
ZERO_ROWS, NAN_ROW, INF_ROW = (5, 500), 77, 350
LARGE_ROW, SMALL_ROW, UNDERFLOWING_ROW, OVERFLOWING_ROW = 300, 301, 302, 303
DUPLICATES = ((400, 10), (401, 10), (599, 598))
SHAPES = [("f16", 768), ("f16", 777), ("bf16", 768), ("bf16", 777), ("f32", 384), ("f32", 389)]


def _store(x: np.ndarray, dtype: str) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        return np.ascontiguousarray(util.to_bf16(x) if dtype == "bf16" else x.astype(util.NP_DTYPE[dtype]))


def dataset(kind: str, ndim: int, dtype: str):
    """→ (rows in the storage kind, the rows that are never pruned)."""
    rng = np.random.default_rng(4000 + ndim)
    if kind == "lowrank":
        rows = sketch_truth.widen(util.make_vectors(ROWS, ndim, dtype, seed=4000 + ndim), dtype)
    elif kind == "rank10":
        rows = rng.standard_normal((ROWS, 10)) @ rng.standard_normal((10, ndim))
    else:
        rows = rng.standard_normal((ROWS, ndim))
    rows[LARGE_ROW] *= F16_LARGEST / np.abs(rows[LARGE_ROW]).max()
    rows[SMALL_ROW] *= F16_SMALLEST_NORMAL / np.abs(rows[SMALL_ROW]).max()
    never = ZERO_ROWS + (NAN_ROW, INF_ROW)
    if dtype == "f32":  # (f16 stores these as zeros and infinities: the cases above)
        rows[UNDERFLOWING_ROW] *= 1e-20 / np.abs(rows[UNDERFLOWING_ROW]).max()
        rows[OVERFLOWING_ROW] *= 1e18 / np.abs(rows[OVERFLOWING_ROW]).max()
        never += (UNDERFLOWING_ROW, OVERFLOWING_ROW)
    for copy, original in DUPLICATES:
        rows[copy] = rows[original]
    for row in ZERO_ROWS:
        rows[row] = 0.0
    rows[NAN_ROW, ndim // 2] = np.nan
    rows[INF_ROW, 1] = np.inf
    return _store(rows, dtype), never


def assert_same_records(device: np.ndarray, twin: np.ndarray, what: str):
    difference = sketch_truth.differences(device, twin)
    print(f"{what}: device against twin, records that differ: {difference}")
    assert np.array_equal(device, twin), f"{what}: the device's records differ from the twin's: {difference}"


def hold(rows: np.ndarray, dtype: str, directions: np.ndarray, defect: float, never, duplicates, what: str):
    """Records of `rows` from the device, from `first` = 0 and from 344, against the truth and the twin."""
    rows64 = sketch_truth.widen(rows, dtype)
    device = ua_index.test_sketch_device_records(rows, dtype, directions, defect, first=0, pattern=PATTERN)
    figures = sketch_truth.check_records(rows64, directions, defect, device, never, duplicates, f"{what}, device")
    assert_same_records(device, ua_index.test_sketch_twin_records(rows, dtype, directions, defect), what)
    later = ua_index.test_sketch_device_records(rows, dtype, directions, defect, first=FIRST, pattern=PATTERN)
    assert np.all(later[:FIRST] == PATTERN), f"{what}: records below `first` were written"
    assert np.array_equal(later[FIRST:], device[FIRST:]), f"{what}: records from row {FIRST} on differ from those of the run from row 0"
    return figures


@pytest.mark.parametrize("kind", ["lowrank", "rank10", "gaussian"])
@pytest.mark.parametrize("dtype,ndim", SHAPES)
def test_device_records_against_the_truth_and_the_twin(dtype, ndim, kind):
    rows, never = dataset(kind, ndim, dtype)
    directions, rank, defect = ua_index.test_sketch_directions(rows, dtype)
    assert rank == sketch_truth.rank_of(directions)
    # (f32 keeps rank-10 rows rank 10 up to a rounding direction or two: the columns behind stay zero; f16 / bf16 rounding adds directions)
    assert 10 <= rank <= (12 if kind == "rank10" and dtype == "f32" else 62)
    hold(rows, dtype, directions, defect, never, DUPLICATES, f"{kind} {ndim} {dtype}, {rank} directions")


@pytest.mark.parametrize("dtype,ndim", [("f16", 777), ("f32", 389)])
def test_fewer_than_62_directions(dtype, ndim):
    rows, never = dataset("lowrank", ndim, dtype)
    directions, rank, defect = ua_index.test_sketch_directions(rows[:40], dtype)
    assert 10 <= rank <= 40 and not directions[:, rank:].any(), "directions from 40 sample rows (seeded slots repeat: fewer than 40)"
    hold(rows, dtype, directions, defect, never, DUPLICATES, f"lowrank {ndim} {dtype}, {rank} directions")


def _read_back_and_hold(built, dtype: str, expected_rows: np.ndarray, fresh: bool, what: str):
    index = built.index
    assert index.arrays.sketch == 1, f"{what}: the snapshot has no sketch"
    records, directions, defect, row_bytes = ua_index.test_sketch_read_back(index)
    rows = row_bytes.view(np.uint16 if dtype == "bf16" else util.NP_DTYPE[dtype])
    assert len(records) == len(index) == len(expected_rows)
    assert np.array_equal(rows.view(np.uint8), np.ascontiguousarray(expected_rows).view(np.uint8)), f"{what}: the stored rows are not the caller's"
    if fresh:  # made anew from these rows: the directions are the ones the twin draws from them
        drawn, _, drawn_defect = ua_index.test_sketch_directions(rows, dtype)
        assert np.array_equal(drawn, directions) and drawn_defect == defect, f"{what}: directions other than the twin draws"
    sketch_truth.check_records(sketch_truth.widen(rows, dtype), directions, defect, records, (), ((len(rows) - 1, 7),), f"{what}, snapshot")
    expected = ua_index.test_sketch_device_records(rows, dtype, directions, defect)
    difference = sketch_truth.differences(records, expected)
    print(f"{what}: snapshot against the kernel over its current rows: {difference}")
    assert np.array_equal(records, expected), f"{what}: {difference}"
    assert_same_records(records, ua_index.test_sketch_twin_records(rows, dtype, directions, defect), what)


@pytest.mark.parametrize("dtype,ndim", [("f16", 777), ("f32", 389)])
def test_snapshot_sketch_as_built_extended_and_updated(dtype, ndim):
    import usearch_amd
    n = 3000
    pool = util.make_vectors(n + 150 + 3, ndim, dtype, seed=4100 + ndim)

    def with_duplicate(rows):  # the last row repeats row 7: equal rows, equal records, wherever the last row's record was made
        rows = rows.copy()
        rows[-1] = pool[7]
        return rows
    rows = with_duplicate(pool[:n])
    built = usearch_amd.build(rows, "cos", dtype, keys=np.arange(n, dtype=np.uint64), seed=41, connectivity=16)
    try:
        _read_back_and_hold(built, dtype, rows, True, f"{ndim} {dtype} as built")
        more = with_duplicate(pool[n:n + 100])
        built.extend(more, np.arange(n, n + 100, dtype=np.uint64))
        rows = np.concatenate([rows, more])
        _read_back_and_hold(built, dtype, rows, False, f"{ndim} {dtype} extended by 100 (first = {n})")
        more = with_duplicate(pool[n + 100:n + 150])
        built.extend(more, np.arange(n + 100, n + 150, dtype=np.uint64))
        rows = np.concatenate([rows, more])
        _read_back_and_hold(built, dtype, rows, False, f"{ndim} {dtype} extended by 50 more (first = {n + 100})")
        slots = np.array([3, 1500, 3100], dtype=np.uint32)
        rows[slots] = pool[n + 150:]
        built.update(slots, pool[n + 150:], slots.astype(np.uint64))
        _read_back_and_hold(built, dtype, rows, True, f"{ndim} {dtype} after an update of three rows")
    finally:
        built.close()
