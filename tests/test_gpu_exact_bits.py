"""GPU: the bit tile (csrc/exact_bits.hip) — batched exact search for hamming, tanimoto and sorensen over b1 — on every route that
reaches it, held to BOTH a numpy truth (tests/exact_truth_bits.py: keys, distance bits and counts for every query) and the
wave-per-query kernel that `exact=True` runs on the same index (bit for bit, NaN cells included: both run on the same hardware).
Hamming distances are small integers, so nearly every query has ties at rank k (tests/test_exact_truth_bits.py asserts the shares):
what these cases check above all is the one order — NaN first, distance ↑, the later slot first among equals."""
import functools

import numpy as np
import pytest

from tests import exact_truth_bits as bits
from tests import util

pytestmark = pytest.mark.gpu
REFUSAL = "No tiled exact-search kernel for this metric / scalar kind / result count"
FIRST_KEY = 1000  # `util.build_image` numbers its members from here, in slot order


@functools.lru_cache(maxsize=None)
def index_of(metric: str, ndim: int, rows: int, removed_every: int = 0):
    """The rows of `bits.data(ndim, rows)` as an index (the graph is irrelevant here: the reference builds a thin one), with the
    member in every `removed_every`-th slot from slot 3 on removed → (index, allowed [rows])."""
    from usearch_amd import Index
    vectors = np.array(bits.data(ndim, rows)[0])
    removed = np.arange(3, rows, removed_every) if removed_every else np.zeros(0, dtype=np.int64)
    image, _, _ = util.build_image(rows, ndim, metric, "b1", vectors=vectors, connectivity=4, expansion_add=16, remove=removed + FIRST_KEY)
    allowed = np.ones(rows, dtype=bool)
    allowed[removed] = False
    return Index.restore(image), allowed


def assert_both(index, truth, queries, k, filter=None):
    """`exact="tiled"` against the truth and against `exact=True` on the same index → the tiled result."""
    tiled = index.search(queries, k, exact="tiled", filter=filter)
    wave = index.search(queries, k, exact=True, filter=filter)
    assert np.array_equal(tiled.counts, wave.counts) and np.array_equal(tiled.keys, wave.keys), "the wave kernel names other rows"
    assert util.same_float_bits(tiled.distances, wave.distances), "the wave kernel's distances carry other bits"
    truth.check(tiled.keys.astype(np.int64) - FIRST_KEY, tiled.distances, tiled.counts, k, padding=tiled.keys)
    return tiled


def assert_partitions(index, rows, count, k, more_than_one=True):
    """Through the planner's test hook: the split this case is there for is the one that runs."""
    from usearch_amd.index import test_plan_exact_bits
    plan = test_plan_exact_bits(rows, index.bytes_per_vector, index.row_stride, count, k)
    assert (plan["partitions"] > 1) == more_than_one, plan
    return plan


@pytest.mark.parametrize("metric,ndim", [("hamming", 128), ("tanimoto", 128), ("sorensen", 128), ("hamming", 8), ("hamming", 72),
                                         ("hamming", 136), ("hamming", 1024), ("hamming", 2056), ("tanimoto", 8), ("tanimoto", 72),
                                         ("tanimoto", 1024), ("sorensen", 8)])
def test_every_metric_and_row_length(reference, metric, ndim):
    """One 16-byte piece (8, 72, 128 bits, the last byte of 72 … whole), a second piece one byte long (136), eight pieces (1 024),
    sixteen and one byte (2 056); at 8 dimensions the empty rows and the empty query bring 0 / 0."""
    index, _ = index_of(metric, ndim, bits.ROWS)
    queries = bits.data(ndim)[1]
    assert_partitions(index, bits.ROWS, len(queries), bits.K)
    got = assert_both(index, bits.truth(metric, ndim), queries, bits.K)
    if ndim == 8 and metric != "hamming":
        empty = ~queries.any(axis=1)  # the last query, and whichever the generator left without a bit
        assert empty[-1] and np.isnan(got.distances[empty]).all() and not np.isnan(got.distances[~empty]).any(), \
            "an empty query meets 25 empty rows, nobody else divides by zero"


@pytest.mark.parametrize("rows,count,k,several", [(9000, 300, 10, True), (100, 65, 64, False), (40, 65, 64, False)])
def test_ragged_tiles_few_rows_and_fewer_rows_than_results(reference, rows, count, k, several):
    """9 000 rows: 29 partitions of 320, the last one of 40 rows (less than a step of 64); 100 rows: one step and a ragged one;
    40 rows for 64 results: every query returns all 40, in order, and 24 padding cells."""
    index, _ = index_of("hamming", 128, rows)
    queries = bits.data(128, rows, count)[1]
    assert_partitions(index, rows, count, k, several)
    got = assert_both(index, bits.truth("hamming", 128, rows, count), queries, k)
    assert np.all(got.counts == min(rows, k))


@pytest.mark.parametrize("count", [1, 63, 65, 300, 600])
def test_batches_that_end_inside_a_wave_and_inside_a_workgroup(reference, count):
    """A wave owns 64 queries and a workgroup four waves: 1 and 63 leave a wave short, 65 starts a second one, 300 a second workgroup
    with one full wave and one of 44, 600 a third."""
    index, _ = index_of("hamming", 128, bits.ROWS)
    queries = bits.data(128, bits.ROWS, 600)[1][:count]
    assert_both(index, bits.truth("hamming", 128, bits.ROWS, 600).restricted(count), queries, bits.K)


@pytest.mark.parametrize("k", [1, 16, 17, 64])
def test_result_counts(reference, k):
    index, _ = index_of("tanimoto", 128, bits.ROWS)
    assert_both(index, bits.truth("tanimoto", 128).restricted(65), bits.data(128)[1][:65], k)


def test_result_counts_without_a_kernel(reference):
    """65 results are refused by name. 0 results never reach a kernel on any route (the snapshot returns before it looks at the pair,
    for `exact=True` too): that the PLANNER refuses 0 is tests/test_exact_bits_plan.py's."""
    index, _ = index_of("hamming", 128, bits.ROWS)
    queries = bits.data(128)[1][:5]
    with pytest.raises(RuntimeError, match=REFUSAL):
        index.search(queries, 65, exact="tiled")
    assert index.search(queries, 0, exact="tiled").keys.shape == index.search(queries, 0, exact=True).keys.shape == (5, 0)


def test_removed_members_are_never_returned(reference):
    index, allowed = index_of("hamming", 128, bits.ROWS, removed_every=11)
    assert 400 < int((~allowed).sum()) < 500
    got = assert_both(index, bits.truth("hamming", 128).restricted(allowed=allowed), bits.data(128)[1], bits.K)
    assert not np.isin(got.keys, np.flatnonzero(~allowed) + FIRST_KEY).any()


@pytest.mark.parametrize("metric", ["hamming", "sorensen"])
@pytest.mark.parametrize("few", [False, True])
def test_a_filter_decides_who_is_scanned(reference, metric, few):
    """About half the rows, and three rows — the first, one in the middle, the last — for ten results: three found, seven cells of
    padding."""
    index, _ = index_of(metric, 128, bits.ROWS)
    allowed = np.zeros(bits.ROWS, dtype=bool)
    if few:
        allowed[[0, 2500, bits.ROWS - 1]] = True
    else:
        allowed[:] = np.random.default_rng(5).random(bits.ROWS) < 0.5
    got = assert_both(index, bits.truth(metric, 128).restricted(allowed=allowed), bits.data(128)[1], bits.K, filter=index.filter_bits(allowed))
    assert np.all(got.counts == (3 if few else bits.K))


def test_forty_copies_across_a_partition_edge_come_back_latest_slot_first(reference):
    from usearch_amd import Index
    rows = np.array(bits.data(128)[0])
    rows[300:340] = rows[7]
    image, _, _ = util.build_image(len(rows), 128, "hamming", "b1", vectors=rows, connectivity=4, expansion_add=16)
    index = Index.restore(image)
    queries = np.ascontiguousarray(rows[[7, 8]])
    plan = assert_partitions(index, len(rows), len(queries), 64)
    assert 300 // plan["rows_per_partition"] != 339 // plan["rows_per_partition"] and 300 // 64 != 339 // 64, "no edge between the copies"
    got = assert_both(index, bits.BitsTruth("hamming", rows, queries), queries, 64)
    assert np.array_equal(got.keys[0, :41], np.concatenate([np.arange(339, 299, -1), [7]]) + FIRST_KEY) and np.all(got.distances[0, :41] == 0)


def unaligned_view(queries: np.ndarray):
    """The same rows as a view at byte offset 1 of a wider buffer, 24 bytes apart."""
    count, width = queries.shape
    buffer = np.zeros(count * (width + 8) + 1, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buffer[1:], shape=(count, width), strides=(width + 8, 1))
    view[:] = queries
    assert view.ctypes.data % 2 == 1 and view.strides[0] % 16
    return buffer, view


@pytest.mark.parametrize("metric", ["hamming", "jaccard"])
def test_raw_datasets(metric):
    """`usearch_amd.exact_search(…, tiled=True)` over rows that are no index: keys are row offsets, equal to the untiled call —
    strided, unaligned query rows, and jaccard, which runs as tanimoto."""
    import usearch_amd
    rows, queries = bits.data(128)
    _, view = unaligned_view(queries[:70])
    keys, distances = usearch_amd.exact_search(rows, view, 5, metric=metric, dtype="b1", tiled=True)
    wave_keys, wave_distances = usearch_amd.exact_search(rows, view, 5, metric=metric, dtype="b1")
    assert np.array_equal(keys, wave_keys) and util.same_float_bits(distances, wave_distances)
    bits.truth(metric, 128).restricted(70).check(keys.astype(np.int64), distances, np.full(70, 5), 5)


@pytest.mark.parametrize("metric,ndim", [("tanimoto", 128), ("hamming", 136)])
def test_the_device_route_takes_unaligned_strided_queries(reference, metric, ndim):
    """`exact_search_device(tiled=True)` on torch tensors, the queries a view at byte offset 1 of a wider buffer (the kernel that pads
    the batch reads it byte by byte): equal to the host route."""
    import torch
    index, _ = index_of(metric, ndim, bits.ROWS)
    queries = bits.data(ndim)[1]
    buffer, view = unaligned_view(queries)
    device = torch.device("cuda", 0)
    held = torch.from_numpy(buffer).to(device)
    keys = torch.zeros((len(queries), bits.K), dtype=torch.int64, device=device)
    distances = torch.zeros((len(queries), bits.K), dtype=torch.float32, device=device)
    counts = torch.zeros(len(queries), dtype=torch.int64, device=device)
    torch.cuda.synchronize()
    index.exact_search_device(held.data_ptr() + 1, len(queries), view.strides[0], bits.K, keys.data_ptr(), distances.data_ptr(),
                              counts.data_ptr(), tiled=True)
    torch.cuda.synchronize()
    host = assert_both(index, bits.truth(metric, ndim), queries, bits.K)
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), host.keys) and np.array_equal(counts.cpu().numpy().view(np.uint64), host.counts)
    assert util.same_float_bits(distances.cpu().numpy(), host.distances)


@pytest.mark.parametrize("metric,dtype", [("l2sq", "f32"), ("pearson", "f32")])
def test_pairs_without_a_tiled_kernel_are_still_refused(reference, metric, dtype):
    from usearch_amd import Index
    image, _, _ = util.build_image(60, 16, metric, dtype, seed=3)
    with pytest.raises(RuntimeError, match=REFUSAL):
        Index.restore(image).search(util.make_vectors(4, 16, dtype, seed=4), 3, exact="tiled")
