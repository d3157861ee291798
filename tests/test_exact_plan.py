"""The tiled exact search's launch planner (csrc/exact_plan.hpp) through its test hook, no GPU in the loop: which of the two
matrix-unit kernels a batch takes, how the rows are split into partitions, and — for the wide kernel, whose workgroups find their
(query tile, partition) by arithmetic on `blockIdx.x` — that the workgroups launched cover every pair exactly once. A pair nobody
takes would lose that partition's rows for 256 queries, silently: the merge takes whatever lists it finds."""
import itertools

import pytest

ROWS = [1, 511, 512, 8191, 8192, 8200, 9000, 12001, 20011, 10 ** 6, 7 * 10 ** 7]
COUNTS = list(range(1, 601)) + [1792, 1793, 2049, 8192, 8193, 40000]
WANTED = [1, 10, 11, 16, 17, 64]
TILES = [0, 64, 256]
BYTES, STRIDE = 192, 192  # 96-d f16: what the split does not depend on (the two 31-bit limits have their own rows in the table)

# The documented route (exact_tiled.hip): the wide tile takes a batch unless the 64 tile is forced, when it wants at
# most 16 results, the index has at least 8 192 rows (eight partitions of four 256-row tiles), the batch has more than 512 queries
# or the wide tile is forced, and 256 rows, stored or padded to whole 128-byte chunks, stay below 2^31 bytes. Restated as the rows on
# either side of every boundary: (rows, bytes per vector, row stride, queries, wanted, forced tile) → wide
WIDE_TABLE = [
    ((8192, BYTES, STRIDE, 513, 16, 0), True),
    ((8191, BYTES, STRIDE, 513, 16, 0), False),     # one row short
    ((8192, BYTES, STRIDE, 512, 16, 0), False),     # one query short …
    ((8192, BYTES, STRIDE, 512, 16, 256), True),    # … unless forced
    ((8192, BYTES, STRIDE, 1, 1, 256), True),
    ((8192, BYTES, STRIDE, 513, 17, 0), False),     # one result too many …
    ((8192, BYTES, STRIDE, 513, 17, 256), False),   # … forced or not
    ((8192, BYTES, STRIDE, 40000, 64, 256), False),
    ((8191, BYTES, STRIDE, 513, 10, 256), False),   # forcing does not shrink the least index
    ((8192, BYTES, STRIDE, 40000, 10, 64), False),  # the 64 tile forced
    ((7 * 10 ** 7, BYTES, STRIDE, 513, 16, 0), True),
    ((8192, 16, 16, 513, 16, 0), True),             # a 16-byte row
    ((8192, 2 ** 23 - 128, 2 ** 23 - 128, 513, 16, 0), True),   # 256 rows: 2^31 − 2^15 bytes
    ((8192, 2 ** 23 - 128, 2 ** 23, 513, 16, 0), False),        # 256 stored rows reach 2^31
    ((8192, 2 ** 23 - 120, 2 ** 23 - 112, 513, 16, 0), False),  # 256 padded queries reach 2^31
]
LEAST_ROWS, MOST_WANTED, MOST_NARROW_COUNT, LDS_LIST_WANTED = 8192, 16, 512, 10  # the table's boundaries, for the sweep


def plan(rows, count, wanted, tile, nbytes=BYTES, stride=STRIDE, global_lists=False):
    from usearch_amd.index import test_plan_exact
    return test_plan_exact(rows, nbytes, stride, count, wanted, forced_tile=tile, global_lists=global_lists)


def wide_pairs(p):
    """exact_wide_kernel's mapping from `blockIdx.x` to (query tile, partition), restated: workgroups go to the eight XCDs round-robin;
    a batch of ≥ 8 query tiles is dealt over them (tile = 8·g + xcd), a smaller one is handled whole by every XCD (partitions ≡ xcd
    mod 8); a workgroup whose tile lies past the batch returns at once. → the pairs of the workgroups that stay."""
    tiles, per_xcd = p["query_tiles"], p["tiles_per_xcd"]
    pairs = []
    for block in range(p["workgroups"]):
        xcd, sequence = block % 8, block // 8
        if tiles >= 8:
            pair = ((sequence % per_xcd) * 8 + xcd, sequence // per_xcd)
        else:
            pair = (sequence % per_xcd, sequence // per_xcd * 8 + xcd)
        if pair[0] < tiles:
            pairs.append(pair)
    return pairs


@pytest.mark.parametrize("shape,wide", WIDE_TABLE, ids=["-".join(map(str, shape)) for shape, _ in WIDE_TABLE])
def test_the_wide_tile_is_chosen_at_its_documented_boundaries(shape, wide):
    rows, nbytes, stride, count, wanted, tile = shape
    assert bool(plan(rows, count, wanted, tile, nbytes, stride)["wide"]) == wide


@pytest.mark.parametrize("rows", ROWS)
def test_every_plan_covers_the_rows_and_every_pair_once(rows):
    for count, wanted, tile in itertools.product(COUNTS, WANTED, TILES):
        p = plan(rows, count, wanted, tile)
        what = (rows, count, wanted, tile, p)
        wide = tile != 64 and wanted <= MOST_WANTED and rows >= LEAST_ROWS and (tile == 256 or count > MOST_NARROW_COUNT)
        assert bool(p["wide"]) == wide, what
        tile_rows, tile_queries = (256, 256) if wide else (128, 64)
        assert p["query_tiles"] == -(-count // tile_queries), what
        assert p["rows_per_partition"] > 0 and p["rows_per_partition"] % tile_rows == 0, what
        assert p["partitions"] >= 1 and p["partitions"] * p["rows_per_partition"] >= rows, what
        if not wide:
            assert (p["partitions"] - 1) * p["rows_per_partition"] < rows, ("an empty partition on the 64 route", what)
            assert p["partitions"] <= 65535, what  # gridDim.y
            continue
        assert bool(p["lds_lists"]) == (wanted <= LDS_LIST_WANTED), what
        pairs = wide_pairs(p)
        assert len(pairs) == len(set(pairs)) == p["query_tiles"] * p["partitions"], ("a pair taken twice or not at all", what)
        assert set(pairs) == set(itertools.product(range(p["query_tiles"]), range(p["partitions"]))), what


def test_the_shapes_the_gpu_tests_lean_on():
    """n = 8 200: eight partitions of 1 280 rows, the seventh ragged, the last one empty; n = 8 192: eight full ones. 1 793 queries:
    eight query tiles, dealt over the XCDs; 2 049: nine, the last round of workgroups one tile long."""
    p = plan(8200, 300, 10, 256)
    assert (p["partitions"], p["rows_per_partition"], p["tiles_per_xcd"], p["workgroups"]) == (8, 1280, 2, 16)
    assert 6 * 1280 < 8200 < 7 * 1280
    p = plan(8192, 300, 10, 256)
    assert (p["partitions"], p["rows_per_partition"]) == (8, 1024)
    p = plan(8200, 1793, 10, 0)
    assert p["wide"] and (p["query_tiles"], p["tiles_per_xcd"], p["workgroups"]) == (8, 1, 8 * p["partitions"])
    p = plan(8200, 2049, 10, 0)
    assert p["wide"] and (p["query_tiles"], p["tiles_per_xcd"]) == (9, 2)
    assert p["workgroups"] == 16 * p["partitions"] and len(wide_pairs(p)) == 9 * p["partitions"]  # seven of sixteen return early


def test_the_global_lists_switch_moves_the_lists_out_of_lds():
    assert plan(8200, 300, 10, 256)["lds_lists"] == 1
    assert plan(8200, 300, 10, 256, global_lists=True)["lds_lists"] == 0
    assert plan(8200, 300, 11, 256)["lds_lists"] == 0


@pytest.mark.parametrize("wanted", [0, 65])
def test_result_counts_without_a_kernel_are_refused(wanted):
    with pytest.raises(RuntimeError, match="No tiled exact-search kernel for this metric / scalar kind / result count"):
        plan(8200, 300, wanted, 0)


def test_the_hook_reads_the_environment_like_the_engine(monkeypatch):
    from usearch_amd.index import test_plan_exact
    for name in ("USEARCH_AMD_EXACT_TILE", "USEARCH_AMD_EXACT_GLOBAL_LISTS"):
        monkeypatch.delenv(name, raising=False)
    assert test_plan_exact(8200, BYTES, STRIDE, 300, 10)["wide"] == 0
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", "256")
    assert test_plan_exact(8200, BYTES, STRIDE, 300, 10) == plan(8200, 300, 10, 256)
    monkeypatch.setenv("USEARCH_AMD_EXACT_GLOBAL_LISTS", "1")
    assert test_plan_exact(8200, BYTES, STRIDE, 300, 10) == plan(8200, 300, 10, 256, global_lists=True)
    monkeypatch.setenv("USEARCH_AMD_EXACT_TILE", "64")
    assert test_plan_exact(8200, BYTES, STRIDE, 700, 10)["wide"] == 0
