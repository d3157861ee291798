"""The model of clustering by the index's own levels (tests/cluster_model.py) against what the compiled reference recorded
(tests/golden/cluster/), hand-made cases of its merge and trace rules, and the names the feature adds to the libraries and the
binding. No GPU."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import usearch_amd
from tests import cluster_model, util
from tests.cluster_feeds import OracleFeed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cluster")
FIXTURES = sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))


def test_the_five_cases_are_recorded():
    assert [os.path.basename(path) for path in FIXTURES] == ["cos_f32_merges.npz", "hamming_b1_72_keys.npz", "l2sq_i8_merges.npz",
                                                             "min_count_zero.npz", "refine_colocated.npz"]
    largest = max(os.path.getsize(path) for path in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert all(os.path.getsize(path) <= largest for path in FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_model_over_the_oracle_equals_the_reference(path):
    fixture = np.load(path)
    metric, dtype, ndim = str(fixture["metric"]), str(fixture["dtype"]), int(fixture["ndim"])
    feed = OracleFeed(fixture["image"], fixture["vectors"], metric, dtype, ndim)
    run = feed.run_members if int(fixture["by_keys"]) else feed.run
    model = run(fixture["queries"], int(fixture["min_count"]), int(fixture["max_count"]))
    assert not model["popularity_ties"], "the fixture is not comparable: equal popularities"
    assert np.array_equal(model["keys"], fixture["cluster_keys"])
    if dtype in ("i8", "b1"):
        assert util.same_float_bits(model["distances"], fixture["cluster_distances"])
    else:
        error = np.abs(model["distances"].astype(np.float64) - fixture["cluster_distances"])
        assert np.all(error <= util.tolerance(dtype) * np.maximum(1.0, np.abs(fixture["cluster_distances"])))
        for winner, runner_up in model["margins"]:
            assert runner_up is None or abs(runner_up - winner) > util.tolerance(dtype) * max(1.0, abs(winner))
    assert model["clusters"] == int(fixture["clusters"])
    assert model["visited_members"] == int(fixture["visited_members"])
    assert model["computed_distances"] == int(fixture["computed_distances"])
    if os.path.basename(path) == "refine_colocated.npz":
        assert model["mapping_passes"] >= 2 and model["level"] == 1
    if os.path.basename(path) == "min_count_zero.npz":
        assert model["level"] == 1 and model["merge_cycles"] == 0


# ---- hand-made cases: entries on a line, the distance between two slots is the distance between their coordinates

def line(coordinates):
    return lambda a, b: abs(coordinates[a] - coordinates[b])


def entries_of(popularities, keys=None):
    return [dict(slot=slot, key=(keys[slot] if keys else 100 + slot), popularity=p) for slot, p in enumerate(popularities)]


def test_a_target_bubbles_over_several_entries():
    # order 0 1 2 3 4 by popularity 9 8 7 6 5; source 4 sits next to 3 on the line: 3 becomes 11 and passes 2, 1 and 0
    entries = entries_of([9, 8, 7, 6, 5])
    order, cycles, _ = cluster_model.merge(entries, 4, line([0.0, 10.0, 20.0, 30.0, 31.0]))
    assert cycles == 1 and [e["slot"] for e in order] == [3, 0, 1, 2] and entries[4]["merged_into"] == 3


def test_equal_popularities_do_not_swap():
    # 2 (popularity 3) takes 3 (popularity 2) and becomes 5, level with 1: strict `<`, it stays behind 1
    entries = entries_of([6, 5, 3, 2])
    order, _, _ = cluster_model.merge(entries, 3, line([0.0, 10.0, 20.0, 21.0]))
    assert [e["slot"] for e in order] == [0, 1, 2] and [e["popularity"] for e in order] == [6, 5, 5]


def test_of_equal_merge_distances_the_lowest_position_wins():
    entries = entries_of([5, 4, 3, 1])
    order, _, margins = cluster_model.merge(entries, 3, line([5.0, 15.0, 5.0, 10.0]))  # 3 is 5 away from 0, 1 and 2
    assert entries[3]["merged_into"] == 0 and margins == [(5.0, 5.0)]
    # nothing below FLT_MAX (NaN, +inf, FLT_MAX itself): position 0
    for nothing in (float("nan"), float("inf"), cluster_model.FLT_MAX):
        entries = entries_of([5, 4, 3, 1])
        cluster_model.merge(entries, 3, lambda a, b: nothing)
        assert entries[3]["merged_into"] == 0


def test_a_chain_in_the_trace_and_max_clusters_of_one():
    # 3 → 2, then 2 (the least popular even so) → 1, then 1 → 0: a query of 3 ends in 0 after three hops
    entries = entries_of([50, 20, 4, 3])
    order, cycles, _ = cluster_model.merge(entries, 1, line([0.0, 10.0, 19.0, 20.0]))
    merged_into = {e["slot"]: e["merged_into"] for e in entries}
    assert cycles == 3 and [e["slot"] for e in order] == [0] and merged_into == {0: None, 1: 0, 2: 1, 3: 2}
    assert cluster_model.trace(3, merged_into) == 0 and cluster_model.chain_length(3, merged_into) == 3
    assert order[0]["popularity"] == 77


def fake_index(reached, max_level=3, nodes=(100, 30, 8, 2)):
    """→ keyword arguments of `cluster_model.cluster`: query q reaches slot reached[level][q]; slots lie on a line at their number."""
    def descend(queries, level):
        slots = np.array(reached[level], dtype=np.uint32)
        return slots.astype(np.uint64) + 100, slots, np.zeros(len(slots), dtype=np.float32), np.full(len(slots), 2), np.full(len(slots), 7)
    return dict(max_level=max_level, nodes_at_or_above=lambda level: nodes[level], descend=descend,
                pair_distance=lambda a, b: float(abs(a - b)), query_distance=lambda q, slot: float(1000 * q + slot))


def test_max_below_min_is_legal_and_every_query_is_measured_again():
    reached = {2: [0, 0, 0, 1, 1, 5, 5, 5, 5, 9]}
    model = cluster_model.cluster(list(range(10)), min_clusters=4, max_clusters=2, **fake_index(reached))
    # level 2 (8 nodes > 4); U = 4 ≥ min; 9 (popularity 1) → 5, then 1 (popularity 2) → 0
    assert model["level"] == 2 and model["unique_before_merge"] == 4 and model["merge_cycles"] == 2 and model["clusters"] == 2
    assert model["keys"].tolist() == [100] * 5 + [105] * 5
    assert model["distances"].tolist() == [float(1000 * q + (0 if q < 5 else 5)) for q in range(10)]
    assert model["visited_members"] == 20 and model["computed_distances"] == 70 and not model["popularity_ties"]


def test_refinement_counts_every_pass_and_min_zero_merges_nothing():
    reached = {2: [3] * 6, 1: [3, 3, 3, 4, 4, 6]}
    model = cluster_model.cluster(list(range(6)), min_clusters=2, max_clusters=3, **fake_index(reached))
    assert model["level"] == 1 and model["mapping_passes"] == 2 and model["visited_members"] == 24 and model["merge_cycles"] == 0
    model = cluster_model.cluster(list(range(6)), **fake_index(reached))
    assert model["level"] == 1 and model["mapping_passes"] == 1 and model["clusters"] == 3 and model["merge_cycles"] == 0


def test_the_tie_rule_and_the_refusals():
    ordered, ties = cluster_model.order_entries(entries_of([2, 5, 2, 2], keys=[40, 10, 30, 20]))
    assert ties and [e["key"] for e in ordered] == [10, 20, 30, 40]
    assert not cluster_model.order_entries(entries_of([3, 2, 1]))[1]
    with pytest.raises(cluster_model.ClusteringError, match="max_clusters"):
        cluster_model.choose_level(3, lambda level: 10, 4, 0)
    with pytest.raises(cluster_model.ClusteringError, match="Index too small to cluster!"):
        cluster_model.choose_level(1, lambda level: 10, 4, 5)
    assert cluster_model.choose_level(3, lambda level: (100, 30, 8, 2)[level], 0, 0) == (1, 2, 30)
    assert cluster_model.choose_level(3, lambda level: (100, 30, 8, 2)[level], 1000, 5)[0] == 1


# ---- the names the feature adds

def test_the_engine_library_exports_clustering():
    library = ctypes.CDLL(usearch_amd.LIBRARY_PATH)
    for name in ("usearch_amd_clustering", "usearch_amd_clustering_members", "usearch_amd_snapshot_live_keys"):
        assert getattr(library, name) is not None
        assert name in usearch_amd.EXPORTED_SYMBOLS


def test_the_binding_mirrors_the_c_structs():
    """Field for field with `usearch_amd_clustering_config_t` / `usearch_amd_clustering_stats_t`: 3 × size_t; 6 × u64, 2 × u32, 3 × f32
    and the padding that rounds the struct up to its 8-byte alignment."""
    assert ctypes.sizeof(usearch_amd.ClusteringConfig) == 3 * ctypes.sizeof(ctypes.c_size_t)
    assert ctypes.sizeof(usearch_amd.ClusteringStats) == 6 * 8 + 2 * 4 + 3 * 4 + 4
    assert [name for name, _ in usearch_amd.ClusteringStats._fields_][:6] == ["clusters", "unique_before_merge", "merge_cycles",
                                                                              "mapping_passes", "visited_members", "computed_distances"]
    assert "level" in usearch_amd.ClusteringStats().as_dict() and "reserved" not in usearch_amd.ClusteringStats().as_dict()
    assert hasattr(usearch_amd.Index, "clustering") and hasattr(usearch_amd.BuiltIndex, "clustering")
    assert hasattr(usearch_amd.Index, "cluster")  # the single descent keeps its name
    for method in ("members_of", "subcluster", "centroids_popularity"):
        assert hasattr(usearch_amd.Clustering, method)


def test_the_drop_in_library_exports_clustering():
    library = ctypes.CDLL(os.path.join(os.path.dirname(usearch_amd.LIBRARY_PATH), "libusearch_c.so"))
    for name in ("usearch_clustering", "usearch_clustering_members"):
        assert getattr(library, name) is not None
    header = open(os.path.join(ROOT, "include", "usearch_c_dropin.h")).read()
    for name in ("usearch_clustering", "usearch_clustering_members"):  # declared under a macro of their own: the list of USEARCH_EXPORT
        assert f"USEARCH_CLUSTERING_API void {name}(" in header      # declarations and the function table are pinned by older tests
    library.usearch_amd_c_api.restype = ctypes.POINTER(ctypes.c_void_p)
    assert library.usearch_amd_c_api()[0] == 52


def build_cluster_surface(directory) -> str:
    lib = os.path.join(ROOT, "usearch_amd", "lib")
    binary = os.path.join(str(directory), "usearch_amd_cluster_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cluster_surface.cpp"), "-L", lib, "-l:libusearch_c.so", f"-Wl,-rpath,{lib}",
                           "-o", binary])
    return binary


def test_a_caller_of_cluster_compiles_against_the_class_surface(tmp_path):
    """Both iterator kinds of the reference's `cluster(begin, end, config, keys, distances)` compile and link against
    include/usearch/index_dense.hpp (run on the device by tests/test_gpu_clustering_dropin.py)."""
    binary = build_cluster_surface(tmp_path)
    assert "cluster through index_dense_t" in subprocess.check_output([binary, "link"]).decode()
