"""Python host side of the MI355X search engine: a thin ctypes binding over the C ABI of `include/usearch_amd.h`.

It mirrors the *search* surface of the reference's Python package (`/root/reference/python/usearch/index.py`):
`Index.restore(path_or_buffer)` (index.py:574-630) gives an object whose `search(vectors, count, ...)` has the argument
meaning of `Index.search` (index.py:700-748) and returns `Matches` / `BatchMatches` shaped like index.py:291-385 —
row-major `keys[Q, k]` (u64), `distances[Q, k]` (f32), `counts[Q]`, plus the two traversal counters. Everything else of
that package (add / remove …) stays with the reference: this engine consumes the index files it writes. `Index.join`
(index.py:1170-1200) runs on the device: preference lists from the batched search, the matching as HIP kernels.

There is no CPU fallback: without `libusearch_amd.so` or without a HIP device, constructing an `Index` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Optional, Union

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# USEARCH_AMD_LIBRARY names an experimental build of the same library (scripts/ A/B runs); the product is the in-tree one
LIBRARY_PATH = os.environ.get("USEARCH_AMD_LIBRARY") or os.path.join(HERE, "lib", "libusearch_amd.so")

# `usearch_scalar_kind_t` / `usearch_metric_kind_t` of c/usearch.h:40-62
SCALAR_KINDS = {"f32": 1, "f64": 2, "f16": 3, "i8": 4, "b1": 5, "bf16": 6}
SCALAR_NAMES = {v: k for k, v in SCALAR_KINDS.items()}
METRIC_NAMES = {1: "cos", 2: "ip", 3: "l2sq", 4: "haversine", 5: "divergence", 6: "pearson", 7: "jaccard",
                8: "hamming", 9: "tanimoto", 10: "sorensen"}
NUMPY_DTYPES = {"f32": np.float32, "f64": np.float64, "f16": np.float16, "i8": np.int8, "b1": np.uint8,
                "bf16": np.uint16}  # numpy has no bfloat16: bf16 rows are handed over as their uint16 bit patterns


def _infer_dtype(array: np.ndarray) -> str:
    """Scalar kind of a numpy array when the caller did not name it: `uint8` means bit-packed `b1` rows; `bf16` has no
    numpy dtype and must always be named (`dtype="bf16"` with a `uint16` array)."""
    dtype = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64", np.dtype(np.float16): "f16",
             np.dtype(np.int8): "i8", np.dtype(np.uint8): "b1"}.get(array.dtype)
    if dtype is None:
        raise ValueError(f"Unsupported dtype {array.dtype}")
    return dtype


class Tuning(C.Structure):
    """`usearch_amd_tuning_t`."""
    _fields_ = [("hash_cap", C.c_uint32), ("next_cap", C.c_uint32), ("variant", C.c_uint32), ("mode", C.c_uint32),
                ("waves_per_cu", C.c_uint32), ("frontier", C.c_uint32), ("wave_clock", C.c_uint32), ("sketch", C.c_uint32)]


class Stats(C.Structure):
    """`usearch_amd_stats_t`."""
    _fields_ = [("passes", C.c_uint32), ("retried_lds", C.c_uint32), ("retried_global", C.c_uint32),
                ("kernel_ms", C.c_float), ("mode", C.c_uint32), ("grid", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("frontier", C.c_uint32), ("variant", C.c_uint32), ("tail_idle", C.c_float), ("span_ms", C.c_float),
                ("top_cells", C.c_uint32), ("probe_mode", C.c_uint32), ("seen_cells", C.c_uint32), ("claim_bits", C.c_uint32),
                ("early_rows", C.c_uint32), ("plain", C.c_uint32), ("aside_cells", C.c_uint32),
                ("sketch_tested", C.c_uint64), ("sketch_pruned", C.c_uint64)]


class Arrays(C.Structure):
    """`usearch_amd_arrays_t`: device pointers and shapes of a snapshot's HBM arrays."""
    _fields_ = [("vectors", C.c_void_p), ("level0", C.c_void_p), ("keys", C.c_void_p), ("size", C.c_uint64),
                ("row_stride", C.c_uint32), ("level0_cells", C.c_uint32), ("device", C.c_int), ("sketch", C.c_uint32)]


class JoinConfig(C.Structure):
    """`usearch_amd_join_config_t`; zeros = the reference's defaults."""
    _fields_ = [("max_proposals", C.c_uint64), ("expansion", C.c_uint64), ("exact", C.c_uint32), ("threads", C.c_uint32)]


class JoinStats(C.Structure):
    """`usearch_amd_join_stats_t`."""
    _fields_ = [("pairs", C.c_uint64), ("rounds", C.c_uint64), ("proposals", C.c_uint64), ("engagements", C.c_uint64),
                ("visited_members", C.c_uint64), ("computed_distances", C.c_uint64), ("max_proposals", C.c_uint64),
                ("expansion", C.c_uint64), ("list_width", C.c_uint64), ("lazy_searches", C.c_uint64), ("a_proposes", C.c_uint32),
                ("frontier", C.c_uint32), ("seconds_lists", C.c_double), ("seconds_matching", C.c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class KMeansConfig(C.Structure):
    """`usearch_amd_kmeans_config_t`."""
    _fields_ = [("struct_bytes", C.c_uint64), ("metric_kind", C.c_int), ("quantization_kind", C.c_int), ("max_iterations", C.c_uint64),
                ("inertia_threshold", C.c_double), ("max_seconds", C.c_double), ("min_shifts", C.c_double), ("seed", C.c_uint64),
                ("device", C.c_int)]


class KMeansStats(C.Structure):
    """`usearch_amd_kmeans_stats_t`."""
    _fields_ = [("iterations", C.c_uint64), ("last_iteration_points_shifted", C.c_uint64), ("computed_distances", C.c_uint64),
                ("last_iteration_inertia", C.c_double), ("aggregate_distance", C.c_double), ("runtime_seconds", C.c_double),
                ("assign_ms", C.c_float), ("update_ms", C.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class BuildConfig(C.Structure):
    """`usearch_amd_build_config_t`; zeros = the reference's defaults."""
    _fields_ = [("connectivity", C.c_uint32), ("connectivity_base", C.c_uint32), ("expansion_add", C.c_uint32),
                ("batch_divisor", C.c_uint32), ("max_batch", C.c_uint32), ("reserved", C.c_uint32),
                ("seed", C.c_uint64)]


class BuildStats(C.Structure):
    """`usearch_amd_build_stats_t`."""
    _fields_ = [("batches", C.c_uint64), ("passes", C.c_uint64), ("search_distances", C.c_uint64),
                ("search_hops", C.c_uint64), ("select_distances", C.c_uint64), ("reverse_distances", C.c_uint64),
                ("repruned_lists", C.c_uint64), ("dropped_requests", C.c_uint64), ("seconds_total", C.c_double),
                ("seconds_search", C.c_double), ("seconds_link", C.c_double), ("seconds_upload", C.c_double),
                ("max_level", C.c_uint32), ("reserved", C.c_uint32), ("refiled_requests", C.c_uint64)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class CompactConfig(C.Structure):
    """`usearch_amd_compact_config_t`."""
    _fields_ = [("struct_bytes", C.c_size_t), ("staging_bytes", C.c_size_t)]


class CompactStats(C.Structure):
    """`usearch_amd_compact_stats_t`."""
    _fields_ = [("pruned_edges", C.c_uint64), ("removed_members", C.c_uint64), ("survivors", C.c_uint64),
                ("moved_bytes", C.c_uint64), ("chunks", C.c_uint64), ("new_entry_slot", C.c_uint32),
                ("new_max_level", C.c_uint32), ("scan_ms", C.c_float), ("lists_ms", C.c_float), ("rows_ms", C.c_float),
                ("reserved", C.c_uint32)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class ClusteringConfig(C.Structure):
    """`usearch_amd_clustering_config_t`."""
    _fields_ = [("struct_size", C.c_size_t), ("min_clusters", C.c_size_t), ("max_clusters", C.c_size_t)]


class ClusteringStats(C.Structure):
    """`usearch_amd_clustering_stats_t`."""
    _fields_ = [("clusters", C.c_uint64), ("unique_before_merge", C.c_uint64), ("merge_cycles", C.c_uint64),
                ("mapping_passes", C.c_uint64), ("visited_members", C.c_uint64), ("computed_distances", C.c_uint64),
                ("level", C.c_uint32), ("reserved", C.c_uint32), ("seconds_map", C.c_float), ("seconds_merge", C.c_float),
                ("seconds_trace", C.c_float)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


_library = None

EXPORTED_SYMBOLS = [
    "usearch_amd_device_count", "usearch_amd_snapshot_from_buffer", "usearch_amd_snapshot_from_file",
    "usearch_amd_snapshot_from_parts",
    "usearch_amd_snapshot_free", "usearch_amd_snapshot_size", "usearch_amd_snapshot_dimensions",
    "usearch_amd_snapshot_connectivity", "usearch_amd_snapshot_max_level", "usearch_amd_snapshot_bytes_per_vector",
    "usearch_amd_snapshot_row_stride", "usearch_amd_snapshot_device_bytes", "usearch_amd_snapshot_placement", "usearch_amd_snapshot_arrays",
    "usearch_amd_note_device_free", "usearch_amd_settle", "usearch_amd_snapshot_settle_ms", "usearch_amd_snapshot_tune",
    "usearch_amd_snapshot_scalar_kind",
    "usearch_amd_snapshot_metric_kind", "usearch_amd_snapshot_lanes_per_row", "usearch_amd_snapshot_inline_rows",
    "usearch_amd_search_many",
    "usearch_amd_search_many_device", "usearch_amd_last_peaks", "usearch_amd_distances",
    "usearch_amd_last_distances_ms", "usearch_amd_merge_many", "usearch_amd_merge_many_device",
    "usearch_amd_exact_search_many", "usearch_amd_exact_search_many_tiled", "usearch_amd_exact_search_dataset",
    "usearch_amd_exact_search_many_device", "usearch_amd_exact_search_dataset_tiled",
    "usearch_amd_cluster_many",
    "usearch_amd_clustering", "usearch_amd_clustering_members", "usearch_amd_snapshot_live_keys",
    "usearch_amd_filter_from_key_range", "usearch_amd_filter_from_keys", "usearch_amd_filter_from_bits",
    "usearch_amd_filter_allowed", "usearch_amd_filter_device_bits", "usearch_amd_filter_free",
    "usearch_amd_filtered_search_many", "usearch_amd_filtered_search_many_device", "usearch_amd_filtered_exact_search_many",
    "usearch_amd_cast",
    "usearch_amd_build", "usearch_amd_build_free", "usearch_amd_build_snapshot", "usearch_amd_build_extend", "usearch_amd_build_update",
    "usearch_amd_build_serialized_length", "usearch_amd_build_save_buffer", "usearch_amd_build_stats",
    "usearch_amd_snapshot_isolate", "usearch_amd_snapshot_compact", "usearch_amd_compact_scan_chunk",
    "usearch_amd_build_remove", "usearch_amd_build_isolate", "usearch_amd_build_compact",
    "usearch_amd_join",
    "usearch_amd_kmeans", "usearch_amd_kmeans_assign",
    # sharded search across GPUs (usearch_amd/sharded.py binds these)
    "usearch_amd_comm_unique_id", "usearch_amd_comm_init_rccl", "usearch_amd_comm_init_custom", "usearch_amd_comm_free",
    "usearch_amd_comm_rank", "usearch_amd_comm_world", "usearch_amd_comm_broadcast", "usearch_amd_sharded_search_many",
]


def _share_hip_runtime() -> None:
    """One HIP runtime per process. PyTorch wheels bundle their own `libamdhip64.so` and `libtorch_hip.so` asks for it by that
    unversioned file name, so the loader does not recognise a system runtime that is already mapped (its SONAME is
    `libamdhip64.so.7`) and maps torch's copy as a second runtime — which then finds no device, the first one holding the
    driver. Mapping torch's copy first makes both sides resolve to it: this library asks for the SONAME, and torch's copy
    carries it. Only the path is looked up, torch is not imported; without torch there is nothing to share."""
    try:
        with open("/proc/self/maps") as maps:
            if "libamdhip64" in maps.read():
                return  # a runtime is mapped already (torch imported first, or the caller's own)
    except OSError:
        pass
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=os.RTLD_GLOBAL)


def library() -> C.CDLL:
    """Loads `usearch_amd/lib/libusearch_amd.so` (built by `make -C usearch_amd/csrc` / `__graft_entry__.build()`)."""
    global _library
    if _library is not None:
        return _library
    if not os.path.exists(LIBRARY_PATH):
        raise RuntimeError(f"{LIBRARY_PATH} is missing: build it with `make -C usearch_amd/csrc` "
                           "(hipcc, gfx950). The engine has no CPU fallback.")
    _share_hip_runtime()
    L = C.CDLL(LIBRARY_PATH, mode=os.RTLD_LOCAL)
    err_p = C.POINTER(C.c_char_p)
    L.usearch_amd_device_count.restype = C.c_int
    L.usearch_amd_device_count.argtypes = [err_p]
    L.usearch_amd_snapshot_from_buffer.restype = C.c_void_p
    L.usearch_amd_snapshot_from_buffer.argtypes = [C.c_void_p, C.c_size_t, C.c_int, err_p]
    L.usearch_amd_snapshot_from_parts.restype = C.c_void_p
    L.usearch_amd_snapshot_from_parts.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, err_p]
    L.usearch_amd_snapshot_from_file.restype = C.c_void_p
    L.usearch_amd_snapshot_from_file.argtypes = [C.c_char_p, C.c_int, err_p]
    L.usearch_amd_snapshot_free.argtypes = [C.c_void_p, err_p]
    for name in ("size", "dimensions", "connectivity", "max_level", "bytes_per_vector", "row_stride", "device_bytes",
                 "lanes_per_row", "inline_rows"):
        f = getattr(L, f"usearch_amd_snapshot_{name}")
        f.restype = C.c_size_t
        f.argtypes = [C.c_void_p]
    L.usearch_amd_note_device_free.restype = None
    L.usearch_amd_note_device_free.argtypes = []
    L.usearch_amd_snapshot_tune.restype = C.c_uint32
    L.usearch_amd_snapshot_tune.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_uint32, err_p]
    L.usearch_amd_settle.restype = C.c_float
    L.usearch_amd_settle.argtypes = []
    L.usearch_amd_snapshot_settle_ms.restype = C.c_float
    L.usearch_amd_snapshot_settle_ms.argtypes = [C.c_void_p]
    L.usearch_amd_snapshot_placement.restype = None
    L.usearch_amd_snapshot_placement.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                                 C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.usearch_amd_snapshot_arrays.restype = None
    L.usearch_amd_snapshot_arrays.argtypes = [C.c_void_p, C.POINTER(Arrays)]
    for name in ("scalar_kind", "metric_kind"):
        f = getattr(L, f"usearch_amd_snapshot_{name}")
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
    L.usearch_amd_search_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                          C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(Tuning), C.POINTER(Stats), err_p]
    L.usearch_amd_search_many_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(Tuning), C.c_int,
                                                 C.POINTER(Stats), err_p]
    L.usearch_amd_merge_many_device.argtypes = [C.c_void_p] * 3 + [C.c_size_t] * 3 + [C.c_void_p] * 4 + [err_p]
    L.usearch_amd_merge_many.argtypes = [C.c_void_p] * 3 + [C.c_size_t] * 3 + [C.c_void_p] * 3 + [err_p]
    L.usearch_amd_cluster_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, err_p]
    L.usearch_amd_clustering.restype = None
    L.usearch_amd_clustering.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(ClusteringConfig),
                                         C.c_void_p, C.c_void_p, C.POINTER(ClusteringStats), err_p]
    L.usearch_amd_clustering_members.restype = None
    L.usearch_amd_clustering_members.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(ClusteringConfig), C.c_void_p,
                                                 C.c_void_p, C.POINTER(ClusteringStats), err_p]
    L.usearch_amd_snapshot_live_keys.restype = C.c_size_t
    L.usearch_amd_snapshot_live_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err_p]
    L.usearch_amd_exact_search_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_size_t,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), err_p]
    L.usearch_amd_exact_search_many_tiled.argtypes = L.usearch_amd_exact_search_many.argtypes
    L.usearch_amd_exact_search_many_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float),
                                                       C.POINTER(C.c_char_p)]
    L.usearch_amd_exact_search_dataset.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                                   C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p,
                                                   C.c_size_t, C.c_void_p, C.c_size_t, err_p]
    L.usearch_amd_exact_search_dataset_tiled.argtypes = L.usearch_amd_exact_search_dataset.argtypes
    L.usearch_amd_filter_from_key_range.restype = C.c_void_p
    L.usearch_amd_filter_from_key_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, err_p]
    L.usearch_amd_filter_from_keys.restype = C.c_void_p
    L.usearch_amd_filter_from_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, err_p]
    L.usearch_amd_filter_from_bits.restype = C.c_void_p
    L.usearch_amd_filter_from_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err_p]
    L.usearch_amd_filter_allowed.restype = C.c_size_t
    L.usearch_amd_filter_allowed.argtypes = [C.c_void_p]
    L.usearch_amd_filter_device_bits.restype = C.c_void_p
    L.usearch_amd_filter_device_bits.argtypes = [C.c_void_p]
    L.usearch_amd_filter_free.argtypes = [C.c_void_p, err_p]
    L.usearch_amd_filtered_search_many.argtypes = [C.c_void_p, C.c_void_p] + L.usearch_amd_search_many.argtypes[1:]
    L.usearch_amd_filtered_search_many_device.argtypes = [C.c_void_p, C.c_void_p] + L.usearch_amd_search_many_device.argtypes[1:]
    L.usearch_amd_filtered_exact_search_many.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_size_t,
                                                         C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.POINTER(C.c_float), err_p]
    L.usearch_amd_last_peaks.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err_p]
    L.usearch_amd_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t,
                                        C.c_void_p, err_p]
    L.usearch_amd_last_distances_ms.restype = C.c_float
    L.usearch_amd_last_distances_ms.argtypes = [C.c_void_p]
    L.usearch_amd_cast.restype = C.c_int
    L.usearch_amd_cast.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.usearch_amd_build.restype = C.c_void_p
    L.usearch_amd_build.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_void_p,
                                    C.POINTER(BuildConfig), C.c_int, C.c_int, err_p]
    L.usearch_amd_build_free.argtypes = [C.c_void_p, err_p]
    L.usearch_amd_build_extend.restype = None
    L.usearch_amd_build_extend.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, err_p]
    L.usearch_amd_build_update.restype = None
    L.usearch_amd_build_update.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, err_p]
    L.usearch_amd_build_snapshot.restype = C.c_void_p
    L.usearch_amd_build_snapshot.argtypes = [C.c_void_p]
    L.usearch_amd_build_serialized_length.restype = C.c_size_t
    L.usearch_amd_build_serialized_length.argtypes = [C.c_void_p]
    L.usearch_amd_build_save_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err_p]
    L.usearch_amd_build_stats.argtypes = [C.c_void_p, C.POINTER(BuildStats)]
    L.usearch_amd_snapshot_isolate.restype = None
    L.usearch_amd_snapshot_isolate.argtypes = [C.c_void_p, C.POINTER(CompactStats), err_p]
    L.usearch_amd_snapshot_compact.restype = None
    L.usearch_amd_snapshot_compact.argtypes = [C.c_void_p, C.POINTER(CompactConfig), C.c_void_p, C.POINTER(CompactStats), err_p]
    L.usearch_amd_compact_scan_chunk.restype = C.c_uint32
    L.usearch_amd_compact_scan_chunk.argtypes = []
    L.usearch_amd_build_remove.restype = None
    L.usearch_amd_build_remove.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, err_p]
    L.usearch_amd_build_isolate.restype = None
    L.usearch_amd_build_isolate.argtypes = [C.c_void_p, C.POINTER(CompactStats), err_p]
    L.usearch_amd_build_compact.restype = None
    L.usearch_amd_build_compact.argtypes = [C.c_void_p, C.POINTER(CompactConfig), C.c_void_p, C.POINTER(CompactStats), err_p]
    L.usearch_amd_join.restype = C.c_size_t
    L.usearch_amd_join.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(JoinConfig), C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.POINTER(JoinStats), err_p]
    L.usearch_amd_kmeans.restype = None
    L.usearch_amd_kmeans.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(KMeansConfig),
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(KMeansStats), err_p]
    L.usearch_amd_kmeans_assign.restype = None
    L.usearch_amd_kmeans_assign.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t,
                                            C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, err_p]
    _library = L
    return L


def _raise(err: C.c_char_p, what: str) -> None:
    if err.value:
        raise RuntimeError(f"{what}: {err.value.decode()}")


def _pointer(array: Optional[np.ndarray]):
    return C.c_void_p(array.ctypes.data) if array is not None else None


@dataclass
class Matches:
    """Results of one query — `usearch.index.Matches` (index.py:303-331)."""
    keys: np.ndarray
    distances: np.ndarray
    visited_members: int = 0
    computed_distances: int = 0

    def __len__(self) -> int:
        return len(self.keys)

    def to_list(self):
        return [(int(k), float(d)) for k, d in zip(self.keys, self.distances)]


@dataclass
class BatchMatches:
    """Results of a batch — `usearch.index.BatchMatches` (index.py:334-385); counters kept per query as well."""
    keys: np.ndarray
    distances: np.ndarray
    counts: np.ndarray
    visited_members: int = 0
    computed_distances: int = 0
    visited_per_query: Optional[np.ndarray] = None
    computed_per_query: Optional[np.ndarray] = None
    stats: Optional[Stats] = None

    def __len__(self) -> int:
        return len(self.counts)

    def __getitem__(self, index: int) -> Matches:
        if isinstance(index, int) and index < len(self):
            n = int(self.counts[index])
            return Matches(self.keys[index, :n], self.distances[index, :n],
                           int(self.visited_per_query[index]), int(self.computed_per_query[index]))
        raise IndexError(f"`index` must be an integer under {len(self)}")

    def count_matches(self, expected: np.ndarray, count: Optional[int] = None) -> int:
        assert len(expected) == len(self)
        count = self.keys.shape[1] if count is None else count
        if count == 1:
            return int(np.sum(self.keys[:, 0] == expected))
        return int(sum(expected[i] in self.keys[i, :count] for i in range(len(self))))

    def mean_recall(self, expected: np.ndarray, count: Optional[int] = None) -> float:
        return self.count_matches(expected, count=count) / len(expected)


class Clustering:
    """What `Index.clustering` returns — `usearch.index.Clustering` (index.py:399-450) without its plotting helpers: `matches`
    holds one (centroid key, distance) per query, `queries` the vectors or member keys that were clustered."""

    def __init__(self, index: "Index", matches: BatchMatches, queries: np.ndarray, stats: dict, by_keys: bool):
        self.index = index
        self.matches = matches
        self.queries = queries
        self.stats = stats
        self._by_keys = by_keys

    def __repr__(self) -> str:
        return f"usearch_amd.Clustering(for {len(self.queries)} queries, {self.stats.get('clusters', 0)} clusters)"

    @property
    def centroids_popularity(self):
        """(centroid keys, how many queries each received), the keys ascending."""
        return np.unique(self.matches.keys[:, 0], return_counts=True)

    def members_of(self, centroid: int, queries_only: bool = False) -> np.ndarray:
        """The queries that ended in `centroid`: their vectors or member keys, or with `queries_only` their positions."""
        positions = np.flatnonzero(self.matches.keys[:, 0] == np.uint64(centroid))
        return positions if queries_only else self.queries[positions]

    def subcluster(self, centroid: int, **clustering_kwargs) -> "Clustering":
        """Clusters the queries of one centroid again (`min_count`, `max_count` as for `Index.clustering`)."""
        sub_queries = self.members_of(centroid)
        if self._by_keys:
            return self.index.clustering(keys=sub_queries, **clustering_kwargs)
        return self.index.clustering(vectors=sub_queries, **clustering_kwargs)


class Filter:
    """A predicate over members as an HBM-resident bitmap (`usearch_amd_filter_t`): made once, reused by any number of batches.
    Stands in for the `predicate(key)` callable of `index_dense_gt::filtered_search` (index_dense.hpp:774-779)."""

    def __init__(self, handle: int, index: "Index"):
        self._handle = handle
        self._index = index  # keeps the snapshot alive

    @property
    def allowed(self) -> int:
        return int(library().usearch_amd_filter_allowed(self._handle))

    @property
    def device_bits(self) -> int:
        return int(library().usearch_amd_filter_device_bits(self._handle) or 0)

    def close(self) -> None:
        if getattr(self, "_handle", None):
            err = C.c_char_p()
            library().usearch_amd_filter_free(self._handle, C.byref(err))
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Index:
    """An immutable HBM-resident snapshot of a serialized USearch index, searchable in batches on one MI355X."""

    def __init__(self, handle: int, expansion_search: int = 0, owner=None):
        self._handle = handle
        self._owner = owner  # a `BuiltIndex` whose builder owns the snapshot: keeps it alive, frees it
        self.expansion_search = expansion_search  # 0 = the reference's default of 64 (index.hpp:3029-3030)

    @classmethod
    def restore(cls, source: Union[str, os.PathLike, bytes, bytearray, memoryview, np.ndarray], device: int = 0,
                expansion_search: int = 0, vectors: Optional[np.ndarray] = None) -> "Index":
        """Uploads a `.usearch` file or an in-memory image (`usearch_save` / `usearch_save_buffer` output). `vectors`: the
        matrix the caller kept for an image saved with `exclude_vectors` (one row per member, in slot order)."""
        L = library()
        err = C.c_char_p()
        if vectors is not None:
            if isinstance(source, (str, os.PathLike)):  # the graph alone sits in the file: map it for the call
                source = np.memmap(os.fspath(source), dtype=np.uint8, mode="r")
            image = np.ascontiguousarray(np.frombuffer(source, dtype=np.uint8)
                                         if not isinstance(source, np.ndarray) else source, dtype=np.uint8)
            vectors = np.asarray(vectors)
            if vectors.ndim != 2 or vectors.strides[1] != vectors.itemsize:
                vectors = np.ascontiguousarray(vectors)
            handle = L.usearch_amd_snapshot_from_parts(_pointer(image), image.size, _pointer(vectors), vectors.strides[0],
                                                       device, C.byref(err))
        elif isinstance(source, (str, os.PathLike)):
            handle = L.usearch_amd_snapshot_from_file(os.fspath(source).encode(), device, C.byref(err))
        else:
            image = np.ascontiguousarray(np.frombuffer(source, dtype=np.uint8)
                                         if not isinstance(source, np.ndarray) else source, dtype=np.uint8)
            handle = L.usearch_amd_snapshot_from_buffer(_pointer(image), image.size, device, C.byref(err))
        _raise(err, "usearch_amd snapshot")
        if not handle:
            raise RuntimeError("usearch_amd snapshot: failed without a message")
        return cls(handle, expansion_search)

    @classmethod
    def restore_placed(cls, source, probe, draws: int = 8, device: int = 0, expansion_search: int = 0,
                       vectors: Optional[np.ndarray] = None, first: Optional["Index"] = None,
                       good_enough: Optional[float] = None, free_bytes=None):
        """`restore`, but choosing WHERE in HBM the index lands. The same index bytes at other physical addresses walk at one
        of two speeds (headline batch: 45.4 or 51.7 ms; stable for the life of an allocation, profiles/r02_placement.log), and
        the allocator decides which. So: upload the image up to `draws` times, time `probe(index) -> milliseconds` (a batch of
        the caller's own queries) on each, keep the fastest. Candidates that lost stay allocated until the end — the next one
        must land somewhere else — as long as `free_bytes()` (device memory still free) leaves room for one more; they are
        released before returning. `good_enough` (milliseconds): stop drawing once a candidate is at least that fast (a deployment
        that knows its fast speed). `first`: an index that is already resident (the builder's own) takes part as draw 0; it is
        never closed here. Returns (index, {"probe_ms": [...], "kept": i}) — `index is first` when nothing beat it."""
        candidates, timings = [], []
        if first is not None:
            candidates.append(first)
            timings.append(float(probe(first)))
        try:
            while len(timings) < max(1, draws):
                if timings and good_enough is not None and min(timings) <= good_enough:
                    break
                if candidates and free_bytes is not None and free_bytes() < 1.25 * candidates[0].memory_usage:
                    # no room next to the ones held: let go of every loser, keep drawing
                    keep = int(np.argmin(timings))
                    for i, candidate in enumerate(candidates):
                        if i != keep and candidate is not None and candidate is not first:
                            candidate.close()
                            candidates[i] = None
                    if free_bytes() < 1.25 * candidates[keep].memory_usage:
                        break
                try:
                    candidate = cls.restore(source, device, expansion_search, vectors)
                except RuntimeError:
                    if not candidates:
                        raise
                    break  # out of device memory next to the ones held: the best so far it is
                candidates.append(candidate)
                timings.append(float("inf"))  # in the list before the probe runs: a failing probe still gets it released
                timings[-1] = float(probe(candidate))
        except BaseException:
            for candidate in candidates:  # nothing is handed out on this path: every copy made here goes, `first` stays the caller's
                if candidate is not None and candidate is not first:
                    candidate.close()
            raise
        kept = int(np.argmin(timings))
        for i, candidate in enumerate(candidates):
            if i != kept and candidate is not None and candidate is not first:
                candidate.close()
        return candidates[kept], {"probe_ms": [round(t, 3) for t in timings], "kept": kept}

    def close(self) -> None:
        if getattr(self, "_handle", None):
            if getattr(self, "_owner", None) is None:
                err = C.c_char_p()
                library().usearch_amd_snapshot_free(self._handle, C.byref(err))
            self._handle = None
            self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def placement(self) -> dict:
        """How the engine placed the matrix of stored rows in HBM (csrc/placement.hpp): the trials made so far — each a fresh copy
        judged against the incumbent on a chip-filling launch's own first queries — how many of them moved the matrix, and both
        times of every trial; `draws == 0` before the first such launch and for arrays too small to bother."""
        draws, kept, probe_ms = C.c_uint32(), C.c_uint32(), C.c_float()
        rates, incumbents = (C.c_float * 8)(), (C.c_float * 8)()
        library().usearch_amd_snapshot_placement(self._handle, C.byref(draws), C.byref(kept), rates, incumbents, C.byref(probe_ms))
        shown = min(int(draws.value), 8)
        return {"settle_ms": round(float(library().usearch_amd_snapshot_settle_ms(self._handle)), 1),
                "draws": int(draws.value), "kept": int(kept.value), "probe_ms": round(float(probe_ms.value), 2),
                "judge_ms": [round(float(rates[i]), 3) for i in range(shown)],
                "incumbent_ms": [round(float(incumbents[i]), 3) for i in range(shown)]}

    def tune_device(self, queries_ptr: int, queries_count: int, queries_stride: int, count: int, expansion: int, max_trials: int = 8) -> int:
        """`usearch_amd_snapshot_tune`: places the matrix of stored rows by trial on a SAMPLE of the batches to come (device-resident
        queries in the storage kind, as for `search_device`): up to `max_trials` fresh copies timed against the incumbent on the
        sample's first queries at `expansion`, the faster stays. Explicit, synchronous, before serving; returns the trials made
        (`placement` has their times)."""
        err = C.c_char_p()
        made = library().usearch_amd_snapshot_tune(self._handle, C.c_void_p(queries_ptr), queries_count, queries_stride, count, expansion,
                                                   max_trials, C.byref(err))
        _raise(err, "usearch_amd_snapshot_tune")
        return int(made)

    @property
    def arrays(self) -> "Arrays":
        """The HBM-resident arrays (`usearch_amd_snapshot_arrays`): device pointers of the padded matrix, the level-0 lists and the
        keys, with their shapes — read-only, for a host's own kernels."""
        out = Arrays()
        library().usearch_amd_snapshot_arrays(self._handle, C.byref(out))
        return out

    # ---- diagnostics of the placement studies (scripts/placement_study.py, fragment_study.py): the probes live in the test-hooks
    #      library, over the arrays above
    def latency_probe(self, lists: bool = False) -> float:
        """Nanoseconds per DEPENDENT read of a random stored row (or, `lists`, of a random level-0 neighbour list)."""
        err, a = C.c_char_p(), self.arrays
        base, row = (a.level0, a.level0_cells * 4) if lists else (a.vectors, a.row_stride)
        value = test_hooks().usearch_amd_test_latency_probe(C.c_void_p(base), a.size * row, row, C.byref(err))
        _raise(err, "usearch_amd_test_latency_probe")
        return float(value)

    def translation_probe(self) -> float:
        """Million random 4-KB pages of the resident matrix touched per second (16 bytes each): the address-translation path."""
        err, a = C.c_char_p(), self.arrays
        rate = test_hooks().usearch_amd_test_translation_probe(C.c_void_p(a.vectors), a.size * a.row_stride, C.byref(err))
        _raise(err, "usearch_amd_test_translation_probe")
        return float(rate)

    def gather_probe(self, first_row: int = 0, rows: int = 0) -> float:
        """GB/s of a dependency-free gather of random stored rows among rows [first_row, first_row + rows) (`rows` = 0: to the end)."""
        err, a = C.c_char_p(), self.arrays
        if first_row >= a.size:
            return 0.0
        rows = a.size - first_row if not rows or first_row + rows > a.size else rows
        rate = test_hooks().usearch_amd_test_gather_probe(C.c_void_p((a.vectors or 0) + first_row * a.row_stride), rows * a.row_stride,
                                                          a.row_stride, C.byref(err))
        _raise(err, "usearch_amd_test_gather_probe")
        return float(rate)

    # ---- introspection (names of usearch.index.Index properties, index.py:1180-1300)
    def __len__(self) -> int:
        return library().usearch_amd_snapshot_size(self._handle)

    @property
    def size(self) -> int:
        return len(self)

    @property
    def ndim(self) -> int:
        return library().usearch_amd_snapshot_dimensions(self._handle)

    @property
    def connectivity(self) -> int:
        return library().usearch_amd_snapshot_connectivity(self._handle)

    @property
    def max_level(self) -> int:
        return library().usearch_amd_snapshot_max_level(self._handle)

    @property
    def dtype(self) -> str:
        return SCALAR_NAMES[library().usearch_amd_snapshot_scalar_kind(self._handle)]

    @property
    def metric_kind(self) -> str:
        return METRIC_NAMES[library().usearch_amd_snapshot_metric_kind(self._handle)]

    @property
    def bytes_per_vector(self) -> int:
        return library().usearch_amd_snapshot_bytes_per_vector(self._handle)

    @property
    def row_stride(self) -> int:
        return library().usearch_amd_snapshot_row_stride(self._handle)

    @property
    def memory_usage(self) -> int:
        return library().usearch_amd_snapshot_device_bytes(self._handle)

    @property
    def lanes_per_row(self) -> int:
        return library().usearch_amd_snapshot_lanes_per_row(self._handle)

    @property
    def inline_rows(self) -> bool:
        """Rows of ≤ 16 bytes are stored next to the neighbour lists (one contiguous read per hop)."""
        return bool(library().usearch_amd_snapshot_inline_rows(self._handle))

    @property
    def hardware_acceleration(self) -> str:
        return "gfx950"

    # ---- filters
    def filter_key_range(self, first: int, last: int) -> Filter:
        """Members whose key lies in [first, last]."""
        err = C.c_char_p()
        handle = library().usearch_amd_filter_from_key_range(self._handle, first, last, C.byref(err))
        _raise(err, "usearch_amd_filter_from_key_range")
        return Filter(handle, self)

    def filter_keys(self, keys, allow: bool = True) -> Filter:
        """Members whose key is (allow) / is not (deny list) among `keys`."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        err = C.c_char_p()
        handle = library().usearch_amd_filter_from_keys(self._handle, _pointer(keys), len(keys), int(allow), C.byref(err))
        _raise(err, "usearch_amd_filter_from_keys")
        return Filter(handle, self)

    def filter_bits(self, bits: np.ndarray) -> Filter:
        """The caller's bitmap: bit `s & 31` of word `s >> 5` = the member in slot `s` passes. A boolean array of one entry per
        slot is packed first."""
        bits = np.asarray(bits)
        if bits.dtype == np.bool_:
            padded = np.zeros((len(bits) + 31) // 32 * 32, dtype=np.uint8)
            padded[:len(bits)] = bits
            bits = np.packbits(padded.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view(np.uint32)
        bits = np.ascontiguousarray(bits, dtype=np.uint32)
        err = C.c_char_p()
        handle = library().usearch_amd_filter_from_bits(self._handle, _pointer(bits), len(bits), C.byref(err))
        _raise(err, "usearch_amd_filter_from_bits")
        return Filter(handle, self)

    # ---- search
    def search(self, vectors: np.ndarray, count: int = 10, *, expansion: Optional[int] = None,
               dtype: Optional[str] = None, tuning: Optional[Tuning] = None,
               exact: Union[bool, str] = False, filter: Optional[Filter] = None) -> Union[Matches, BatchMatches]:
        """`Index.search` (index.py:700-748): one vector → `Matches`, a 2-D batch → `BatchMatches`.

        `dtype` names the scalar kind of `vectors` when numpy cannot tell (bit-packed `b1` rows are `uint8`);
        by default it is derived from the array's dtype, `uint8` meaning bits."""
        vectors = np.asarray(vectors)
        single = vectors.ndim == 1
        if single:
            vectors = vectors[None, :]
        if vectors.ndim != 2:
            raise ValueError("Expects a matrix or a vector")
        if dtype is None:
            dtype = _infer_dtype(vectors)
        expected_columns = (self.ndim + 7) // 8 if dtype == "b1" else self.ndim
        if vectors.shape[1] != expected_columns:
            raise ValueError(f"The number of columns {vectors.shape[1]} must match the index ({expected_columns})")
        if vectors.strides[1] != vectors.itemsize:  # rows may be strided (python/lib.cpp:415-461), scalars may not
            vectors = np.ascontiguousarray(vectors)
        q = vectors.shape[0]
        keys = np.zeros((q, count), dtype=np.uint64)
        distances = np.zeros((q, count), dtype=np.float32)
        counts = np.zeros(q, dtype=np.uint64)
        visited = np.zeros(q, dtype=np.uint64)
        computed = np.zeros(q, dtype=np.uint64)
        stats = Stats()
        err = C.c_char_p()
        if exact and filter is not None:  # brute force over the members the filter lets through (index.hpp:4260-4263)
            kernel_ms = C.c_float()
            library().usearch_amd_filtered_exact_search_many(
                self._handle, filter._handle, _pointer(vectors), SCALAR_KINDS[dtype], q,
                vectors.shape[1] * vectors.itemsize if q <= 1 else vectors.strides[0], count, _pointer(keys), _pointer(distances),
                _pointer(counts), int(exact == "tiled"), C.byref(kernel_ms), C.byref(err))
            _raise(err, "usearch_amd_filtered_exact_search_many")
            stats.kernel_ms = kernel_ms.value
            batch = BatchMatches(keys, distances, counts, 0, 0, visited, computed, stats)
            return batch[0] if single else batch
        if exact:  # brute force over every stored vector (Index.search(..., exact=True), index.py:700-748)
            kernel_ms = C.c_float()
            # exact="tiled": the matrix-unit kernel (f16 / bf16 within float tolerance; f32 within a derived bound; i8 bit-identical)
            # or, for b1, the bit tile (hamming / tanimoto / jaccard / sorensen: bit-identical, NaN included)
            entry = (library().usearch_amd_exact_search_many_tiled if exact == "tiled"
                     else library().usearch_amd_exact_search_many)
            entry(self._handle, _pointer(vectors), SCALAR_KINDS[dtype], q,
                                                    vectors.shape[1] * vectors.itemsize if q <= 1 else vectors.strides[0],
                                                    count, _pointer(keys), _pointer(distances), _pointer(counts),
                                                    C.byref(kernel_ms), C.byref(err))
            _raise(err, "usearch_amd_exact_search_many")
            stats.kernel_ms = kernel_ms.value
            computed[:] = len(self)
            batch = BatchMatches(keys, distances, counts, 0, int(computed.sum()), visited, computed, stats)
            return batch[0] if single else batch
        ef = self.expansion_search if expansion is None else expansion
        if filter is not None:
            library().usearch_amd_filtered_search_many(self._handle, filter._handle, _pointer(vectors), SCALAR_KINDS[dtype], q,
                                                       vectors.shape[1] * vectors.itemsize if q <= 1 else vectors.strides[0],
                                                       count, ef, _pointer(keys), _pointer(distances), _pointer(counts),
                                                       _pointer(visited), _pointer(computed),
                                                       C.byref(tuning) if tuning is not None else None, C.byref(stats), C.byref(err))
            _raise(err, "usearch_amd_filtered_search_many")
            batch = BatchMatches(keys, distances, counts, int(visited.sum()), int(computed.sum()), visited, computed, stats)
            return batch[0] if single else batch
        library().usearch_amd_search_many(self._handle, _pointer(vectors), SCALAR_KINDS[dtype], q,
                                          vectors.shape[1] * vectors.itemsize if q <= 1 else vectors.strides[0],
                                          count, ef, _pointer(keys),
                                          _pointer(distances), _pointer(counts), _pointer(visited),
                                          _pointer(computed), C.byref(tuning) if tuning is not None else None,
                                          C.byref(stats), C.byref(err))
        _raise(err, "usearch_amd_search_many")
        batch = BatchMatches(keys, distances, counts, int(visited.sum()), int(computed.sum()), visited, computed,
                             stats)
        return batch[0] if single else batch

    def search_device(self, queries_ptr: int, queries_count: int, queries_stride: int, count: int, expansion: int,
                      keys_ptr: int, distances_ptr: int, counts_ptr: int, visited_ptr: int, computed_ptr: int,
                      stream: int = 0, timed: bool = False, tuning: Optional[Tuning] = None,
                      filter: Optional[Filter] = None) -> Stats:
        """HBM-resident batch: raw device addresses in and out (e.g. `torch.Tensor.data_ptr()`), storage scalar kind."""
        stats = Stats()
        err = C.c_char_p()
        if filter is not None:
            library().usearch_amd_filtered_search_many_device(
                self._handle, filter._handle, C.c_void_p(queries_ptr), queries_count, queries_stride, count, expansion,
                C.c_void_p(keys_ptr), C.c_void_p(distances_ptr), C.c_void_p(counts_ptr), C.c_void_p(visited_ptr),
                C.c_void_p(computed_ptr), C.c_void_p(stream), C.byref(tuning) if tuning is not None else None, int(timed),
                C.byref(stats), C.byref(err))
            _raise(err, "usearch_amd_filtered_search_many_device")
            return stats
        library().usearch_amd_search_many_device(self._handle, C.c_void_p(queries_ptr), queries_count, queries_stride,
                                                 count, expansion, C.c_void_p(keys_ptr), C.c_void_p(distances_ptr),
                                                 C.c_void_p(counts_ptr), C.c_void_p(visited_ptr),
                                                 C.c_void_p(computed_ptr), C.c_void_p(stream),
                                                 C.byref(tuning) if tuning is not None else None, int(timed),
                                                 C.byref(stats), C.byref(err))
        _raise(err, "usearch_amd_search_many_device")
        return stats

    def exact_search_device(self, queries_ptr: int, queries_count: int, queries_stride: int, count: int, keys_ptr: int,
                            distances_ptr: int, counts_ptr: int, stream: int = 0, tiled: bool = True) -> float:
        """Exact search of an HBM-resident batch into HBM-resident results (`search(…, exact = true)` of the class for a batch);
        returns the kernels' HIP-event time in ms. `tiled`: the matrix-unit kernel (exact_tiled.hip), for b1 the bit tile (exact_bits.hip)."""
        kernel_ms = C.c_float(0)
        err = C.c_char_p()
        library().usearch_amd_exact_search_many_device(self._handle, C.c_void_p(queries_ptr), queries_count, queries_stride,
                                                       count, C.c_void_p(keys_ptr), C.c_void_p(distances_ptr),
                                                       C.c_void_p(counts_ptr), C.c_void_p(stream), int(tiled),
                                                       C.byref(kernel_ms), C.byref(err))
        _raise(err, "usearch_amd_exact_search_many_device")
        return float(kernel_ms.value)

    @property
    def last_distances_ms(self) -> float:
        return float(library().usearch_amd_last_distances_ms(self._handle))

    def last_peaks(self, queries_count: int) -> np.ndarray:
        """[Q, 2] = {peak frontier size, visited-set size} of the most recent search (scratch-sizing telemetry)."""
        out = np.zeros((queries_count, 2), dtype=np.uint32)
        err = C.c_char_p()
        library().usearch_amd_last_peaks(self._handle, _pointer(out), queries_count, C.byref(err))
        _raise(err, "usearch_amd_last_peaks")
        return out

    def cluster(self, vectors: np.ndarray, level: int = 1, dtype: Optional[str] = None):
        """`index_dense_gt::cluster(query, level)` for a batch (index_dense.hpp:788-793 → index.hpp:3089-3125):
        → (keys[Q], distances[Q], visited[Q], computed[Q]) — per query the member the greedy descent reaches on `level`."""
        vectors = np.asarray(vectors)
        if vectors.ndim == 1:
            vectors = vectors[None, :]
        if dtype is None:
            dtype = _infer_dtype(vectors)
        if vectors.strides[1] != vectors.itemsize:
            vectors = np.ascontiguousarray(vectors)
        q = len(vectors)
        keys = np.zeros(q, dtype=np.uint64)
        distances = np.zeros(q, dtype=np.float32)
        visited = np.zeros(q, dtype=np.uint64)
        computed = np.zeros(q, dtype=np.uint64)
        err = C.c_char_p()
        library().usearch_amd_cluster_many(self._handle, _pointer(vectors), SCALAR_KINDS[dtype], q,
                                           vectors.shape[1] * vectors.itemsize if q <= 1 else vectors.strides[0], level,
                                           _pointer(keys), _pointer(distances), _pointer(visited), _pointer(computed),
                                           C.byref(err))
        _raise(err, "usearch_amd_cluster_many")
        return keys, distances, visited, computed

    def clustering(self, *, vectors: Optional[np.ndarray] = None, keys: Optional[np.ndarray] = None, min_count: Optional[int] = None,
                   max_count: Optional[int] = None, dtype: Optional[str] = None) -> Clustering:
        """`Index.cluster(vectors=… | keys=…, min_count=…, max_count=…)` of the reference (index.py:1202-1261 →
        index_dense.hpp:1819-1981) on the device: every query descends to the level with more than `min_count` nodes, the least
        popular centroids merge into their nearest until `max_count` are left. Neither input: every member is clustered. Equal
        popularities are ordered by centroid key. `min_count` without `max_count` is refused (the reference never returns from
        it). Named `clustering` because `cluster(vectors, level)` is the single descent."""
        if vectors is not None and keys is not None:
            raise ValueError("clustering takes `vectors` or `keys`, not both")
        config = ClusteringConfig(C.sizeof(ClusteringConfig), int(min_count or 0), int(max_count or 0))
        stats, err = ClusteringStats(), C.c_char_p()
        if vectors is not None:
            vectors = np.asarray(vectors)
            if vectors.ndim == 1:
                vectors = vectors[None, :]
            if dtype is None:
                dtype = _infer_dtype(vectors)
            if vectors.strides[1] != vectors.itemsize:
                vectors = np.ascontiguousarray(vectors)
            q = len(vectors)
            queries = vectors
            out_keys, out_distances = np.zeros(q, dtype=np.uint64), np.zeros(q, dtype=np.float32)
            library().usearch_amd_clustering(self._handle, _pointer(vectors), SCALAR_KINDS[dtype], q,
                                             vectors.shape[1] * vectors.itemsize if q <= 1 else vectors.strides[0], C.byref(config),
                                             _pointer(out_keys), _pointer(out_distances), C.byref(stats), C.byref(err))
        else:
            if keys is None:  # every member that was not removed, in slot order
                queries = np.zeros(len(self), dtype=np.uint64)  # one read-back: room for every slot, cut to the live ones
                live = library().usearch_amd_snapshot_live_keys(self._handle, _pointer(queries), len(queries), C.byref(err))
                _raise(err, "usearch_amd_snapshot_live_keys")
                queries = queries[:live].copy()
                given = None
            else:
                queries = given = np.ascontiguousarray(np.atleast_1d(keys), dtype=np.uint64)
            q = len(queries)
            out_keys, out_distances = np.zeros(q, dtype=np.uint64), np.zeros(q, dtype=np.float32)
            library().usearch_amd_clustering_members(self._handle, _pointer(given), q, C.byref(config), _pointer(out_keys),
                                                     _pointer(out_distances), C.byref(stats), C.byref(err))
        _raise(err, "usearch_amd_clustering")
        matches = BatchMatches(out_keys[:, None], out_distances[:, None], np.ones(q, dtype=np.uint64),
                               int(stats.visited_members), int(stats.computed_distances))
        return Clustering(self, matches, queries, stats.as_dict(), vectors is None)

    # ---- semantic join
    def join(self, other: "Index", max_proposals: int = 0, exact: bool = False, *, expansion: Optional[int] = None,
             threads: int = 0) -> Dict[int, int]:
        """`Index.join` (index.py:1170-1200 → python/lib.cpp:780-797): a one-to-one mapping from keys of `self` to keys of `other`,
        the man-optimal stable matching in which the smaller index proposes to its nearest members. `expansion` defaults to the
        larger of the two indexes' `expansion_search`; `threads` is the `executor.size()` term of the default `max_proposals`
        (log(proposers) + threads). Members removed from either index take no part. The numbers of the run: `join_stats()`."""
        if not isinstance(other, Index):
            raise TypeError("join needs another usearch_amd.Index")
        a_keys, b_keys, stats = self.join_arrays(other, max_proposals, exact, expansion=expansion, threads=threads)
        return dict(zip(a_keys.tolist(), b_keys.tolist()))

    def join_arrays(self, other: "Index", max_proposals: int = 0, exact: bool = False, *, expansion: Optional[int] = None,
                    threads: int = 0):
        """`join` as two aligned key arrays in ascending order of `self`'s slots, and the `JoinStats` of the run."""
        if expansion is None:
            expansion = max(self.expansion_search or 64, other.expansion_search or 64)
        config = JoinConfig(max_proposals=max_proposals, expansion=expansion, exact=int(bool(exact)), threads=threads)
        capacity = min(len(self), len(other))
        a_keys = np.zeros(max(1, capacity), dtype=np.uint64)
        b_keys = np.zeros(max(1, capacity), dtype=np.uint64)
        stats = JoinStats()
        err = C.c_char_p()
        pairs = library().usearch_amd_join(self._handle, other._handle, C.byref(config), _pointer(a_keys), _pointer(b_keys), capacity,
                                           C.byref(stats), C.byref(err))
        _raise(err, "usearch_amd_join")
        self._join_stats = stats
        return a_keys[:pairs].copy(), b_keys[:pairs].copy(), stats

    def join_stats(self) -> dict:
        """Numbers of the last `join` called on this index: pairs, rounds, proposals, engagements, the list searches' visited and
        computed sums, P, ef, and the seconds of the lists and of the matching. `engagements` and the two counters are not the
        reference's: parallel rounds make no intermediate engagements, and one search stands for up to P of the reference's."""
        stats = getattr(self, "_join_stats", None)
        return stats.as_dict() if stats is not None else {}

    def isolate(self) -> int:
        """`index_dense_gt::isolate`: members whose key is the tombstone value leave every neighbour list, the rest of each list keeps
        its order. Returns the number of list cells erased; `compact_stats` has the rest."""
        stats, err = CompactStats(), C.c_char_p()
        if self._owner is not None:
            library().usearch_amd_build_isolate(self._owner._builder, C.byref(stats), C.byref(err))
        else:
            library().usearch_amd_snapshot_isolate(self._handle, C.byref(stats), C.byref(err))
        _raise(err, "usearch_amd_snapshot_isolate")
        self._compact_stats = stats
        return int(stats.pruned_edges)

    def compact(self, staging_bytes: int = 0, slot_map: bool = False):
        """`isolate`, then the removed members leave the index for good: survivors keep their order and are renumbered by rank, and
        the index has no tombstones afterwards (not the reference's `compact`, which permutes slots and keeps them). The stored
        rows move in place through a staging buffer of `staging_bytes` (0 = 64 MiB). Filters made before are refused afterwards.
        Returns the number of members dropped, or with `slot_map` the u32 array old slot → new slot (0xFFFFFFFF = removed)."""
        stats, err = CompactStats(), C.c_char_p()
        config = CompactConfig(C.sizeof(CompactConfig), staging_bytes)
        mapping = np.empty(self.size, dtype=np.uint32) if slot_map else None
        if self._owner is not None:  # the builder's levels and keys follow
            library().usearch_amd_build_compact(self._owner._builder, C.byref(config), _pointer(mapping), C.byref(stats), C.byref(err))
        else:
            library().usearch_amd_snapshot_compact(self._handle, C.byref(config), _pointer(mapping), C.byref(stats), C.byref(err))
        _raise(err, "usearch_amd_snapshot_compact")
        self._compact_stats = stats
        return mapping if slot_map else int(stats.removed_members)

    @property
    def compact_stats(self) -> dict:
        """Numbers of the last `isolate` / `compact` on this index (`usearch_amd_compact_stats_t`)."""
        stats = getattr(self, "_compact_stats", None)
        return stats.as_dict() if stats is not None else {}

    def distances(self, queries: np.ndarray, slots: np.ndarray) -> np.ndarray:
        """out[q, j] = metric(queries[q], stored vector of slot slots[q, j]); queries in the storage kind."""
        queries = np.ascontiguousarray(queries)
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        assert queries.ndim == 2 and slots.ndim == 2 and len(queries) == len(slots)
        out = np.zeros(slots.shape, dtype=np.float32)
        err = C.c_char_p()
        library().usearch_amd_distances(self._handle, _pointer(queries), len(queries), queries.strides[0],
                                        _pointer(slots), slots.shape[1], _pointer(out), C.byref(err))
        _raise(err, "usearch_amd_distances")
        return out


class BuiltIndex:
    """An index constructed on the MI355X (`usearch_amd_build`): a searchable `Index` (`.index`) plus the reference's
    serialized form (`.save_buffer()` / `.save(path)`), so the reference — or anything else that reads `.usearch` files —
    can load what was built. Mirrors the `Index(...)` + `add(keys, vectors)` + `save` sequence of python/usearch/index.py
    (index.py:400-520, 640-700, 1060-1100) collapsed into one call."""

    def __init__(self, handle: int):
        self._builder = handle
        self.index = Index(library().usearch_amd_build_snapshot(handle), owner=self)

    @property
    def stats(self) -> BuildStats:
        out = BuildStats()
        library().usearch_amd_build_stats(self._builder, C.byref(out))
        return out

    @property
    def serialized_length(self) -> int:
        return library().usearch_amd_build_serialized_length(self._builder)

    def extend(self, vectors: np.ndarray, keys: Optional[np.ndarray] = None) -> None:
        """Adds more members (rows of the storage kind) and links them in place (`usearch_amd_build_extend`)."""
        vectors = np.ascontiguousarray(vectors)
        keys = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
        err = C.c_char_p()
        library().usearch_amd_build_extend(C.c_void_p(self._builder), _pointer(vectors), len(vectors), vectors.strides[0], _pointer(keys),
                                           C.byref(err))
        _raise(err, "usearch_amd_build_extend")

    def update(self, slots: np.ndarray, vectors: np.ndarray, keys: np.ndarray) -> None:
        """Overwrites the members in `slots` with new rows and keys and links them anew in place (`usearch_amd_build_update`)."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        vectors, keys = np.ascontiguousarray(vectors), np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(slots) == len(vectors) == len(keys)
        err = C.c_char_p()
        library().usearch_amd_build_update(C.c_void_p(self._builder), _pointer(slots), len(slots), _pointer(vectors), vectors.strides[0],
                                           _pointer(keys), C.byref(err))
        _raise(err, "usearch_amd_build_update")

    def remove(self, slots, compact: bool = False) -> int:
        """Turns the members in `slots` into tombstones (`usearch_amd_build_remove`): they keep routing and stop matching. `compact`
        is the reference's keyword (python/lib.cpp:811-818): True calls `isolate` afterwards. Returns the number removed."""
        slots = np.ascontiguousarray(np.atleast_1d(slots), dtype=np.uint32)
        err = C.c_char_p()
        library().usearch_amd_build_remove(C.c_void_p(self._builder), _pointer(slots), len(slots), C.byref(err))
        _raise(err, "usearch_amd_build_remove")
        if compact:
            self.isolate()
        return len(slots)

    def isolate(self) -> int:
        """`Index.isolate` on the built index."""
        return self.index.isolate()

    def compact(self, staging_bytes: int = 0, slot_map: bool = False):
        """`Index.compact` on the built index: `save_buffer`, `extend` and `update` go on working over the survivors."""
        return self.index.compact(staging_bytes, slot_map)

    def clustering(self, **kwargs) -> Clustering:
        """`Index.clustering` on the built index."""
        return self.index.clustering(**kwargs)

    def save_buffer(self) -> np.ndarray:
        image = np.empty(self.serialized_length, dtype=np.uint8)
        err = C.c_char_p()
        library().usearch_amd_build_save_buffer(self._builder, _pointer(image), image.size, C.byref(err))
        _raise(err, "usearch_amd_build_save_buffer")
        return image

    def save(self, path) -> None:
        self.save_buffer().tofile(os.fspath(path))

    def close(self) -> None:
        if getattr(self, "_builder", None):
            self.index._handle = None
            self.index._owner = None
            err = C.c_char_p()
            library().usearch_amd_build_free(self._builder, C.byref(err))
            self._builder = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build(vectors, metric: str = "cos", dtype: Optional[str] = None, *, keys: Optional[np.ndarray] = None,
          connectivity: int = 16, expansion_add: int = 128, connectivity_base: int = 0, device: int = 0,
          max_batch: int = 0, batch_divisor: int = 0, seed: int = 0, ndim: Optional[int] = None,
          device_pointer: Optional[int] = None, count: Optional[int] = None, stride: Optional[int] = None) -> BuiltIndex:
    """Builds an HNSW index on the device. `vectors` is a [N, d] numpy matrix in the storage scalar kind (bit-packed
    `uint8` rows for `b1`); or pass `device_pointer` / `count` / `stride` / `ndim` / `dtype` for rows already in HBM."""
    err = C.c_char_p()
    config = BuildConfig(connectivity, connectivity_base, expansion_add, batch_divisor, max_batch, 0, seed)
    metric_kind = {name: kind for kind, name in METRIC_NAMES.items()}[metric]
    if keys is not None:
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if device_pointer is not None:
        assert dtype and ndim and count and stride
        handle = library().usearch_amd_build(C.c_void_p(device_pointer), count, stride, SCALAR_KINDS[dtype], ndim,
                                             metric_kind, _pointer(keys), C.byref(config), device, 1, C.byref(err))
    else:
        vectors = np.asarray(vectors)
        if dtype is None:
            dtype = _infer_dtype(vectors)
        if vectors.ndim != 2 or vectors.strides[1] != vectors.itemsize:
            vectors = np.ascontiguousarray(vectors)
        if ndim is None:
            ndim = vectors.shape[1] * 8 if dtype == "b1" else vectors.shape[1]
        handle = library().usearch_amd_build(_pointer(vectors), len(vectors), vectors.strides[0], SCALAR_KINDS[dtype],
                                             ndim, metric_kind, _pointer(keys), C.byref(config), device, 0,
                                             C.byref(err))
    _raise(err, "usearch_amd_build")
    if not handle:
        raise RuntimeError("usearch_amd_build: failed without a message")
    return BuiltIndex(handle)


def exact_search(dataset: np.ndarray, queries: np.ndarray, count: int, metric: str = "cos",
                 dtype: Optional[str] = None, tiled: bool = False):
    """`usearch.index.search(dataset, queries, count, exact=True)` (index.py:1608-1700) → (keys = row offsets [Q, k],
    distances [Q, k]); both matrices in the same scalar kind, rows may be strided. `tiled`: the matrix-unit kernel
    (csrc/exact_tiled.hip) over the uploaded rows — cos / ip / l2sq over f16, bf16 and i8, cos / ip over f32 — or the bit tile
    (csrc/exact_bits.hip: hamming / tanimoto / jaccard / sorensen over b1, the wave kernel's bits), count ≤ 64, any
    other pair is refused; float distances then lie within a derived bound of the f64 distance instead of being the wave kernel's bits (f32:
    not promised within 1e-5 of them). The default stays the bit-exact wave-per-query kernel."""
    dataset, queries = np.asarray(dataset), np.asarray(queries)
    if dtype is None:
        dtype = _infer_dtype(dataset)
    ndim = dataset.shape[1] * 8 if dtype == "b1" else dataset.shape[1]
    metric_kind = {name: kind for kind, name in METRIC_NAMES.items()}[metric]
    keys = np.zeros((len(queries), count), dtype=np.uint64)
    distances = np.zeros((len(queries), count), dtype=np.float32)
    err = C.c_char_p()
    entry = "usearch_amd_exact_search_dataset_tiled" if tiled else "usearch_amd_exact_search_dataset"
    getattr(library(), entry)(_pointer(dataset), len(dataset), dataset.strides[0], _pointer(queries), len(queries),
                              queries.strides[0], SCALAR_KINDS[dtype], ndim, metric_kind, count, _pointer(keys), keys.strides[0],
                              _pointer(distances), distances.strides[0], C.byref(err))
    _raise(err, entry)
    return keys, distances


def merge_many(distances: np.ndarray, keys: np.ndarray, counts: np.ndarray):
    """Host-buffer form of the shard merge: [P, Q, k] distances/keys + [P, Q] counts → ([Q, k] keys, distances, [Q] counts)."""
    distances = np.ascontiguousarray(distances, dtype=np.float32)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    shards, queries, wanted = distances.shape
    out_d = np.zeros((queries, wanted), dtype=np.float32)
    out_k = np.zeros((queries, wanted), dtype=np.uint64)
    out_c = np.zeros(queries, dtype=np.uint64)
    err = C.c_char_p()
    library().usearch_amd_merge_many(_pointer(distances), _pointer(keys), _pointer(counts), shards, queries, wanted,
                                     _pointer(out_d), _pointer(out_k), _pointer(out_c), C.byref(err))
    _raise(err, "usearch_amd_merge_many")
    return out_k, out_d, out_c


def merge_many_device(distances_ptr: int, keys_ptr: int, counts_ptr: int, shards: int, queries: int, wanted: int,
                      out_distances_ptr: int, out_keys_ptr: int, out_counts_ptr: int, stream: int = 0) -> None:
    err = C.c_char_p()
    library().usearch_amd_merge_many_device(C.c_void_p(distances_ptr), C.c_void_p(keys_ptr), C.c_void_p(counts_ptr),
                                            shards, queries, wanted, C.c_void_p(out_distances_ptr),
                                            C.c_void_p(out_keys_ptr), C.c_void_p(out_counts_ptr), C.c_void_p(stream),
                                            C.byref(err))
    _raise(err, "usearch_amd_merge_many_device")


def note_device_free() -> None:
    """Tells the engine that the host just released device memory through another allocator (`torch.cuda.empty_cache()`): the next
    loader or builder waits out the driver's settle window before it places its matrix (csrc/placement.hpp)."""
    library().usearch_amd_note_device_free()


def settle() -> float:
    """Waits out what is left of the settle window (at most USEARCH_AMD_SETTLE_MS = 1000); returns the milliseconds waited."""
    return float(library().usearch_amd_settle())


def device_count() -> int:
    err = C.c_char_p()
    n = library().usearch_amd_device_count(C.byref(err))
    return n


def cast(vector: np.ndarray, from_dtype: str, to_dtype: str, ndim: int) -> Optional[np.ndarray]:
    """Host-side query cast (`usearch_amd_cast`); None when the kinds are equal."""
    vector = np.ascontiguousarray(vector)
    nbytes = {"b1": (ndim + 7) // 8, "i8": ndim, "f16": 2 * ndim, "bf16": 2 * ndim, "f32": 4 * ndim,
              "f64": 8 * ndim}[to_dtype]
    out = np.zeros(nbytes, dtype=np.uint8)
    done = library().usearch_amd_cast(SCALAR_KINDS[from_dtype], SCALAR_KINDS[to_dtype], _pointer(vector), ndim,
                                      _pointer(out))
    return out if done else None


METRIC_KINDS = {name: kind for kind, name in METRIC_NAMES.items()}


def _matrix_to_cluster(X, dtype: Optional[str], what: str):
    """The checks of the reference's binding (python/lib.cpp:580-583): a rank-2 array whose rows are contiguous."""
    if not isinstance(X, np.ndarray) or X.ndim != 2:
        raise ValueError(f"Expects a matrix (rank-2 tensor) of {what}!")
    if X.strides[1] != X.itemsize:
        raise ValueError(f"{what.capitalize()} rows must be contiguous, try `ascontiguousarray`.")
    kind = "bf16" if X.dtype == np.uint16 else _infer_dtype(X)  # bf16 rows travel as their uint16 bit patterns
    if dtype not in SCALAR_KINDS:
        raise ValueError(f"Unsupported dtype {dtype}")
    return kind


def kmeans(X: np.ndarray, k: int, metric: str = "l2sq", dtype: str = "bf16", max_iterations: int = 300, inertia_threshold: float = 1e-4,
           max_seconds: float = 60.0, min_shifts: float = 0.01, seed: Optional[int] = None, *, device: int = 0,
           return_stats: bool = False):
    """`usearch.index.kmeans` (python/usearch/index.py:1618-1712) on the device: clusters the rows of `X` into `k` groups, the loop
    running in the scalar kind `dtype`. → (assignments uint64[N], distances float32[N], centroids [k, ndim] in X's dtype), and the
    run's `KMeansStats` as a fourth element with `return_stats`. `seed=None` draws one from `os.urandom`. The reference's behaviour
    is kept as it is, seeds that may repeat and an inertia exit that cannot fire included (csrc/kmeans.hip)."""
    kind = _matrix_to_cluster(X, dtype, "dataset to cluster")
    if metric not in METRIC_KINDS:
        raise ValueError(f"Unsupported metric {metric}")
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")
    count, ndim = X.shape
    config = KMeansConfig(C.sizeof(KMeansConfig), METRIC_KINDS[metric], SCALAR_KINDS[dtype], int(max_iterations), float(inertia_threshold),
                          float(max_seconds), float(min_shifts), int(seed) & (2**64 - 1), int(device))
    assignments = np.zeros(count, dtype=np.uint64)
    distances = np.zeros(count, dtype=np.float32)
    centroids = np.zeros((max(int(k), 0), ndim), dtype=X.dtype)
    stats, err = KMeansStats(), C.c_char_p()
    library().usearch_amd_kmeans(_pointer(X), count, X.strides[0], SCALAR_KINDS[kind], ndim, max(int(k), 0), C.byref(config),
                                 _pointer(centroids), centroids.strides[0], _pointer(assignments), _pointer(distances), C.byref(stats),
                                 C.byref(err))
    if err.value:
        raise ValueError(err.value.decode())  # the reference's binding raises the class's message as a ValueError (python/lib.cpp:159)
    return (assignments, distances, centroids, stats) if return_stats else (assignments, distances, centroids)


def kmeans_assign(X: np.ndarray, centroids: np.ndarray, metric: str = "l2sq", dtype: str = "bf16", *, device: int = 0):
    """The assignment step of `kmeans` alone: rows of `X` and of `centroids` (one numpy dtype) are cast to `dtype` on the device and
    every point gets its nearest centroid, the lowest index among equals → (assignments uint64[N], distances float32[N])."""
    kind = _matrix_to_cluster(X, dtype, "dataset to assign")
    if _matrix_to_cluster(centroids, dtype, "centroids") != kind or centroids.shape[1] != X.shape[1]:
        raise ValueError("The points and the centroids must have one dtype and one number of dimensions")
    if metric not in METRIC_KINDS:
        raise ValueError(f"Unsupported metric {metric}")
    count, ndim = X.shape
    assignments = np.zeros(count, dtype=np.uint64)
    distances = np.zeros(count, dtype=np.float32)
    err = C.c_char_p()
    library().usearch_amd_kmeans_assign(_pointer(X), count, X.strides[0], _pointer(centroids), len(centroids), centroids.strides[0],
                                        SCALAR_KINDS[kind], ndim, METRIC_KINDS[metric], SCALAR_KINDS[dtype], int(device),
                                        _pointer(assignments), _pointer(distances), C.byref(err))
    if err.value:
        raise ValueError(err.value.decode())
    return assignments, distances


TEST_HOOKS_PATH = os.path.join(os.path.dirname(LIBRARY_PATH), "libusearch_amd_testhooks.so")
_test_hooks = None


def test_hooks() -> C.CDLL:
    """The self-test / micro-benchmark entry points of the device containers: their own library (csrc/test_hooks.hip), which the
    product library does not carry."""
    global _test_hooks
    if _test_hooks is None:
        library()  # one HIP runtime per process, mapped by the product library's loader
        if not os.path.exists(TEST_HOOKS_PATH):
            raise RuntimeError(f"{TEST_HOOKS_PATH} is missing: build it with `make -C usearch_amd/csrc`")
        _test_hooks = C.CDLL(TEST_HOOKS_PATH, mode=os.RTLD_LOCAL)
        for name, arguments in (("gather_probe", [C.c_void_p, C.c_size_t, C.c_size_t]), ("translation_probe", [C.c_void_p, C.c_size_t]),
                                ("latency_probe", [C.c_void_p, C.c_size_t, C.c_size_t])):
            probe = getattr(_test_hooks, f"usearch_amd_test_{name}")
            probe.restype = C.c_float
            probe.argtypes = arguments + [C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_containers.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p,
                                                            C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p,
                                                            C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_merge.restype = None
        _test_hooks.usearch_amd_test_merge.argtypes = [C.c_void_p] * 3 + [C.c_size_t] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [
            C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_top.restype = None
        _test_hooks.usearch_amd_test_top.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_sketch_bounds.restype = None
        _test_hooks.usearch_amd_test_sketch_bounds.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int,
                                                               C.c_size_t, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_char_p)]
        error = C.POINTER(C.c_char_p)
        for name, restype, arguments in (
                ("device_records", None, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_void_p, C.c_double, C.c_void_p]),
                ("directions", None, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
                ("twin_records", None, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_double, C.c_void_p]),
                ("twin_bounds", None, [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_void_p]),
                ("read_back", C.c_uint64, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)])):
            hook = getattr(_test_hooks, f"usearch_amd_test_sketch_{name}")
            hook.restype, hook.argtypes = restype, arguments + [error]
        _test_hooks.usearch_amd_test_plan_search.restype = C.c_size_t
        _test_hooks.usearch_amd_test_plan_search.argtypes = [C.POINTER(PlanShape), C.POINTER(PlanTuning), C.c_void_p, C.c_size_t,
                                                             C.POINTER(PlanKnobs), C.POINTER(Plan), C.POINTER(PlanRung),
                                                             C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_plan_exact.restype = C.c_int
        _test_hooks.usearch_amd_test_plan_exact.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int,
                                                            C.POINTER(ExactPlan), C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_exact_tiled_pair.restype = C.c_int
        _test_hooks.usearch_amd_test_exact_tiled_pair.argtypes = [C.c_int, C.c_int, C.c_uint64]
        _test_hooks.usearch_amd_test_exact_bits_pair.restype = C.c_int
        _test_hooks.usearch_amd_test_exact_bits_pair.argtypes = [C.c_int, C.c_int, C.c_uint64]
        _test_hooks.usearch_amd_test_plan_exact_bits.restype = C.c_int
        _test_hooks.usearch_amd_test_plan_exact_bits.argtypes = [C.c_uint64] * 5 + [C.c_void_p, C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_kmeans_quantize.restype = None
        _test_hooks.usearch_amd_test_kmeans_quantize.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                                                 C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p)]
        _test_hooks.usearch_amd_test_device_scratch.restype = None
        _test_hooks.usearch_amd_test_device_scratch.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                                                C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)]
    return _test_hooks


class _PlainStruct(C.Structure):
    def as_dict(self) -> dict:
        values = ((name, getattr(self, name)) for name, _ in self._fields_)
        return {name: ({field: getattr(value, field) for field, _ in value._fields_} if isinstance(value, C.Structure) else value)
                for name, value in values}


def _struct(name: str, *groups) -> type:
    return type(name, (_PlainStruct,), {"_fields_": [(field, kind) for kind, fields in groups for field in fields.split()]})


# the planner's plain structs (csrc/engine.hpp: search_shape_t, search_tuning_t, search_knobs_t, search_plan_t, search_rung_t)
PlanShape = _struct("PlanShape", (C.c_uint64, "size count wanted expansion"), (C.c_int32, "metric scalar"),
                    (C.c_uint32, "lanes chunks m0 compute_units has_tombstones nbr0 nbr0_rows sketch query_ids beam_level descent_only "
                                 "allow_bits exclude_own reference_frontier"))
PlanTuning = _struct("PlanTuning", (C.c_uint32, "hash_cap next_cap variant mode waves_per_cu top_in_memory frontier wave_clock sketch"))
PlanKnobs = _struct("PlanKnobs", (C.c_size_t, "lds_budget hash_cap hash_load_pct next_cap mode top_in_memory no_two_cells frontier variant "
                                              "no_team no_plain waves_per_cu no_small_batch_lds early_rows aside_cells "
                                              "plain_whatever_the_room seen_cells"))
Plan = _struct("Plan", (C.c_uint32, "ef query_lds entries_per_lane waves_cap hash_cap next_cap"), (C.c_int32, "mode variant frontier"),
               (C.c_uint32, "team plain_possible sketch"), (Stats, "stats"))
PlanRung = _struct("PlanRung", (C.c_int32, "mode frontier"),
                   (C.c_uint32, "team plain entries_per_lane grid lds_bytes hash_cap next_cap early_rows "
                                "aside_offset aside_cells seen_offset seen_cells sketch_offset team_offset"),
                   (C.c_uint64, "slab visits_offset bitmap_bytes"))


def test_plan_search(shape: dict, tuning: dict, pending, knobs: Optional[dict] = None):
    """The launch planner (csrc/search_plan.hpp) on plain values, no GPU involved: what a search of `shape` (fields of `PlanShape`;
    `metric` and `dtype` by name) under `tuning` settles, and one rung of the retry ladder per entry of `pending` until one is the
    global rung. `knobs` (fields of `PlanKnobs`) replace the environment's overrides; None reads USEARCH_AMD_* as the engine does.
    → (plan, [rung, …]) as dicts, `plan["stats"]` holding what `Stats` would report of these decisions; a refusal raises."""
    shape = dict(shape)  # metric_kind_t (jaccard walks as tanimoto) and scalar_kind_t of csrc/common.hpp
    shape["metric"] = ord({"ip": "i", "cos": "c", "l2sq": "e", "hamming": "b", "pearson": "p", "haversine": "h", "divergence": "d",
                           "jaccard": "t", "tanimoto": "t", "sorensen": "s"}[shape["metric"]])
    shape["scalar"] = {"b1": 1, "bf16": 4, "f64": 10, "f32": 11, "f16": 12, "i8": 23}[shape.pop("dtype")]
    pending = np.ascontiguousarray(pending, dtype=np.uint32)
    plan, rungs, err = Plan(), (PlanRung * max(1, len(pending)))(), C.c_char_p()
    planned = test_hooks().usearch_amd_test_plan_search(C.byref(PlanShape(**shape)), C.byref(PlanTuning(**tuning)), _pointer(pending),
                                                        len(pending), C.byref(PlanKnobs(**knobs)) if knobs is not None else None,
                                                        C.byref(plan), rungs, C.byref(err))
    _raise(err, "usearch_amd_test_plan_search")
    return plan.as_dict(), [rungs[i].as_dict() for i in range(planned)]


# the tiled exact search's plan (csrc/exact_plan.hpp: exact_plan_t)
ExactPlan = _struct("ExactPlan", (C.c_uint32, "wide lds_lists"), (C.c_uint64, "query_tiles partitions rows_per_partition tiles_per_xcd workgroups"))


def test_plan_exact(rows: int, bytes_per_vector: int, row_stride: int, count: int, wanted: int, forced_tile: Optional[int] = None,
                    global_lists: Optional[bool] = None) -> dict:
    """The tiled exact search's planner (csrc/exact_plan.hpp) on plain values, no GPU involved: which kernel a batch of `count` queries
    for `wanted` results over `rows` rows takes and how the rows are split. `forced_tile` / `global_lists` replace
    USEARCH_AMD_EXACT_TILE / USEARCH_AMD_EXACT_GLOBAL_LISTS; None reads them as the engine does. → the fields of `ExactPlan` as a dict;
    a refusal raises."""
    plan, err = ExactPlan(), C.c_char_p()
    test_hooks().usearch_amd_test_plan_exact(rows, bytes_per_vector, row_stride, count, wanted, -1 if forced_tile is None else int(forced_tile),
                                             -1 if global_lists is None else int(bool(global_lists)), C.byref(plan), C.byref(err))
    _raise(err, "usearch_amd_test_plan_exact")
    return plan.as_dict()


def test_exact_tiled_pair(metric: str, dtype: str, wanted: int) -> bool:
    """Is there a tiled (matrix-unit) exact-search kernel for `metric` over `dtype` rows and `wanted` results per query? The table of
    csrc/exact_plan.hpp (`exact_tiled_pair`) that `exact="tiled"` and `exact_search(…, tiled=True)` are refused by; no GPU involved."""
    metric_kind = ord({"ip": "i", "cos": "c", "l2sq": "e", "hamming": "b", "pearson": "p", "haversine": "h", "divergence": "d",
                       "jaccard": "j", "tanimoto": "t", "sorensen": "s"}[metric])  # metric_kind_t and scalar_kind_t of csrc/common.hpp
    scalar_kind = {"b1": 1, "bf16": 4, "f64": 10, "f32": 11, "f16": 12, "i8": 23}[dtype]
    return bool(test_hooks().usearch_amd_test_exact_tiled_pair(metric_kind, scalar_kind, wanted))


# the bit tile's plan (csrc/exact_plan.hpp: exact_bits_plan_t)
ExactBitsPlan = _struct("ExactBitsPlan", (C.c_uint64, "query_tiles partitions rows_per_partition padded_queries padded_query_bytes lds_bytes"))


def test_exact_bits_pair(metric: str, dtype: str, wanted: int) -> bool:
    """Does the bit tile (csrc/exact_bits.hip) take `metric` over `dtype` rows for `wanted` results per query? The table of
    csrc/exact_plan.hpp (`exact_bits_pair`): hamming, tanimoto, jaccard and sorensen over b1, 1 … 64 results; no GPU involved."""
    metric_kind = ord({"ip": "i", "cos": "c", "l2sq": "e", "hamming": "b", "pearson": "p", "haversine": "h", "divergence": "d",
                       "jaccard": "j", "tanimoto": "t", "sorensen": "s"}[metric])  # metric_kind_t and scalar_kind_t of csrc/common.hpp
    scalar_kind = {"b1": 1, "bf16": 4, "f64": 10, "f32": 11, "f16": 12, "i8": 23}[dtype]
    return bool(test_hooks().usearch_amd_test_exact_bits_pair(metric_kind, scalar_kind, wanted))


def test_plan_exact_bits(rows: int, bytes_per_vector: int, row_stride: int, count: int, wanted: int) -> dict:
    """The bit tile's planner (csrc/exact_plan.hpp, `plan_exact_bits`) on plain values, no GPU involved: the grid of (query tiles of 256,
    row partitions) a batch of `count` queries for `wanted` results over `rows` rows takes. One variant: nothing to force, and the
    environment is not read. → the fields of `ExactBitsPlan` as a dict; a refusal raises."""
    plan, err = ExactBitsPlan(), C.c_char_p()
    test_hooks().usearch_amd_test_plan_exact_bits(rows, bytes_per_vector, row_stride, count, wanted, C.byref(plan), C.byref(err))
    _raise(err, "usearch_amd_test_plan_exact_bits")
    return plan.as_dict()


def test_kmeans_quantize(X: np.ndarray, from_dtype: str, to_dtype: str, device: int = 0) -> np.ndarray:
    """The matrix `kmeans` clusters: the rows of `X` after the device cast (csrc/kmeans.hip) → uint8 [N, bytes per quantised row]."""
    X = np.ascontiguousarray(X)
    kinds = {"bf16": 4, "f64": 10, "f32": 11, "f16": 12, "i8": 23}  # scalar_kind_t of csrc/common.hpp
    count, ndim = X.shape
    width = {"i8": ndim, "f16": 2 * ndim, "bf16": 2 * ndim, "f32": 4 * ndim}[to_dtype]
    out = np.zeros((count, width), dtype=np.uint8)
    err = C.c_char_p()
    test_hooks().usearch_amd_test_kmeans_quantize(_pointer(X), count, X.strides[0], kinds[from_dtype], ndim, kinds[to_dtype], device,
                                                  _pointer(out), out.strides[0], C.byref(err))
    _raise(err, "usearch_amd_test_kmeans_quantize")
    return out


def test_sketch_bounds(rows: np.ndarray, queries: np.ndarray, dtype: str):
    """Host twins of the sketch (csrc/sketch.hpp): records of `rows` under directions drawn from them, and for every (query, row)
    the lower bound of the cos distance the walk would compare with its radius → (bounds [queries, rows] f32, number of directions)."""
    rows, queries = np.ascontiguousarray(rows), np.ascontiguousarray(queries)
    assert rows.ndim == 2 and queries.ndim == 2 and rows.shape[1] == queries.shape[1] and rows.dtype == queries.dtype
    kind = {"f32": 11, "f16": 12, "bf16": 4}[dtype]  # scalar_kind_t of csrc/common.hpp
    bounds = np.zeros((len(queries), len(rows)), dtype=np.float32)
    rank, err = C.c_uint32(), C.c_char_p()
    test_hooks().usearch_amd_test_sketch_bounds(_pointer(rows), len(rows), _pointer(queries), len(queries), rows.shape[1], kind,
                                                rows.strides[0], _pointer(bounds), C.byref(rank), C.byref(err))
    _raise(err, "usearch_amd_test_sketch_bounds")
    return bounds, int(rank.value)


_SKETCH_KINDS = {"f32": 11, "f16": 12, "bf16": 4}  # scalar_kind_t of csrc/common.hpp
SKETCH_COLUMNS, SKETCH_RECORD_BYTES = 64, 128


def _sketch_rows(rows: np.ndarray, directions: Optional[np.ndarray] = None):
    rows = np.ascontiguousarray(rows)
    assert rows.ndim == 2
    if directions is None:
        return rows
    directions = np.ascontiguousarray(directions, dtype=np.float32)
    assert directions.shape == (rows.shape[1], SKETCH_COLUMNS), "directions are [dimensions][64] f32"
    return rows, directions


def test_sketch_directions(rows: np.ndarray, dtype: str):
    """The directions the engine draws from `rows` (csrc/sketch.hpp `sketch_orthonormalise` over the rows at the seeded slots), no GPU
    involved → (transposed [dimensions, 64] f32, number of directions, gram defect)."""
    rows = _sketch_rows(rows)
    transposed = np.zeros((rows.shape[1], SKETCH_COLUMNS), dtype=np.float32)
    rank, defect, err = C.c_uint32(), C.c_double(), C.c_char_p()
    test_hooks().usearch_amd_test_sketch_directions(_pointer(rows), len(rows), rows.strides[0], rows.shape[1], _SKETCH_KINDS[dtype],
                                                    _pointer(transposed), C.byref(rank), C.byref(defect), C.byref(err))
    _raise(err, "usearch_amd_test_sketch_directions")
    return transposed, int(rank.value), float(defect.value)


def test_sketch_twin_records(rows: np.ndarray, dtype: str, directions: np.ndarray, gram_defect: float) -> np.ndarray:
    """`sketch_record_host` (the host twin of the record builder) for every row under `directions`, no GPU involved → uint8 [rows, 128]."""
    rows, directions = _sketch_rows(rows, directions)
    records = np.zeros((len(rows), SKETCH_RECORD_BYTES), dtype=np.uint8)
    err = C.c_char_p()
    test_hooks().usearch_amd_test_sketch_twin_records(_pointer(rows), len(rows), rows.strides[0], rows.shape[1], _SKETCH_KINDS[dtype],
                                                      _pointer(directions), float(gram_defect), _pointer(records), C.byref(err))
    _raise(err, "usearch_amd_test_sketch_twin_records")
    return records


def test_sketch_twin_bounds(queries: np.ndarray, sums_of_squares: np.ndarray, dtype: str, directions: np.ndarray, records: np.ndarray):
    """`sketch_query_host` and `sketch_bound_host` (the host twins of the walk's side), no GPU involved: `queries` in the storage kind,
    `sums_of_squares[q]` the f32 Σa² the kernel has for query q → (bounds [queries, records] f32, −inf for a query that does not use the
    sketch; used [queries] bool)."""
    queries, directions = _sketch_rows(queries, directions)
    records = np.ascontiguousarray(records, dtype=np.uint8)
    sums = np.ascontiguousarray(sums_of_squares, dtype=np.float32)
    assert records.ndim == 2 and records.shape[1] == SKETCH_RECORD_BYTES and sums.shape == (len(queries),)
    bounds = np.zeros((len(queries), len(records)), dtype=np.float32)
    used = np.zeros(len(queries), dtype=np.uint8)
    err = C.c_char_p()
    test_hooks().usearch_amd_test_sketch_twin_bounds(_pointer(queries), len(queries), queries.strides[0], _pointer(sums), queries.shape[1],
                                                     _SKETCH_KINDS[dtype], _pointer(directions), _pointer(records), len(records),
                                                     _pointer(bounds), _pointer(used), C.byref(err))
    _raise(err, "usearch_amd_test_sketch_twin_bounds")
    return bounds, used.astype(bool)


def test_sketch_device_records(rows: np.ndarray, dtype: str, directions: np.ndarray, gram_defect: float, first: int = 0,
                               pattern: int = 0xA5) -> np.ndarray:
    """The device's record builder (csrc/sketch.hip `sketch_records_kernel`, launched as `make_sketch` launches it) over rows
    [first, len(rows)) under `directions` → uint8 [rows, 128]; the buffer is filled with `pattern` first, which rows below `first` keep."""
    rows, directions = _sketch_rows(rows, directions)
    records = np.full((len(rows), SKETCH_RECORD_BYTES), pattern, dtype=np.uint8)
    err = C.c_char_p()
    test_hooks().usearch_amd_test_sketch_device_records(_pointer(rows), len(rows), rows.strides[0], rows.shape[1], _SKETCH_KINDS[dtype],
                                                        int(first), _pointer(directions), float(gram_defect), _pointer(records),
                                                        C.byref(err))
    _raise(err, "usearch_amd_test_sketch_device_records")
    return records


def test_sketch_read_back(index: "Index"):
    """The sketch a snapshot holds, copied to the host → (records uint8 [members, 128], directions f32 [dimensions, 64], gram defect,
    stored rows uint8 [members, bytes per vector]), or None when the snapshot has no sketch."""
    err = C.c_char_p()
    hook = test_hooks().usearch_amd_test_sketch_read_back
    count = int(hook(index._handle, None, None, None, None, C.byref(err)))
    _raise(err, "usearch_amd_test_sketch_read_back")
    if not count:
        return None
    records = np.zeros((count, SKETCH_RECORD_BYTES), dtype=np.uint8)
    directions = np.zeros((index.ndim, SKETCH_COLUMNS), dtype=np.float32)
    rows = np.zeros((count, index.bytes_per_vector), dtype=np.uint8)
    defect = C.c_double()
    hook(index._handle, _pointer(records), _pointer(directions), _pointer(rows), C.byref(defect), C.byref(err))
    _raise(err, "usearch_amd_test_sketch_read_back")
    return records, directions, float(defect.value), rows


def test_device_scratch(home: int, current: int) -> dict:
    """The holder of per-call device memory (csrc/device_scratch.hpp), no kernel involved: with device `current` selected, a holder for
    device `home` takes blocks of 0, 1 and 4096 bytes, then is refused 2^60 bytes. → what was read after the refusal: `pointers`,
    `devices` and `room` (bytes behind each pointer) of the three blocks, the refusal's `refused` (a hipError_t, 0 = it was granted)
    and `refused_pointer` (what the refused request left in its out-pointer; 0 = null)."""
    pointers, room = np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    devices = np.full(3, -1, dtype=np.int32)
    refused, refused_pointer, err = C.c_int(), C.c_void_p(1), C.c_char_p()
    test_hooks().usearch_amd_test_device_scratch(home, current, _pointer(pointers), _pointer(devices), _pointer(room), C.byref(refused),
                                                 C.byref(refused_pointer), C.byref(err))
    _raise(err, "usearch_amd_test_device_scratch")
    return {"pointers": [int(p) for p in pointers], "devices": [int(d) for d in devices], "room": [int(r) for r in room],
            "refused": int(refused.value), "refused_pointer": int(refused_pointer.value or 0)}


def test_containers(kinds: np.ndarray, keys: np.ndarray, slots: np.ndarray, limit: int, global_memory: bool = False, remains: bool = False):
    """Device container self-test hook → (popped[(key, slot)], top[(distance, slot)]), and with `remains` the heap's cells as they lie
    after the script as a third pair. `global_memory`: heap and buffer in device memory (the all-global fallback's accessors), else LDS."""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint32)
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    n = len(kinds)
    popped = np.zeros(n + 1, dtype=np.uint64)
    top = np.zeros(limit + 1, dtype=np.uint64)
    heap = np.zeros(int((kinds == 0).sum()) + 1, dtype=np.uint64)
    popped_count, top_count, heap_count = C.c_size_t(), C.c_size_t(), C.c_size_t()
    err = C.c_char_p()
    test_hooks().usearch_amd_test_containers(_pointer(kinds), _pointer(keys), _pointer(slots), n, limit, int(bool(global_memory)),
                                             _pointer(popped), C.byref(popped_count), _pointer(top), C.byref(top_count), _pointer(heap),
                                             C.byref(heap_count), C.byref(err))
    _raise(err, "usearch_amd_test_containers")

    def unpack(a):
        bits = (a & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        return bits.view(np.float32), (a >> np.uint64(32)).astype(np.uint32)

    pairs = unpack(popped[: popped_count.value]), unpack(top[: top_count.value])
    return pairs + (unpack(heap[: heap_count.value]),) if remains else pairs


TOP_CLOSED_BIT = 0x80000000  # `top_gt::closed_bit_k`: the frontier flag in a cell's slot word
TOP_NONE = 0xFFFFFFFF  # `none_slot_k`


def test_top(epl: int, flags: bool, global_memory: bool, kinds: np.ndarray, keys: np.ndarray, slots: np.ndarray, limit: int):
    """Self-test hook of `top` as the search kernels hold it: one wave replays the script on `top_gt<epl, global_memory, flags>` (epl
    1, 2, 4, 8, 16 = cells per lane in registers; 0 = scratch memory, LDS or with `global_memory` device memory). kinds: 0 = insert
    under the traversal's acceptance rule, 1 = the same, closed on arrival (flagged layouts), 2 = `first_open` + `close`.
    → (records uint32[n, 6] = accepted-or-found, size, radius bits, popped distance bits, popped slot, popped cell number;
    cell distance bits and cell slot words, all 64 · epl cells of a register layout or the first `size` of a scratch one; size).
    Cells the kernel does not write come back as 0xDEADBEEF."""
    kinds = np.ascontiguousarray(kinds, dtype=np.uint32)
    keys = np.ascontiguousarray(keys, dtype=np.float32)
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    n, cells = len(kinds), (64 * epl if epl else limit)
    records = np.zeros((n, 6), dtype=np.uint32)
    cell_bits = np.full(cells, 0xDEADBEEF, dtype=np.uint32)
    cell_slots = np.full(cells, 0xDEADBEEF, dtype=np.uint32)
    size, err = C.c_uint32(), C.c_char_p()
    test_hooks().usearch_amd_test_top(epl, int(bool(flags)), int(bool(global_memory)), _pointer(kinds), _pointer(keys), _pointer(slots), n,
                                      limit, _pointer(records), _pointer(cell_bits), _pointer(cell_slots), C.byref(size), C.byref(err))
    _raise(err, "usearch_amd_test_top")
    shown = cells if epl else int(size.value)
    return records, cell_bits[:shown], cell_slots[:shown], int(size.value)


def test_merge(distances: np.ndarray, keys: np.ndarray, counts: np.ndarray, later_position_first: bool = True, on_host: bool = False,
               key_sentinel: int = 0xABABABABABABABAB, distance_sentinel_bits: int = 0xCDCDCDCD):
    """Self-test hook of the fold of per-shard lists, `merge_many` with the order inside a shard exposed: `later_position_first` as
    `merge_into` (the sharded step), False = the earlier position in front (the partitions of an exact search). `on_host`: `merge_rank`
    walked as the sharded step's host path walks it, no device involved; else the merge kernel. The output buffers hold the sentinels
    before the merge, so a cell it never writes shows. → ([Q, k] keys, distances, [Q] counts)."""
    distances = np.ascontiguousarray(distances, dtype=np.float32)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    shards, queries, wanted = distances.shape
    out_d = np.full((queries, wanted), distance_sentinel_bits, dtype=np.uint32).view(np.float32)
    out_k = np.full((queries, wanted), key_sentinel, dtype=np.uint64)
    out_c = np.full(queries, key_sentinel, dtype=np.uint64)
    err = C.c_char_p()
    test_hooks().usearch_amd_test_merge(_pointer(distances), _pointer(keys), _pointer(counts), shards, queries, wanted,
                                        int(bool(later_position_first)), int(bool(on_host)), _pointer(out_d), _pointer(out_k),
                                        _pointer(out_c), C.byref(err))
    _raise(err, "usearch_amd_test_merge")
    return out_k, out_d, out_c
