"""The engine library exports `isolate` / `compact` (include/usearch_amd.h) and the binding declares them: looked up by name after
`build()`, as every other CPU test finds its symbols. Without the feature the lookup fails."""
import ctypes
import os
import subprocess

import usearch_amd

ENGINE_SYMBOLS = ["usearch_amd_snapshot_isolate", "usearch_amd_snapshot_compact", "usearch_amd_build_remove",
                  "usearch_amd_build_isolate", "usearch_amd_build_compact"]


def test_the_engine_library_exports_isolate_and_compact():
    library = ctypes.CDLL(usearch_amd.LIBRARY_PATH)
    for name in ENGINE_SYMBOLS:
        assert getattr(library, name) is not None
        assert name in usearch_amd.EXPORTED_SYMBOLS


def test_the_binding_mirrors_the_c_structs():
    """Field for field with `usearch_amd_compact_config_t` / `usearch_amd_compact_stats_t`: 2 × size_t; 5 × u64, 2 × u32, 3 × f32, u32."""
    assert ctypes.sizeof(usearch_amd.CompactConfig) == 2 * ctypes.sizeof(ctypes.c_size_t)
    assert ctypes.sizeof(usearch_amd.CompactStats) == 5 * 8 + 2 * 4 + 3 * 4 + 4
    assert [name for name, _ in usearch_amd.CompactStats._fields_][:5] == ["pruned_edges", "removed_members", "survivors", "moved_bytes", "chunks"]
    assert usearch_amd.library().usearch_amd_compact_scan_chunk() == 1024
    for method in ("isolate", "compact", "compact_stats"):
        assert hasattr(usearch_amd.Index, method)
    for method in ("remove", "isolate", "compact"):
        assert hasattr(usearch_amd.BuiltIndex, method)


def test_the_drop_in_library_exports_isolate_and_compact():
    library = ctypes.CDLL(os.path.join(os.path.dirname(usearch_amd.LIBRARY_PATH), "libusearch_c.so"))
    for name in ("usearch_isolate", "usearch_compact"):
        assert getattr(library, name) is not None


def build_compact_surface(directory) -> str:
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "usearch_amd", "lib")
    binary = os.path.join(str(directory), "usearch_amd_compact_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "compact_surface.cpp"), "-L", lib, "-l:libusearch_c.so", f"-Wl,-rpath,{lib}",
                           "-o", binary])
    return binary


def test_a_caller_of_isolate_and_compact_compiles_against_the_class_surface(tmp_path):
    """The reference's `test_isolate` (cpp/test.cpp:1147-1180) plus `compact()` compile and link against
    include/usearch/index_dense.hpp (run on the device by tests/test_gpu_compact_dropin.py)."""
    binary = build_compact_surface(tmp_path)
    assert "isolate and compact through index_dense_t" in subprocess.check_output([binary, "link"]).decode()
