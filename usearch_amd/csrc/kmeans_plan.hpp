/**
 *  usearch_amd/csrc/kmeans_plan.hpp — the ONE place that chooses how the k-means assignment over f16 / bf16 / i8 rows (kmeans.hip) is
 *  launched: the 64 × 128 register-staged tile (`assign_tiled_kernel`) or the 256 × 256 LDS-DMA tile (`assign_wide_kernel`). Pure
 *  integer arithmetic over plain values, like exact_plan.hpp's planner: no HIP runtime call, no look at the environment (the caller
 *  reads USEARCH_AMD_KMEANS_TILE and passes it in). tests/test_gpu_kmeans_wide.py asserts its routes through
 *  `usearch_amd_test_plan_kmeans_assign`.
 *
 *  f32 rows have a sibling decision, `plan_kmeans_assign_f32`: the wave-per-point kernel (`assign_f32_kernel`) or the screened
 *  64 × 128 tile (`assign_screened_kernel`), which returns the wave kernel's bits. There is no 256 × 256 tile for f32 — the screen's
 *  contender sets would have to live beside eight accumulators per lane, and nobody has measured whether that pays: out of scope.
 */
#pragma once
#include <cstdint>

#include "wide_stage.hpp"

namespace usearch_amd {

constexpr int kmeans_tile_points_k = staged_a_rows_k;    ///< points per workgroup of the 64 tile
constexpr int kmeans_tile_centroids_k = staged_b_rows_k; ///< centroids per inner tile of the 64 tile: 128

/// Unforced, the wide tile takes a run from here on; both numbers are read off the sweep in profiles/r16_kmeans_wide/README.md
/// (768-d bf16 on an MI355X). 65 536 points are 256 point tiles, one per compute unit of the chip (a workgroup's two staging
/// buffers leave room for one workgroup per compute unit): at 16 384 points three quarters of the chip stand idle for the whole
/// launch and the 64 tile is 1.3 × faster at every centroid count. 1 024 centroids are four centroid tiles: from there the wide tile
/// is 1.2 … 1.5 × faster at every point count ≥ 65 536; at 256 centroids — one tile, a 12-chunk pipeline that is mostly prologue
/// and epilogue — the two are within 4 % of each other either way. (512 was not measured: it stays with the 64 tile.)
constexpr std::uint64_t kmeans_wide_least_centroids_k = 1024;
constexpr std::uint64_t kmeans_wide_least_points_k = 256u * wide_tile_k;

/// LDS of a wide workgroup: the two staging buffers and its points' Σx² (the running pairs live in registers).
constexpr std::uint32_t kmeans_wide_lds_bytes_k = wide_buffers_k * wide_stage_bytes_k + wide_tile_k * 4;

/// What both matrices look like to the wide tile: whole 128-byte chunks of every row, whole tiles of 256 rows, zeros beyond the data.
inline std::uint64_t kmeans_wide_stride(std::uint64_t stride) { return (stride + chunk_bytes_k - 1) / chunk_bytes_k * chunk_bytes_k; }
inline std::uint64_t kmeans_wide_rows(std::uint64_t rows) { return (rows + wide_tile_k - 1) / wide_tile_k * wide_tile_k; }

struct kmeans_assign_plan_t {
    std::uint32_t wide = 0;           ///< 1: the 256 × 256 tile
    std::uint32_t lds_bytes = 0;      ///< dynamic LDS of a workgroup
    std::uint64_t point_tiles = 0;    ///< = workgroups
    std::uint64_t centroid_tiles = 0; ///< tiles every workgroup streams past its points
};

/// `count` points against `clusters` centroids, quantised rows `stride` bytes apart (16-byte pieces, as the 64 tile wants them).
/// `forced_tile`: USEARCH_AMD_KMEANS_TILE — 64 / 256 force a tile where it can run, anything else leaves the choice here.
inline kmeans_assign_plan_t plan_kmeans_assign(std::uint64_t count, std::uint64_t clusters, std::uint64_t stride, std::uint64_t forced_tile) {
    kmeans_assign_plan_t plan;
    // (a tile of 256 padded rows is one buffer resource with 32-bit offsets: rows of < 8 MB)
    const bool can = count && clusters && stride && kmeans_wide_stride(stride) * wide_tile_k < (1ull << 31);
    const bool wants = forced_tile == 256 ||
                       (forced_tile != 64 && clusters >= kmeans_wide_least_centroids_k && count >= kmeans_wide_least_points_k);
    plan.wide = can && wants ? 1u : 0u;
    if (plan.wide) {
        plan.point_tiles = (count + wide_tile_k - 1) / wide_tile_k;
        plan.centroid_tiles = (clusters + wide_tile_k - 1) / wide_tile_k;
        plan.lds_bytes = kmeans_wide_lds_bytes_k;
    } else {
        plan.point_tiles = (count + kmeans_tile_points_k - 1) / kmeans_tile_points_k;
        plan.centroid_tiles = (clusters + kmeans_tile_centroids_k - 1) / kmeans_tile_centroids_k;
        plan.lds_bytes = 0; // the 64 tile's LDS is static
    }
    return plan;
}

/// From this many centroids on, unforced f32 rows take the screened tile. Still the PLACEHOLDER of one centroid tile: the sweep in
/// profiles/r17_kmeans_f32/README.md (65 536 × 768 on an MI355X, `scripts/kmeans_bench.py --dtype f32`, USEARCH_AMD_KMEANS_TILE = 1
/// against = 64, three runs each) has the screened tile ahead at every centroid count it covers — 0.34 against 0.90 ms at 32, 0.36
/// against 3.5 ms at 128, 12.7 against 32.0 ms at 1 024 — so the crossover lies below 32 centroids, where nothing was measured, nor
/// was any other point count: the number stays where a tile is full until a sweep below 32 places it.
constexpr std::uint64_t kmeans_screen_least_centroids_k = kmeans_tile_centroids_k;

/// f32 rows: does the assignment run on the screened tile? `forced_tile`: USEARCH_AMD_KMEANS_TILE — 64 forces the screened tile at
/// any shape, 1 the wave-per-point kernel; 256 (there is no wide f32 tile) and anything else leave the choice here.
inline bool plan_kmeans_assign_f32(std::uint64_t count, std::uint64_t clusters, std::uint64_t forced_tile) {
    if (!count || !clusters || forced_tile == 1)
        return false;
    return forced_tile == 64 || clusters >= kmeans_screen_least_centroids_k;
}

} // namespace usearch_amd
