/**
 *  usearch_amd/csrc/kmeans.hip — k-means clustering with every buffer resident in HBM for the whole run.
 *
 *  The reference's `kmeans_clustering_gt` (/root/reference/include/usearch/index_plugins.hpp:2199-2500; Python surface
 *  python/usearch/index.py:1618-1712 through python/lib.cpp:565-640) is mirrored in its OBSERVABLE behaviour, quirks included:
 *    · 2255-2262  the three refusals and their messages;
 *    · 2317-2322  every point is cast to `quantization_kind` with the `cast_gt` family (bf16 truncates, i8 normalises by the
 *                 vector's magnitude and scales to ±127) — here by a kernel whose bits equal `cast_vector` of casts.hpp;
 *    · 2325-2350  seeds are `std::mt19937_64(seed)() % N`; the "uniqueness" loop compares `point_to_centroid_index[j]` (an
 *                 ASSIGNMENT, for j < i) with the drawn POINT index, so it does not keep seeds distinct — kept as it is;
 *    · 2366-2375  ascending scan with strict `<` from FLT_MAX: the lowest centroid index wins among equals, a NaN never wins,
 *                 a point whose distances are all NaN ends at index 0 with FLT_MAX;
 *    · 2355, 2391 `last_aggregate_distance` is DBL_MAX and never assigned again, so `last_iteration_inertia` is
 *                 |Σ − DBL_MAX| / DBL_MAX ≈ 1 in every iteration and the inertia exit cannot fire for thresholds below 1 — kept;
 *    · 2401-2409  exits in the order inertia, shifts, seconds — all BEFORE the update, so a run that exits early returns the
 *                 centroids its last assignment was measured against;
 *    · 2415-2477  centroid = f64 sum of its members (each decompressed from the quantised kind; i8 is x / 127.f), divided by
 *                 the member count for l2sq (an empty cluster stays the zero sum), by its f64 norm for cos (a zero norm stays),
 *                 untouched for other metrics, then cast f64 → quantised kind;
 *    · 2491-2496  centroids leave in the CALLER's scalar kind.
 *  There is no "fixed" mode.
 *
 *  Kernels:
 *    cast         rows of the caller's kind → quantised rows, zero padded to 16 bytes (`cast_vector`'s bits; the i8 magnitude is an
 *                 f64 sum in ascending dimension order, one lane per row);
 *    assignment   f16 / bf16 / i8: a tile of 64 points × 128 centroids per step on `v_mfma_f32_32x32x16_{f16,bf16}` /
 *                 `v_mfma_i32_32x32x32_i8`. The staged tile's stream and product, the fragment layout, Σx² and the closing arithmetic
 *                 are device_math.hpp's — the very code the 64-query tile of exact search (exact_tiled.hip) runs, so the two close
 *                 a pair to the same bits (tests/test_gpu_kmeans.py) and i8 distances are bit-identical to the wave kernel's. The
 *                 epilogue keeps ONE (distance, index) per point under (distance ↑, centroid index ↑). The centroids (k · row
 *                 bytes, a few MB) stay in L2; the points are read from HBM once per iteration.
 *                 From 65 536 points and 1 024 centroids on (`plan_kmeans_assign`, kmeans_plan.hpp; USEARCH_AMD_KMEANS_TILE = 64 / 256
 *                 forces either) the same pairs run on a tile of 256 points × 256 centroids per workgroup of 8 waves
 *                 (`assign_wide_kernel`): both operands go global → LDS by LDS-DMA into the two swizzled buffers of wide_stage.hpp,
 *                 shared with exact search's wide tile; a wave multiplies its 32 points with all 256 centroids of every tile and
 *                 keeps one running (distance, index) per accumulator register — the sums never visit LDS — and the lanes that
 *                 share a point fold their pairs once at the end. Same `multiply` calls in the same chunk order: the same float
 *                 bits as the 64 tile (tests/test_gpu_kmeans_wide.py). 1M × 768 bf16, k = 1 024: 2.73 ms against 3.55 ms.
 *                 f32: the bits of a plain wave per point (`assign_f32_kernel`: f32 FMAs over 64 lanes, shuffle reduction, within the
 *                 f32 tolerance) — below 128 centroids by that kernel alone, from there on (`plan_kmeans_assign_f32`;
 *                 USEARCH_AMD_KMEANS_TILE = 64 / 1 forces either) by `assign_screened_kernel`: the 64 tile over
 *                 `v_mfma_f32_32x32x2_f32` only SCREENS — a score and a derived error per pair, up to four contenders per point in
 *                 registers — and the contenders are re-measured by the wave kernel's own device function (`wave_distance_f32`);
 *                 points with more contenders, or with a Σx² the derivation does not cover, go to the wave kernel through a list.
 *                 1M × 768, k = 1 024: 17.2 ms against 517 ms (profiles/r17_kmeans_f32/).
 *                 The same kernel counts the points whose index changed (integer atomics) and writes the per-point distances;
 *    aggregate    one workgroup sums the f32 distances in f64 in a fixed tree: the same bits run after run;
 *    update       assignments → per-(chunk of points, centroid) counts → exclusive scans → a STABLE scatter of point ids, so every
 *                 centroid's members are listed in ascending point index; a wave owns (centroid, 64 dimensions), walks that list in
 *                 order and adds each member's decompressed value to one f64 accumulator per lane — the sums carry the bits of
 *                 the reference run on one thread; a finalising lane per centroid divides, takes the cos norm in ascending
 *                 dimension order and casts f64 → kind with `cast_vector`'s bits.
 *  No float atomics anywhere.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "casts.hpp"
#include "common.hpp"
#include "device_math.hpp"
#include "device_scratch.hpp"
#include "host_util.hpp"
#include "kmeans.hpp"
#include "kmeans_plan.hpp"
#include "screen_math.hpp"
#include "wide_stage.hpp"

namespace usearch_amd {

namespace {

constexpr int tile_points_k = kmeans_tile_points_k;       ///< points per workgroup of the 64 tile
constexpr int tile_centroids_k = kmeans_tile_centroids_k; ///< centroids per inner tile of the 64 tile
constexpr float float_max_k = 3.402823466e+38f;
constexpr std::uint32_t norms_blocks_k = 65536; ///< the grid of the Σx² launches at most

// ---------------------------------------------------------------------------------------------------------------------
//  Scalars (the four 16-bit conversions are casts.hpp's own, for host and device)
// ---------------------------------------------------------------------------------------------------------------------

/// `load_scalar` of casts.hpp, with aligned loads.
__device__ __forceinline__ double load_scalar_device(int kind, const std::uint8_t* p, std::uint32_t i) {
    switch (kind) {
    case scalar_f64_k: return reinterpret_cast<const double*>(p)[i];
    case scalar_f32_k: return reinterpret_cast<const float*>(p)[i];
    case scalar_f16_k: return f16_bits_to_f32(reinterpret_cast<const std::uint16_t*>(p)[i]);
    case scalar_bf16_k: return bf16_bits_to_f32(reinterpret_cast<const std::uint16_t*>(p)[i]);
    case scalar_i8_k: return (double)(std::int8_t)p[i];
    default: return 0;
    }
}

/// `store_scalar` of casts.hpp for the float kinds a run can be quantised to.
__device__ __forceinline__ void store_scalar_device(int kind, std::uint8_t* p, std::uint32_t i, float as_float) {
    switch (kind) {
    case scalar_f32_k: reinterpret_cast<float*>(p)[i] = as_float; break;
    case scalar_f16_k: reinterpret_cast<std::uint16_t*>(p)[i] = f32_to_f16_bits(as_float); break;
    case scalar_bf16_k: reinterpret_cast<std::uint16_t*>(p)[i] = f32_to_bf16_bits(as_float); break;
    default: break;
    }
}

/// A quantised scalar as the update sees it: `casts.to.f64` (exact for the float kinds, x / 127.f in f64 for i8).
template <int scalar_ak> __device__ __forceinline__ double decompress(const std::uint8_t* row, std::uint32_t i) {
    if constexpr (scalar_ak == scalar_i8_k)
        return (double)(std::int8_t)row[i] / 127.f;
    else if constexpr (scalar_ak == scalar_f16_k)
        return f16_bits_to_f32(reinterpret_cast<const std::uint16_t*>(row)[i]);
    else if constexpr (scalar_ak == scalar_bf16_k)
        return bf16_bits_to_f32(reinterpret_cast<const std::uint16_t*>(row)[i]);
    else
        return reinterpret_cast<const float*>(row)[i];
}

// ---------------------------------------------------------------------------------------------------------------------
//  Casts: caller's kind → quantised kind (`cast_vector` of casts.hpp, from != to, neither b1)
// ---------------------------------------------------------------------------------------------------------------------

/// Element-wise casts (every pair but → i8): one thread per scalar, grid-stride.
__global__ __launch_bounds__(256) void cast_elements_kernel(const std::uint8_t* input, std::uint64_t input_stride, int from,
                                                            std::uint8_t* output, std::uint64_t output_stride, int to,
                                                            std::uint64_t rows, std::uint32_t dimensions) {
    const std::uint64_t total = rows * dimensions;
    for (std::uint64_t cell = blockIdx.x * 256ull + threadIdx.x; cell < total; cell += (std::uint64_t)gridDim.x * 256) {
        const std::uint64_t row = cell / dimensions;
        const std::uint32_t i = (std::uint32_t)(cell % dimensions);
        const std::uint8_t* source = input + row * input_stride;
        std::uint8_t* target = output + row * output_stride;
        if (from == scalar_i8_k) {
            const std::int8_t x = (std::int8_t)source[i];
            float value;
            if (to == scalar_f32_k)
                value = (float)x / 127.f;
            else if (to == scalar_f16_k) // f16_t(int) then a float division, rounded back to f16
                value = f16_bits_to_f32(f32_to_f16_bits((float)x)) / 127.f;
            else
                value = bf16_bits_to_f32(f32_to_bf16_bits((float)x)) / 127.f;
            store_scalar_device(to, target, i, value);
        } else {
            store_scalar_device(to, target, i, (float)load_scalar_device(from, source, i));
        }
    }
}

/// → i8: L2-normalise in double, × 127, clamp to ±127, truncate toward zero; the magnitude is summed in ascending dimension
/// order, so one lane owns a row.
__global__ __launch_bounds__(64) void cast_to_i8_kernel(const std::uint8_t* input, std::uint64_t input_stride, int from,
                                                        std::uint8_t* output, std::uint64_t output_stride, std::uint64_t rows,
                                                        std::uint32_t dimensions) {
    const std::uint64_t row = blockIdx.x * 64ull + threadIdx.x;
    if (row >= rows)
        return;
    const std::uint8_t* source = input + row * input_stride;
    std::uint8_t* target = output + row * output_stride;
    double magnitude = 0.0;
    for (std::uint32_t i = 0; i != dimensions; ++i) {
        const double x = load_scalar_device(from, source, i);
        magnitude += x * x;
    }
    magnitude = __builtin_sqrt(magnitude);
    for (std::uint32_t i = 0; i != dimensions; ++i) {
        double v = load_scalar_device(from, source, i) * 127.0 / magnitude;
        v = v < -127.0 ? -127.0 : (v > 127.0 ? 127.0 : v);
        target[i] = (std::uint8_t)(std::int8_t)(int)v; // a NaN (zero magnitude) becomes 0, as on the host
    }
}

/// Row `ids[j]` of `source` → row j of `target` (the seeds), 16 bytes per thread.
__global__ __launch_bounds__(256) void gather_rows_kernel(const std::uint8_t* source, const std::uint32_t* ids, std::uint8_t* target,
                                                          std::uint32_t rows, std::uint32_t stride) {
    const std::uint32_t pieces = stride / 16;
    const std::uint64_t total = (std::uint64_t)rows * pieces;
    for (std::uint64_t cell = blockIdx.x * 256ull + threadIdx.x; cell < total; cell += (std::uint64_t)gridDim.x * 256) {
        const std::uint64_t j = cell / pieces, piece = cell % pieces;
        reinterpret_cast<uint4*>(target + j * stride)[piece] = reinterpret_cast<const uint4*>(source + (std::uint64_t)ids[j] * stride)[piece];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
//  Assignment
// ---------------------------------------------------------------------------------------------------------------------

/// What every assignment kernel ends in for its point: the new index and distance, and whether the index moved.
__device__ __forceinline__ void publish_assignment(std::uint32_t point, bool inside, std::uint32_t index, float distance,
                                                   std::uint32_t* assignments, float* distances, std::uint32_t* shifted,
                                                   std::uint32_t lane) {
    bool moved = false;
    if (inside) {
        moved = assignments[point] != index;
        assignments[point] = index;
        distances[point] = distance;
    }
    const std::uint32_t movers = (std::uint32_t)__popcll(__ballot(moved));
    if (lane == 0 && movers)
        atomicAdd(shifted, movers);
}

/// Rows [first, end) of one of k-means' own matrices as the staged tile reads them: `stride` bytes apart, 16-byte aligned and zero
/// padded up to `stride`.
__device__ __forceinline__ staged_rows_gt<std::uint32_t, std::uint32_t> kmeans_rows(const std::uint8_t* rows, std::uint32_t first, std::uint32_t end, std::uint32_t stride) {
    return {rows, stride, first, end, stride, true};
}

/**
 *  grid = point tiles, 256 threads = 4 waves. Wave w multiplies all 64 points of the tile with centroids [32w, 32w + 32) of every
 *  centroid tile: two 32 × 32 accumulators.
 */
template <int metric_ak, int scalar_ak>
__global__ __launch_bounds__(256) void assign_tiled_kernel(const std::uint8_t* points, std::uint32_t count, const std::uint8_t* centroids,
                                                           std::uint32_t clusters, std::uint32_t stride,
                                                           const std::uint32_t* point_norms, const std::uint32_t* centroid_norms,
                                                           std::uint32_t* assignments, float* distances, std::uint32_t* shifted) {
    using accumulator_t = typename accumulator_gt<scalar_ak>::type;
    __shared__ __attribute__((aligned(16))) std::uint8_t lds[staged_tile_bytes(tile_points_k, tile_centroids_k)];
    __shared__ float part_d[4][tile_points_k];         // the best of every quarter of a centroid tile, per point
    __shared__ std::uint32_t part_i[4][tile_points_k];
    __shared__ std::uint32_t norms_p[tile_points_k];
    __shared__ std::uint32_t norms_c[tile_centroids_k];
    float* tile_d = reinterpret_cast<float*>(lds);               // [64][129], aliases the staging area after the products

    const std::uint32_t thread = threadIdx.x, wave = thread / 64, lane = thread % 64;
    const std::uint32_t first_point = blockIdx.x * tile_points_k;
    const std::uint32_t chunks = (stride + chunk_bytes_k - 1) / chunk_bytes_k;

    if (thread < tile_points_k)
        norms_p[thread] = first_point + thread < count ? point_norms[first_point + thread] : 0u;
    // thread i < 64 carries point i's best so far: the scan of index_plugins.hpp:2366-2375
    float best_d = float_max_k;
    std::uint32_t best_i = 0;
    __syncthreads();

    // ---- the staged-tile stream of device_math.hpp: the next step's rows are in flight behind this step's products
    staged_stream_gt stream(kmeans_rows(points, first_point, count, stride), kmeans_rows(centroids, 0, clusters, stride), lds, thread);
    stream.fetch(0, 0);

    for (std::uint32_t tile = 0; tile < clusters; tile += tile_centroids_k) {
        accumulator_t acc[2];
        multiply_staged_tile<scalar_ak>(stream, tile, chunks, acc, [&] {
            if (thread < tile_centroids_k)
                norms_c[thread] = tile + thread < clusters ? centroid_norms[tile + thread] : 0u;
        });

        // ---- distances of the tile into LDS (the staging area is free now): D[point][centroid of the tile]
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const std::uint32_t i = t * 32 + accumulator_row(r, lane);
                const std::uint32_t j = wave * 32 + accumulator_column(lane);
                // (l2sq over floats: a NaN stays a NaN — it must never win the scan below; device_math.hpp)
                const float distance = closing_distance<metric_ak, scalar_ak, l2sq_nan_stays_k>(acc[t][r], norms_p[i], norms_c[j]);
                tile_d[i * (tile_centroids_k + 1) + j] = tile + j < clusters ? distance : __builtin_inff();
            }
        }
        __syncthreads();

        // ---- thread (point i = thread % 64, quarter q = thread / 64) scans centroids [32q, 32q + 32) of the tile in ascending order
        {
            const std::uint32_t i = thread % tile_points_k, quarter = thread / tile_points_k;
            float d = __builtin_inff();
            std::uint32_t at = 0;
            for (std::uint32_t s = 0; s < tile_centroids_k / 4; ++s) {
                const float candidate = tile_d[i * (tile_centroids_k + 1) + quarter * (tile_centroids_k / 4) + s];
                if (candidate < d)
                    d = candidate, at = quarter * (tile_centroids_k / 4) + s;
            }
            part_d[quarter][i] = d, part_i[quarter][i] = tile + at;
        }
        __syncthreads(); // the tile's distances are consumed: the area becomes staging again
        if (thread < tile_points_k) {
#pragma unroll
            for (int quarter = 0; quarter < 4; ++quarter)
                if (part_d[quarter][thread] < best_d)
                    best_d = part_d[quarter][thread], best_i = part_i[quarter][thread];
        }
        // (the quarters are written again two barriers from here at the earliest: every tile has at least one chunk)
    }
    if (thread < tile_points_k) // wave 0
        publish_assignment(first_point + thread, first_point + thread < count, best_i, best_d, assignments, distances, shifted, lane);
}

/**
 *  The wide tile. grid = tiles of 256 points, 512 threads = 8 waves, one workgroup per compute unit (two staging buffers of 64 KB).
 *  Every centroid tile of 256 rows streams past the workgroup's points; wave w multiplies points [32w, 32w + 32) with all 256
 *  centroids of the tile: eight 32 × 32 accumulators, `multiply` in the chunk order of the 64 tile — the same float bits. A
 *  workgroup sees every centroid: no partitions, nothing to merge between workgroups.
 *
 *  Staging is wide_stage.hpp's: both operands go global → LDS by LDS-DMA into two XOR-swizzled buffers of [512][128] bytes, chunk
 *  c + 1 is requested before chunk c is multiplied, a wave waits for ITS fills and meets the others at a bare barrier. Both
 *  matrices are k-means' own and hold whole tiles of whole chunks, zeros beyond the data (`kmeans_wide_stride`, `kmeans_wide_rows`):
 *  every fill reads inside its allocation, no clamp, no branch. Fragment reads are inline assembly that waits for its own reads —
 *  a read the compiler can see would wait for every fill in flight first (for all it knows the fill writes the very cell), and the
 *  next chunk would no longer land behind this one's products; the wave's partner on the SIMD multiplies while it waits.
 *
 *  The epilogue never leaves the registers. Accumulator register r of a lane is point 32w + accumulator_row(r, lane), its column
 *  the centroid residue lane & 31: a lane keeps one running (distance, index) per register and meets "its" centroids in ascending
 *  index — blocks ascend inside a tile, tiles ascend — so the strict `<` from FLT_MAX is the reference's scan (index_plugins.hpp:
 *  2366-2375) restricted to the lane. After the last tile the 32 lanes that share a point fold their pairs once under
 *  (distance ↑, index ↑); a NaN never entered a pair, and a point nobody took stays (FLT_MAX, 0). Rows ≥ `count` are not published,
 *  columns ≥ `clusters` never compared: padding cannot win.
 */
template <int metric_ak, int scalar_ak>
__global__ __launch_bounds__(wide_threads_k) void assign_wide_kernel(const std::uint8_t* points, std::uint32_t count, const std::uint8_t* centroids,
                                                                     std::uint32_t clusters, std::uint32_t stride,
                                                                     const std::uint32_t* point_norms, const std::uint32_t* centroid_norms,
                                                                     std::uint32_t* assignments, float* distances, std::uint32_t* shifted) {
    using accumulator_t = typename accumulator_gt<scalar_ak>::type;
    using u32x4_t = std::uint32_t __attribute__((ext_vector_type(4))); // a native 128-bit register operand for the assembler
    extern __shared__ __attribute__((aligned(1024))) std::uint8_t wide_lds[]; // [2][512][128]

    // (the wave's number as a scalar: the LDS targets of the fills travel in M0)
    const std::uint32_t thread = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(thread / 64), lane = thread % 64;
    const std::uint32_t first_point = blockIdx.x * wide_tile_k;
    const std::uint32_t chunks = stride / chunk_bytes_k; // whole chunks: kmeans_wide_stride
    const std::uint32_t tiles = (clusters + wide_tile_k - 1) / wide_tile_k;
    const std::uint32_t column = accumulator_column(lane);

    // ---- the points' Σa² behind the staging buffers (written here, before any fill is in flight; read by `ds_read` in assembly)
    std::uint32_t* norms_p = reinterpret_cast<std::uint32_t*>(wide_lds + wide_buffers_k * wide_stage_bytes_k); // [256]
    if (thread < wide_tile_k)
        norms_p[thread] = first_point + thread < count ? point_norms[first_point + thread] : 0u;
    __syncthreads();

    // ---- per lane: the best so far of the 16 points its accumulator registers belong to
    std::uint32_t best_i[16];
    float best_d[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)
        best_d[r] = float_max_k, best_i[r] = 0;

    // ---- fills: wave w brings rows 64·pass + 8w … + 8 of either operand, four passes each; lane i the piece that belongs in slot i
    const std::uint32_t fill_row = wave * 8 + lane / 8;
    const std::uint32_t lane_offset = fill_row * stride + wide_swizzle(fill_row, lane & 7u) * 16;
    const std::uint32_t tile_bytes = wide_tile_k * stride, pass_bytes = 64u * stride; // < 2^31: plan_kmeans_assign
    const __amdgpu_buffer_rsrc_t point_resource = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<std::uint8_t*>(points + (std::uint64_t)first_point * stride), 0, (int)tile_bytes, wide_resource_flags_k);
    auto fill = [&](std::uint32_t buffer, std::uint32_t tile, std::uint32_t chunk) {
        std::uint8_t* stage = wide_lds + buffer * wide_stage_bytes_k;
        const __amdgpu_buffer_rsrc_t centroid_resource = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<std::uint8_t*>(centroids + (std::uint64_t)tile * tile_bytes), 0, (int)tile_bytes, wide_resource_flags_k);
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) // the centroids first: the points of a workgroup come back from L2 after the first tile
            wide_fill(centroid_resource, stage + (wide_tile_k + pass * 64 + wave * 8) * chunk_bytes_k, lane_offset,
                      __builtin_amdgcn_readfirstlane(pass * pass_bytes + chunk * chunk_bytes_k));
#pragma unroll
        for (int pass = 0; pass < 4; ++pass)
            wide_fill(point_resource, stage + (pass * 64 + wave * 8) * chunk_bytes_k, lane_offset,
                      __builtin_amdgcn_readfirstlane(pass * pass_bytes + chunk * chunk_bytes_k));
    };

    // ---- fragment reads. Lane L reads row (base + (L & 31)), piece 2·step + (L >> 5), through the swizzle of that row; row bases
    //      are multiples of 32, so the swizzled piece only depends on the lane and the step. A statement requests a point fragment
    //      and four centroid fragments (or the other four) and waits for them: what leaves it has landed.
    const std::uint32_t lane_swizzle = ((lane & 31u) >> 1) & 7u, lane_half = lane >> 5;
    const std::uint32_t lds_base = (std::uint32_t)(std::uintptr_t)(lds_bytes_t)wide_lds;
    const std::uint32_t point_fragments = lds_base + (wave * 32 + (lane & 31)) * chunk_bytes_k;
    const std::uint32_t centroid_fragments = lds_base + (wide_tile_k + (lane & 31)) * chunk_bytes_k;
    accumulator_t acc[wide_blocks_k];
    static_assert(wide_blocks_k == 8 && chunk_bytes_k / 32 == 4, "multiply_chunk is written out for four steps of eight centroid blocks");
    auto multiply_chunk = [&](std::uint32_t buffer) {
#pragma unroll
        for (std::uint32_t step = 0; step < 4; ++step) {
            const std::uint32_t piece = buffer * wide_stage_bytes_k + ((2u * step + lane_half) ^ lane_swizzle) * 16u;
            u32x4_t a, b0, b1, b2, b3;
            asm volatile("ds_read_b128 %0, %5\n\t"
                         "ds_read_b128 %1, %6\n\t"
                         "ds_read_b128 %2, %6 offset:4096\n\t"
                         "ds_read_b128 %3, %6 offset:8192\n\t"
                         "ds_read_b128 %4, %6 offset:12288\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(a), "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3)
                         : "v"(point_fragments + piece), "v"(centroid_fragments + piece)
                         : "memory");
            acc[0] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b0), acc[0]);
            acc[1] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b1), acc[1]);
            acc[2] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b2), acc[2]);
            acc[3] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b3), acc[3]);
            asm volatile("ds_read_b128 %0, %4 offset:16384\n\t"
                         "ds_read_b128 %1, %4 offset:20480\n\t"
                         "ds_read_b128 %2, %4 offset:24576\n\t"
                         "ds_read_b128 %3, %4 offset:28672\n\t"
                         "s_waitcnt lgkmcnt(0)"
                         : "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3)
                         : "v"(centroid_fragments + piece)
                         : "memory");
            acc[4] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b0), acc[4]);
            acc[5] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b1), acc[5]);
            acc[6] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b2), acc[6]);
            acc[7] = multiply<scalar_ak>(__builtin_bit_cast(uint4, a), __builtin_bit_cast(uint4, b3), acc[7]);
        }
    };

    // ---- the pipeline: chunk c is multiplied out of buffer c & 1 while the DMA fills the other buffer with chunk c + 1. What a
    //      buffer holds is read one iteration after the wait + barrier that completed it, and refilled one barrier after its last read.
    fill(0, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    std::uint32_t c = 0;
    for (std::uint32_t tile = 0; tile < tiles; ++tile) {
#pragma unroll
        for (int u = 0; u < wide_blocks_k; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[u][r] = 0;
        for (std::uint32_t chunk = 0; chunk < chunks; ++chunk, ++c) {
            const bool last_of_tile = chunk + 1 == chunks;
            // the tile's Σb² ahead of the fills: they are there when the products are, whatever is still in flight behind them
            std::uint32_t b2[wide_blocks_k] = {};
            if (last_of_tile) {
#pragma unroll
                for (int u = 0; u < wide_blocks_k; ++u) {
                    const std::uint32_t j = tile * wide_tile_k + u * 32 + column;
                    b2[u] = j < clusters ? centroid_norms[j] : 0u;
                }
            }
            if (!last_of_tile)
                fill((c + 1) & 1u, tile, chunk + 1);
            else if (tile + 1 < tiles)
                fill((c + 1) & 1u, tile + 1, 0);
            multiply_chunk(c & 1u);
            if (last_of_tile) {
                // the points' Σa² by a hand-waited read, like the fragments (registers 4q … 4q + 3 ↔ points 8q + 4·(lane >> 5) + 0 … 3)
                u32x4_t n0, n1, n2, n3;
                asm volatile("ds_read_b128 %0, %4\n\t"
                             "ds_read_b128 %1, %4 offset:32\n\t"
                             "ds_read_b128 %2, %4 offset:64\n\t"
                             "ds_read_b128 %3, %4 offset:96\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&v"(n0), "=&v"(n1), "=&v"(n2), "=&v"(n3)
                             : "v"(lds_base + wide_buffers_k * wide_stage_bytes_k + (wave * 32 + 4 * lane_half) * 4)
                             : "memory");
                const std::uint32_t a2[16] = {n0[0], n0[1], n0[2], n0[3], n1[0], n1[1], n1[2], n1[3],
                                              n2[0], n2[1], n2[2], n2[3], n3[0], n3[1], n3[2], n3[3]};
#pragma unroll
                for (int u = 0; u < wide_blocks_k; ++u) {
                    const std::uint32_t j = tile * wide_tile_k + u * 32 + column;
                    const bool live = j < clusters;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        // (l2sq over floats: a NaN stays a NaN and fails the `<`; device_math.hpp)
                        float distance;
                        if constexpr (metric_ak == metric_cos_k && scalar_ak != scalar_i8_k) {
                            // closing_distance's answers for a zero norm taken as selects around its general expression, which is
                            // told that it sees none: its early returns are divergent branches otherwise, 128 of them in a row
                            const float a2f = __builtin_bit_cast(float, a2[r]), b2f = __builtin_bit_cast(float, b2[u]);
                            const bool zero_a = a2f == 0.f, zero_b = b2f == 0.f;
                            const float a2_safe = zero_a ? 1.f : a2f, b2_safe = zero_b ? 1.f : b2f;
                            __builtin_assume(a2_safe != 0.f && b2_safe != 0.f);
                            const float general = closing_distance<metric_ak, scalar_ak, l2sq_nan_stays_k>(
                                acc[u][r], __builtin_bit_cast(std::uint32_t, a2_safe), __builtin_bit_cast(std::uint32_t, b2_safe));
                            distance = zero_a && zero_b ? 0.f : (zero_a || zero_b ? 1.f : general);
                        } else if constexpr (metric_ak == metric_cos_k) { // i8: the same for its `ab == 0 → 0`
                            const int ab = acc[u][r], ab_safe = ab != 0 ? ab : 1;
                            __builtin_assume(ab_safe != 0);
                            const float general = closing_distance<metric_ak, scalar_ak, l2sq_nan_stays_k>(ab_safe, a2[r], b2[u]);
                            distance = ab != 0 ? general : 0.f;
                        } else
                            distance = closing_distance<metric_ak, scalar_ak, l2sq_nan_stays_k>(acc[u][r], a2[r], b2[u]);
                        if (live && distance < best_d[r])
                            best_d[r] = distance, best_i[r] = j;
                        if constexpr (metric_ak == metric_cos_k) // one division at a time: sixteen interleaved do not fit the registers
                            __builtin_amdgcn_sched_barrier(0);
                    }
                    __builtin_amdgcn_sched_barrier(0); // block by block
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's share of the next chunk is in LDS
            __builtin_amdgcn_s_barrier();
        }
    }

    // ---- the 32 lanes of a half hold a point's 32 residues: fold them, then lane r of the half (r < 16) publishes register r's point
    float mine_d = float_max_k;
    std::uint32_t mine_i = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float d = best_d[r];
        std::uint32_t i = best_i[r];
#pragma unroll
        for (int offset = 1; offset <= 16; offset <<= 1) {
            const float other_d = __shfl_xor(d, offset, 64);
            const std::uint32_t other_i = (std::uint32_t)__shfl_xor((int)i, offset, 64);
            if (other_d < d || (other_d == d && other_i < i))
                d = other_d, i = other_i;
        }
        if ((lane & 31u) == (std::uint32_t)r)
            mine_d = d, mine_i = i;
    }
    const std::uint32_t point = first_point + wave * 32 + accumulator_row(lane & 15u, lane);
    publish_assignment(point, (lane & 31u) < 16u && point < count, mine_i, mine_d, assignments, distances, shifted, lane);
}

/// The f32 distance of one (point, centroid) pair as a whole wave measures it — the reference's expressions (metric_l2sq_gt /
/// metric_cos_gt / metric_ip_gt over f32) with the dimensions dealt over the lanes, a lane's fmaf chain in ascending dimension, six
/// shuffle-adds. `wave_square_f32` is the point's Σa² for cos, summed the same way. Every lane returns the result. Both f32
/// assignment kernels call these two and nothing else for a distance that is published: one set of bits.
__device__ __forceinline__ float wave_square_f32(const float* a, std::uint32_t dimensions, std::uint32_t lane) {
    float a2 = 0.f;
    for (std::uint32_t i = lane; i < dimensions; i += 64)
        a2 = __builtin_fmaf(a[i], a[i], a2);
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1)
        a2 += __shfl_xor(a2, offset, 64);
    return a2;
}
template <int metric_ak>
__device__ __forceinline__ float wave_distance_f32(const float* a, float a2, const float* b, std::uint32_t dimensions, std::uint32_t lane) {
    float x = 0.f, b2 = 0.f;
    for (std::uint32_t i = lane; i < dimensions; i += 64) {
        const float ai = a[i], bi = b[i];
        if constexpr (metric_ak == metric_l2sq_k) {
            const float difference = ai - bi;
            x = __builtin_fmaf(difference, difference, x);
        } else {
            x = __builtin_fmaf(ai, bi, x);
            if constexpr (metric_ak == metric_cos_k)
                b2 = __builtin_fmaf(bi, bi, b2);
        }
    }
#pragma unroll
    for (int offset = 32; offset >= 1; offset >>= 1) {
        x += __shfl_xor(x, offset, 64);
        b2 += __shfl_xor(b2, offset, 64);
    }
    if constexpr (metric_ak == metric_cos_k) {
        if (a2 == 0.f && b2 == 0.f)
            return 0.f;
        if (a2 == 0.f || b2 == 0.f)
            return 1.f;
        return 1.f - x / (__builtin_sqrtf(a2) * __builtin_sqrtf(b2));
    } else if constexpr (metric_ak == metric_ip_k) {
        return 1.f - x;
    } else {
        return x;
    }
}

/// f32 rows: a wave per point, every centroid in ascending order. `list` null: wave s takes point s, and the grid holds a wave per
/// point. `list` set (the points the screened tile handed over): wave s takes point list[s] for s < *list_count, grid-stride.
template <int metric_ak>
__global__ __launch_bounds__(256) void assign_f32_kernel(const std::uint8_t* points, std::uint32_t count, const std::uint8_t* centroids,
                                                         std::uint32_t clusters, std::uint32_t stride, std::uint32_t dimensions,
                                                         std::uint32_t* assignments, float* distances, std::uint32_t* shifted,
                                                         const std::uint32_t* list, const std::uint32_t* list_count) {
    const std::uint32_t lane = threadIdx.x % 64;
    const std::uint32_t total = list ? *list_count : count;
    for (std::uint32_t slot = blockIdx.x * 4u + threadIdx.x / 64; slot < total; slot += gridDim.x * 4u) {
        const std::uint32_t point = list ? list[slot] : slot;
        const float* a = reinterpret_cast<const float*>(points + (std::uint64_t)point * stride);
        const float a2 = metric_ak == metric_cos_k ? wave_square_f32(a, dimensions, lane) : 0.f;
        float best_d = float_max_k;
        std::uint32_t best_i = 0;
        for (std::uint32_t c = 0; c < clusters; ++c) {
            const float distance =
                wave_distance_f32<metric_ak>(a, a2, reinterpret_cast<const float*>(centroids + (std::uint64_t)c * stride), dimensions, lane);
            if (distance < best_d)
                best_d = distance, best_i = c;
        }
        // one lane per wave publishes and counts its mover
        if (lane == 0) {
            const bool moved = assignments[point] != best_i;
            assignments[point] = best_i;
            distances[point] = best_d;
            if (moved)
                atomicAdd(shifted, 1u);
        }
    }
}

/**
 *  f32 rows on the matrix units, with the wave kernel's bits. The 64 tile's geometry and staging (64 points per workgroup, centroid
 *  tiles of 128 streamed past them, `multiply_staged_chunk<scalar_f32_k>`); what differs is what a sum is used for. The matrix unit
 *  adds in another order than `wave_distance_f32`, so its sums only SCREEN: per (point, centroid) the score s and the error e of
 *  screen_math.hpp, with `wave_distance_f32` as the measuring kernel (`screen_g_wave`).
 *  A centroid can be the wave kernel's answer only if s − e ≤ min over all centroids of (s + e): whoever fails that is farther than
 *  the holder of the minimum in the wave kernel's own arithmetic. Thread (point i, quarter q) scans centroids [32q, 32q + 32) of every
 *  tile, as the 64 tile's epilogue does, and keeps in registers the running bound min (s + e) and up to four contenders (s − e, j)
 *  at or below it; a lower bound prunes the set when it is full. After the last tile the four quarters of a point fold their sets under the
 *  lowest bound, and wave w re-measures the contenders of points [16w, 16w + 16) with `wave_distance_f32` — the lowest
 *  (distance ↑, index ↑) from FLT_MAX with strict `<`, the scan of index_plugins.hpp:2366-2375 restricted to the only centroids that
 *  can win it.
 *
 *  Handed to `assign_f32_kernel` through `overflow_list` (an append by an integer atomic) instead: a point with more than four
 *  contenders (in a quarter at any time, or after the fold), and a point that met a Σx² outside [2⁻⁶⁰, 2⁶⁰] other than 0 — its own or
 *  any centroid's; a NaN or an infinity anywhere in a row makes its Σx² one — because the derivation of e assumes sums that neither
 *  overflow nor lose bits to underflow; under cos also a point with Σa² = 0 (fᵢ = A). `contenders` (tests only, or null): per point
 *  the number re-measured, 0 for a point handed over.
 */
constexpr int screen_slots_k = 4;

template <int metric_ak>
__global__ __launch_bounds__(256) void assign_screened_kernel(const std::uint8_t* points, std::uint32_t count, const std::uint8_t* centroids,
                                                              std::uint32_t clusters, std::uint32_t stride, std::uint32_t dimensions,
                                                              const std::uint32_t* point_norms, const std::uint32_t* centroid_norms,
                                                              std::uint32_t* assignments, float* distances, std::uint32_t* shifted,
                                                              std::uint32_t* overflow_list, std::uint32_t* overflow_count,
                                                              std::uint32_t* contenders) {
    constexpr int scalar_ak = scalar_f32_k;
    __shared__ __attribute__((aligned(16))) std::uint8_t lds[staged_tile_bytes(tile_points_k, tile_centroids_k)];
    __shared__ float squares_c[tile_centroids_k]; // Σb² of the tile's centroids, and their roots
    __shared__ float roots_c[tile_centroids_k];
    __shared__ std::uint32_t out_of_band;         // some centroid's Σb² was: nothing of this workgroup is decided here
    __shared__ std::uint32_t final_count[tile_points_k];
    __shared__ std::uint32_t final_index[tile_points_k][screen_slots_k];
    float* tile_s = reinterpret_cast<float*>(lds);             // [64][129], aliases the staging area after the products
    static_assert(sizeof(lds) >= 256 * (2 * screen_slots_k + 2) * 4, "the quarters' sets are folded through the staging area");

    const std::uint32_t thread = threadIdx.x, wave = thread / 64, lane = thread % 64;
    const std::uint32_t first_point = blockIdx.x * tile_points_k;
    const std::uint32_t chunks = (stride + chunk_bytes_k - 1) / chunk_bytes_k;
    const float g = screen_g_wave(dimensions);

    // ---- thread (point i = thread % 64, quarter = thread / 64): the point's part of e, its running bound and its contenders
    const std::uint32_t scan_point = first_point + thread % tile_points_k;
    const float a2 = scan_point < count ? __builtin_bit_cast(float, point_norms[scan_point]) : 0.f;
    const float root_a = __builtin_sqrtf(a2);
    bool handed_over = square_out_of_band(a2, false) || (metric_ak == metric_cos_k && a2 == 0.f);
    float bound = __builtin_inff();
    float low[screen_slots_k];
    std::uint32_t index[screen_slots_k];
    std::uint32_t held = 0;
#pragma unroll
    for (int s = 0; s < screen_slots_k; ++s)
        low[s] = 0.f, index[s] = 0;
    if (thread == 0)
        out_of_band = 0;
    __syncthreads();
    // drops what the bound has left behind, keeping the order
    auto prune = [&]() {
        std::uint32_t kept = 0;
#pragma unroll
        for (int s = 0; s < screen_slots_k; ++s) {
            const bool stays = (std::uint32_t)s < held && low[s] <= bound;
            const float l = low[s];
            const std::uint32_t j = index[s];
#pragma unroll
            for (int target = 0; target <= s; ++target)
                if (stays && kept == (std::uint32_t)target)
                    low[target] = l, index[target] = j;
            kept += stays ? 1u : 0u;
        }
        held = kept;
    };
    auto offer = [&](float s, float e, std::uint32_t j) {
        const float upper = s + e, lower = s - e;
        if (upper < bound)
            bound = upper;
        if (lower <= bound) {
            if (held == screen_slots_k)
                prune();
            if (held == screen_slots_k)
                handed_over = true;
            else {
#pragma unroll
                for (int slot = 0; slot < screen_slots_k; ++slot)
                    if (held == (std::uint32_t)slot)
                        low[slot] = lower, index[slot] = j;
                ++held;
            }
        }
    };

    // ---- staging: the 64 tile's (assign_tiled_kernel), next step's rows requested before this step's products
    staged_stream_gt stream(kmeans_rows(points, first_point, count, stride), kmeans_rows(centroids, 0, clusters, stride), lds, thread);
    stream.fetch(0, 0);

    for (std::uint32_t tile = 0; tile < clusters; tile += tile_centroids_k) {
        f32x16_t acc[2];
        multiply_staged_tile<scalar_ak>(stream, tile, chunks, acc, [&] {
            if (thread < tile_centroids_k) { // read after the chunks' barriers; written again after the scan's
                const float b2 = tile + thread < clusters ? __builtin_bit_cast(float, centroid_norms[tile + thread]) : 0.f;
                squares_c[thread] = b2, roots_c[thread] = __builtin_sqrtf(b2);
                if (square_out_of_band(b2, false))
                    out_of_band = 1;
            }
        });

        // ---- scores of the tile into LDS (the staging area is free now): S[point][centroid of the tile]
        store_screen_scores<metric_ak>(acc, squares_c, roots_c, wave, lane, tile_s);
        __syncthreads();

        // ---- thread (point i, quarter q) offers centroids [32q, 32q + 32) of the tile to its set, in ascending order
        {
            const std::uint32_t i = thread % tile_points_k, first = (thread / tile_points_k) * (tile_centroids_k / 4);
            const std::uint32_t live = tile + first < clusters ? min((std::uint32_t)(tile_centroids_k / 4), clusters - tile - first) : 0u;
            for (std::uint32_t s = 0; s < live; ++s)
                offer(tile_s[i * (tile_centroids_k + 1) + first + s], screen_error<metric_ak>(g, root_a, roots_c[first + s]), tile + first + s);
        }
        __syncthreads(); // the tile's scores are consumed: the area becomes staging again, the norms the next tile's
    }

    // ---- the four quarters of a point fold their sets through LDS: [256] bounds, counts (all ones: handed over), then the slots
    float* fold_bound = reinterpret_cast<float*>(lds);
    std::uint32_t* fold_held = reinterpret_cast<std::uint32_t*>(lds) + 256;
    float* fold_low = reinterpret_cast<float*>(lds) + 512;                          // [256][slots]
    std::uint32_t* fold_index = reinterpret_cast<std::uint32_t*>(lds) + 512 + 256 * screen_slots_k;
    fold_bound[thread] = bound;
    fold_held[thread] = handed_over ? 0xFFFFFFFFu : held;
#pragma unroll
    for (int s = 0; s < screen_slots_k; ++s)
        fold_low[thread * screen_slots_k + s] = low[s], fold_index[thread * screen_slots_k + s] = index[s];
    __syncthreads();
    if (thread < tile_points_k) {
        float lowest = __builtin_inff();
        bool over = out_of_band != 0;
#pragma unroll
        for (int quarter = 0; quarter < 4; ++quarter) {
            lowest = fminf(lowest, fold_bound[quarter * tile_points_k + thread]);
            over = over || fold_held[quarter * tile_points_k + thread] == 0xFFFFFFFFu;
        }
        std::uint32_t kept = 0;
        if (!over)
            for (int quarter = 0; quarter < 4; ++quarter) {
                const std::uint32_t from = quarter * tile_points_k + thread;
                for (std::uint32_t s = 0; s < fold_held[from]; ++s)
                    if (fold_low[from * screen_slots_k + s] <= lowest) {
                        if (kept < screen_slots_k)
                            final_index[thread][kept] = fold_index[from * screen_slots_k + s];
                        ++kept;
                    }
            }
        over = over || kept == 0 || kept > screen_slots_k;
        const bool inside = first_point + thread < count;
        final_count[thread] = inside && !over ? kept : 0u;
        if (inside && over)
            overflow_list[atomicAdd(overflow_count, 1u)] = first_point + thread;
        if (inside && contenders)
            contenders[first_point + thread] = over ? 0u : kept;
    }
    __syncthreads();

    // ---- closing: wave w re-measures the contenders of points [16w, 16w + 16), one after the other, in the wave kernel's arithmetic
    std::uint32_t movers = 0;
    for (std::uint32_t i = wave * (tile_points_k / 4); i < (wave + 1) * (tile_points_k / 4); ++i) {
        const std::uint32_t wanted = final_count[i]; // the same for the whole wave
        if (!wanted)
            continue;
        const std::uint32_t point = first_point + i;
        const float* a = reinterpret_cast<const float*>(points + (std::uint64_t)point * stride);
        const float wave_a2 = metric_ak == metric_cos_k ? wave_square_f32(a, dimensions, lane) : 0.f;
        float best_d = float_max_k;
        std::uint32_t best_i = 0;
        for (std::uint32_t s = 0; s < wanted; ++s) {
            const std::uint32_t c = final_index[i][s];
            const float distance =
                wave_distance_f32<metric_ak>(a, wave_a2, reinterpret_cast<const float*>(centroids + (std::uint64_t)c * stride), dimensions, lane);
            // the ascending scan's winner whatever the order the set is held in: the lowest index among equals, nothing at FLT_MAX
            if (distance < best_d || (distance == best_d && distance < float_max_k && c < best_i))
                best_d = distance, best_i = c;
        }
        if (lane == 0) {
            movers += assignments[point] != best_i ? 1u : 0u;
            assignments[point] = best_i;
            distances[point] = best_d;
        }
    }
    if (movers)
        atomicAdd(shifted, movers);
}

/// Σ of the f32 distances in f64, a fixed tree: thread t adds distances t, t + 1024, … in that order, then the 1 024 partial sums
/// are folded pairwise.
__global__ __launch_bounds__(1024) void aggregate_kernel(const float* distances, std::uint32_t count, double* out) {
    __shared__ double partial[1024];
    double sum = 0.0;
    for (std::uint32_t i = threadIdx.x; i < count; i += 1024)
        sum += (double)distances[i];
    partial[threadIdx.x] = sum;
    __syncthreads();
    for (std::uint32_t width = 512; width >= 1; width >>= 1) {
        if (threadIdx.x < width)
            partial[threadIdx.x] += partial[threadIdx.x + width];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        *out = partial[0];
}

// ---------------------------------------------------------------------------------------------------------------------
//  Update
// ---------------------------------------------------------------------------------------------------------------------

/**
 *  A wave owns a chunk of `steps` × 64 consecutive points and walks it in order. `scatter_ak` = false: cells[chunk][c] += members
 *  of c in the chunk. `scatter_ak` = true (cells now hold where the chunk's members of c start inside c's list): point ids go to
 *  their places, ascending inside every list. Lanes with the same centroid find each other in registers; one integer atomic per
 *  (step, centroid present) touches the cell — cells of a chunk belong to its wave alone, and a wave's atomics on one address
 *  execute in program order.
 */
template <bool scatter_ak>
__global__ __launch_bounds__(64) void members_kernel(const std::uint32_t* assignments, std::uint32_t count, std::uint32_t clusters,
                                                     std::uint32_t steps, std::uint32_t* cells, const std::uint32_t* offsets,
                                                     std::uint32_t* members) {
    const std::uint32_t lane = threadIdx.x;
    std::uint32_t* mine = cells + (std::uint64_t)blockIdx.x * clusters;
    for (std::uint32_t step = 0; step < steps; ++step) {
        const std::uint64_t wide = ((std::uint64_t)blockIdx.x * steps + step) * 64 + lane;
        const bool inside = wide < count;
        const std::uint32_t point = (std::uint32_t)wide;
        const std::uint32_t c = inside ? assignments[point] : 0xFFFFFFFFu;
        std::uint32_t rank = 0, size = 0, leader = lane;
        std::uint64_t pending = __ballot(inside);
        while (pending) {
            const std::uint32_t first = (std::uint32_t)__ffsll((long long)pending) - 1;
            const std::uint32_t wanted = (std::uint32_t)__shfl((int)c, (int)first, 64);
            const std::uint64_t group = __ballot(inside && c == wanted);
            if (inside && c == wanted) {
                rank = (std::uint32_t)__popcll(group & ((1ull << lane) - 1ull));
                size = (std::uint32_t)__popcll(group);
                leader = first;
            }
            pending &= ~group;
        }
        if constexpr (!scatter_ak) {
            if (inside && leader == lane && c < clusters)
                atomicAdd(mine + c, size);
        } else {
            std::uint32_t start = 0;
            if (inside && leader == lane && c < clusters)
                start = atomicAdd(mine + c, size);
            start = (std::uint32_t)__shfl((int)start, (int)leader, 64);
            if (inside && c < clusters)
                members[offsets[c] + start + rank] = point;
        }
    }
}

/// cells[chunk][c] → the exclusive scan over the chunks, per centroid; counts[c] = the total.
__global__ __launch_bounds__(256) void chunk_scan_kernel(std::uint32_t* cells, std::uint32_t chunks, std::uint32_t clusters,
                                                         std::uint32_t* counts) {
    const std::uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= clusters)
        return;
    std::uint32_t running = 0;
    for (std::uint32_t chunk = 0; chunk < chunks; ++chunk) {
        const std::uint32_t here = cells[(std::uint64_t)chunk * clusters + c];
        cells[(std::uint64_t)chunk * clusters + c] = running;
        running += here;
    }
    counts[c] = running;
}

/// offsets[0 … clusters] = exclusive scan of counts, one workgroup: a thread scans its own run of cells, thread 0 the 1 024 runs.
__global__ __launch_bounds__(1024) void offsets_kernel(const std::uint32_t* counts, std::uint32_t clusters, std::uint32_t* offsets) {
    __shared__ std::uint32_t runs[1024];
    const std::uint32_t per = (clusters + 1023) / 1024;
    const std::uint32_t begin = threadIdx.x * per < clusters ? threadIdx.x * per : clusters;
    const std::uint32_t end = begin + per < clusters ? begin + per : clusters;
    std::uint32_t sum = 0;
    for (std::uint32_t c = begin; c < end; ++c)
        sum += counts[c];
    runs[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        std::uint32_t running = 0;
        for (std::uint32_t t = 0; t < 1024; ++t) {
            const std::uint32_t here = runs[t];
            runs[t] = running;
            running += here;
        }
        offsets[clusters] = running;
    }
    __syncthreads();
    std::uint32_t running = runs[threadIdx.x];
    for (std::uint32_t c = begin; c < end; ++c) {
        offsets[c] = running;
        running += counts[c];
    }
}

/**
 *  grid = (centroids, slices of 64 dimensions), one wave each. The lane's accumulator takes the members' values one after the
 *  other in list order (ascending point index) — the only dependent chain; eight rows' loads are in flight ahead of it.
 *  sums[dimension][centroid] (transposed: the finalising lanes read it coalesced).
 */
template <int scalar_ak>
__global__ __launch_bounds__(64) void sums_kernel(const std::uint8_t* points, std::uint32_t stride, std::uint32_t dimensions,
                                                  std::uint32_t clusters, const std::uint32_t* offsets, const std::uint32_t* members,
                                                  double* sums) {
    const std::uint32_t c = blockIdx.x, dimension = blockIdx.y * 64u + threadIdx.x;
    if (dimension >= dimensions)
        return;
    const std::uint32_t begin = offsets[c], end = offsets[c + 1];
    double sum = 0.0;
    std::uint32_t m = begin;
    for (; m + 8 <= end; m += 8) {
        double values[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            values[u] = decompress<scalar_ak>(points + (std::uint64_t)members[m + u] * stride, dimension);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            sum += values[u];
    }
    for (; m < end; ++m)
        sum += decompress<scalar_ak>(points + (std::uint64_t)members[m] * stride, dimension);
    sums[(std::uint64_t)dimension * clusters + c] = sum;
}

/// One lane per centroid: index_plugins.hpp:2451-2476 — the metric's normalisation in f64 (in place) and the cast f64 → kind
/// (`cast_vector`'s generic path; → i8 its magnitude path), every loop in ascending dimension order.
template <int metric_ak, int scalar_ak>
__global__ __launch_bounds__(64) void finalize_kernel(double* sums, std::uint32_t dimensions, std::uint32_t clusters,
                                                      const std::uint32_t* offsets, std::uint8_t* centroids, std::uint32_t stride) {
    const std::uint32_t c = blockIdx.x * 64u + threadIdx.x;
    if (c >= clusters)
        return;
    double* column = sums + c;
    if constexpr (metric_ak == metric_l2sq_k) {
        const std::uint32_t size = offsets[c + 1] - offsets[c];
        if (size > 0)
            for (std::uint32_t i = 0; i != dimensions; ++i)
                column[(std::uint64_t)i * clusters] /= (double)size;
    } else if constexpr (metric_ak == metric_cos_k) {
        double norm = 0.0;
        for (std::uint32_t i = 0; i != dimensions; ++i) {
            const double x = column[(std::uint64_t)i * clusters];
            norm += x * x;
        }
        norm = __builtin_sqrt(norm);
        if (norm > 0.0)
            for (std::uint32_t i = 0; i != dimensions; ++i)
                column[(std::uint64_t)i * clusters] /= norm;
    }
    std::uint8_t* row = centroids + (std::uint64_t)c * stride;
    if constexpr (scalar_ak == scalar_i8_k) {
        double magnitude = 0.0;
        for (std::uint32_t i = 0; i != dimensions; ++i) {
            const double x = column[(std::uint64_t)i * clusters];
            magnitude += x * x;
        }
        magnitude = __builtin_sqrt(magnitude);
        for (std::uint32_t i = 0; i != dimensions; ++i) {
            double v = column[(std::uint64_t)i * clusters] * 127.0 / magnitude;
            v = v < -127.0 ? -127.0 : (v > 127.0 ? 127.0 : v);
            row[i] = (std::uint8_t)(std::int8_t)(int)v; // a NaN (an empty cluster's zero magnitude) becomes 0, as on the host
        }
    } else {
        for (std::uint32_t i = 0; i != dimensions; ++i)
            store_scalar_device(scalar_ak, row, i, (float)column[(std::uint64_t)i * clusters]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
//  Host side
// ---------------------------------------------------------------------------------------------------------------------

inline std::uint32_t grid_for(std::uint64_t cells, std::uint32_t per_block) {
    const std::uint64_t blocks = (cells + per_block - 1) / per_block;
    return (std::uint32_t)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

inline bool quantizable(scalar_kind_t kind) {
    return kind == scalar_bf16_k || kind == scalar_f16_k || kind == scalar_i8_k || kind == scalar_f32_k;
}
inline bool castable(scalar_kind_t kind) { return quantizable(kind) || kind == scalar_f64_k; }

const char* refuse_kinds(scalar_kind_t kind, scalar_kind_t quantization) {
    if (quantization == scalar_f64_k)
        return "k-means on the device does not quantise to f64: use bf16, f16, i8 or f32";
    if (quantization == scalar_b1x8_k)
        return "k-means on the device does not quantise to b1: use bf16, f16, i8 or f32";
    if (!quantizable(quantization))
        return "Unsupported metric or scalar kind";
    if (!castable(kind))
        return "k-means on the device takes points of f64, f32, f16, bf16 or i8";
    return nullptr;
}

/// Host rows of `kind` → device rows of `quantization`, `quantized_stride` bytes apart and zero padded, slab by slab; the matrix
/// holds `allocated_rows` ≥ `count` rows, zeros after the data (whole tiles for the wide assignment).
const char* quantize_rows(const std::uint8_t* rows, std::size_t count, std::size_t stride, scalar_kind_t kind,
                          std::size_t dimensions, scalar_kind_t quantization, std::uint8_t* quantized, std::size_t quantized_stride,
                          std::size_t allocated_rows) {
    UA_HIP(hipMemset(quantized, 0, allocated_rows * quantized_stride));
    const std::size_t row_bytes = bytes_per_vector(kind, dimensions);
    if (kind == quantization) {
        UA_HIP(hipMemcpy2D(quantized, quantized_stride, rows, stride, row_bytes, count, hipMemcpyHostToDevice));
        return nullptr;
    }
    const std::size_t slab_rows = std::max<std::size_t>(1, std::min<std::size_t>(count, (std::size_t(1) << 30) / row_bytes));
    device_scratch_t scratch(current_device_k); // the device of `quantized`, which the caller has selected
    std::uint8_t* slab = nullptr;
    UA_HIP(scratch.allocate(&slab, slab_rows * row_bytes));
    for (std::size_t first = 0; first < count; first += slab_rows) {
        const std::size_t here = std::min(slab_rows, count - first);
        UA_HIP(hipMemcpy2D(slab, row_bytes, rows + first * stride, stride, row_bytes, here, hipMemcpyHostToDevice));
        std::uint8_t* target = quantized + first * quantized_stride;
        if (quantization == scalar_i8_k)
            cast_to_i8_kernel<<<(std::uint32_t)((here + 63) / 64), 64>>>(slab, row_bytes, (int)kind, target, quantized_stride, here,
                                                                         (std::uint32_t)dimensions);
        else
            cast_elements_kernel<<<grid_for(here * dimensions, 256), 256>>>(slab, row_bytes, (int)kind, target, quantized_stride,
                                                                            (int)quantization, here, (std::uint32_t)dimensions);
        UA_HIP(hipGetLastError());
        UA_HIP(hipDeviceSynchronize()); // the slab is written again
    }
    return nullptr;
}

const char* launch_norms(scalar_kind_t quantization, const std::uint8_t* rows, std::size_t count, std::size_t stride, std::uint32_t bytes,
                         std::uint32_t* norms) {
    if (quantization == scalar_f16_k)
        UA_HIP(launch_row_norms<scalar_f16_k>(rows, count, stride, bytes, norms, norms_blocks_k, nullptr));
    else if (quantization == scalar_bf16_k)
        UA_HIP(launch_row_norms<scalar_bf16_k>(rows, count, stride, bytes, norms, norms_blocks_k, nullptr));
    else if (quantization == scalar_i8_k)
        UA_HIP(launch_row_norms<scalar_i8_k>(rows, count, stride, bytes, norms, norms_blocks_k, nullptr));
    else if (quantization == scalar_f32_k) // what the screened tile measures its scores and their error by
        UA_HIP(launch_row_norms<scalar_f32_k>(rows, count, stride, bytes, norms, norms_blocks_k, nullptr));
    return nullptr;
}

struct assign_args_t {
    const std::uint8_t* points;
    std::uint32_t count;
    const std::uint8_t* centroids;
    std::uint32_t clusters, stride, dimensions;
    const std::uint32_t *point_norms, *centroid_norms;
    std::uint32_t* assignments;
    float* distances;
    std::uint32_t* shifted;
    kmeans_assign_plan_t plan; ///< f16 / bf16 / i8: which tile (kmeans_plan.hpp); the matrices are laid out for it
    // f32 on the screened tile (`plan_kmeans_assign_f32`): the points it hands to the wave kernel (`count` cells) and how many they
    // are — zero before every launch —, and for the test hook the contenders re-measured per point. Null: the wave kernel alone.
    std::uint32_t* overflow_list = nullptr;
    std::uint32_t* overflow_count = nullptr;
    std::uint32_t* contenders = nullptr;
};

/// Which tile a run over `quantization` rows takes, and with it how its two matrices are laid out: USEARCH_AMD_KMEANS_TILE = 64 /
/// 256 forces either, anything else leaves the choice to the planner. f32 rows keep the plain layout whichever kernel takes them
/// (`screened_assign`).
kmeans_assign_plan_t plan_assign(scalar_kind_t quantization, std::size_t count, std::size_t clusters, std::size_t dimensions) {
    if (quantization == scalar_f32_k)
        return kmeans_assign_plan_t{};
    return plan_kmeans_assign(count, clusters, (bytes_per_vector(quantization, dimensions) + 15) / 16 * 16, env_size("USEARCH_AMD_KMEANS_TILE", 0));
}

/// f32 rows: the screened tile or the wave kernel alone (kmeans_plan.hpp; USEARCH_AMD_KMEANS_TILE = 64 / 1 forces either).
bool screened_assign(scalar_kind_t quantization, std::size_t count, std::size_t clusters) {
    return quantization == scalar_f32_k && plan_kmeans_assign_f32(count, clusters, env_size("USEARCH_AMD_KMEANS_TILE", 0));
}

/// The grid of the wave kernel's second launch, over the points the screen handed over: enough waves to fill the chip, each taking
/// its share of the list; with an empty list every wave leaves at once.
constexpr std::uint32_t overflow_blocks_k = 2048;

template <int metric_ak, int scalar_ak> const char* launch_assign_wide(const assign_args_t& a) {
    auto kernel = assign_wide_kernel<metric_ak, scalar_ak>;
    UA_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.plan.lds_bytes));
    hipLaunchKernelGGL(kernel, dim3((std::uint32_t)a.plan.point_tiles), dim3(wide_threads_k), a.plan.lds_bytes, nullptr, a.points, a.count,
                       a.centroids, a.clusters, a.stride, a.point_norms, a.centroid_norms, a.assignments, a.distances, a.shifted);
    UA_HIP(hipGetLastError());
    return nullptr;
}

template <int metric_ak> const char* launch_assign_metric(scalar_kind_t quantization, const assign_args_t& a) {
    const std::uint32_t tiles = (a.count + tile_points_k - 1) / tile_points_k;
    if (a.plan.wide && quantization == scalar_f16_k)
        return launch_assign_wide<metric_ak, scalar_f16_k>(a);
    if (a.plan.wide && quantization == scalar_bf16_k)
        return launch_assign_wide<metric_ak, scalar_bf16_k>(a);
    if (a.plan.wide && quantization == scalar_i8_k)
        return launch_assign_wide<metric_ak, scalar_i8_k>(a);
    if (quantization == scalar_f32_k && a.overflow_list) {
        assign_screened_kernel<metric_ak><<<tiles, 256>>>(a.points, a.count, a.centroids, a.clusters, a.stride, a.dimensions, a.point_norms,
                                                          a.centroid_norms, a.assignments, a.distances, a.shifted, a.overflow_list,
                                                          a.overflow_count, a.contenders);
        UA_HIP(hipGetLastError());
        assign_f32_kernel<metric_ak><<<std::min(overflow_blocks_k, (a.count + 3) / 4), 256>>>(
            a.points, a.count, a.centroids, a.clusters, a.stride, a.dimensions, a.assignments, a.distances, a.shifted, a.overflow_list,
            a.overflow_count);
    } else if (quantization == scalar_f32_k)
        assign_f32_kernel<metric_ak><<<(a.count + 3) / 4, 256>>>(a.points, a.count, a.centroids, a.clusters, a.stride, a.dimensions,
                                                                 a.assignments, a.distances, a.shifted, nullptr, nullptr);
    else if (quantization == scalar_f16_k)
        assign_tiled_kernel<metric_ak, scalar_f16_k><<<tiles, 256>>>(a.points, a.count, a.centroids, a.clusters, a.stride, a.point_norms,
                                                                     a.centroid_norms, a.assignments, a.distances, a.shifted);
    else if (quantization == scalar_bf16_k)
        assign_tiled_kernel<metric_ak, scalar_bf16_k><<<tiles, 256>>>(a.points, a.count, a.centroids, a.clusters, a.stride, a.point_norms,
                                                                      a.centroid_norms, a.assignments, a.distances, a.shifted);
    else
        assign_tiled_kernel<metric_ak, scalar_i8_k><<<tiles, 256>>>(a.points, a.count, a.centroids, a.clusters, a.stride, a.point_norms,
                                                                    a.centroid_norms, a.assignments, a.distances, a.shifted);
    UA_HIP(hipGetLastError());
    return nullptr;
}

const char* launch_assign(metric_kind_t metric, scalar_kind_t quantization, const assign_args_t& a) {
    if (metric == metric_l2sq_k)
        return launch_assign_metric<metric_l2sq_k>(quantization, a);
    if (metric == metric_cos_k)
        return launch_assign_metric<metric_cos_k>(quantization, a);
    return launch_assign_metric<metric_ip_k>(quantization, a);
}

template <int metric_ak, int scalar_ak>
void launch_finalize(double* sums, std::uint32_t dimensions, std::uint32_t clusters, const std::uint32_t* offsets, std::uint8_t* centroids,
                     std::uint32_t stride) {
    finalize_kernel<metric_ak, scalar_ak><<<(clusters + 63) / 64, 64>>>(sums, dimensions, clusters, offsets, centroids, stride);
}

template <int scalar_ak>
const char* launch_update_kind(metric_kind_t metric, const std::uint8_t* points, std::uint32_t stride, std::uint32_t dimensions,
                               std::uint32_t clusters, const std::uint32_t* offsets, const std::uint32_t* members, double* sums,
                               std::uint8_t* centroids) {
    sums_kernel<scalar_ak><<<dim3(clusters, (dimensions + 63) / 64), 64>>>(points, stride, dimensions, clusters, offsets, members, sums);
    UA_HIP(hipGetLastError());
    if (metric == metric_l2sq_k)
        launch_finalize<metric_l2sq_k, scalar_ak>(sums, dimensions, clusters, offsets, centroids, stride);
    else if (metric == metric_cos_k)
        launch_finalize<metric_cos_k, scalar_ak>(sums, dimensions, clusters, offsets, centroids, stride);
    else
        launch_finalize<metric_ip_k, scalar_ak>(sums, dimensions, clusters, offsets, centroids, stride);
    UA_HIP(hipGetLastError());
    return nullptr;
}

inline std::size_t quantized_stride_of(scalar_kind_t quantization, std::size_t dimensions) {
    return (bytes_per_vector(quantization, dimensions) + 15) / 16 * 16;
}
/// The two matrices as the planned tile reads them: the wide tile fills LDS with whole 128-byte chunks of whole tiles of 256 rows,
/// so both hold them (zeros beyond the data); every other kernel of the run only ever sees the pitch.
inline std::size_t planned_stride(const kmeans_assign_plan_t& plan, scalar_kind_t quantization, std::size_t dimensions) {
    const std::size_t stride = quantized_stride_of(quantization, dimensions);
    return plan.wide ? kmeans_wide_stride(stride) : stride;
}
inline std::size_t planned_rows(const kmeans_assign_plan_t& plan, std::size_t rows) { return plan.wide ? kmeans_wide_rows(rows) : rows; }

const char* check_shape(std::size_t count, std::size_t dimensions, std::size_t clusters) {
    if (count >= (std::size_t(1) << 32))
        return "k-means on the device takes fewer than 2^32 points";
    if (dimensions == 0 || dimensions > 65535u * 64u) // a wave per 64 dimensions in the second grid dimension of the sums
        return "k-means on the device takes between 1 and 4194240 dimensions";
    if (clusters > 65535u * 64u) // the grid of the finalising kernel and of the sums
        return "The number of clusters is too large for the device";
    return nullptr;
}

const char* metric_supported(metric_kind_t metric) {
    return metric == metric_l2sq_k || metric == metric_cos_k || metric == metric_ip_k
               ? nullptr
               : "k-means on the device takes the metrics l2sq, cos and ip";
}

} // namespace

const char* kmeans_quantize(const std::uint8_t* points, std::size_t count, std::size_t stride, scalar_kind_t kind,
                            std::size_t dimensions, scalar_kind_t quantization, int device, std::uint8_t* out, std::size_t out_stride) {
    if (const char* e = refuse_kinds(kind, quantization))
        return e;
    if (const char* e = check_shape(count, dimensions, 0))
        return e;
    if (!count)
        return nullptr;
    UA_HIP(hipSetDevice(device));
    const std::size_t quantized_stride = quantized_stride_of(quantization, dimensions);
    device_scratch_t scratch(device);
    std::uint8_t* quantized = nullptr;
    UA_HIP(scratch.allocate(&quantized, count * quantized_stride));
    if (const char* e = quantize_rows(points, count, stride, kind, dimensions, quantization, quantized, quantized_stride, count))
        return e;
    UA_HIP(hipMemcpy2D(out, out_stride, quantized, quantized_stride, bytes_per_vector(quantization, dimensions), count,
                       hipMemcpyDeviceToHost));
    return nullptr;
}

namespace {

/// `kmeans_assign`, and `kmeans_screen` with `contenders` set: f32 rows on the screened tile whatever the planner would choose.
const char* assign_once(const std::uint8_t* points, std::size_t count, std::size_t stride, const std::uint8_t* centroids,
                        std::size_t clusters, std::size_t centroids_stride, scalar_kind_t kind, std::size_t dimensions,
                        metric_kind_t metric, scalar_kind_t quantization, int device, std::uint64_t* assignments, float* distances,
                        std::uint32_t* contenders) {
    if (const char* e = refuse_kinds(kind, quantization))
        return e;
    if (const char* e = metric_supported(metric))
        return e;
    if (clusters < 1)
        return "The number of clusters must be at least 1";
    if (const char* e = check_shape(count, dimensions, clusters))
        return e;
    if (!count)
        return nullptr;
    UA_HIP(hipSetDevice(device));
    const kmeans_assign_plan_t plan = plan_assign(quantization, count, clusters, dimensions);
    const bool screened = contenders || screened_assign(quantization, count, clusters);
    const std::size_t quantized_stride = planned_stride(plan, quantization, dimensions);
    const std::size_t point_rows = planned_rows(plan, count), centroid_rows = planned_rows(plan, clusters);
    const std::uint32_t bytes = (std::uint32_t)bytes_per_vector(quantization, dimensions);
    device_scratch_t scratch(device);
    std::uint8_t *quantized = nullptr, *quantized_centroids = nullptr;
    std::uint32_t *point_norms = nullptr, *centroid_norms = nullptr, *indexes = nullptr, *shifted = nullptr, *overflow_list = nullptr,
                  *contenders_device = nullptr;
    float* nearest = nullptr;
    UA_HIP(scratch.allocate(&quantized, point_rows * quantized_stride));
    UA_HIP(scratch.allocate(&quantized_centroids, centroid_rows * quantized_stride));
    UA_HIP(scratch.allocate(&point_norms, count * 4));
    UA_HIP(scratch.allocate(&centroid_norms, clusters * 4));
    UA_HIP(scratch.allocate(&indexes, count * 4));
    UA_HIP(scratch.allocate(&nearest, count * 4));
    UA_HIP(scratch.allocate(&shifted, 8)); // and the count of points the screen hands over
    if (screened)
        UA_HIP(scratch.allocate(&overflow_list, count * 4));
    if (contenders)
        UA_HIP(scratch.allocate(&contenders_device, count * 4));
    const char* e = nullptr;
    if ((e = quantize_rows(points, count, stride, kind, dimensions, quantization, quantized, quantized_stride, point_rows)) ||
        (e = quantize_rows(centroids, clusters, centroids_stride, kind, dimensions, quantization, quantized_centroids, quantized_stride,
                           centroid_rows)))
        return e;
    if (quantization != scalar_f32_k || screened)
        if ((e = launch_norms(quantization, quantized, count, quantized_stride, bytes, point_norms)) ||
            (e = launch_norms(quantization, quantized_centroids, clusters, quantized_stride, bytes, centroid_norms)))
            return e;
    UA_HIP(hipMemset(indexes, 0xFF, count * 4));
    UA_HIP(hipMemset(shifted, 0, 8));
    assign_args_t args{quantized, (std::uint32_t)count, quantized_centroids, (std::uint32_t)clusters, (std::uint32_t)quantized_stride,
                       (std::uint32_t)dimensions, point_norms, centroid_norms, indexes, nearest, shifted, plan};
    if (screened)
        args.overflow_list = overflow_list, args.overflow_count = shifted + 1, args.contenders = contenders_device;
    if ((e = launch_assign(metric, quantization, args)))
        return e;
    std::vector<std::uint32_t> narrow(count);
    UA_HIP(hipMemcpy(narrow.data(), indexes, count * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(distances, nearest, count * 4, hipMemcpyDeviceToHost));
    if (contenders)
        UA_HIP(hipMemcpy(contenders, contenders_device, count * 4, hipMemcpyDeviceToHost));
    for (std::size_t i = 0; i != count; ++i)
        assignments[i] = narrow[i];
    return nullptr;
}

} // namespace

const char* kmeans_assign(const std::uint8_t* points, std::size_t count, std::size_t stride, const std::uint8_t* centroids,
                          std::size_t clusters, std::size_t centroids_stride, scalar_kind_t kind, std::size_t dimensions,
                          metric_kind_t metric, scalar_kind_t quantization, int device, std::uint64_t* assignments, float* distances) {
    return assign_once(points, count, stride, centroids, clusters, centroids_stride, kind, dimensions, metric, quantization, device,
                       assignments, distances, nullptr);
}

const char* kmeans_screen(const std::uint8_t* points, std::size_t count, std::size_t stride, const std::uint8_t* centroids,
                          std::size_t clusters, std::size_t centroids_stride, std::size_t dimensions, metric_kind_t metric, int device,
                          std::uint64_t* assignments, float* distances, std::uint32_t* contenders) {
    if (!contenders)
        return "kmeans_screen reports the contenders of every point";
    return assign_once(points, count, stride, centroids, clusters, centroids_stride, scalar_f32_k, dimensions, metric, scalar_f32_k, device,
                       assignments, distances, contenders);
}

const char* kmeans_run(const std::uint8_t* points, std::size_t count, std::size_t stride, scalar_kind_t kind, std::size_t dimensions,
                       std::size_t clusters, const kmeans_config_t& config, std::uint8_t* centroids, std::size_t centroids_stride,
                       std::uint64_t* assignments, float* distances, kmeans_stats_t* stats) {
    // ---- index_plugins.hpp:2255-2266
    if (config.max_iterations < 1)
        return "The number of iterations must be at least 1";
    if (clusters < 2)
        return "The number of clusters must be at least 2";
    if (clusters >= count)
        return "The number of clusters must be less than the number of vectors";
    const scalar_kind_t quantization = config.quantization;
    const metric_kind_t metric = config.metric;
    if (const char* e = refuse_kinds(kind, quantization))
        return e;
    if (const char* e = metric_supported(metric))
        return e;
    if (const char* e = check_shape(count, dimensions, clusters))
        return e;
    UA_HIP(hipSetDevice(config.device)); // before any allocation

    const kmeans_assign_plan_t plan = plan_assign(quantization, count, clusters, dimensions);
    const std::size_t quantized_stride = planned_stride(plan, quantization, dimensions);
    const std::size_t point_rows = planned_rows(plan, count), centroid_rows = planned_rows(plan, clusters);
    const std::uint32_t bytes = (std::uint32_t)bytes_per_vector(quantization, dimensions);
    // chunks of the stable scatter: 64 points each while a cell per (chunk, centroid) fits 256 MB, longer ones beyond
    constexpr std::uint64_t max_cells = std::uint64_t(1) << 26;
    std::uint64_t steps = 1;
    while (((count + 64 * steps - 1) / (64 * steps)) * clusters > max_cells)
        steps *= 2;
    const std::uint64_t chunks = (count + 64 * steps - 1) / (64 * steps);
    if (chunks > 0x7FFFFFFFull || steps > 0xFFFFFFFFull)
        return "The number of clusters is too large for the device";

    // what the f64 sums and the rest need in HBM, against what is free
    const bool screened = screened_assign(quantization, count, clusters);
    const std::size_t needed = point_rows * quantized_stride + centroid_rows * quantized_stride + count * (screened ? 20 : 16) + clusters * 16 +
                               chunks * clusters * 4 + clusters * dimensions * 8 +
                               (kind == quantization ? 0 : std::min<std::size_t>(count * bytes_per_vector(kind, dimensions), std::size_t(1) << 30));
    std::size_t free_bytes = 0, total_bytes = 0;
    UA_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    if (needed > free_bytes)
        return "The points, the centroids and their f64 sums do not fit in free device memory";

    device_scratch_t scratch(config.device);
    std::uint8_t *quantized = nullptr, *quantized_centroids = nullptr;
    std::uint32_t *point_norms = nullptr, *centroid_norms = nullptr, *indexes = nullptr, *scalars = nullptr, *seeds = nullptr,
                  *cells = nullptr, *counts = nullptr, *offsets = nullptr, *members = nullptr, *overflow_list = nullptr;
    float* nearest = nullptr;
    double* sums = nullptr;
    UA_HIP(scratch.allocate(&quantized, point_rows * quantized_stride));
    UA_HIP(scratch.allocate(&quantized_centroids, centroid_rows * quantized_stride));
    UA_HIP(scratch.allocate(&point_norms, count * 4));
    UA_HIP(scratch.allocate(&centroid_norms, clusters * 4));
    UA_HIP(scratch.allocate(&indexes, count * 4));
    UA_HIP(scratch.allocate(&nearest, count * 4));
    UA_HIP(scratch.allocate(&scalars, 16)); // the f64 aggregate, the count of points that changed centroid, of points the screen handed over
    if (screened)
        UA_HIP(scratch.allocate(&overflow_list, count * 4));
    UA_HIP(scratch.allocate(&seeds, clusters * 4));
    UA_HIP(scratch.allocate(&cells, chunks * clusters * 4));
    UA_HIP(scratch.allocate(&counts, clusters * 4));
    UA_HIP(scratch.allocate(&offsets, (clusters + 1) * 4));
    UA_HIP(scratch.allocate(&members, count * 4));
    UA_HIP(scratch.allocate(&sums, clusters * dimensions * 8));
    event_pair_t events;
    UA_HIP(events.create());

    const char* e = nullptr;
    if ((e = quantize_rows(points, count, stride, kind, dimensions, quantization, quantized, quantized_stride, point_rows)))
        return e;
    UA_HIP(hipMemset(quantized_centroids, 0, centroid_rows * quantized_stride));

    // ---- seeding, index_plugins.hpp:2308-2350, the uniqueness test as the reference has it
    std::vector<std::uint32_t> index(count, (std::uint32_t)clusters), seed_points(clusters);
    {
        std::mt19937_64 random_engine;
        random_engine.seed(config.seed);
        for (std::size_t i = 0; i < clusters; i++) {
            std::size_t random_index;
            do {
                random_index = random_engine() % count;
                bool is_unique = true;
                for (std::size_t j = 0; j < i; j++)
                    if (index[j] == random_index) {
                        is_unique = false;
                        break;
                    }
                if (is_unique)
                    break;
            } while (true);
            seed_points[i] = (std::uint32_t)random_index;
            index[random_index] = (std::uint32_t)i;
        }
    }
    UA_HIP(hipMemcpy(indexes, index.data(), count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(seeds, seed_points.data(), clusters * 4, hipMemcpyHostToDevice));
    gather_rows_kernel<<<grid_for(clusters * (quantized_stride / 16), 256), 256>>>(quantized, seeds, quantized_centroids, (std::uint32_t)clusters,
                                                                                   (std::uint32_t)quantized_stride);
    UA_HIP(hipGetLastError());
    if (quantization != scalar_f32_k || screened)
        if ((e = launch_norms(quantization, quantized, count, quantized_stride, bytes, point_norms)))
            return e;
    UA_HIP(hipDeviceSynchronize());

    assign_args_t args{quantized, (std::uint32_t)count, quantized_centroids, (std::uint32_t)clusters, (std::uint32_t)quantized_stride,
                       (std::uint32_t)dimensions, point_norms, centroid_norms, indexes, nearest, scalars + 2, plan};
    if (screened)
        args.overflow_list = overflow_list, args.overflow_count = scalars + 3; // zeroed with the other scalars, every iteration
    struct {
        double aggregate;
        std::uint32_t shifted, unused;
    } readback{};
    kmeans_stats_t result;
    const auto start_time = std::chrono::high_resolution_clock::now();
    std::uint64_t iterations = 0;
    const std::size_t min_points_shifted_per_iteration = static_cast<std::size_t>(config.min_shifts * count);
    const double last_aggregate_distance = std::numeric_limits<double>::max(); // never assigned again: index_plugins.hpp:2355

    while (iterations < config.max_iterations) {
        iterations++;
        // ---- assignment: the centroids' norms, every point against every centroid, the aggregate
        UA_HIP(hipMemsetAsync(scalars, 0, 16));
        UA_HIP(hipEventRecord(events.begin));
        if (quantization != scalar_f32_k || screened)
            if ((e = launch_norms(quantization, quantized_centroids, clusters, quantized_stride, bytes, centroid_norms)))
                return e;
        if ((e = launch_assign(metric, quantization, args)))
            return e;
        aggregate_kernel<<<1, 1024>>>(nearest, (std::uint32_t)count, reinterpret_cast<double*>(scalars));
        UA_HIP(hipGetLastError());
        UA_HIP(hipEventRecord(events.end));
        UA_HIP(hipMemcpy(&readback, scalars, 16, hipMemcpyDeviceToHost));
        float milliseconds = 0;
        UA_HIP(hipEventElapsedTime(&milliseconds, events.begin, events.end));
        result.assign_ms += milliseconds;

        const double aggregate_distance = readback.aggregate;
        const double aggregate_distance_change = std::abs(aggregate_distance - last_aggregate_distance) / last_aggregate_distance;
        const std::chrono::duration<double> elapsed_time = std::chrono::high_resolution_clock::now() - start_time;
        result.runtime_seconds = elapsed_time.count();
        result.last_iteration_inertia = aggregate_distance_change;
        result.last_iteration_points_shifted = readback.shifted;
        result.aggregate_distance = aggregate_distance;

        // ---- early exits, index_plugins.hpp:2401-2409
        if (last_aggregate_distance != 0.0 && config.inertia_threshold != 0.0)
            if (aggregate_distance_change <= config.inertia_threshold)
                break;
        if (min_points_shifted_per_iteration != 0 || result.last_iteration_points_shifted == 0)
            if (result.last_iteration_points_shifted <= min_points_shifted_per_iteration)
                break;
        if (config.max_seconds != 0)
            if (result.runtime_seconds >= config.max_seconds)
                break;

        // ---- update
        UA_HIP(hipEventRecord(events.begin));
        UA_HIP(hipMemsetAsync(cells, 0, chunks * clusters * 4));
        members_kernel<false><<<(std::uint32_t)chunks, 64>>>(indexes, (std::uint32_t)count, (std::uint32_t)clusters, (std::uint32_t)steps, cells,
                                                             nullptr, nullptr);
        chunk_scan_kernel<<<(std::uint32_t)((clusters + 255) / 256), 256>>>(cells, (std::uint32_t)chunks, (std::uint32_t)clusters, counts);
        offsets_kernel<<<1, 1024>>>(counts, (std::uint32_t)clusters, offsets);
        members_kernel<true><<<(std::uint32_t)chunks, 64>>>(indexes, (std::uint32_t)count, (std::uint32_t)clusters, (std::uint32_t)steps, cells,
                                                            offsets, members);
        UA_HIP(hipGetLastError());
        if (quantization == scalar_f32_k)
            e = launch_update_kind<scalar_f32_k>(metric, quantized, (std::uint32_t)quantized_stride, (std::uint32_t)dimensions,
                                                 (std::uint32_t)clusters, offsets, members, sums, quantized_centroids);
        else if (quantization == scalar_f16_k)
            e = launch_update_kind<scalar_f16_k>(metric, quantized, (std::uint32_t)quantized_stride, (std::uint32_t)dimensions,
                                                 (std::uint32_t)clusters, offsets, members, sums, quantized_centroids);
        else if (quantization == scalar_bf16_k)
            e = launch_update_kind<scalar_bf16_k>(metric, quantized, (std::uint32_t)quantized_stride, (std::uint32_t)dimensions,
                                                  (std::uint32_t)clusters, offsets, members, sums, quantized_centroids);
        else
            e = launch_update_kind<scalar_i8_k>(metric, quantized, (std::uint32_t)quantized_stride, (std::uint32_t)dimensions,
                                                (std::uint32_t)clusters, offsets, members, sums, quantized_centroids);
        if (e)
            return e;
        UA_HIP(hipEventRecord(events.end));
        UA_HIP(hipEventSynchronize(events.end));
        UA_HIP(hipEventElapsedTime(&milliseconds, events.begin, events.end));
        result.update_ms += milliseconds;
    }

    // ---- export, index_plugins.hpp:2480-2496
    result.iterations = iterations;
    result.computed_distances = (std::uint64_t)count * clusters * iterations;
    UA_HIP(hipMemcpy(index.data(), indexes, count * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(distances, nearest, count * 4, hipMemcpyDeviceToHost));
    for (std::size_t i = 0; i != count; ++i)
        assignments[i] = index[i];
    std::vector<std::uint8_t> rows(clusters * quantized_stride);
    UA_HIP(hipMemcpy(rows.data(), quantized_centroids, rows.size(), hipMemcpyDeviceToHost));
    for (std::size_t i = 0; i != clusters; ++i) {
        const std::uint8_t* row = rows.data() + i * quantized_stride;
        std::uint8_t* target = centroids + i * centroids_stride;
        if (!cast_vector(quantization, kind, row, dimensions, target))
            std::memcpy(target, row, bytes);
    }
    if (stats)
        *stats = result;
    return nullptr;
}

} // namespace usearch_amd
