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
 *                 `v_mfma_i32_32x32x32_i8`. The product of a staged chunk, the fragment layout, Σx² and the closing arithmetic
 *                 are device_math.hpp's — the very code the 64-query tile of exact search (exact_tiled.hip) runs, so the two close
 *                 a pair to the same bits (tests/test_gpu_kmeans.py) and i8 distances are bit-identical to the wave kernel's. The
 *                 epilogue keeps ONE (distance, index) per point under (distance ↑, centroid index ↑). The centroids (k · row
 *                 bytes, a few MB) stay in L2; the points are read from HBM once per iteration.
 *                 f32: a plain wave per point (f32 FMAs over 64 lanes, shuffle reduction), within the f32 tolerance.
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

namespace usearch_amd {

namespace {

constexpr int tile_points_k = 64;     ///< points per workgroup
constexpr int tile_centroids_k = 128; ///< centroids per inner tile
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

/**
 *  grid = point tiles, 256 threads = 4 waves. Wave w multiplies all 64 points of the tile with centroids [32w, 32w + 32) of every
 *  centroid tile: two 32 × 32 accumulators. Rows of both matrices are `stride` bytes apart, 16-byte aligned and zero padded.
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
    std::uint8_t* stage_p = lds;                                 // [64][pitch]
    std::uint8_t* stage_c = stage_p + tile_points_k * pitch_k;   // [128][pitch]
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

    // ---- the rows of a step (centroid tile, chunk) travel global → registers → LDS: 8 consecutive threads fetch one row's 128 bytes,
    //      two passes of points and four of centroids per thread. The NEXT step's rows are requested before this step's products
    //      (also across the epilogue of a tile), so their flight hides behind the matrix unit.
    const std::uint32_t segment = thread % 8;
    uint4 fetched[(tile_points_k + tile_centroids_k) / 32];
    auto fetch = [&](std::uint32_t tile, std::uint32_t chunk) {
        const std::uint32_t byte = chunk * chunk_bytes_k + segment * 16;
#pragma unroll
        for (std::uint32_t pass = 0; pass < tile_points_k / 32; ++pass) {
            const std::uint32_t i = pass * 32 + thread / 8;
            uint4 value = {0u, 0u, 0u, 0u};
            if (first_point + i < count && byte < stride)
                value = *reinterpret_cast<const uint4*>(points + (std::uint64_t)(first_point + i) * stride + byte);
            fetched[pass] = value;
        }
#pragma unroll
        for (std::uint32_t pass = 0; pass < tile_centroids_k / 32; ++pass) {
            const std::uint32_t j = pass * 32 + thread / 8;
            uint4 value = {0u, 0u, 0u, 0u};
            if (tile + j < clusters && byte < stride)
                value = *reinterpret_cast<const uint4*>(centroids + (std::uint64_t)(tile + j) * stride + byte);
            fetched[tile_points_k / 32 + pass] = value;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (std::uint32_t pass = 0; pass < tile_points_k / 32; ++pass)
            *reinterpret_cast<uint4*>(stage_p + (pass * 32 + thread / 8) * pitch_k + segment * 16) = fetched[pass];
#pragma unroll
        for (std::uint32_t pass = 0; pass < tile_centroids_k / 32; ++pass)
            *reinterpret_cast<uint4*>(stage_c + (pass * 32 + thread / 8) * pitch_k + segment * 16) = fetched[tile_points_k / 32 + pass];
    };
    fetch(0, 0);

    for (std::uint32_t tile = 0; tile < clusters; tile += tile_centroids_k) {
        accumulator_t acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[t][r] = 0;
        if (thread < tile_centroids_k)
            norms_c[thread] = tile + thread < clusters ? centroid_norms[tile + thread] : 0u;
        for (std::uint32_t chunk = 0; chunk < chunks; ++chunk) {
            stash();
            __syncthreads();
            if (chunk + 1 < chunks)
                fetch(tile, chunk + 1);
            else if (tile + tile_centroids_k < clusters)
                fetch(tile + tile_centroids_k, 0);
            multiply_staged_chunk<scalar_ak>(stage_p, stage_c, wave, lane, acc);
            __syncthreads();
        }

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

/// f32 rows: a wave per point, the reference's expressions (metric_l2sq_gt / metric_cos_gt / metric_ip_gt over f32) with the
/// dimensions dealt over the lanes.
template <int metric_ak>
__global__ __launch_bounds__(256) void assign_f32_kernel(const std::uint8_t* points, std::uint32_t count, const std::uint8_t* centroids,
                                                         std::uint32_t clusters, std::uint32_t stride, std::uint32_t dimensions,
                                                         std::uint32_t* assignments, float* distances, std::uint32_t* shifted) {
    const std::uint32_t lane = threadIdx.x % 64;
    const std::uint32_t point = blockIdx.x * 4u + threadIdx.x / 64;
    const bool inside = point < count;
    const float* a = reinterpret_cast<const float*>(points + (std::uint64_t)(inside ? point : 0u) * stride);
    float a2 = 0.f;
    if constexpr (metric_ak == metric_cos_k) {
        for (std::uint32_t i = lane; i < dimensions; i += 64)
            a2 = __builtin_fmaf(a[i], a[i], a2);
#pragma unroll
        for (int offset = 32; offset >= 1; offset >>= 1)
            a2 += __shfl_xor(a2, offset, 64);
    }
    float best_d = float_max_k;
    std::uint32_t best_i = 0;
    for (std::uint32_t c = 0; c < clusters; ++c) {
        const float* b = reinterpret_cast<const float*>(centroids + (std::uint64_t)c * stride);
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
        float distance;
        if constexpr (metric_ak == metric_cos_k) {
            if (a2 == 0.f && b2 == 0.f)
                distance = 0.f;
            else if (a2 == 0.f || b2 == 0.f)
                distance = 1.f;
            else
                distance = 1.f - x / (__builtin_sqrtf(a2) * __builtin_sqrtf(b2));
        } else if constexpr (metric_ak == metric_ip_k) {
            distance = 1.f - x;
        } else {
            distance = x;
        }
        if (distance < best_d)
            best_d = distance, best_i = c;
    }
    // one lane per wave publishes; the four leaders of a workgroup count their movers one by one
    bool moved = false;
    if (inside && lane == 0) {
        moved = assignments[point] != best_i;
        assignments[point] = best_i;
        distances[point] = best_d;
    }
    if (moved)
        atomicAdd(shifted, 1u);
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

/// Host rows of `kind` → device rows of `quantization`, `quantized_stride` bytes apart and zero padded, slab by slab.
const char* quantize_rows(const std::uint8_t* rows, std::size_t count, std::size_t stride, scalar_kind_t kind,
                          std::size_t dimensions, scalar_kind_t quantization, std::uint8_t* quantized, std::size_t quantized_stride) {
    UA_HIP(hipMemset(quantized, 0, count * quantized_stride));
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
};

template <int metric_ak> const char* launch_assign_metric(scalar_kind_t quantization, const assign_args_t& a) {
    const std::uint32_t tiles = (a.count + tile_points_k - 1) / tile_points_k;
    if (quantization == scalar_f32_k)
        assign_f32_kernel<metric_ak><<<(a.count + 3) / 4, 256>>>(a.points, a.count, a.centroids, a.clusters, a.stride, a.dimensions,
                                                                 a.assignments, a.distances, a.shifted);
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
    if (const char* e = quantize_rows(points, count, stride, kind, dimensions, quantization, quantized, quantized_stride))
        return e;
    UA_HIP(hipMemcpy2D(out, out_stride, quantized, quantized_stride, bytes_per_vector(quantization, dimensions), count,
                       hipMemcpyDeviceToHost));
    return nullptr;
}

const char* kmeans_assign(const std::uint8_t* points, std::size_t count, std::size_t stride, const std::uint8_t* centroids,
                          std::size_t clusters, std::size_t centroids_stride, scalar_kind_t kind, std::size_t dimensions,
                          metric_kind_t metric, scalar_kind_t quantization, int device, std::uint64_t* assignments, float* distances) {
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
    const std::size_t quantized_stride = quantized_stride_of(quantization, dimensions);
    const std::uint32_t bytes = (std::uint32_t)bytes_per_vector(quantization, dimensions);
    device_scratch_t scratch(device);
    std::uint8_t *quantized = nullptr, *quantized_centroids = nullptr;
    std::uint32_t *point_norms = nullptr, *centroid_norms = nullptr, *indexes = nullptr, *shifted = nullptr;
    float* nearest = nullptr;
    UA_HIP(scratch.allocate(&quantized, count * quantized_stride));
    UA_HIP(scratch.allocate(&quantized_centroids, clusters * quantized_stride));
    UA_HIP(scratch.allocate(&point_norms, count * 4));
    UA_HIP(scratch.allocate(&centroid_norms, clusters * 4));
    UA_HIP(scratch.allocate(&indexes, count * 4));
    UA_HIP(scratch.allocate(&nearest, count * 4));
    UA_HIP(scratch.allocate(&shifted, 4));
    const char* e = nullptr;
    if ((e = quantize_rows(points, count, stride, kind, dimensions, quantization, quantized, quantized_stride)) ||
        (e = quantize_rows(centroids, clusters, centroids_stride, kind, dimensions, quantization, quantized_centroids, quantized_stride)))
        return e;
    if (quantization != scalar_f32_k)
        if ((e = launch_norms(quantization, quantized, count, quantized_stride, bytes, point_norms)) ||
            (e = launch_norms(quantization, quantized_centroids, clusters, quantized_stride, bytes, centroid_norms)))
            return e;
    UA_HIP(hipMemset(indexes, 0xFF, count * 4));
    UA_HIP(hipMemset(shifted, 0, 4));
    const assign_args_t args{quantized, (std::uint32_t)count, quantized_centroids, (std::uint32_t)clusters, (std::uint32_t)quantized_stride,
                             (std::uint32_t)dimensions, point_norms, centroid_norms, indexes, nearest, shifted};
    if ((e = launch_assign(metric, quantization, args)))
        return e;
    std::vector<std::uint32_t> narrow(count);
    UA_HIP(hipMemcpy(narrow.data(), indexes, count * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(distances, nearest, count * 4, hipMemcpyDeviceToHost));
    for (std::size_t i = 0; i != count; ++i)
        assignments[i] = narrow[i];
    return nullptr;
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

    const std::size_t quantized_stride = quantized_stride_of(quantization, dimensions);
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
    const std::size_t needed = count * quantized_stride + clusters * quantized_stride + count * 16 + clusters * 16 +
                               chunks * clusters * 4 + clusters * dimensions * 8 +
                               (kind == quantization ? 0 : std::min<std::size_t>(count * bytes_per_vector(kind, dimensions), std::size_t(1) << 30));
    std::size_t free_bytes = 0, total_bytes = 0;
    UA_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    if (needed > free_bytes)
        return "The points, the centroids and their f64 sums do not fit in free device memory";

    device_scratch_t scratch(config.device);
    std::uint8_t *quantized = nullptr, *quantized_centroids = nullptr;
    std::uint32_t *point_norms = nullptr, *centroid_norms = nullptr, *indexes = nullptr, *scalars = nullptr, *seeds = nullptr,
                  *cells = nullptr, *counts = nullptr, *offsets = nullptr, *members = nullptr;
    float* nearest = nullptr;
    double* sums = nullptr;
    UA_HIP(scratch.allocate(&quantized, count * quantized_stride));
    UA_HIP(scratch.allocate(&quantized_centroids, clusters * quantized_stride));
    UA_HIP(scratch.allocate(&point_norms, count * 4));
    UA_HIP(scratch.allocate(&centroid_norms, clusters * 4));
    UA_HIP(scratch.allocate(&indexes, count * 4));
    UA_HIP(scratch.allocate(&nearest, count * 4));
    UA_HIP(scratch.allocate(&scalars, 16)); // the f64 aggregate, then the count of points that changed centroid
    UA_HIP(scratch.allocate(&seeds, clusters * 4));
    UA_HIP(scratch.allocate(&cells, chunks * clusters * 4));
    UA_HIP(scratch.allocate(&counts, clusters * 4));
    UA_HIP(scratch.allocate(&offsets, (clusters + 1) * 4));
    UA_HIP(scratch.allocate(&members, count * 4));
    UA_HIP(scratch.allocate(&sums, clusters * dimensions * 8));
    event_pair_t events;
    UA_HIP(events.create());

    const char* e = nullptr;
    if ((e = quantize_rows(points, count, stride, kind, dimensions, quantization, quantized, quantized_stride)))
        return e;
    UA_HIP(hipMemset(quantized_centroids, 0, clusters * quantized_stride));

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
    if (quantization != scalar_f32_k)
        if ((e = launch_norms(quantization, quantized, count, quantized_stride, bytes, point_norms)))
            return e;
    UA_HIP(hipDeviceSynchronize());

    const assign_args_t args{quantized, (std::uint32_t)count, quantized_centroids, (std::uint32_t)clusters, (std::uint32_t)quantized_stride,
                             (std::uint32_t)dimensions, point_norms, centroid_norms, indexes, nearest, scalars + 2};
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
        if (quantization != scalar_f32_k)
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
