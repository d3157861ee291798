/**
 *  usearch_amd/csrc/device_math.hpp — what several kernel files must agree on TO THE BIT, stated once: the matrix-unit product and
 *  its fragment geometry, the 64 × 128 staged tile, Σx² of a row, the metrics' closing arithmetic, the order-preserving float →
 *  u32 map. Users: exact_tiled.hip (both tiles), kmeans.hip (the assignment), join.hip and clustering.hip (ordered bits).
 *  Depends on common.hpp and the HIP runtime only — kmeans.o is linked without the engine.
 *
 *  Fragment geometry of `v_mfma_f32_32x32x16_{f16,bf16}` / `v_mfma_i32_32x32x32_i8` / `v_mfma_f32_32x32x2_f32`. Both operands are
 *  row-major with the summation index contiguous, and the A and B fragments of these shapes use the same (lane half, element) → k
 *  assignment, so every lane simply loads 16 consecutive bytes of "its" A row and of "its" B row: no transposition anywhere. Lane
 *  half h = lane >> 5 owns bytes [32·step + 16h, +16) of row lane & 31 (`fragment_row`, `fragment_byte`). f32: those 16 bytes are
 *  four scalars and each feeds one 32x32x2 step — lanes 0 … 31 carry k = e, lanes 32 … 63 k = 4 + e, for A and B alike — so the sum
 *  is right as it is; only the order of its terms is the kernel's own. C/D: column (B row) = lane & 31 (`accumulator_column`),
 *  row (A row) = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5) (`accumulator_row`).
 */
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace usearch_amd {

// ---- the staged tile: a workgroup of 4 waves multiplies 64 A rows with 128 B rows, `chunk_bytes_k` bytes of every row at a time
constexpr int chunk_bytes_k = 128;          ///< bytes of every row staged per step of the summation loop (4 MFMA steps of 32 bytes)
constexpr int pitch_k = chunk_bytes_k + 16; ///< LDS row pitch: keeps 16-byte reads of consecutive rows off the same banks

/// LDS bytes of the staged tile: one chunk of both operands ([a_rows + b_rows][pitch]), and — aliasing it once the products are
/// done — the tile's distances ([a_rows][b_rows + 1] floats), whichever is larger.
constexpr std::uint32_t staged_tile_bytes(int a_rows, int b_rows) {
    const std::uint32_t staging = (a_rows + b_rows) * pitch_k, distances = a_rows * (b_rows + 1) * 4;
    return staging > distances ? staging : distances;
}

using f32x16_t = float __attribute__((ext_vector_type(16)));
using i32x16_t = int __attribute__((ext_vector_type(16)));
using f16x8_t = _Float16 __attribute__((ext_vector_type(8)));
using bf16x8_t = __bf16 __attribute__((ext_vector_type(8)));
using i32x4_t = int __attribute__((ext_vector_type(4)));
using f32x4_t = float __attribute__((ext_vector_type(4)));

template <int scalar_ak> struct accumulator_gt {
    using type = f32x16_t;
};
template <> struct accumulator_gt<scalar_i8_k> {
    using type = i32x16_t;
};

/// One 32 × 32 block: c += A·Bᵀ over the 16 bytes each lane holds of its A row and of its B row.
template <int scalar_ak>
__device__ __forceinline__ typename accumulator_gt<scalar_ak>::type multiply(uint4 a, uint4 b,
                                                                             typename accumulator_gt<scalar_ak>::type c) {
    if constexpr (scalar_ak == scalar_f16_k)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else if constexpr (scalar_ak == scalar_bf16_k)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    else if constexpr (scalar_ak == scalar_f32_k) {
        // the lane's 16 bytes are four scalars, each one step of `v_mfma_f32_32x32x2_f32` (lanes 0 … 31: k = e, lanes 32 … 63:
        // k = 4 + e, for A and B alike) chained on the one accumulator: an fmaf chain in k order, one rounding per product. The
        // dependent latency of the instruction equals its issue interval: the chain costs what four independent ones would.
        const f32x4_t x = __builtin_bit_cast(f32x4_t, a), y = __builtin_bit_cast(f32x4_t, b);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0], y[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(x[1], y[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(x[2], y[2], c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x2f32(x[3], y[3], c, 0, 0, 0);
    } else
        return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4_t, a), __builtin_bit_cast(i32x4_t, b), c, 0, 0, 0);
}

/// A/B fragments: the row of its 32-row block a lane loads from, and where in the row's staged chunk its 16 bytes of `step` lie.
__device__ __forceinline__ std::uint32_t fragment_row(std::uint32_t lane) { return lane & 31; }
__device__ __forceinline__ std::uint32_t fragment_byte(std::uint32_t step, std::uint32_t lane) { return step * 32 + (lane >> 5) * 16; }
/// C/D: the (A row, B row) of the 32 × 32 block that accumulator register `reg` of `lane` holds.
__device__ __forceinline__ std::uint32_t accumulator_row(std::uint32_t reg, std::uint32_t lane) {
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
}
__device__ __forceinline__ std::uint32_t accumulator_column(std::uint32_t lane) { return lane & 31; }

/// The products of one staged chunk: four steps of 32 bytes. Wave w multiplies all 64 A rows (two 32 × 32 accumulators) with
/// B rows [32w, 32w + 32) of the tile; `stage_a` is [64][pitch_k] and `stage_b` [128][pitch_k] in LDS.
template <int scalar_ak>
__device__ __forceinline__ void multiply_staged_chunk(const std::uint8_t* stage_a, const std::uint8_t* stage_b, std::uint32_t wave,
                                                      std::uint32_t lane, typename accumulator_gt<scalar_ak>::type (&acc)[2]) {
    // (one address per operand and lane, blocks and steps as constant offsets from it: the compiler then keeps them in the
    // instructions' offset fields)
    const std::uint8_t* a_row = stage_a + fragment_row(lane) * pitch_k + fragment_byte(0, lane);
    const std::uint8_t* b_row = stage_b + (wave * 32 + fragment_row(lane)) * pitch_k + fragment_byte(0, lane);
#pragma unroll
    for (std::uint32_t step = 0; step < chunk_bytes_k / 32; ++step) {
        const uint4 b = *reinterpret_cast<const uint4*>(b_row + step * 32);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 a = *reinterpret_cast<const uint4*>(a_row + t * 32 * pitch_k + step * 32);
            acc[t] = multiply<scalar_ak>(a, b, acc[t]);
        }
    }
}

/**
 *  The metric's closing arithmetic from the matrix unit's sum Σab and the two stored Σx² (bits of an f32, or an exact int32 for
 *  i8). `finalize_distance` of kernels.hpp is the bit-exact original of these expressions (it feeds every search kernel and is not
 *  built on this header); i8 sums are exact, so i8 distances here carry the wave kernel's bits.
 *
 *  Σ(a−b)² over floats is computed as Σa² + Σb² − 2Σab and held at 0 from below. The two callers hold it differently, and each
 *  form is that caller's contract, so the caller names it:
 *    `l2sq_nan_to_zero_k`  d > 0 ? d : 0 — a NaN becomes 0. Exact search: its lists order candidates with `<` and `==`, which a
 *                          NaN would break, and nothing promises that a NaN distance reaches a search at all ("Open:
 *                          the order of NaN distances in `top`").
 *    `l2sq_nan_stays_k`    d < 0 ? 0 : d — a NaN stays a NaN. K-means: the reference's scan (index_plugins.hpp:2366-2375) takes a
 *                          centroid on strict `<` only, so a NaN never wins; turned into 0 it would win against everybody.
 */
enum l2sq_clamp_t { l2sq_nan_to_zero_k, l2sq_nan_stays_k };

template <int metric_ak, int scalar_ak, l2sq_clamp_t clamp_ak, typename sum_at>
__device__ __forceinline__ float closing_distance(sum_at sum, std::uint32_t a2_bits, std::uint32_t b2_bits) {
    if constexpr (scalar_ak == scalar_i8_k) {
        const int ab = sum, a2 = (int)a2_bits, b2 = (int)b2_bits;
        if constexpr (metric_ak == metric_cos_k) { // metric_cos_i8_t, index_plugins.hpp:1583-1607, incl. `ab == 0 → 0`
            const float a2f = __builtin_sqrtf((float)a2), b2f = __builtin_sqrtf((float)b2);
            return ab != 0 ? 1.f - (float)ab / (a2f * b2f) : 0.f;
        } else if constexpr (metric_ak == metric_ip_k) {
            return 1.f - (float)ab;
        } else { // metric_l2sq_i8_t 1613-1630
            return (float)(a2 + b2 - 2 * ab);
        }
    } else if constexpr (scalar_ak == scalar_b1x8_k) {
        // `sum` is the `ix` of kernels.hpp's `partial_t` — |a⊕b| for hamming, |a∧b| for the other two — and the two stored values
        // are |a| and |b|, from which its `iy` follows in integers: |a∨b| = |a| + |b| − |a∧b| (tanimoto), |a| + |b| (sorensen).
        // One IEEE division of exact integers; 0 / 0 (both vectors empty) is the NaN the reference returns, and stays one.
        const int ab = sum, a2 = (int)a2_bits, b2 = (int)b2_bits;
        if constexpr (metric_ak == metric_hamming_k) // metric_hamming_gt<b1x8_t> 1392-1414
            return (float)ab;
        else if constexpr (metric_ak == metric_sorensen_k) // 1451-1476
            return 1 - 2 * (float)ab / (float)(a2 + b2);
        else // tanimoto, jaccard 1420-1445
            return 1 - (float)ab / (float)(a2 + b2 - ab);
    } else {
        const float ab = sum, a2 = __builtin_bit_cast(float, a2_bits), b2 = __builtin_bit_cast(float, b2_bits);
        if constexpr (metric_ak == metric_cos_k) { // metric_cos_gt, index_plugins.hpp:1334-1359
            if (a2 == 0.f && b2 == 0.f)
                return 0.f;
            if (a2 == 0.f || b2 == 0.f)
                return 1.f;
            return 1.f - ab / (__builtin_sqrtf(a2) * __builtin_sqrtf(b2));
        } else if constexpr (metric_ak == metric_l2sq_k) { // Σ(a−b)² (index_plugins.hpp:1365-1385) as Σa² + Σb² − 2Σab, never below 0
            const float d = a2 + b2 - 2.f * ab;
            if constexpr (clamp_ak == l2sq_nan_to_zero_k)
                return d > 0.f ? d : 0.f;
            else
                return d < 0.f ? 0.f : d;
        } else {
            return 1.f - ab;
        }
    }
}

/// A float as an unsigned integer of the same order (negative distances exist: 1 − Σab), so that an integer `atomicMin` or a
/// comparison of (bits << 32 | payload) keeps the smallest. −0 goes before +0: a caller to whom they are equal adds 0.f first.
__device__ __forceinline__ std::uint32_t ordered_bits(float x) {
    const std::uint32_t bits = __builtin_bit_cast(std::uint32_t, x);
    return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
/// All ones ("nothing published yet") decode to a NaN.
__device__ __forceinline__ float from_ordered_bits(std::uint32_t ordered) {
    return __builtin_bit_cast(float, ordered ^ ((ordered >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

namespace { // a kernel and its launcher per translation unit: every code object registers and launches its own instance

/// Σx² of every row, as the closing arithmetic wants it: f32 for the float kinds, exact int32 for i8 (stored as bits).
template <int scalar_ak>
__global__ __launch_bounds__(256) void row_norms_kernel(const std::uint8_t* rows, std::uint64_t count, std::uint64_t stride,
                                                        std::uint32_t bytes, std::uint32_t* out) {
    // one wave per row, grid-stride: a launch may not exceed 2^32 threads, and 100M rows × 64 lanes would
    const std::uint32_t lane = threadIdx.x % 64;
    for (std::uint64_t row = blockIdx.x * 4ull + threadIdx.x / 64; row < count; row += (std::uint64_t)gridDim.x * 4) {
        const std::uint8_t* p = rows + row * stride;
        float sum = 0.f;
        int exact = 0;
        // bytes a lane takes per round: one f32, one 16-bit scalar, or two i8. `bytes` is what the row holds, whatever its pitch
        // (a query row is not padded to 16 bytes, and a caller's batch need not be aligned to more than its scalars)
        constexpr std::uint32_t width = scalar_ak == scalar_f32_k ? 4 : 2;
        for (std::uint32_t b = lane * width; b < bytes; b += 64 * width) {
            if constexpr (scalar_ak == scalar_i8_k) {
                const int x = (std::int8_t)p[b], y = b + 1 < bytes ? (std::int8_t)p[b + 1] : 0;
                exact += x * x + y * y;
            } else if constexpr (scalar_ak == scalar_f32_k) {
                const float x = (std::uintptr_t)(p + b) % 4 == 0
                                    ? *reinterpret_cast<const float*>(p + b)
                                    : __builtin_bit_cast(float, (std::uint32_t)p[b] | ((std::uint32_t)p[b + 1] << 8) |
                                                                    ((std::uint32_t)p[b + 2] << 16) | ((std::uint32_t)p[b + 3] << 24));
                sum = __builtin_fmaf(x, x, sum);
            } else {
                const std::uint32_t bits = (std::uint32_t)p[b] | ((std::uint32_t)p[b + 1] << 8);
                const float x = scalar_ak == scalar_bf16_k ? __builtin_bit_cast(float, bits << 16)
                                                           : (float)__builtin_bit_cast(_Float16, (std::uint16_t)bits);
                sum = __builtin_fmaf(x, x, sum);
            }
        }
#pragma unroll
        for (int offset = 32; offset >= 1; offset >>= 1) {
            sum += __shfl_xor(sum, offset, 64);
            exact += __shfl_xor(exact, offset, 64);
        }
        if (lane == 0)
            out[row] = scalar_ak == scalar_i8_k ? (std::uint32_t)exact : __builtin_bit_cast(std::uint32_t, sum);
    }
}

/// `max_blocks`: the caller's cap on the grid (four rows to a block; the kernel is grid-stride, results do not depend on it).
template <int scalar_ak>
hipError_t launch_row_norms(const std::uint8_t* rows, std::uint64_t count, std::uint64_t stride, std::uint32_t bytes,
                            std::uint32_t* out, std::uint32_t max_blocks, hipStream_t stream) {
    if (!count)
        return hipSuccess;
    const std::uint64_t blocks = (count + 3) / 4;
    hipLaunchKernelGGL(row_norms_kernel<scalar_ak>, dim3((unsigned)(blocks < max_blocks ? blocks : max_blocks)), dim3(256), 0, stream,
                       rows, count, stride, bytes, out);
    return hipGetLastError();
}

} // namespace

} // namespace usearch_amd
