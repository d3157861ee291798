/**
 *  usearch_amd/csrc/device_math.hpp — what several kernel files must agree on TO THE BIT, stated once: the matrix-unit product and
 *  its fragment geometry; the 64 × 128 staged tile — its LDS layout, the stream that brings a step's rows global → registers → LDS
 *  (`staged_rows_gt`, `staged_stream_gt`), the product of a chunk and the pipelined product of a B tile; Σx² of a row; the metrics'
 *  closing arithmetic; the order-preserving float → u32 map; "a live member the caller allows" (`row_is_allowed`).
 *  Users: exact_tiled.hip (`exact_tiled_kernel`: the stream and the product of a chunk; the wide tile: `multiply` and the geometry),
 *  exact_screened.hip (`screen_kernel`) and kmeans.hip (`assign_tiled_kernel`, `assign_screened_kernel`; the wide tile as above): the
 *  pipelined product — screen_math.hpp, built on this header, holds what the two screens share besides — exact_bits.hip (the closing
 *  arithmetic, `row_is_allowed`), wide_stage.hpp (`chunk_bytes_k`), join.hip and clustering.hip (ordered bits).
 *  Depends on common.hpp and the HIP runtime only — kmeans.o is linked without the engine.
 *
 *  Fragment geometry of `v_mfma_f32_32x32x16_{f16,bf16}` / `v_mfma_i32_32x32x32_i8` / `v_mfma_f32_32x32x2_f32`. Both operands are
 *  row-major with the summation index contiguous, and the A and B fragments of these shapes use the same (lane half, element) → k
 *  assignment, so every lane simply loads 16 consecutive bytes of "its" A row and of "its" B row: no transposition anywhere. Lane
 *  half h = lane >> 5 owns bytes [32·step + 16h, +16) of row lane & 31 (`fragment_row`, `fragment_byte`). f32: those 16 bytes are
 *  four scalars and each feeds one 32x32x2 step — lanes 0 … 31 carry k = e, lanes 32 … 63 k = 4 + e, for A and B alike — so the sum
 *  is right as it is; only the order of its terms is the kernel's own. C/D: column (B row) = lane & 31 (`accumulator_column`),
 *  row (A row) = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5) (`accumulator_row`).
 *
 *  f8 (OCP e4m3 codes, a byte each): the lane's 16 bytes are decoded in registers to sixteen f16 values — exact, every e4m3 value is
 *  an f16 value — and go through the f16 instruction as two operands, chained (`multiply`, `decode_f8x16`); any split of the 16
 *  scalars into two operands gives the right sum, because the query's scalar and the row's scalar land on the same k. What f8 buys
 *  here is bytes — half of an f16 row's from HBM to LDS to registers, which is what bounds the tiles — not matrix-unit rate.
 *  gfx950's fp8 instructions were tried first, with the same geometry, and are NOT used: on an MI355X both `v_mfma_f32_32x32x16_fp8_fp8`
 *  (twice per 16 bytes) and `v_mfma_scale_f32_32x32x64_f8f6f4` (k = 64, two steps to an instruction, unit scales) decode every code
 *  exactly but return sums about 2·10⁻⁵ of their own size from the f64 value — 1.5 … 1.9 of the bounds of tests/exact_truth.py for
 *  64-d cos, 96-d l2sq and 200-d ip, whatever the length of the row — where this route's f32 sums of the (exact) products are exact for ip and l2sq
 *  and within 0.011 of the bound for cos: inside those instructions the products are not summed in f32. The bound is the contract, so the products go the f16 way.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace usearch_amd {

// ---- the staged tile: a workgroup of 4 waves multiplies 64 A rows with 128 B rows, `chunk_bytes_k` bytes of every row at a time
constexpr int staged_a_rows_k = 64, staged_b_rows_k = 128;
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

/// Sixteen e4m3 codes → their sixteen f16 values, in order, as two operands of the f16 instruction: `v_cvt_pk_f32_fp8` (OCP e4m3 on
/// gfx950) decodes two codes exactly, `v_cvt_pkrtz_f16_f32` packs them — nothing to round, the values are f16 values.
__device__ __forceinline__ void decode_f8x16(uint4 codes, f16x8_t& low, f16x8_t& high) {
    const std::uint32_t words[4] = {codes.x, codes.y, codes.z, codes.w};
    std::uint32_t packed[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const auto first = __builtin_amdgcn_cvt_pk_f32_fp8((int)words[w], false), second = __builtin_amdgcn_cvt_pk_f32_fp8((int)words[w], true);
        packed[2 * w] = __builtin_bit_cast(std::uint32_t, __builtin_amdgcn_cvt_pkrtz(first[0], first[1]));
        packed[2 * w + 1] = __builtin_bit_cast(std::uint32_t, __builtin_amdgcn_cvt_pkrtz(second[0], second[1]));
    }
    low = __builtin_bit_cast(f16x8_t, uint4{packed[0], packed[1], packed[2], packed[3]});
    high = __builtin_bit_cast(f16x8_t, uint4{packed[4], packed[5], packed[6], packed[7]});
}

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
    } else if constexpr (scalar_ak == scalar_f8_k) {
        f16x8_t a_low, a_high, b_low, b_high;
        decode_f8x16(a, a_low, a_high);
        decode_f8x16(b, b_low, b_high);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_low, b_low, c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a_high, b_high, c, 0, 0, 0);
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

/// One operand's rows in global memory, as the staged tile reads them. A tile's rows at and beyond `end` and a row's bytes at and
/// beyond `bytes` are staged as zeros. `row_at`, `stride_at`: the caller's own integer widths (row numbers of 32 bits are compared
/// in 32 bits). `ragged_ak`: a caller's query batch — a row may end inside a 16-byte piece, and nothing is promised about alignment.
template <typename row_at, typename stride_at, bool ragged_ak = false> struct staged_rows_gt {
    using row_t = row_at;
    static constexpr bool ragged_k = ragged_ak;
    const std::uint8_t* base; ///< of row 0
    stride_at stride;         ///< bytes from a row to the next
    row_at first, end;        ///< the rows the workgroup multiplies: A rows [first, first + 64), B tiles of 128 rows from `first` on
    std::uint32_t bytes;      ///< of every row that may be read — the caller's bound; whole 16-byte pieces unless `ragged_ak`
    bool aligned;             ///< `base` and `stride` are multiples of 16: 16-byte loads are safe (always, unless `ragged_ak`)
};

/// A snapshot's stored rows [first, end): 16-byte aligned and zero padded to whole 16-byte pieces (`ix.chunks`).
__device__ __forceinline__ staged_rows_gt<std::uint64_t, std::uint32_t> stored_rows(const snapshot_view_t& ix, std::uint64_t first,
                                                                                   std::uint64_t end) {
    return {ix.vectors, ix.row_stride, first, end, ix.chunks * 16u, true};
}
/// Rows [first, end) of a caller's query batch, `bytes` each, at whatever stride and alignment.
__device__ __forceinline__ staged_rows_gt<std::uint32_t, std::uint64_t, true> query_rows(const std::uint8_t* queries, std::uint64_t stride,
                                                                                         std::uint32_t first, std::uint32_t end,
                                                                                         std::uint32_t bytes) {
    return {queries, stride, first, end, bytes, stride % 16 == 0 && (std::uintptr_t)queries % 16 == 0};
}

/// 16 bytes of a row from `byte` on; byte by byte where a ragged operand's row ends inside them or the operand is not aligned.
template <typename rows_at> __device__ __forceinline__ i32x4_t fetch_staged_piece(const rows_at& rows, typename rows_at::row_t row, std::uint32_t byte) {
    i32x4_t value = {0, 0, 0, 0}; // (one 128-bit value, not HIP's struct of four: nothing tempts the compiler to take it apart)
    if (row < rows.end && byte < rows.bytes) {
        const std::uint8_t* source = rows.base + (std::uint64_t)row * rows.stride + byte;
        if (!rows_at::ragged_k || (byte + 16 <= rows.bytes && rows.aligned))
            value = *reinterpret_cast<const i32x4_t*>(source);
        else {
            std::uint8_t parts[16] = {0};
#pragma clang loop vectorize(disable) unroll(disable) // (the rare path stays one small loop: widened eight times, its 16-way
                                                      // selects are half of a kernel's code)
            for (std::uint32_t b = 0; b < 16 && byte + b < rows.bytes; ++b)
                parts[b] = source[b];
            value = *reinterpret_cast<const i32x4_t*>(parts);
        }
    }
    return value;
}

/**
 *  The staged tile's stream: the rows of a step (B tile, chunk) travel global → registers → LDS. 8 consecutive threads take one
 *  row's 128 bytes of the chunk, 16 each; a thread makes two passes of A rows and four of B rows (row 32·pass + thread / 8 of the
 *  tile): six 16-byte loads (`fetch`), six LDS stores (`stash`). The registers in between are what lets the NEXT step's rows fly
 *  behind this step's products (`multiply_staged_tile`). The byte-by-byte path exists only where A is a ragged operand
 *  (`query_rows`); B is never one.
 */
template <typename a_rows_at, typename b_rows_at> struct staged_stream_gt {
    static_assert(!b_rows_at::ragged_k, "B rows are read in whole 16-byte pieces");
    using b_row_t = typename b_rows_at::row_t;
    a_rows_at a;
    b_rows_at b;
    std::uint8_t* stage; ///< LDS: [64][pitch_k] of A, then [128][pitch_k] of B
    std::uint32_t thread;
    i32x4_t fetched[(staged_a_rows_k + staged_b_rows_k) / 32];

    __device__ __forceinline__ staged_stream_gt(a_rows_at a_rows, b_rows_at b_rows, std::uint8_t* lds, std::uint32_t thread_in_block)
        : a(a_rows), b(b_rows), stage(lds), thread(thread_in_block) {}
    __device__ __forceinline__ std::uint8_t* stage_a() const { return stage; }
    __device__ __forceinline__ std::uint8_t* stage_b() const { return stage + staged_a_rows_k * pitch_k; }

    /// Requests chunk `chunk` of the A rows and of the B tile that begins at row `b_row`.
    __device__ __forceinline__ void fetch(b_row_t b_row, std::uint32_t chunk) {
        const std::uint32_t byte = chunk * chunk_bytes_k + thread % 8 * 16;
#pragma unroll
        for (std::uint32_t pass = 0; pass < staged_a_rows_k / 32; ++pass)
            fetched[pass] = fetch_staged_piece(a, a.first + pass * 32 + thread / 8, byte);
#pragma unroll
        for (std::uint32_t pass = 0; pass < staged_b_rows_k / 32; ++pass)
            fetched[staged_a_rows_k / 32 + pass] = fetch_staged_piece(b, b_row + pass * 32 + thread / 8, byte);
    }
    /// What was fetched, into the staging area (the caller's barrier follows).
    __device__ __forceinline__ void stash() {
#pragma unroll
        for (std::uint32_t pass = 0; pass < staged_a_rows_k / 32; ++pass)
            *reinterpret_cast<i32x4_t*>(stage_a() + (pass * 32 + thread / 8) * pitch_k + thread % 8 * 16) = fetched[pass];
#pragma unroll
        for (std::uint32_t pass = 0; pass < staged_b_rows_k / 32; ++pass)
            *reinterpret_cast<i32x4_t*>(stage_b() + (pass * 32 + thread / 8) * pitch_k + thread % 8 * 16) = fetched[staged_a_rows_k / 32 + pass];
    }
};

/**
 *  The pipelined product of the A rows with the B tile that begins at row `b_row`, whose chunk 0 has been fetched: `acc` = 0, then
 *  per chunk stash, barrier, request the next step's rows — the next chunk, or chunk 0 of the next B tile if there is one: that
 *  flight crosses the caller's epilogue — `multiply_staged_chunk`, barrier. `announce` runs between the zeroing and
 *  the first barrier: the caller's per-tile norms and flags in LDS, which nobody reads before that barrier.
 */
template <int scalar_ak, typename stream_at, typename announce_at>
__device__ __forceinline__ void multiply_staged_tile(stream_at& stream, typename stream_at::b_row_t b_row, std::uint32_t chunks,
                                                     typename accumulator_gt<scalar_ak>::type (&acc)[2], announce_at&& announce) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            acc[t][r] = 0;
    announce();
    for (std::uint32_t chunk = 0; chunk < chunks; ++chunk) {
        stream.stash();
        __syncthreads();
        if (chunk + 1 < chunks)
            stream.fetch(b_row, chunk + 1);
        else if (b_row + staged_b_rows_k < stream.b.end)
            stream.fetch(b_row + staged_b_rows_k, 0);
        multiply_staged_chunk<scalar_ak>(stream.stage_a(), stream.stage_b(), stream.thread / 64, stream.thread % 64, acc);
        __syncthreads();
    }
}

/// Row `row` of the snapshot is a live member the caller allows: no tombstone, and the row's bit of `allow_bits` set (one bit per
/// slot, index.hpp:4260-4263; null = no predicate).
__device__ __forceinline__ bool row_is_allowed(const snapshot_view_t& ix, const std::uint32_t* allow_bits, std::uint64_t row) {
    bool member = !ix.has_tombstones || ix.keys[row] != free_key_k;
    if (allow_bits && member)
        member = ((allow_bits[row >> 5] >> (row & 31)) & 1u) != 0;
    return member;
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
        // bytes a lane takes per round: one f32, one 16-bit scalar, two i8, or one f8. `bytes` is what the row holds, whatever its pitch
        // (a query row is not padded to 16 bytes, and a caller's batch need not be aligned to more than its scalars)
        constexpr std::uint32_t width = scalar_ak == scalar_f32_k ? 4 : scalar_ak == scalar_f8_k ? 1 : 2;
        for (std::uint32_t b = lane * width; b < bytes; b += 64 * width) {
            if constexpr (scalar_ak == scalar_f8_k) {
                // `v_cvt_pk_f32_fp8` (OCP e4m3 on gfx950; decoding is exact): element 0 of the pair is the code. A lane takes every
                // 64th element by fmaf, as for f16: the bound derived for that scheme (tests/exact_truth.py) carries over
                const float x = __builtin_amdgcn_cvt_pk_f32_fp8((int)p[b], false)[0];
                sum = __builtin_fmaf(x, x, sum);
            } else if constexpr (scalar_ak == scalar_i8_k) {
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

/// Σx² of the stored rows and of a batch of queries in their kind, what the exact-search tiles close cos and l2sq with.
template <int scalar_ak>
hipError_t launch_exact_norms(const snapshot_view_t& view, const std::uint8_t* queries, std::uint64_t count, std::uint64_t stride,
                              std::uint32_t* row_norms, std::uint32_t* query_norms, hipStream_t stream) {
    constexpr std::uint32_t norms_blocks = 1u << 20; // the grid of either launch at most
    const hipError_t e = launch_row_norms<scalar_ak>(view.vectors, view.size, view.row_stride, view.bytes_per_vector, row_norms,
                                                     norms_blocks, stream);
    return e != hipSuccess ? e : launch_row_norms<scalar_ak>(queries, count, stride, view.bytes_per_vector, query_norms, norms_blocks, stream);
}

} // namespace

} // namespace usearch_amd
