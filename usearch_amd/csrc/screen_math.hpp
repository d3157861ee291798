/**
 *  usearch_amd/csrc/screen_math.hpp — the f32 screen, stated once: what the matrix unit's sums are allowed to decide about f32 rows
 *  whose published distances carry another kernel's bits. Users: kmeans.hip (`assign_screened_kernel`) and exact_screened.hip
 *  (`screen_kernel`). Depends on common.hpp and device_math.hpp only — kmeans.o is linked without the engine.
 *
 *  The contract. The 64 × 128 staged tile (`multiply_staged_chunk<scalar_f32_k>`) adds in the matrix unit's order, so a pair's sum
 *  Σab only SCREENS. Per (A row, B row) it gives a score s and an error e with
 *      | s − (d − c)·f | ≤ e
 *  where d is the distance the MEASURING kernel gives the pair — the one whose bits are published — and c, f > 0 depend on the A row
 *  alone: s is an order-preserving image of d, e wide. With A = √Σa², B = √Σb² (`launch_row_norms<scalar_f32_k>`):
 *      l2sq  s = Σb² − 2Σab        e = g·(A + B)²
 *      ip    s = −Σab              e = g·A·B + 2⁻²³
 *      cos   s = −Σab / √Σb²       e = g·A            (Σb² = 0: s = 0, which is (1 − 1)·A to the bit)
 *  g counts the roundings of both kernels and so depends on how the measuring kernel sums (`screen_g_*` below; DESIGN.md §9 derives
 *  the formula once and g twice). A B row can be among an A row's nearest only if s − e is at or below the bound the others' s + e set.
 *
 *  The band. The derivation assumes sums that neither overflow nor lose bits to underflow: below 2⁻⁶⁰ per Σx² an underflowed product
 *  could matter against e, above 2⁶⁰ a sum could overflow; a NaN or an infinity anywhere in a row puts its Σx² outside. A row whose
 *  Σx² is out of band is never decided by (s, e): what happens to it instead is its kernel's business.
 */
#pragma once
#include "common.hpp"
#include "device_math.hpp"

namespace usearch_amd {

constexpr float screen_least_square_k = 0x1p-60f, screen_most_square_k = 0x1p+60f;

/// Σx² for which the derivation of e does not hold. `zero_too`: a caller whose closing arithmetic special-cases a zero norm.
__device__ __forceinline__ bool square_out_of_band(float x2, bool zero_too) {
    if (x2 == 0.f)
        return zero_too;
    return !(x2 >= screen_least_square_k && x2 <= screen_most_square_k); // a NaN is out of band
}

/// g where `wave_distance_f32` (kmeans.hip) measures: 64 lanes deal the dimensions, a lane's chain has n/64 terms, six shuffle-adds
/// ("f32 rows: screened on the matrix units, measured by the wave kernel").
__device__ __forceinline__ float screen_g_wave(std::uint32_t dimensions) { return 2.f * (float)(dimensions + 16) * 0x1p-24f; }
/// g where `measure_rows` (kernels.hpp) measures: a lane group of 1 … 8 lanes owns the row, a lane's chain has up to n terms
/// ("Exact search of f32 rows: screened on the matrix units, measured by the wave kernel").
__device__ __forceinline__ float screen_g_lane_groups(std::uint32_t dimensions) { return 4.f * (float)(dimensions + 16) * 0x1p-24f; }

/// s from the matrix unit's Σab, the B row's Σb² and its root.
template <int metric_ak> __device__ __forceinline__ float screen_score(float ab, float b2, float root_b) {
    if constexpr (metric_ak == metric_l2sq_k)
        return b2 - 2.f * ab;
    else if constexpr (metric_ak == metric_ip_k)
        return -ab;
    else // (`screen_kernel` has a zero row out of band under cos and never looks at its score: the select changes no result there)
        return b2 == 0.f ? 0.f : -ab / root_b;
}

/// e from g and the two roots.
template <int metric_ak> __device__ __forceinline__ float screen_error(float g, float root_a, float root_b) {
    if constexpr (metric_ak == metric_l2sq_k) {
        const float both = root_a + root_b;
        return g * both * both;
    } else if constexpr (metric_ak == metric_ip_k)
        return __builtin_fmaf(g * root_a, root_b, 0x1p-23f);
    else
        return g * root_a;
}

/// A wave's two accumulators of the staged tile as scores, transposed into LDS: S[A row][B row of the tile], the pitch of
/// `staged_tile_bytes`. `squares_b` / `roots_b`: Σb² and √Σb² of the tile's B rows.
template <int metric_ak>
__device__ __forceinline__ void store_screen_scores(const f32x16_t (&acc)[2], const float* squares_b, const float* roots_b,
                                                    std::uint32_t wave, std::uint32_t lane, float* tile_s) {
    const std::uint32_t j = wave * 32 + accumulator_column(lane);
    const float b2 = squares_b[j], root_b = roots_b[j];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const std::uint32_t i = t * 32 + accumulator_row(r, lane);
            tile_s[i * (staged_b_rows_k + 1) + j] = screen_score<metric_ak>(acc[t][r], b2, root_b);
        }
    }
}

} // namespace usearch_amd
