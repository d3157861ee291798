/**
 *  usearch_amd/csrc/sketch.hpp — a low-rank sketch of the stored rows that PROVES a candidate of the level-0 beam too far to matter,
 *  so that the walk need not fetch its row (DESIGN.md §3.1 "the sketch").
 *
 *  cos only. R ≤ 62 fixed directions D (rows of an [R][dimensions] matrix, close to orthonormal; stored transposed and padded to 64
 *  columns, f32). A stored row b gets one 128-byte record: ĉ = f16(D b̂), b̂ = b / ‖b‖, in halves 0 … 61 and, in the last four bytes,
 *  an f32 ρ ≥ ‖b̂ − Dᵀĉ‖. For any query a, with p = D a:
 *
 *      a·b̂ = a·(Dᵀĉ) + a·(b̂ − Dᵀĉ) = p·ĉ + a·(b̂ − Dᵀĉ) ≤ p·ĉ + ‖a‖ ρ            (Cauchy–Schwarz)
 *      cos(a, b) ≤ (p / ‖a‖)·ĉ + ρ,      distance = 1 − cos ≥ 1 − (p / ‖a‖)·ĉ − ρ
 *
 *  The first identity is plain algebra: it holds for ANY matrix D and ANY vector ĉ — orthonormality, the rounding of the coefficients
 *  to f16 and of the directions to f32 only decide how small ρ is, never whether the bound holds, because ρ is taken against the
 *  STORED ĉ and the STORED D:
 *
 *      ‖b̂ − Dᵀĉ‖² = 1 − 2 ĉ·(D b̂) + ĉᵀ(D Dᵀ)ĉ ≤ 1 − 2 ĉ·c + (1 + δ) ‖ĉ‖²,     c = D b̂,  δ = ‖D Dᵀ − I‖_F
 *
 *  c, ‖b‖² and the three sums are accumulated in f64 (the products of two f32 values are exact there; 768 terms lose 768 · 2⁻⁵³),
 *  δ is computed in f64 from the stored f32 directions, and ρ is rounded up. What the f64 arithmetic can lose (≈ 1e-13) is covered
 *  by the 1e-9 added under the root.
 *
 *  THE SLACK. The walk compares the bound with the distance ITS kernel computes, an f32 sum in the lane-group layout, and computes
 *  p in f32 itself. With u = 2⁻²⁴ and n = dimensions, relative to ‖a‖ ‖b‖ = 1:
 *    · the kernel's Σab, Σa², Σb² are fused multiply-add chains of at most n terms: each off by at most n·u of Σ|ab| ≤ ‖a‖‖b‖ (resp.
 *      of itself); the two roots halve the relative error of the squares, the product, the quotient and the subtraction add 4u:
 *      the computed distance is at least the real one − (2n + 4) u;
 *    · p_j is a chain of n terms: off by at most n·u·‖a‖‖D_j‖; against ĉ that is n·u·Σ|ĉ_j| ≤ n·u·√62·‖ĉ‖ < 8 n u (‖ĉ‖ ≤ 1 + 2⁻¹⁰,
 *      ‖D_j‖ ≤ 1 + 2⁻²⁰); dividing by √Σa² (itself off by n·u / 2 + 2u) adds at most (n / 2 + 3) u;
 *    · the 64-term dot product of p / ‖a‖ with ĉ: 64 u · Σ|p̂_j ĉ_j| ≤ 64 u;
 *    · the final additions: 3u.
 *  Together < (10.5 n + 80) u. The slack is 16 n u + 2⁻¹⁶ (7.5e-4 at 768 dimensions): a candidate is pruned only when
 *  1 − (p̂·ĉ + ρ + slack) ≥ radius. At the headline the 608th and the 14 170th nearest distances are 0.12 apart, and about 20 of a
 *  query's 14 170 candidates lie within 1e-3 of its radius: the slack costs nothing that can be measured.
 *
 *  NEVER PRUNED: a row whose Σb² is zero, not finite or outside the range in which f32 chains are safe (`sketch_norm_in_range`), or
 *  whose coefficients are not finite, gets ρ = +∞ (zero coefficients): the bound is −∞. A query whose Σa² is outside that range does
 *  not use the sketch at all. So the special cases of `finalize_distance`, NaN rows and rows at the edges of the f32 range stay on
 *  the exact path.
 */
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "common.hpp"

#ifndef __HIPCC__
#define USEARCH_AMD_SKETCH_BOTH inline
#else
#define USEARCH_AMD_SKETCH_BOTH __host__ __device__ inline
#endif

namespace usearch_amd {

constexpr std::uint32_t sketch_rank_k = 62;          ///< directions at most: 62 halves + one f32 fill a 128-byte line
constexpr std::uint32_t sketch_columns_k = 64;       ///< columns of the transposed direction array (the last two stay zero)
constexpr std::uint32_t sketch_record_bytes_k = 128; ///< one record per member
/// Rows of twelve 16-byte chunks per lane and more: the kernel builds that carry the sketch path (kernels.hpp `sketch_ak`) are the ones
/// such rows run — and below a dozen lines per row the saving would hardly pay for the extra round trip anyway.
constexpr std::uint32_t sketch_min_row_bytes_k = 1536;
constexpr std::uint64_t sketch_seed_k = 0x5EEDC0DE5EEDC0DEull;

/// Which indexes get a sketch at all.
inline bool sketch_eligible(metric_kind_t metric, scalar_kind_t scalar, std::size_t bytes_per_row) {
    return metric == metric_cos_k && (scalar == scalar_f32_k || scalar == scalar_f16_k || scalar == scalar_bf16_k) &&
           bytes_per_row >= sketch_min_row_bytes_k;
}

/// The slack assumes that the kernel's f32 chains neither overflow nor lose their sum to underflow: a row whose Σb², or a query whose
/// Σa², lies outside [2⁻¹⁰⁰, 2¹⁰⁰] (elements around 1e-17 and below, 1e13 and above at 768 dimensions) is never pruned / never prunes.
/// Inside, no partial sum reaches 2¹²⁸, and a product that underflows (below 2⁻¹²⁶) loses at most 2⁻¹²⁶ of a sum of at least 2⁻¹⁰⁰:
/// n such terms cost n · 2⁻²⁶ = n u / 4 per chain, which the gap between the derived (10.5 n + 80) u and the 16 n u taken covers.
USEARCH_AMD_SKETCH_BOTH bool sketch_norm_in_range(double n2) { return n2 >= 0x1p-100 && n2 <= 0x1p100; }

/// See "THE SLACK" above.
USEARCH_AMD_SKETCH_BOTH float sketch_slack(std::uint32_t dimensions) { return 16.f * (float)dimensions * 0x1p-24f + 0x1p-16f; }

/// ρ from the f64 sums s1 = Σ c_j ĉ_j and s2 = Σ ĉ_j², rounded up.
USEARCH_AMD_SKETCH_BOTH float sketch_residual(double s1, double s2, double gram_defect) {
    double r2 = 1.0 - 2.0 * s1 + (1.0 + gram_defect) * s2 + 1e-9;
    r2 = r2 > 0.0 ? r2 : 0.0;
    return (float)sqrt(r2) * 1.000001f + 1e-30f;
}

/// The lower bound of the distance from the f32 dot product p̂·ĉ and ρ: what the walk compares with its radius.
USEARCH_AMD_SKETCH_BOTH float sketch_lower_bound(float dot, float residual, float slack) { return 1.f - ((dot + residual) + slack); }

/// Element `i` of a stored row as the kernels read it.
USEARCH_AMD_SKETCH_BOTH float sketch_scalar(const std::uint8_t* row, std::uint32_t i, scalar_kind_t scalar) {
    if (scalar == scalar_f32_k) {
        float v;
        memcpy(&v, row + 4 * (std::size_t)i, 4);
        return v;
    }
    std::uint16_t bits;
    memcpy(&bits, row + 2 * (std::size_t)i, 2);
    if (scalar == scalar_bf16_k) {
        const std::uint32_t wide = (std::uint32_t)bits << 16;
        float v;
        memcpy(&v, &wide, 4);
        return v;
    }
    _Float16 h;
    memcpy(&h, &bits, 2);
    return (float)h;
}

/// The directions of one snapshot: host copy of the transposed, padded f32 array plus what the records need of it.
struct sketch_directions_t {
    std::vector<float> transposed; ///< [dimensions][sketch_columns_k], column j = direction j; columns ≥ rank are zero
    std::uint32_t rank = 0;
    double gram_defect = 0.0; ///< ‖D Dᵀ − I‖_F over the `rank` stored directions
};

/// Slot of the k-th row the directions are drawn from: seeded, the same for every load of the same image.
inline std::uint64_t sketch_sample_slot(std::uint64_t k, std::uint64_t size) {
    std::uint64_t z = sketch_seed_k + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return size ? z % size : 0;
}

/// Orthonormalises `count` sample rows ([count][dimensions], f64) on the host: Gram–Schmidt with re-orthogonalisation; a row whose
/// remainder falls below 1e-6 of its norm (or whose norm is zero or not finite) is dropped. Fewer than 62 usable rows: fewer directions.
inline sketch_directions_t sketch_orthonormalise(const std::vector<double>& samples, std::uint32_t count, std::uint32_t dimensions) {
    sketch_directions_t out;
    out.transposed.assign((std::size_t)dimensions * sketch_columns_k, 0.f);
    std::vector<std::vector<double>> basis;
    std::vector<double> w(dimensions);
    for (std::uint32_t s = 0; s < count && basis.size() < sketch_rank_k; ++s) {
        const double* v = samples.data() + (std::size_t)s * dimensions;
        double n2 = 0;
        for (std::uint32_t i = 0; i < dimensions; ++i)
            n2 += v[i] * v[i];
        if (!(n2 > 0) || !std::isfinite(n2))
            continue;
        const double inverse = 1.0 / std::sqrt(n2);
        for (std::uint32_t i = 0; i < dimensions; ++i)
            w[i] = v[i] * inverse;
        for (int pass = 0; pass < 2; ++pass)
            for (const std::vector<double>& q : basis) {
                double dot = 0;
                for (std::uint32_t i = 0; i < dimensions; ++i)
                    dot += w[i] * q[i];
                for (std::uint32_t i = 0; i < dimensions; ++i)
                    w[i] -= dot * q[i];
            }
        double r2 = 0;
        for (std::uint32_t i = 0; i < dimensions; ++i)
            r2 += w[i] * w[i];
        if (!(r2 >= 1e-12) || !std::isfinite(r2)) // remainder below 1e-6 of the (unit) norm
            continue;
        const double scale = 1.0 / std::sqrt(r2);
        for (std::uint32_t i = 0; i < dimensions; ++i)
            w[i] *= scale;
        basis.push_back(w);
    }
    out.rank = (std::uint32_t)basis.size();
    for (std::uint32_t j = 0; j < out.rank; ++j)
        for (std::uint32_t i = 0; i < dimensions; ++i)
            out.transposed[(std::size_t)i * sketch_columns_k + j] = (float)basis[j][i];
    double defect2 = 0; // against the STORED (f32) directions
    for (std::uint32_t j = 0; j < out.rank; ++j)
        for (std::uint32_t k = 0; k < out.rank; ++k) {
            double g = 0;
            for (std::uint32_t i = 0; i < dimensions; ++i)
                g += (double)out.transposed[(std::size_t)i * sketch_columns_k + j] * (double)out.transposed[(std::size_t)i * sketch_columns_k + k];
            g -= j == k ? 1.0 : 0.0;
            defect2 += g * g;
        }
    out.gram_defect = std::sqrt(defect2);
    return out;
}

/// Host twin of the record builder (sketch.hip `sketch_records_kernel`): the same sums in f64, the same closing arithmetic.
inline void sketch_record_host(const std::uint8_t* row, scalar_kind_t scalar, std::uint32_t dimensions, const sketch_directions_t& d,
                               std::uint8_t* record) {
    double c[sketch_columns_k] = {0}, n2 = 0;
    for (std::uint32_t i = 0; i < dimensions; ++i) {
        const double b = (double)sketch_scalar(row, i, scalar);
        n2 = fma(b, b, n2);
        const float* column = d.transposed.data() + (std::size_t)i * sketch_columns_k;
        for (std::uint32_t j = 0; j < sketch_columns_k; ++j)
            c[j] = fma(b, (double)column[j], c[j]);
    }
    _Float16 halves[sketch_columns_k];
    bool never = !sketch_norm_in_range(n2);
    const double inverse = never ? 0.0 : 1.0 / sqrt(n2);
    double lane_s1[8], lane_s2[8]; // as the device sums them: eight directions per lane, then a butterfly over the eight lanes
    for (std::uint32_t sub = 0; sub < 8; ++sub) {
        double s1 = 0, s2 = 0;
        for (std::uint32_t e = 0; e < 8; ++e) {
            const std::uint32_t j = sub * 8 + e;
            const double cj = c[j] * inverse;
            halves[j] = (_Float16)cj;
            const double stored = (double)halves[j];
            never |= !std::isfinite(stored);
            s1 = fma(cj, stored, s1), s2 = fma(stored, stored, s2);
        }
        lane_s1[sub] = s1, lane_s2[sub] = s2;
    }
    for (std::uint32_t offset = 1; offset < 8; offset <<= 1) {
        double next_s1[8], next_s2[8];
        for (std::uint32_t sub = 0; sub < 8; ++sub)
            next_s1[sub] = lane_s1[sub] + lane_s1[sub ^ offset], next_s2[sub] = lane_s2[sub] + lane_s2[sub ^ offset];
        memcpy(lane_s1, next_s1, sizeof(lane_s1)), memcpy(lane_s2, next_s2, sizeof(lane_s2));
    }
    const double s1 = lane_s1[0], s2 = lane_s2[0];
    float residual = sketch_residual(s1, s2, d.gram_defect);
    if (never || !std::isfinite(residual)) {
        for (std::uint32_t j = 0; j < sketch_columns_k; ++j)
            halves[j] = (_Float16)0.f;
        residual = INFINITY;
    }
    memcpy(record, halves, 124);
    memcpy(record + 124, &residual, 4);
}

/// Host twin of the query side (kernels.hpp `search_one`): p̂ = (D a) / √Σa² in f32; false = this query does not use the sketch.
inline bool sketch_query_host(const float* query, float a2, std::uint32_t dimensions, const sketch_directions_t& d, float* coefficients) {
    for (std::uint32_t j = 0; j < sketch_columns_k; ++j) { // the kernel's chains: element i of a block of 16 goes to chain i mod 4
        float sums[4] = {0.f, 0.f, 0.f, 0.f};
        std::uint32_t i = 0;
        for (; i + 16 <= dimensions; i += 16)
            for (std::uint32_t u = 0; u < 16; ++u)
                sums[u & 3] = fmaf(query[i + u], d.transposed[(std::size_t)(i + u) * sketch_columns_k + j], sums[u & 3]);
        for (; i < dimensions; ++i)
            sums[0] = fmaf(query[i], d.transposed[(std::size_t)i * sketch_columns_k + j], sums[0]);
        coefficients[j] = (sums[0] + sums[1]) + (sums[2] + sums[3]);
    }
    if (!sketch_norm_in_range((double)a2)) {
        for (std::uint32_t j = 0; j < sketch_columns_k; ++j)
            coefficients[j] = 0.f;
        return false;
    }
    const float norm = sqrtf(a2);
    for (std::uint32_t j = 0; j < sketch_columns_k; ++j)
        coefficients[j] = coefficients[j] / norm;
    return true;
}

/// Host twin of the bound the walk evaluates for one record (eight lanes of eight halves each, butterfly over the lanes).
inline float sketch_bound_host(const float* coefficients, const std::uint8_t* record, std::uint32_t dimensions) {
    float lanes[8];
    for (std::uint32_t sub = 0; sub < 8; ++sub) {
        float sum = 0.f;
        for (std::uint32_t e = 0; e < 8; ++e) {
            const std::uint32_t j = sub * 8 + e;
            if (j >= sketch_rank_k)
                break;
            _Float16 h;
            memcpy(&h, record + 2 * j, 2);
            sum = fmaf((float)h, coefficients[j], sum);
        }
        lanes[sub] = sum;
    }
    float residual;
    memcpy(&residual, record + 124, 4);
    for (std::uint32_t offset = 1; offset < 8; offset <<= 1) {
        float next[8];
        for (std::uint32_t sub = 0; sub < 8; ++sub)
            next[sub] = lanes[sub] + lanes[sub ^ offset];
        memcpy(lanes, next, sizeof(lanes));
    }
    return sketch_lower_bound(lanes[0], residual, sketch_slack(dimensions));
}

} // namespace usearch_amd
