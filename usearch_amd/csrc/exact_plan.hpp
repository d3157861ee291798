/**
 *  usearch_amd/csrc/exact_plan.hpp — the ONE place that chooses how a tiled exact search (exact_tiled.hip) is launched: the wide tile
 *  (256 queries × 256 rows per workgroup) or the 64-query tile, the split of the rows into partitions, the wide kernel's deal of
 *  (query tile, partition) pairs over its workgroups, and where the wide kernel keeps its lists. Pure integer arithmetic over plain
 *  values: no HIP runtime call, no snapshot, no look at the environment (the caller reads USEARCH_AMD_EXACT_TILE and
 *  USEARCH_AMD_EXACT_GLOBAL_LISTS and passes them in). tests/test_exact_plan.py pins it through `usearch_amd_test_plan_exact`.
 *  The table of pairs that have a tiled kernel at all (`exact_tiled_pair`) lives here too, for the same reason: checkable without a GPU.
 */
#pragma once
#include <algorithm>
#include <cstdint>

#include "common.hpp"
#include "device_math.hpp" // chunk_bytes_k: the staged tile is the kernels', the planner pads query rows to it

namespace usearch_amd {

constexpr int tile_queries_k = 64;  ///< queries per workgroup
constexpr int tile_rows_k = 128;    ///< dataset rows per inner tile
constexpr int max_wanted_k = 64;    ///< per-query results the epilogue keeps (one lane per entry)

constexpr int wide_queries_k = 256; ///< queries per workgroup: a row is read once per 256 queries
constexpr int wide_rows_k = 256;    ///< dataset rows per tile: a query chunk is read once per 256 rows
constexpr int wide_wanted_k = 16;   ///< results per query this kernel keeps (a lane per entry in the ordered insert, entries in the output arrays)
/// Results per query up to which the lists fit LDS next to the two staging buffers (an insert is then an LDS affair of a few
/// hundred cycles instead of a global round trip and a fence: the epilogue and, through it, the barrier shrink).
constexpr int wide_lds_lists_k = 10;
constexpr std::uint64_t wide_least_rows_k = 8u * 4u * wide_rows_k; ///< the wide tile wants eight partitions of four tiles at least

inline std::uint64_t wide_padded_stride(std::uint64_t bytes_per_vector) {
    return (bytes_per_vector + chunk_bytes_k - 1) / chunk_bytes_k * chunk_bytes_k;
}

/// Which (metric, scalar kind) pairs have a tiled kernel, and for how many results per query: cos, ip and l2sq over f16, bf16 and
/// i8, cos and ip over f32, 1 … `max_wanted_k` results. Both kernels are instantiated for every pair here — which of them runs is
/// a matter of the batch's shape (`plan_exact`), never of the kind. tests/test_exact_tiled_pairs.py pins it through
/// `usearch_amd_test_exact_tiled_pair`.
/// l2sq over f32 is NOT here, on purpose: that `exact="tiled"` over an l2sq f32 index is refused is behaviour the suite pins
/// (tests/test_gpu_exact.py: "no matrix-unit kernel for this pair: said so, not silently rerouted"), and giving the pair a kernel
/// changes it. Nothing in the kernels stands in the way — l2sq closes through the float branch every kind shares — so it is this
/// row and three instantiations, in a change that also moves that assertion to a pair that stays without a kernel.
inline bool exact_tiled_pair(metric_kind_t metric, scalar_kind_t scalar, std::uint64_t wanted) {
    if (!wanted || wanted > (std::uint64_t)max_wanted_k)
        return false;
    if (scalar == scalar_f32_k)
        return metric == metric_cos_k || metric == metric_ip_k;
    if (scalar != scalar_f16_k && scalar != scalar_bf16_k && scalar != scalar_i8_k)
        return false;
    return metric == metric_cos_k || metric == metric_ip_k || metric == metric_l2sq_k;
}

/// What `plan_exact` settles. The 64-query tile runs a grid of (query tiles, partitions); the wide tile a 1-D grid of `workgroups`,
/// each of which finds its (query tile, partition) from `query_tiles` and `tiles_per_xcd` (exact_wide_kernel).
struct exact_plan_t {
    std::uint32_t wide = 0;      ///< 1: the wide tile
    std::uint32_t lds_lists = 0; ///< wide only — 1: the lists live in LDS, 0: in the output arrays
    std::uint64_t query_tiles = 0;
    std::uint64_t partitions = 0;
    std::uint64_t rows_per_partition = 0;
    std::uint64_t tiles_per_xcd = 0; ///< wide only
    std::uint64_t workgroups = 0;    ///< wide only
};

/// `forced_tile`: USEARCH_AMD_EXACT_TILE (64 / 256 force either kernel where it can run, anything else leaves the choice here);
/// `global_lists`: USEARCH_AMD_EXACT_GLOBAL_LISTS. → nullptr, or why the call is refused.
inline const char* plan_exact(std::uint64_t rows, std::uint64_t bytes_per_vector, std::uint64_t row_stride, std::uint64_t count,
                              std::uint64_t wanted, std::uint64_t forced_tile, bool global_lists, exact_plan_t& plan) {
    plan = exact_plan_t{};
    if (!wanted || wanted > (std::uint64_t)max_wanted_k)
        return "No tiled exact-search kernel for this metric / scalar kind / result count";
    if (!count)
        return nullptr;
    if (!rows)
        return "Nothing to scan";
    // The wide tile (256 queries per workgroup: a quarter of the dataset passes) takes batches that fill the chip with it; the
    // 64-query tile keeps the small batches and the long result lists. USEARCH_AMD_EXACT_TILE=64 / 256 forces either.
    // (a tile of 256 rows, stored or padded, must lie inside one buffer resource with 32-bit offsets: rows of < 8 MB)
    const bool wide = forced_tile != 64 && wanted <= (std::uint64_t)wide_wanted_k && rows >= wide_least_rows_k &&
                      (forced_tile == 256 || count > 512) && row_stride * wide_rows_k < (1ull << 31) &&
                      wide_padded_stride(bytes_per_vector) * wide_queries_k < (1ull << 31);
    plan.wide = wide ? 1u : 0u;
    if (wide) {
        // ONE round of the chip (32 compute units per XCD) with as few partitions as that takes (exact_wide_kernel)
        const std::uint64_t query_tiles = plan.query_tiles = (count + wide_queries_k - 1) / wide_queries_k;
        const std::uint64_t most = std::max<std::uint64_t>(1, rows / (4 * wide_rows_k)); // a partition is at least four tiles
        if (query_tiles >= 8) { // tiles dealt over the XCDs, every XCD sees every partition
            plan.tiles_per_xcd = (query_tiles + 7) / 8;
            plan.partitions = std::min<std::uint64_t>(std::max<std::uint64_t>(1, 32 / plan.tiles_per_xcd), most);
            plan.workgroups = 8 * plan.tiles_per_xcd * plan.partitions;
        } else { // every XCD works on all the tiles, partitions ≡ xcd (mod 8)
            plan.tiles_per_xcd = query_tiles;
            plan.partitions = std::max<std::uint64_t>(8, 32 / query_tiles * 8);
            while (plan.partitions > 8 && plan.partitions > most)
                plan.partitions -= 8;
            plan.workgroups = plan.tiles_per_xcd * plan.partitions;
        }
        plan.rows_per_partition = (rows + plan.partitions - 1) / plan.partitions;
        plan.rows_per_partition = (plan.rows_per_partition + wide_rows_k - 1) / wide_rows_k * wide_rows_k;
        plan.lds_lists = wanted <= (std::uint64_t)wide_lds_lists_k && !global_lists ? 1u : 0u;
    } else {
        // enough (query tile, partition) workgroups to fill the chip several times over; few enough lists per query to fold
        const std::uint64_t query_tiles = plan.query_tiles = (count + tile_queries_k - 1) / tile_queries_k;
        std::uint64_t partitions = std::max<std::uint64_t>(1, (2048 + query_tiles - 1) / query_tiles);
        partitions = std::min<std::uint64_t>(partitions, std::max<std::uint64_t>(1, 8192 / wanted));
        partitions = std::min<std::uint64_t>(partitions, std::max<std::uint64_t>(1, rows / (4 * tile_rows_k)));
        partitions = std::min<std::uint64_t>(partitions, 65535);
        plan.rows_per_partition = (rows + partitions - 1) / partitions;
        plan.rows_per_partition = (plan.rows_per_partition + tile_rows_k - 1) / tile_rows_k * tile_rows_k;
        plan.partitions = (rows + plan.rows_per_partition - 1) / plan.rows_per_partition;
    }
    return nullptr;
}

// ---- the bit tile (exact_bits.hip): hamming, tanimoto / jaccard and sorensen over b1, popcount(a ∧ b) on the vector ALU

constexpr int bits_wave_queries_k = 64; ///< queries a wave owns: their lists are its own, no wave ever inserts into another's
constexpr int bits_waves_k = 4;         ///< waves per workgroup: 256 queries meet a partition's rows together (one pass through L1 / L2)
constexpr int bits_rows_k = 64;         ///< rows per step of a wave: lane ↔ row
constexpr int bits_block_k = 16;        ///< queries per block of accumulators: what a lane holds while a long row passes piece by piece

/// Which (metric, scalar kind) pairs the bit tile takes, and for how many results per query: hamming, tanimoto, jaccard (which
/// `kernel_metric` maps to tanimoto) and sorensen over b1, 1 … `max_wanted_k` results. NOT part of `exact_tiled_pair`, which stays
/// the table of the matrix-unit pairs. tests/test_exact_bits_plan.py pins it through `usearch_amd_test_exact_bits_pair`.
inline bool exact_bits_pair(metric_kind_t metric, scalar_kind_t scalar, std::uint64_t wanted) {
    if (!wanted || wanted > (std::uint64_t)max_wanted_k || scalar != scalar_b1x8_k)
        return false;
    return metric == metric_hamming_k || metric == metric_tanimoto_k || metric == metric_jaccard_k || metric == metric_sorensen_k;
}

/// What `plan_exact_bits` settles: a grid of (query_tiles, partitions) workgroups of `bits_waves_k` waves, workgroup (x, y) takes
/// queries [256x, 256x + 256) and rows [y · rows_per_partition, (y + 1) · rows_per_partition).
struct exact_bits_plan_t {
    std::uint64_t query_tiles = 0;
    std::uint64_t partitions = 0;
    std::uint64_t rows_per_partition = 0;
    std::uint64_t padded_queries = 0;     ///< rows of the padded copy of the batch: whole waves of 64 queries
    std::uint64_t padded_query_bytes = 0; ///< … and its pitch: whole 16-byte pieces, as the stored rows have them
    std::uint64_t lds_bytes = 0;          ///< the workgroup's lists: [4 waves][64 queries][wanted] cells of 8 bytes
};

/// One variant, so nothing to force and no environment to read. → nullptr, or why the call is refused.
inline const char* plan_exact_bits(std::uint64_t rows, std::uint64_t bytes_per_vector, std::uint64_t row_stride, std::uint64_t count,
                                   std::uint64_t wanted, exact_bits_plan_t& plan) {
    plan = exact_bits_plan_t{};
    if (!wanted || wanted > (std::uint64_t)max_wanted_k)
        return "No tiled exact-search kernel for this metric / scalar kind / result count";
    if (!count)
        return nullptr;
    if (!rows)
        return "Nothing to scan";
    const std::uint64_t pieces = (bytes_per_vector + 15) / 16;
    if (!bytes_per_vector || row_stride < pieces * 16 || pieces >= (1ull << 27))
        return "Row pitch is smaller than the row's 16-byte pieces";
    constexpr std::uint64_t tile = (std::uint64_t)bits_wave_queries_k * bits_waves_k;
    plan.query_tiles = (count + tile - 1) / tile;
    if (plan.query_tiles >= (1ull << 31))
        return "Batch is too large";
    plan.padded_queries = (count + bits_wave_queries_k - 1) / bits_wave_queries_k * bits_wave_queries_k;
    plan.padded_query_bytes = pieces * 16;
    plan.lds_bytes = tile * wanted * 8;
    // enough workgroups to fill the chip several times over (the tail of a round is a smaller share of the run, and a compute unit
    // holds several of them); few enough lists per query for one merge wave; a partition is at least four steps of 64 rows
    std::uint64_t partitions = std::max<std::uint64_t>(1, (2048 + plan.query_tiles - 1) / plan.query_tiles);
    partitions = std::min<std::uint64_t>(partitions, std::max<std::uint64_t>(1, 8192 / wanted));
    partitions = std::min<std::uint64_t>(partitions, std::max<std::uint64_t>(1, rows / (4 * bits_rows_k)));
    partitions = std::min<std::uint64_t>(partitions, 65535);
    plan.rows_per_partition = (rows + partitions - 1) / partitions;
    plan.rows_per_partition = (plan.rows_per_partition + bits_rows_k - 1) / bits_rows_k * bits_rows_k;
    plan.partitions = (rows + plan.rows_per_partition - 1) / plan.rows_per_partition;
    return nullptr;
}

} // namespace usearch_amd
