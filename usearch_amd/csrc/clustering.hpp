/**
 *  usearch_amd/csrc/clustering.hpp — `index_dense_gt::cluster` of a whole batch by the index's own levels
 *  (index_dense.hpp:1819-1981), on the device. NOT `cluster(query, level)` (the descent alone: `snapshot_t::cluster_host`), which
 *  is one step of it, and not k-means (kmeans.hpp).
 *
 *  The rules, restated from the reference (clustering.hip has the kernels):
 *    1. LEVEL  `min_clusters > 0`: from `max_level` down while level > 1, the first level with MORE than `min_clusters` nodes at or
 *              above it (removed members count: `stats(level)` walks every slot, index.hpp:3167-3184). `min_clusters == 0`:
 *              level 1, `max_clusters` = the nodes at or above level 1, `min_clusters` = 2 — nothing is ever merged.
 *              `max_level < 2`: "Index too small to cluster!" (after the level loop, as there).
 *    2. MAP    every query takes the greedy descent to that level (`search_extras_t::descent_only`). Like the reference's
 *              (index.hpp:3123 drops the predicate) it does not ask whether a member was removed: a removed member of that level
 *              can be where it ends. Such a centroid is an entry of its own here, reported under `free_key_k`; entries of one
 *              key are told apart by slot (the reference folds every removed centroid into one entry).
 *              `visited_members` / `computed_distances` sum over every mapping pass, repeated ones included; nothing later counts.
 *    3. COUNT  how many queries reached each centroid; U = the distinct centroids.
 *    4. REFINE U < min_clusters and level > 1: one level down, map again.
 *    5. ORDER  popularity descending, THEN CENTROID KEY ASCENDING (then slot). The reference leaves equal popularities wherever
 *              libstdc++'s `std::sort` drops them; this is the project's rule, and the only point where the two may part.
 *    6. MERGE  while U > max_clusters: the last entry is the source; candidates are positions 0 … U−2 in the current order; the
 *              nearest by metric(source's stored row, candidate's stored row) under strict `<` from FLT_MAX wins, the first of
 *              equals; nothing below FLT_MAX (NaN, +inf, FLT_MAX itself): position 0. The target takes the source's popularity and
 *              moves towards the front while the entry before it is STRICTLY less popular. U−−.
 *    7. TRACE  only if anything merged: every query follows `merged_into` to a centroid that survived (chains happen), and its
 *              distance is measured again against that centroid's stored row — for every query, moved or not.
 *    8. REFUSED `min_clusters > 0` with `max_clusters == 0`: the reference's last cycle would merge entry 0 into itself and its trace
 *              would never end. `max_clusters < min_clusters` is legal and merges down to `max_clusters`.
 *
 *  Every distance of 6 and 7 goes through the kernel behind `usearch_amd_distances` (same functors, same lanes per row): same bits.
 */
#pragma once
#include <cstddef>
#include <cstdint>

namespace usearch_amd {

struct clustering_config_t {
    std::size_t min_clusters = 0, max_clusters = 0;
};

struct clustering_stats_t {
    std::uint64_t clusters = 0;            ///< centroids left after the merges
    std::uint64_t unique_before_merge = 0; ///< U of the last mapping pass
    std::uint64_t merge_cycles = 0;
    std::uint64_t mapping_passes = 0;
    std::uint64_t visited_members = 0, computed_distances = 0;
    std::uint32_t level = 0;               ///< the level of the last mapping pass
    float seconds_map = 0.f, seconds_merge = 0.f, seconds_trace = 0.f;
};

} // namespace usearch_amd
