/**
 *  usearch_amd/csrc/compact.hpp — `isolate` and `compact` of a device index: removed members leave the neighbour lists, and
 *  then the index itself, without a rebuild.
 *
 *  `usearch_remove` leaves a tombstone: the member's key becomes `free_key_k`, it keeps routing and stops matching
 *  (index_dense.hpp:1479-1511). From then on every search pays for the predicate: the heap frontier instead of the open cells of
 *  `top`, no build cut for plain batches (engine.hip `search_begin`). The reference's remedies are `index_dense_gt::isolate`
 *  (index_dense.hpp:1709-1720 → index.hpp:3700-3728) and `compact` (index_dense.hpp:1740-1760 → index.hpp:3595-3682).
 *
 *  ISOLATE is the reference's, list for list: for every member, removed ones included, and every level it exists on, every
 *  neighbour whose key is `free_key_k` is erased; the rest of the list keeps its order (`neighbors_ref_t::erase_if`,
 *  index.hpp:2181-2194). Slots, keys, rows, levels, the entry point and `has_tombstones` stay.
 *
 *  COMPACT deviates from the reference's (which permutes slots by level and nearest upper-level member with an unstable sort, and
 *  keeps the tombstones; row order buys nothing on this engine, profiles/r04_locality/). Ours:
 *    1. survivors = members with key != free_key_k in ascending old slot; new slot = rank among them (stable)
 *    2. every list is what `isolate` leaves, cells renumbered; levels are kept
 *    3. upper-level lists are repacked in new-slot order: the arrays equal what loading the saved image would produce
 *    4. the entry point follows its member; if that was removed, the survivor of the highest level, lowest slot among equals,
 *       takes over and `max_level` becomes its level
 *    5. has_tombstones = 0, size = survivors
 *    6. nothing removed: nothing happens, nothing is allocated; everything removed: an empty index that still takes `extend`
 *    7. rows move IN PLACE in ascending chunks through a staging buffer of `staging_bytes`: new slot ≤ old slot, so a chunk's
 *       destination ends no later than its last source and no later chunk's source is overwritten. The graph arrays (4 bytes a
 *       cell) get a second copy for the duration of the call; the matrix never does and keeps the placement it has.
 *    8. `nbr0_rows` and the sketch are made anew by the code that makes them at load time (the sketch's directions are sampled at
 *       slots that depend on the size: moved records would not equal a fresh load's)
 */
#pragma once
#include <cstddef>
#include <cstdint>

namespace usearch_amd {

/// Members per workgroup of the liveness scan (compact.hip): 256 threads × 4 members.
constexpr std::uint32_t compact_scan_chunk_k = 1024;
/// Staging buffer of the row mover when the caller does not say: 64 MiB, 43 690 rows of the headline's 1 536 bytes a chunk —
/// large enough that the two launches per chunk vanish behind the copy, small next to any index worth compacting.
constexpr std::size_t compact_default_staging_bytes_k = (std::size_t)64 << 20;

struct compact_config_t {
    std::size_t staging_bytes = 0; ///< bound of the row mover's staging buffer; 0 = compact_default_staging_bytes_k; at least one row is staged
};

struct compact_stats_t {
    std::uint64_t pruned_edges = 0;    ///< list cells erased because they named a removed member
    std::uint64_t removed_members = 0; ///< members dropped (`compact`) / members whose key is `free_key_k` (`isolate`)
    std::uint64_t survivors = 0;
    std::uint64_t moved_bytes = 0;     ///< bytes of stored rows that changed place
    std::uint64_t chunks = 0;          ///< staging chunks the rows took
    std::uint32_t new_entry_slot = 0, new_max_level = 0;
    float scan_ms = 0.f, lists_ms = 0.f, rows_ms = 0.f;
};

} // namespace usearch_amd
