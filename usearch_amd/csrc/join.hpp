/**
 *  usearch_amd/csrc/join.hpp — semantic join of two snapshots: the man-optimal stable matching of `unum::usearch::join`
 *  (the reference's include/usearch/index.hpp:4359-4545) as a batch of searches plus rounds of matching kernels (join.hip).
 *
 *  The reference pops one free man at a time from a mutex-guarded queue and runs one search per proposal. Here:
 *    - one search per man gives his whole preference list: the beam runs with ef = max(expansion, k) and keeps k results
 *      (index.hpp:3049-3068), so for every i <= expansion, search(k = i) is the first i rows of search(k = min(P, expansion));
 *      proposals beyond `expansion` get a search of their own with k = i, one batch per distinct i (the beam widens with i);
 *    - every free man proposes at once, each woman keeps the best offer: with strict preferences man-proposing deferred
 *      acceptance ends in the same man-optimal stable matching whatever the order of proposals.
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace usearch_amd {

struct join_config_t {
    std::uint64_t max_proposals = 0; ///< P; 0 = log(men) + threads (index.hpp:4390-4391), capped at the men's size
    std::uint64_t expansion = 0;     ///< ef of every list search; 0 = 64
    bool exact = false;              ///< lists from the bit-exact brute-force scan instead of the walk
    std::uint64_t threads = 1;       ///< the `executor.size()` term of the default P
};

struct join_stats_t {
    std::uint64_t pairs = 0;
    std::uint64_t rounds = 0;             ///< matching rounds (propose → resolve → requeue)
    std::uint64_t proposals = 0;          ///< offers made, over all rounds
    std::uint64_t engagements = 0;        ///< offers a woman accepted (intermediate engagements of one round are never made)
    std::uint64_t visited_members = 0;    ///< sums over the list searches (one search stands for i of the reference's)
    std::uint64_t computed_distances = 0;
    std::uint64_t max_proposals = 0;      ///< P after the default and the cap
    std::uint64_t expansion = 0;
    std::uint64_t list_width = 0;         ///< entries per man of the first list search: P exact, min(P, expansion) otherwise
    std::uint64_t lazy_searches = 0;      ///< searches for proposals beyond `expansion`
    std::uint32_t a_proposes = 1;         ///< 0 = the roles swapped: `b` was the smaller and proposed
    std::uint32_t frontier = 0;           ///< frontier of the first list search (1 = heap, 2 = open cells of `top`; 0 exact)
    double seconds_lists = 0, seconds_matching = 0;
};

/// Joins `a` with `b`: `a_keys[j]` ↔ `b_keys[j]`, in ascending order of `a`'s slots. Tombstoned members take no part on either
/// side. Returns nullptr or a static message.
const char* join_snapshots(snapshot_t& a, snapshot_t& b, const join_config_t& config, std::vector<std::uint64_t>& a_keys,
                           std::vector<std::uint64_t>& b_keys, join_stats_t* stats);

} // namespace usearch_amd
