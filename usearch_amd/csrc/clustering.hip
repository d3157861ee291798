/**
 *  usearch_amd/csrc/clustering.hip — `index_dense_gt::cluster` of a batch by the index's own levels on the device (clustering.hpp
 *  has the rules). Between the first descent and the copy-out nothing but three numbers per mapping pass reaches the host.
 *
 *    levels  starts of the upper-level lists → every member's level → one count per level (integer atomics); the host reads
 *            `max_level + 1` numbers and picks the level
 *    map     the search kernel's descent (`descent_only`, `emit_slots`) into device buffers
 *    count   u32 atomic counts per centroid slot; the non-zero cells are collected, then RANKED by (popularity ↓, key ↑, slot ↑):
 *            every entry counts the entries that precede it — U² comparisons, no atomics, one defined order. The host reads U and
 *            the two counters.
 *    merge   two launches a cycle on the snapshot's stream, nobody waits in between:
 *              1. the kernel behind `usearch_amd_distances` measures the source's stored row against the candidates, 64 to a wave
 *                 (the `queries` stride is 0: every wave stages the same row), into one float per position
 *              2. one workgroup picks the winner as the minimum of (order-preserving bits of the distance << 32 | position) over the
 *                 values below FLT_MAX — nothing below it: the initial cell, which names position 0 —, adds the popularities, moves
 *                 the target forward, shortens the order and stages the next source's row
 *            No float atomics and no atomics at all in here: two runs leave identical bytes.
 *    trace   a thread per query follows `merged_into` through a slot-indexed table; the closing distances go through the distance
 *            kernel again, one row per query
 */
#include "clustering.hpp"

#include <cfloat>
#include <chrono>
#include <cstring>
#include <mutex>

#include "casts.hpp"
#include "device_math.hpp"
#include "device_scratch.hpp"
#include "engine.hpp"
#include "host_util.hpp"
#include "search_plan.hpp"

namespace usearch_amd {

namespace {

using u32 = std::uint32_t;
using u64 = std::uint64_t;

/// What a mapping pass hands back to the host.
struct clustering_totals_t {
    unsigned long long visited, computed;
    u32 unique, live;
};

/// counts[l] = members of level exactly l, for l ≥ 1 (level 0 is everybody else): lists of one member are consecutive, the run up
/// to the next start is its level.
__global__ void clustering_level_counts_kernel(const u32* upper_ref, const std::uint8_t* starts, u64 members, u64 lists, u32 top_level,
                                               u32* counts) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= members)
        return;
    const u32 first = upper_ref[i];
    if (first == none_slot_k || first >= lists)
        return;
    u32 level = 1;
    while (first + (u64)level < lists && !starts[first + level])
        ++level;
    atomicAdd(&counts[level < top_level ? level : top_level], 1u);
}

/// dense[q] = the stored row of member slots[q].
__global__ void clustering_gather_rows_kernel(const std::uint8_t* rows, u32 row_stride, const u32* slots, u64 count, u32 bytes,
                                              std::uint8_t* dense) {
    const u64 total = count * bytes;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < total; i += gridDim.x * (u64)blockDim.x) {
        const u64 q = i / bytes, b = i - q * bytes;
        dense[i] = rows[(u64)slots[q] * row_stride + b];
    }
}

/// One count per centroid slot, and the sums of the two per-query counters of this pass.
__global__ __launch_bounds__(256) void clustering_histogram_kernel(const u64* slots, const u64* visited, const u64* computed, u64 count,
                                                                    u64 members, u32* histogram, clustering_totals_t* totals) {
    __shared__ unsigned long long sums[2];
    if (threadIdx.x < 2)
        sums[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long v = 0, c = 0;
    for (u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x; q < count; q += gridDim.x * (u64)blockDim.x) {
        const u64 slot = slots[q];
        if (slot < members)
            atomicAdd(&histogram[slot], 1u);
        v += visited[q], c += computed[q];
    }
    atomicAdd(&sums[0], v), atomicAdd(&sums[1], c); // LDS: integer sums, any order
    __syncthreads();
    if (threadIdx.x == 0)
        atomicAdd(&totals->visited, sums[0]), atomicAdd(&totals->computed, sums[1]);
}

/// The non-zero cells of the histogram, in whatever order the waves arrive: the ranking below is what orders them.
__global__ void clustering_collect_kernel(const u32* histogram, u64 members, u32 capacity, u32* found_slots, u32* found_popularity,
                                          clustering_totals_t* totals) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    const u32 popularity = i < members ? histogram[i] : 0;
    const u64 mask = __ballot(popularity != 0);
    if (!mask)
        return;
    const u32 lane = threadIdx.x & 63;
    u32 base = 0;
    if (lane == (u32)__ffsll((long long)mask) - 1)
        base = atomicAdd(&totals->unique, (u32)__popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1);
    if (popularity) {
        const u32 at = base + (u32)__popcll(mask & ((1ull << lane) - 1));
        if (at < capacity)
            found_slots[at] = (u32)i, found_popularity[at] = popularity;
    }
}

/**
 *  Entry e of the order = the found cell that e others precede under (popularity ↓, key ↑, slot ↑). Writes the entry tables, the
 *  identity order, `merged_into` = none, the slot → entry table over the histogram's cells, and pads the positions' slots up to a
 *  multiple of 64 with a valid slot (the distance kernel measures whole tiles).
 */
__global__ __launch_bounds__(256) void clustering_rank_kernel(const u32* found_slots, const u32* found_popularity, const u64* keys, u32 unique,
                                                               u32 padded, u32* entry_slot, u64* entry_key, u32* popularity, u32* merged_into,
                                                               u32* order, u32* position_slot, u32* slot_to_entry) {
    __shared__ u32 tile_slot[256], tile_popularity[256];
    __shared__ u64 tile_key[256];
    const u32 i = blockIdx.x * 256 + threadIdx.x;
    const bool mine = i < unique;
    const u32 my_slot = mine ? found_slots[i] : 0, my_popularity = mine ? found_popularity[i] : 0;
    const u64 my_key = mine ? keys[my_slot] : 0;
    u32 rank = 0;
    for (u32 base = 0; base < unique; base += 256) {
        const u32 j = base + threadIdx.x;
        if (j < unique) {
            tile_slot[threadIdx.x] = found_slots[j], tile_popularity[threadIdx.x] = found_popularity[j];
            tile_key[threadIdx.x] = keys[tile_slot[threadIdx.x]];
        }
        __syncthreads();
        const u32 here = unique - base < 256 ? unique - base : 256;
        if (mine)
            for (u32 t = 0; t < here; ++t) {
                const u32 p = tile_popularity[t];
                const u64 k = tile_key[t];
                rank += p > my_popularity || (p == my_popularity && (k < my_key || (k == my_key && tile_slot[t] < my_slot)));
            }
        __syncthreads();
    }
    if (mine) {
        entry_slot[rank] = my_slot, entry_key[rank] = my_key, popularity[rank] = my_popularity, merged_into[rank] = none_slot_k;
        order[rank] = rank, position_slot[rank] = my_slot, slot_to_entry[my_slot] = rank;
        if (rank == 0)
            for (u32 p = unique; p < padded; ++p)
                position_slot[p] = my_slot;
    }
}

/// Copies the stored row of the last entry of the order to where the distance kernel reads its query.
__device__ void stage_source_row(const std::uint8_t* rows, u32 row_stride, u32 bytes, u32 slot, std::uint8_t* query_row) {
    for (u32 b = threadIdx.x; b < bytes; b += blockDim.x)
        query_row[b] = rows[(u64)slot * row_stride + b];
}

__global__ __launch_bounds__(256) void clustering_first_source_kernel(const std::uint8_t* rows, u32 row_stride, u32 bytes, const u32* order,
                                                                       const u32* entry_slot, const clustering_totals_t* totals,
                                                                       std::uint8_t* query_row) {
    const u32 live = totals->live;
    if (live)
        stage_source_row(rows, row_stride, bytes, entry_slot[order[live - 1]], query_row);
}

__device__ u64 block_min(u64 value, u64* cells) {
    cells[threadIdx.x] = value;
    __syncthreads();
    for (u32 step = 128; step; step >>= 1) {
        if (threadIdx.x < step && cells[threadIdx.x + step] < cells[threadIdx.x])
            cells[threadIdx.x] = cells[threadIdx.x + step];
        __syncthreads();
    }
    const u64 result = cells[0];
    __syncthreads();
    return result;
}

/**
 *  One merge cycle after its distances are in `distance[0 … live − 1)`: rule 6 of clustering.hpp. One workgroup of 256.
 */
__global__ __launch_bounds__(256) void clustering_merge_kernel(const std::uint8_t* rows, u32 row_stride, u32 bytes, const float* distance,
                                                                const u32* entry_slot, u32* popularity, u32* merged_into, u32* order,
                                                                u32* position_slot, clustering_totals_t* totals, std::uint8_t* query_row) {
    __shared__ u64 cells[256];
    const u32 live = totals->live;
    if (live < 2)
        return;
    const u32 candidates = live - 1;
    // the nearest candidate: strict `<` from FLT_MAX, the first of equals; what is not below FLT_MAX never beats the initial cell
    u64 best = 0xFFFFFFFF00000000ull;
    for (u32 p = threadIdx.x; p < candidates; p += 256) {
        const float d = distance[p];
        if (d < FLT_MAX) {
            const u64 cell = ((u64)ordered_bits(d + 0.f) << 32) | p; // (+ 0.f: −0 → +0, they compare equal)
            best = cell < best ? cell : best;
        }
    }
    const u32 target_position = (u32)block_min(best, cells);
    const u32 source = order[live - 1], target = order[target_position];
    const u32 merged_popularity = popularity[target] + popularity[source];
    __syncthreads();
    if (threadIdx.x == 0)
        merged_into[source] = target, popularity[target] = merged_popularity, popularity[source] = 0;
    // the target moves forward while the entry before it is strictly less popular: the order is non-increasing, so it lands on the
    // first position whose entry is less popular than it has become, and what lay between moves back by one
    u64 first_less = target_position;
    for (u32 p = threadIdx.x; p < target_position; p += 256)
        if (popularity[order[p]] < merged_popularity) {
            first_less = p;
            break; // positions rise with the loop: the first hit is this thread's lowest
        }
    const u32 landing = (u32)block_min(first_less, cells);
    for (u32 high = target_position; high > landing;) { // from the back, a tile at a time: read, wait, write one further
        const u32 low = high - landing > 256 ? high - 256 : landing;
        const u32 p = low + threadIdx.x;
        u32 entry = 0, slot = 0;
        if (p < high)
            entry = order[p], slot = position_slot[p];
        __syncthreads();
        if (p < high)
            order[p + 1] = entry, position_slot[p + 1] = slot;
        __syncthreads();
        high = low;
    }
    if (threadIdx.x == 0) {
        order[landing] = target, position_slot[landing] = entry_slot[target];
        totals->live = live - 1;
    }
    __syncthreads();
    if (live - 1 >= 2)
        stage_source_row(rows, row_stride, bytes, entry_slot[order[live - 2]], query_row);
}

/// No merges: the centroid a query reached is its cluster.
__global__ void clustering_keys_kernel(const u64* slots, const u64* keys, u64 count, u64 members, u64* out) {
    const u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (q < count)
        out[q] = slots[q] < members ? keys[slots[q]] : 0;
}

/// Rule 7: follow `merged_into` to an entry that was not merged.
__global__ void clustering_trace_kernel(const u64* slots, const u32* slot_to_entry, const u32* merged_into, const u32* entry_slot,
                                        const u64* entry_key, u64 count, u64 members, u32 unique, u32* final_slots, u64* out_keys) {
    const u64 q = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (q >= count)
        return;
    u32 entry = slots[q] < members ? slot_to_entry[slots[q]] : 0;
    for (u32 hop = 0; hop < unique && entry < unique && merged_into[entry] != none_slot_k; ++hop) // a chain is shorter than U
        entry = merged_into[entry];
    entry = entry < unique ? entry : 0;
    final_slots[q] = entry_slot[entry];
    out_keys[q] = entry_key[entry];
}

float seconds_since(std::chrono::steady_clock::time_point start) {
    return std::chrono::duration<float>(std::chrono::steady_clock::now() - start).count();
}

} // namespace

const char* snapshot_t::clustering(const void* queries, scalar_kind_t query_kind, std::size_t count, std::size_t stride_bytes,
                                   const std::uint32_t* member_slots, const clustering_config_t& config_in, std::uint64_t* keys,
                                   float* distances, clustering_stats_t* stats_out) {
    clustering_stats_t stats{};
    clustering_config_t config = config_in;
    if (config.min_clusters && !config.max_clusters)
        return "Clustering needs max_clusters when min_clusters is set";
    if (count >= none_slot_k)
        return "Batch is too large";
    if (!queries && multi_)
        return "Clustering by member keys is not available for a multi-index";
    {
        std::lock_guard<std::mutex> lock(pool_mutex_);
        if (placing_ || idle_.size() != workspaces_.size())
            return "The index is being searched: clustering needs it to itself";
    }
    const u64 n = view_.size;
    const u32 top_level = n ? view_.max_level : 0;
    UA_HIP(hipSetDevice(device_));
    device_scratch_t scratch(device_);

    // ---- the level (rule 1)
    std::vector<u64> at_or_above(top_level + 2, 0);
    if (n && top_level) {
        const u64 lists = upper_lists_;
        std::uint8_t* d_starts = nullptr;
        u32* d_counts = nullptr;
        UA_HIP(scratch.allocate(&d_starts, lists));
        UA_HIP(scratch.allocate(&d_counts, (std::size_t)(top_level + 1) * 4));
        UA_HIP(hipMemsetAsync(d_counts, 0, (std::size_t)(top_level + 1) * 4, stream_));
        const unsigned member_blocks = (unsigned)((n + 255) / 256);
        if (const char* e = mark_list_starts(view_.upper_ref, n, lists, d_starts, stream_))
            return e;
        hipLaunchKernelGGL(clustering_level_counts_kernel, dim3(member_blocks), dim3(256), 0, stream_, view_.upper_ref, d_starts, n, lists,
                           top_level, d_counts);
        UA_HIP(hipGetLastError());
        std::vector<u32> exactly(top_level + 1, 0);
        UA_HIP(hipMemcpyAsync(exactly.data(), d_counts, (std::size_t)(top_level + 1) * 4, hipMemcpyDeviceToHost, stream_));
        UA_HIP(hipStreamSynchronize(stream_));
        for (u32 l = top_level; l >= 1; --l)
            at_or_above[l] = at_or_above[l + 1] + exactly[l];
    }
    at_or_above[0] = n;
    u32 level = top_level;
    if (config.min_clusters) {
        for (; level > 1; --level)
            if (at_or_above[level] > config.min_clusters)
                break;
    } else {
        level = 1, config.max_clusters = top_level ? at_or_above[1] : 0, config.min_clusters = 2;
    }
    if (top_level < 2)
        return "Index too small to cluster!";
    stats.level = level;
    if (!count) {
        if (stats_out)
            *stats_out = stats;
        return nullptr;
    }
    if (!keys || !distances)
        return "Clustering needs the key and distance buffers";

    // ---- the queries, in the storage kind, on the device
    const std::size_t bpv = view_.bytes_per_vector, dims = view_.dimensions;
    const std::uint8_t* d_queries = nullptr;
    std::size_t d_stride = bpv;
    if (queries) {
        if (query_kind != scalar_ && bytes_per_vector(query_kind, dims) == 0)
            return "Unsupported query scalar kind";
        std::vector<std::uint8_t> dense(count * bpv, 0);
        const std::uint8_t* source = static_cast<const std::uint8_t*>(queries);
        parallel_ranges(count, [&](u64 begin, u64 end) {
            for (u64 q = begin; q < end; ++q)
                if (!cast_vector(query_kind, scalar_, source + q * stride_bytes, dims, dense.data() + q * bpv))
                    std::memcpy(dense.data() + q * bpv, source + q * stride_bytes, bpv);
        });
        std::uint8_t* d_dense = nullptr;
        UA_HIP(scratch.allocate(&d_dense, count * bpv + 256));
        UA_HIP(hipMemcpyAsync(d_dense, dense.data(), count * bpv, hipMemcpyHostToDevice, stream_));
        UA_HIP(hipStreamSynchronize(stream_)); // `dense` leaves with this block
        d_queries = d_dense;
    } else {
        std::vector<u32> live_slots;
        if (!member_slots) {
            if (!view_.has_tombstones) { // everybody, in slot order: the stored rows are the queries where they lie
                if (count != n)
                    return "The number of results does not match the number of members";
                d_queries = view_.vectors, d_stride = view_.row_stride;
            } else {
                std::vector<u64> host_keys(n);
                UA_HIP(hipMemcpy(host_keys.data(), view_.keys, n * 8, hipMemcpyDeviceToHost));
                for (u64 i = 0; i < n; ++i)
                    if (host_keys[i] != free_key_k)
                        live_slots.push_back((u32)i);
                if (live_slots.size() != count)
                    return "The number of results does not match the number of members";
                member_slots = live_slots.data();
            }
        }
        if (!d_queries) {
            for (std::size_t q = 0; q < count; ++q)
                if (member_slots[q] >= n)
                    return "Key missing!";
            u32* d_slots = nullptr;
            std::uint8_t* d_dense = nullptr;
            UA_HIP(scratch.allocate(&d_slots, count * 4));
            UA_HIP(scratch.allocate(&d_dense, count * bpv + 256));
            UA_HIP(hipMemcpyAsync(d_slots, member_slots, count * 4, hipMemcpyHostToDevice, stream_));
            hipLaunchKernelGGL(clustering_gather_rows_kernel, dim3(blocks_for(count * bpv, compute_units_)), dim3(256), 0, stream_, view_.vectors,
                               view_.row_stride, d_slots, (u64)count, (u32)bpv, d_dense);
            UA_HIP(hipGetLastError());
            UA_HIP(hipStreamSynchronize(stream_)); // `live_slots` leaves with this block
            d_queries = d_dense;
        }
    }

    // ---- device state of the call
    u64 *d_reached = nullptr, *d_counts = nullptr, *d_visited = nullptr, *d_computed = nullptr, *d_out_keys = nullptr;
    float* d_distances = nullptr;
    u32 *d_histogram = nullptr, *d_found_slots = nullptr, *d_found_popularity = nullptr;
    clustering_totals_t* d_totals = nullptr;
    const u64 most_entries = std::min<u64>(n, count);
    UA_HIP(scratch.allocate(&d_reached, count * 8));
    UA_HIP(scratch.allocate(&d_counts, count * 8));
    UA_HIP(scratch.allocate(&d_visited, count * 8));
    UA_HIP(scratch.allocate(&d_computed, count * 8));
    UA_HIP(scratch.allocate(&d_out_keys, count * 8));
    UA_HIP(scratch.allocate(&d_distances, count * 4));
    UA_HIP(scratch.allocate(&d_histogram, n * 4));
    UA_HIP(scratch.allocate(&d_found_slots, most_entries * 4));
    UA_HIP(scratch.allocate(&d_found_popularity, most_entries * 4));
    UA_HIP(scratch.allocate(&d_totals, sizeof(clustering_totals_t)));
    UA_HIP(hipMemsetAsync(d_totals, 0, sizeof(clustering_totals_t), stream_));

    // ---- map, count, refine (rules 2 - 4)
    auto started = std::chrono::steady_clock::now();
    clustering_totals_t totals{};
    for (;;) {
        search_extras_t extras;
        extras.descent_only = true, extras.emit_slots = true;
        extras.beam_level = level - 1;
        search_stats_t search_stats;
        if (const char* e = search_device(d_queries, count, d_stride, 1, 1, d_reached, d_distances, d_counts, d_visited, d_computed, stream_,
                                          search_tuning_t{}, &search_stats, false, &extras))
            return e;
        ++stats.mapping_passes;
        UA_HIP(hipMemsetAsync(d_histogram, 0, std::max<std::size_t>(n * 4, 16), stream_));
        UA_HIP(hipMemsetAsync(&d_totals->unique, 0, 4, stream_));
        hipLaunchKernelGGL(clustering_histogram_kernel, dim3(blocks_for(count, compute_units_)), dim3(256), 0, stream_, d_reached, d_visited,
                           d_computed, (u64)count, n, d_histogram, d_totals);
        UA_HIP(hipGetLastError());
        hipLaunchKernelGGL(clustering_collect_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, d_histogram, n, (u32)most_entries,
                           d_found_slots, d_found_popularity, d_totals);
        UA_HIP(hipGetLastError());
        UA_HIP(hipMemcpyAsync(&totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, stream_));
        UA_HIP(hipStreamSynchronize(stream_));
        if (totals.unique > most_entries)
            return "The index is inconsistent: more centroids than queries";
        if (totals.unique < config.min_clusters && level > 1) {
            --level;
            continue;
        }
        break;
    }
    const u32 unique = totals.unique;
    stats.level = level;
    stats.unique_before_merge = unique;
    stats.visited_members = totals.visited, stats.computed_distances = totals.computed;
    stats.seconds_map = seconds_since(started);
    const u64 cycles = unique > config.max_clusters ? unique - config.max_clusters : 0;
    stats.merge_cycles = cycles;
    stats.clusters = unique - cycles;

    if (!cycles) {
        hipLaunchKernelGGL(clustering_keys_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream_, d_reached, view_.keys, (u64)count,
                           n, d_out_keys);
        UA_HIP(hipGetLastError());
    } else {
        // ---- order and merge (rules 5, 6)
        started = std::chrono::steady_clock::now();
        const u32 padded = (unique + 63) & ~63u;
        u32 *d_entry_slot = nullptr, *d_popularity = nullptr, *d_merged_into = nullptr, *d_order = nullptr, *d_position_slot = nullptr;
        u64* d_entry_key = nullptr;
        float* d_merge_distance = nullptr;
        std::uint8_t* d_query_row = nullptr;
        UA_HIP(scratch.allocate(&d_entry_slot, (std::size_t)unique * 4));
        UA_HIP(scratch.allocate(&d_popularity, (std::size_t)unique * 4));
        UA_HIP(scratch.allocate(&d_merged_into, (std::size_t)unique * 4));
        UA_HIP(scratch.allocate(&d_order, (std::size_t)padded * 4));
        UA_HIP(scratch.allocate(&d_position_slot, (std::size_t)padded * 4));
        UA_HIP(scratch.allocate(&d_entry_key, (std::size_t)unique * 8));
        UA_HIP(scratch.allocate(&d_merge_distance, (std::size_t)padded * 4));
        UA_HIP(scratch.allocate(&d_query_row, (std::size_t)view_.row_stride + 256));
        UA_HIP(hipMemsetAsync(d_query_row, 0, (std::size_t)view_.row_stride + 256, stream_));
        hipLaunchKernelGGL(clustering_rank_kernel, dim3((unique + 255) / 256), dim3(256), 0, stream_, d_found_slots, d_found_popularity, view_.keys,
                           unique, padded, d_entry_slot, d_entry_key, d_popularity, d_merged_into, d_order, d_position_slot, d_histogram);
        UA_HIP(hipGetLastError());
        UA_HIP(hipMemcpyAsync(&d_totals->live, &unique, 4, hipMemcpyHostToDevice, stream_));
        hipLaunchKernelGGL(clustering_first_source_kernel, dim3(1), dim3(256), 0, stream_, view_.vectors, view_.row_stride, (u32)bpv, d_order,
                           d_entry_slot, d_totals, d_query_row);
        UA_HIP(hipGetLastError());
        distances_params_t p{};
        p.metric = metric_;
        p.lanes = lanes_;
        p.lds_bytes = view_.chunks * (query_chunk_bytes_of(scalar_)) + 512;
        p.stream = stream_;
        p.queries = d_query_row;
        p.query_stride = 0; // every wave measures against the same row: the source's
        p.slots = d_position_slot;
        p.slots_per_query = 64;
        p.out = d_merge_distance;
        for (u64 cycle = 0; cycle < cycles; ++cycle) {
            const u32 candidates = unique - (u32)cycle - 1;
            p.count = (candidates + 63) / 64;
            UA_HIP(launch_distances(metric_, scalar_, p, view_));
            hipLaunchKernelGGL(clustering_merge_kernel, dim3(1), dim3(256), 0, stream_, view_.vectors, view_.row_stride, (u32)bpv, d_merge_distance,
                               d_entry_slot, d_popularity, d_merged_into, d_order, d_position_slot, d_totals, d_query_row);
            UA_HIP(hipGetLastError());
        }
        UA_HIP(hipStreamSynchronize(stream_));
        stats.seconds_merge = seconds_since(started);

        // ---- trace (rule 7)
        started = std::chrono::steady_clock::now();
        u32* d_final_slots = nullptr;
        UA_HIP(scratch.allocate(&d_final_slots, count * 4));
        hipLaunchKernelGGL(clustering_trace_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream_, d_reached, d_histogram,
                           d_merged_into, d_entry_slot, d_entry_key, (u64)count, n, unique, d_final_slots, d_out_keys);
        UA_HIP(hipGetLastError());
        // one wave per query for ONE row each: the kernel as `usearch_amd_distances` launches it, hence its bits; 1M workgroups for 1M
        // queries is launch-bound work (0.6 ms there, profiles/r10_clustering/) that a kernel measuring 64 (query, row) pairs a wave
        // would shorten
        distances_params_t closing = p;
        closing.queries = d_queries;
        closing.query_stride = d_stride;
        closing.slots = d_final_slots;
        closing.slots_per_query = 1;
        closing.count = (u32)count;
        closing.out = d_distances;
        UA_HIP(launch_distances(metric_, scalar_, closing, view_));
        UA_HIP(hipStreamSynchronize(stream_));
        stats.seconds_trace = seconds_since(started);
    }
    UA_HIP(hipMemcpyAsync(keys, d_out_keys, count * 8, hipMemcpyDeviceToHost, stream_));
    UA_HIP(hipMemcpyAsync(distances, d_distances, count * 4, hipMemcpyDeviceToHost, stream_));
    UA_HIP(hipStreamSynchronize(stream_));
    if (stats_out)
        *stats_out = stats;
    return nullptr;
}

} // namespace usearch_amd
