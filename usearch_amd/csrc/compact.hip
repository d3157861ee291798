/**
 *  usearch_amd/csrc/compact.hip — `isolate` and `compact` on the device (compact.hpp has the rules): a scan over the members, one
 *  pass over the neighbour lists, one pass over the stored rows. All of it is memory-bound; nothing here computes a distance.
 *
 *    scan    liveness (key != free_key_k) and level of every member → per-chunk counts → exclusive scan over the chunks → per
 *            member: old slot → new slot, new slot → old slot, the new `upper_ref`, where each upper-level list goes
 *    lists   a wave owns whole lists: cells are loaded coalesced, looked up in the slot map, squeezed with a ballot (order kept),
 *            padded with `none_slot_k`; erased cells are counted per wave and added with one integer atomic
 *    rows    chunk by chunk in ascending new slot: gathered into the staging buffer, copied down to where they belong
 *
 *  Integer atomics only (a count, a minimum, a maximum): two runs over equal inputs leave identical bytes.
 */
#include "compact.hpp"

#include <chrono>
#include <mutex>

#include "build.hpp"
#include "device_scratch.hpp"
#include "engine.hpp"
#include "host_util.hpp"

namespace usearch_amd {

namespace {

using u32 = std::uint32_t;
using u64 = std::uint64_t;

/// What the scan kernels hand back to the host, one 64-byte block.
struct compact_totals_t {
    unsigned long long pruned;    ///< cells erased by the list kernel
    unsigned long long best;      ///< max over surviving members of (level << 32 | ~new slot): the highest level, lowest slot
    unsigned long long survivors; ///< members that stay
    unsigned long long lists;     ///< upper-level lists that stay
    u32 first_removed;            ///< lowest removed slot: rows below it do not move
    u32 removed_seen;             ///< `isolate`: members whose key is free_key_k
    u32 padding[6];
};

/// Exclusive scan of one value per thread over a workgroup of 256; `total` = the sum. Live count in the low half, list count in
/// the high half of one u64: both scans in one go (a chunk holds ≤ 1 024 members of level ≤ 32 767: neither half can carry).
__device__ u64 block_exclusive_scan(u64 value, u64* cells, u64& total) {
    const u32 t = threadIdx.x;
    cells[t] = value;
    __syncthreads();
    for (u32 step = 1; step < 256; step <<= 1) {
        const u64 below = t >= step ? cells[t - step] : 0;
        __syncthreads();
        cells[t] += below;
        __syncthreads();
    }
    total = cells[255];
    const u64 exclusive = cells[t] - value;
    __syncthreads();
    return exclusive;
}

/// starts[r] = 1 where an upper-level list is a member's first: lists of one member are consecutive and members own them in
/// slot order, so the run of lists up to the next start is the member's level.
__global__ void compact_starts_kernel(const u32* upper_ref, u64 members, u64 lists, std::uint8_t* starts) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i >= members)
        return;
    const u32 first = upper_ref[i];
    if (first != none_slot_k && first < lists)
        starts[first] = 1;
}

/// One workgroup per chunk of `compact_scan_chunk_k` members: every member's level (written out), and the chunk's survivors and
/// the upper-level lists they own.
__global__ __launch_bounds__(256) void compact_counts_kernel(const u64* keys, const u32* upper_ref, const std::uint8_t* starts,
                                                              u64 members, u64 lists, std::uint16_t* levels, u32* chunk_live,
                                                              u32* chunk_lists) {
    __shared__ u64 cells[256];
    u64 mine = 0;
    for (u32 k = 0; k < compact_scan_chunk_k / 256; ++k) {
        const u64 i = blockIdx.x * (u64)compact_scan_chunk_k + k * 256 + threadIdx.x; // coalesced: a sum does not mind the order
        if (i >= members)
            continue;
        const u32 first = upper_ref[i];
        u32 level = 0;
        if (first != none_slot_k && first < lists)
            for (level = 1; first + (u64)level < lists && !starts[first + level];)
                ++level;
        levels[i] = (std::uint16_t)level;
        if (keys[i] != free_key_k)
            mine += 1ull | ((u64)level << 32);
    }
    u64 total = 0;
    (void)block_exclusive_scan(mine, cells, total);
    if (threadIdx.x == 0)
        chunk_live[blockIdx.x] = (u32)total, chunk_lists[blockIdx.x] = (u32)(total >> 32);
}

/// One workgroup: the per-chunk counts become exclusive sums over the chunks, 256 chunks a round with a carry.
__global__ __launch_bounds__(256) void compact_chunk_scan_kernel(u32* chunk_live, u32* chunk_lists, u32 chunks, compact_totals_t* totals) {
    __shared__ u64 cells[256];
    u64 carry_live = 0, carry_lists = 0;
    for (u32 base = 0; base < chunks; base += 256) {
        const u32 c = base + threadIdx.x;
        u64 total = 0;
        const u64 live = c < chunks ? chunk_live[c] : 0;
        const u64 before_live = block_exclusive_scan(live, cells, total);
        const u64 round_live = total;
        const u64 own_lists = c < chunks ? chunk_lists[c] : 0;
        const u64 before_lists = block_exclusive_scan(own_lists, cells, total);
        if (c < chunks)
            chunk_live[c] = (u32)(carry_live + before_live), chunk_lists[c] = (u32)(carry_lists + before_lists);
        carry_live += round_live, carry_lists += total;
    }
    if (threadIdx.x == 0)
        totals->survivors = carry_live, totals->lists = carry_lists;
}

/// One workgroup per chunk, a thread per 4 consecutive members: the renumbering itself. Survivors get their rank; their key, their
/// `upper_ref` and the destination of each of their upper-level lists are written at the new slot; removed members get `none_slot_k`
/// and so do their lists.
__global__ __launch_bounds__(256) void compact_apply_kernel(const u64* keys, const u32* upper_ref, const std::uint16_t* levels,
                                                             u64 members, const u32* chunk_live, const u32* chunk_lists,
                                                             u32* slot_map, u32* old_of, u64* new_keys, u32* new_upper_ref,
                                                             u32* list_target, compact_totals_t* totals) {
    __shared__ u64 cells[256];
    __shared__ u32 lowest_removed;
    __shared__ unsigned long long tallest;
    if (threadIdx.x == 0)
        lowest_removed = none_slot_k, tallest = 0;
    constexpr u32 per_thread = compact_scan_chunk_k / 256;
    const u64 first = blockIdx.x * (u64)compact_scan_chunk_k + threadIdx.x * per_thread;
    u64 key[per_thread];
    u32 level[per_thread];
    u64 mine = 0;
    for (u32 k = 0; k < per_thread; ++k) {
        const u64 i = first + k;
        key[k] = i < members ? keys[i] : free_key_k;
        level[k] = i < members ? levels[i] : 0;
        if (key[k] != free_key_k)
            mine += 1ull | ((u64)level[k] << 32);
    }
    u64 total = 0;
    const u64 before = block_exclusive_scan(mine, cells, total); // also orders the writes of `lowest_removed` and `tallest` before their use
    u32 next_slot = chunk_live[blockIdx.x] + (u32)before;
    u32 next_list = chunk_lists[blockIdx.x] + (u32)(before >> 32);
    for (u32 k = 0; k < per_thread; ++k) {
        const u64 i = first + k;
        if (i >= members)
            break;
        const u32 old_first = upper_ref[i];
        if (key[k] != free_key_k) {
            slot_map[i] = next_slot;
            old_of[next_slot] = (u32)i;
            new_keys[next_slot] = key[k];
            new_upper_ref[next_slot] = level[k] ? next_list : none_slot_k;
            for (u32 l = 0; l < level[k]; ++l)
                list_target[old_first + l] = next_list + l;
            if (level[k]) // settled in LDS: one atomic per workgroup reaches memory
                atomicMax(&tallest, ((unsigned long long)level[k] << 32) | (0xFFFFFFFFu - next_slot));
            ++next_slot;
            next_list += level[k];
        } else {
            slot_map[i] = none_slot_k;
            for (u32 l = 0; l < level[k]; ++l)
                list_target[old_first + l] = none_slot_k;
            atomicMin(&lowest_removed, (u32)i);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && lowest_removed != none_slot_k)
        atomicMin(&totals->first_removed, lowest_removed);
    if (threadIdx.x == 0 && tallest)
        atomicMax(&totals->best, tallest);
}

/// keys[slots[i]] = free_key_k: `remove` in bulk.
__global__ void compact_tombstones_kernel(const u32* slots, u64 count, u64 members, u64* keys) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    if (i < count && slots[i] < members)
        keys[slots[i]] = free_key_k;
}

/// `isolate` renumbers nobody: the map is the identity over the members that stay.
__global__ void compact_identity_kernel(const u64* keys, u64 members, u32* slot_map, compact_totals_t* totals) {
    const u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x;
    const bool removed = i < members && keys[i] == free_key_k;
    if (i < members)
        slot_map[i] = removed ? none_slot_k : (u32)i;
    const u32 count = (u32)__popcll(__ballot(removed));
    if (count && (threadIdx.x & 63) == 0)
        atomicAdd(&totals->removed_seen, count);
}

/**
 *  The list kernel of both operations. List `l` of `source` (`width` cells, prefix-compact, `none_slot_k` padding) is written to
 *  list `targets[l]` of `destination` (`targets` null: to list `l`; `none_slot_k`: nowhere — its owner is leaving) with every cell
 *  sent through `slot_map`; cells that map to `none_slot_k` are erased, the others close up in order, the tail is padded.
 *  `source == destination` with no `targets` is `isolate` in place: a wave reads every cell of a tile before it writes one, and
 *  what it writes lies at or below what it has read.
 *  Lists narrower than a wave share one: ⌊64 / width⌋ lists side by side, each squeezed inside its own segment of the ballot.
 */
__global__ __launch_bounds__(256) void compact_lists_kernel(const u32* source, u32* destination, u32 width, u64 lists, const u32* targets,
                                                             const u32* slot_map, u64 members, compact_totals_t* totals) {
    const u32 lane = threadIdx.x & 63;
    const u64 wave = (blockIdx.x * (u64)blockDim.x + threadIdx.x) >> 6, waves = (gridDim.x * (u64)blockDim.x) >> 6;
    u32 erased_here = 0; // wave-uniform
    if (width < 64) {
        const u32 per_wave = 64 / width;
        const u32 segment = lane / width, j = lane - segment * width;
        const u64 segment_mask = ((1ull << width) - 1) << (segment * width);
        const u64 tasks = (lists + per_wave - 1) / per_wave;
        for (u64 task = wave; task < tasks; task += waves) {
            const u64 list = task * per_wave + segment;
            const bool active = segment < per_wave && list < lists;
            u32 target = none_slot_k, cell = none_slot_k, mapped = none_slot_k;
            if (active) {
                target = targets ? targets[list] : (u32)list;
                cell = source[list * width + j];
            }
            if (cell != none_slot_k && cell < members)
                mapped = slot_map[cell];
            const bool keep = mapped != none_slot_k;
            const u64 kept_mask = __ballot(keep) & segment_mask;
            erased_here += (u32)__popcll(__ballot(cell != none_slot_k && !keep));
            const u32 rank = (u32)__popcll(kept_mask & ((1ull << lane) - 1)), kept = (u32)__popcll(kept_mask);
            if (active && target != none_slot_k) {
                u32* out = destination + (u64)target * width;
                if (keep)
                    out[rank] = mapped;
                if (j >= kept)
                    out[j] = none_slot_k;
            }
        }
    } else {
        for (u64 list = wave; list < lists; list += waves) {
            const u32 target = targets ? targets[list] : (u32)list; // wave-uniform
            const u32* in = source + list * width;
            u32* out = destination + (u64)target * width;
            u32 kept = 0;
            for (u32 tile = 0; tile < width; tile += 64) { // order is kept across tiles: `kept` carries over
                const u32 j = tile + lane;
                u32 cell = j < width ? in[j] : none_slot_k, mapped = none_slot_k;
                if (cell != none_slot_k && cell < members)
                    mapped = slot_map[cell];
                const bool keep = mapped != none_slot_k;
                const u64 kept_mask = __ballot(keep);
                erased_here += (u32)__popcll(__ballot(cell != none_slot_k && !keep));
                if (keep && target != none_slot_k)
                    out[kept + (u32)__popcll(kept_mask & ((1ull << lane) - 1))] = mapped;
                kept += (u32)__popcll(kept_mask);
            }
            if (target != none_slot_k)
                for (u32 j = kept + lane; j < width; j += 64)
                    out[j] = none_slot_k;
        }
    }
    if (erased_here && lane == 0)
        atomicAdd(&totals->pruned, (unsigned long long)erased_here);
}

/// staging[r] = rows[old_of[first + r]] for r < count, 16 bytes a thread: consecutive threads read consecutive 16-byte units of
/// one row and write consecutive units of the staging buffer.
__global__ void compact_gather_rows_kernel(const uint4* rows, const u32* old_of, u64 first, u64 count, u32 units_per_row, uint4* staging) {
    const u64 total = count * units_per_row;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < total; i += gridDim.x * (u64)blockDim.x) {
        const u64 r = i / units_per_row, unit = i - r * units_per_row;
        staging[i] = rows[(u64)old_of[first + r] * units_per_row + unit];
    }
}

float milliseconds_since(std::chrono::steady_clock::time_point start) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - start).count();
}

const char* launch_lists(const u32* source, u32* destination, u32 width, u64 lists, const u32* targets, const u32* slot_map, u64 members,
                         compact_totals_t* totals, int compute_units, hipStream_t stream) {
    if (!lists || !width)
        return nullptr;
    const u64 per_wave = width < 64 ? 64 / width : 1;
    const u64 waves = (lists + per_wave - 1) / per_wave;
    hipLaunchKernelGGL(compact_lists_kernel, dim3(blocks_for(waves * 64, compute_units)), dim3(256), 0, stream, source, destination, width,
                       lists, targets, slot_map, members, totals);
    UA_HIP(hipGetLastError());
    return nullptr;
}

} // namespace

const char* mark_list_starts(const std::uint32_t* upper_ref, std::uint64_t members, std::uint64_t lists, std::uint8_t* starts,
                             hipStream_t stream) {
    UA_HIP(hipMemsetAsync(starts, 0, std::max<std::size_t>(lists, 16), stream));
    if (!members)
        return nullptr;
    hipLaunchKernelGGL(compact_starts_kernel, dim3((unsigned)((members + 255) / 256)), dim3(256), 0, stream, upper_ref, members, lists, starts);
    UA_HIP(hipGetLastError());
    return nullptr;
}

const char* snapshot_t::isolate(compact_stats_t* stats_out) {
    compact_stats_t stats{};
    {
        std::lock_guard<std::mutex> lock(pool_mutex_);
        if (placing_ || idle_.size() != workspaces_.size())
            return "The index is being searched: isolate needs it to itself";
    }
    const u64 n = view_.size;
    stats.survivors = n;
    stats.new_entry_slot = view_.entry_slot, stats.new_max_level = view_.max_level;
    if (n) {
        UA_HIP(hipSetDevice(device_));
        device_scratch_t scratch(device_, release_t::placed_free);
        u32* d_map = nullptr;
        compact_totals_t* d_totals = nullptr;
        UA_HIP(scratch.allocate(&d_map, n * 4));
        UA_HIP(scratch.allocate(&d_totals, sizeof(compact_totals_t)));
        UA_HIP(hipMemsetAsync(d_totals, 0, sizeof(compact_totals_t), stream_));
        auto started = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(compact_identity_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream_, view_.keys, n, d_map, d_totals);
        UA_HIP(hipGetLastError());
        UA_HIP(hipStreamSynchronize(stream_));
        stats.scan_ms = milliseconds_since(started);
        started = std::chrono::steady_clock::now();
        view_.nbr0_rows = nullptr; // copies of the neighbours' rows in list order: made anew below
        if (const char* e = launch_lists(view_.nbr0, mutable_nbr0(), view_.m0, n, nullptr, d_map, n, d_totals, compute_units_, stream_))
            return e;
        if (const char* e = launch_lists(view_.upper, mutable_upper(), view_.m, upper_lists_, nullptr, d_map, n, d_totals, compute_units_, stream_))
            return e;
        compact_totals_t totals{};
        UA_HIP(hipMemcpyAsync(&totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, stream_));
        UA_HIP(hipStreamSynchronize(stream_));
        stats.lists_ms = milliseconds_since(started);
        stats.pruned_edges = totals.pruned;
        stats.removed_members = totals.removed_seen;
        stats.survivors = n - totals.removed_seen;
        if (const char* e = finalize_layout())
            return e;
    }
    if (stats_out)
        *stats_out = stats;
    return nullptr;
}

const char* snapshot_t::compact(const compact_config_t& config, std::uint32_t* slot_map, compact_stats_t* stats_out) {
    compact_stats_t stats{};
    {
        std::lock_guard<std::mutex> lock(pool_mutex_);
        if (placing_ || idle_.size() != workspaces_.size())
            return "The index is being searched: compact needs it to itself";
    }
    const u64 n = view_.size;
    stats.survivors = n;
    stats.new_entry_slot = view_.entry_slot, stats.new_max_level = view_.max_level;
    if (!n || !view_.has_tombstones) { // nothing was removed: nothing moves, nothing is allocated
        if (slot_map)
            for (u64 i = 0; i < n; ++i)
                slot_map[i] = (u32)i;
        if (stats_out)
            *stats_out = stats;
        return nullptr;
    }
    UA_HIP(hipSetDevice(device_));
    const u32 m = view_.m, m0 = view_.m0, row_stride = view_.row_stride;
    if (row_stride % 16)
        return "Rows are not a multiple of 16 bytes apart";
    const u64 lists = upper_lists_;
    const u64 capacity = std::max<u64>(build_capacity_, n), lists_capacity = std::max<u64>(std::max<u64>(build_lists_capacity_, lists), 1);
    const u32 chunks = (u32)((n + compact_scan_chunk_k - 1) / compact_scan_chunk_k);

    // ---- scan: who stays, where everybody goes
    auto started = std::chrono::steady_clock::now();
    device_scratch_t scratch(device_, release_t::placed_free);
    std::uint8_t* d_starts = nullptr;
    std::uint16_t* d_levels = nullptr;
    u32 *d_chunk_live = nullptr, *d_chunk_lists = nullptr, *d_map = nullptr, *d_old_of = nullptr, *d_list_target = nullptr;
    compact_totals_t* d_totals = nullptr;
    UA_HIP(scratch.allocate(&d_starts, lists));
    UA_HIP(scratch.allocate(&d_levels, n * 2));
    UA_HIP(scratch.allocate(&d_chunk_live, (std::size_t)chunks * 4));
    UA_HIP(scratch.allocate(&d_chunk_lists, (std::size_t)chunks * 4));
    UA_HIP(scratch.allocate(&d_map, n * 4));
    UA_HIP(scratch.allocate(&d_old_of, n * 4));
    UA_HIP(scratch.allocate(&d_list_target, lists * 4));
    UA_HIP(scratch.allocate(&d_totals, sizeof(compact_totals_t)));
    compact_totals_t totals{};
    totals.best = 0xFFFFFFFFull; // level 0, new slot 0: what an index of level-0 survivors elects
    totals.first_removed = none_slot_k;
    UA_HIP(hipMemcpyAsync(d_totals, &totals, sizeof(totals), hipMemcpyHostToDevice, stream_));
    // a list no member owns (there should be none) goes nowhere instead of wherever the fresh allocation points
    UA_HIP(hipMemsetAsync(d_list_target, 0xFF, std::max<std::size_t>(lists * 4, 16), stream_));
    if (const char* e = mark_list_starts(view_.upper_ref, n, lists, d_starts, stream_))
        return e;
    hipLaunchKernelGGL(compact_counts_kernel, dim3(chunks), dim3(256), 0, stream_, view_.keys, view_.upper_ref, d_starts, n, lists, d_levels,
                       d_chunk_live, d_chunk_lists);
    UA_HIP(hipGetLastError());
    hipLaunchKernelGGL(compact_chunk_scan_kernel, dim3(1), dim3(256), 0, stream_, d_chunk_live, d_chunk_lists, chunks, d_totals);
    UA_HIP(hipGetLastError());
    UA_HIP(hipMemcpyAsync(&totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, stream_));
    UA_HIP(hipStreamSynchronize(stream_));
    const u64 survivors = totals.survivors, new_lists = totals.lists;
    if (survivors > n || new_lists > lists)
        return "The index is inconsistent: more survivors than members";

    // ---- the graph arrays of the survivors: a second copy while the call lasts, as roomy as the ones they replace
    void *fresh_nbr0 = nullptr, *fresh_upper_ref = nullptr, *fresh_upper = nullptr, *fresh_keys = nullptr;
    struct fresh_t { // released unless the call gets as far as adopting them
        void** pointers[4];
        bool adopted = false;
        ~fresh_t() {
            if (!adopted)
                for (void** p : pointers)
                    if (*p)
                        placed_free(*p);
        }
    } fresh{{&fresh_nbr0, &fresh_upper_ref, &fresh_upper, &fresh_keys}};
    UA_HIP(placed_malloc(&fresh_nbr0, (std::size_t)capacity * m0 * 4, (std::size_t)m0 * 4, nullptr));
    UA_HIP(hipMalloc(&fresh_upper_ref, std::max<std::size_t>((std::size_t)capacity * 4, 16)));
    UA_HIP(hipMalloc(&fresh_upper, std::max<std::size_t>((std::size_t)lists_capacity * m * 4, 16)));
    UA_HIP(hipMalloc(&fresh_keys, std::max<std::size_t>((std::size_t)capacity * 8, 16)));
    UA_HIP(hipMemsetAsync(fresh_nbr0, 0xFF, (std::size_t)capacity * m0 * 4, stream_));
    UA_HIP(hipMemsetAsync(fresh_upper_ref, 0xFF, (std::size_t)capacity * 4, stream_));
    UA_HIP(hipMemsetAsync(fresh_upper, 0xFF, (std::size_t)lists_capacity * m * 4, stream_));
    UA_HIP(hipMemsetAsync(fresh_keys, 0, (std::size_t)capacity * 8, stream_));
    hipLaunchKernelGGL(compact_apply_kernel, dim3(chunks), dim3(256), 0, stream_, view_.keys, view_.upper_ref, d_levels, n, d_chunk_live,
                       d_chunk_lists, d_map, d_old_of, static_cast<u64*>(fresh_keys), static_cast<u32*>(fresh_upper_ref), d_list_target,
                       d_totals);
    UA_HIP(hipGetLastError());
    u32 entry_goes_to = none_slot_k;
    UA_HIP(hipMemcpyAsync(&entry_goes_to, d_map + view_.entry_slot, 4, hipMemcpyDeviceToHost, stream_));
    if (slot_map)
        UA_HIP(hipMemcpyAsync(slot_map, d_map, n * 4, hipMemcpyDeviceToHost, stream_));
    UA_HIP(hipStreamSynchronize(stream_));
    stats.scan_ms = milliseconds_since(started);

    // ---- lists: isolated and renumbered in one pass, level 0 and the levels above
    started = std::chrono::steady_clock::now();
    if (const char* e = launch_lists(view_.nbr0, static_cast<u32*>(fresh_nbr0), m0, n, d_map, d_map, n, d_totals, compute_units_, stream_))
        return e;
    if (const char* e = launch_lists(view_.upper, static_cast<u32*>(fresh_upper), m, lists, d_list_target, d_map, n, d_totals, compute_units_, stream_))
        return e;
    UA_HIP(hipMemcpyAsync(&totals, d_totals, sizeof(totals), hipMemcpyDeviceToHost, stream_));
    UA_HIP(hipStreamSynchronize(stream_));
    stats.lists_ms = milliseconds_since(started);

    // ---- rows: in place, ascending, through the staging buffer. Rows below the first removed slot stay where they are.
    //      (The pitch of stored rows is a multiple of 16 bytes by construction — `row_geometry` — so 16-byte units cover a row
    //      exactly: there is no tail.) From the first chunk on the old lists no longer describe the matrix: a failure in here
    //      leaves the index unusable, and the message says so.
    started = std::chrono::steady_clock::now();
    const u64 first_moved = std::min<u64>(totals.first_removed, survivors);
    const auto move_rows = [&]() -> const char* {
        const std::size_t staging_bytes = config.staging_bytes ? config.staging_bytes : compact_default_staging_bytes_k;
        const u64 chunk_rows = std::max<u64>(1, std::min<u64>(staging_bytes / row_stride, survivors - first_moved));
        uint4* d_staging = nullptr;
        UA_HIP(scratch.allocate(&d_staging, (std::size_t)chunk_rows * row_stride)); // nothing has moved yet
        std::uint8_t* rows = static_cast<std::uint8_t*>(d_vectors_);
        const u32 units = row_stride / 16;
        const char* const broken = "Compaction failed while the stored rows were moving: the index is inconsistent, load or build it again";
        for (u64 first = first_moved; first < survivors; first += chunk_rows) {
            const u64 count = std::min<u64>(chunk_rows, survivors - first);
            hipLaunchKernelGGL(compact_gather_rows_kernel, dim3(blocks_for(count * units, compute_units_)), dim3(256), 0, stream_,
                               reinterpret_cast<const uint4*>(rows), d_old_of, first, count, units, d_staging);
            if (hipGetLastError() != hipSuccess ||
                hipMemcpyAsync(rows + first * row_stride, d_staging, (std::size_t)count * row_stride, hipMemcpyDeviceToDevice, stream_) != hipSuccess)
                return broken;
            ++stats.chunks;
        }
        stats.moved_bytes = (survivors - first_moved) * row_stride;
        return hipStreamSynchronize(stream_) == hipSuccess ? nullptr : broken;
    };
    if (first_moved < survivors)
        if (const char* e = move_rows())
            return e;
    stats.rows_ms = milliseconds_since(started);

    // ---- the snapshot adopts the new arrays
    if (d_nbr0_rows_) {
        placed_free(d_nbr0_rows_);
        device_bytes_ -= std::min<std::size_t>(device_bytes_, (std::size_t)n * m0 * 16);
        d_nbr0_rows_ = nullptr;
    }
    view_.nbr0_rows = nullptr;
    drop_sketch();
    for (void* p : {d_nbr0_, d_upper_ref_, d_upper_, d_keys_})
        placed_free(p);
    fresh.adopted = true;
    d_nbr0_ = fresh_nbr0, d_upper_ref_ = fresh_upper_ref, d_upper_ = fresh_upper, d_keys_ = fresh_keys;
    view_.nbr0 = static_cast<const u32*>(d_nbr0_);
    view_.upper_ref = static_cast<const u32*>(d_upper_ref_);
    view_.upper = static_cast<const u32*>(d_upper_);
    view_.keys = static_cast<const u64*>(d_keys_);
    view_.size = survivors;
    view_.has_tombstones = 0;
    if (entry_goes_to != none_slot_k) {
        view_.entry_slot = entry_goes_to;
    } else {
        view_.entry_slot = survivors ? 0xFFFFFFFFu - (u32)(totals.best & 0xFFFFFFFFull) : 0;
        view_.max_level = survivors ? (u32)(totals.best >> 32) : 0;
    }
    upper_lists_ = new_lists;
    count_present_ = survivors; // (device_bytes_ stays: the arrays keep their capacity, the room of the dropped members is spare)
    ++mutations_; // a bitmap made before describes the old numbering (filter.hpp: `check`)

    stats.pruned_edges = totals.pruned;
    stats.removed_members = n - survivors;
    stats.survivors = survivors;
    stats.new_entry_slot = view_.entry_slot, stats.new_max_level = view_.max_level;
    if (stats_out)
        *stats_out = stats;
    return finalize_layout(); // rows of ≤ 16 bytes move next to the new lists; long cos rows get their sketch
}

const char* builder_t::remove(const std::uint32_t* slots, std::uint64_t count) {
    if (!count)
        return nullptr;
    if (!slots)
        return "Nothing to remove";
    for (std::uint64_t i = 0; i < count; ++i)
        if (slots[i] >= size_)
            return "No such member";
    if (const char* e = set_key(slots[0], free_key_k)) // the first the usual way: identity keys become real ones, flags are set
        return e;
    for (std::uint64_t i = 1; i < count; ++i)
        keys_[slots[i]] = free_key_k;
    if (count > 1) { // the rest in one upload and one launch
        UA_HIP(hipSetDevice(snapshot_.device()));
        device_scratch_t scratch(snapshot_.device(), release_t::placed_free);
        u32* d_slots = nullptr;
        UA_HIP(scratch.allocate(&d_slots, (count - 1) * 4));
        UA_HIP(hipMemcpyAsync(d_slots, slots + 1, (count - 1) * 4, hipMemcpyHostToDevice, snapshot_.stream()));
        hipLaunchKernelGGL(compact_tombstones_kernel, dim3((unsigned)((count - 1 + 255) / 256)), dim3(256), 0, snapshot_.stream(), d_slots,
                           count - 1, size_, const_cast<u64*>(snapshot_.view().keys));
        UA_HIP(hipGetLastError());
        UA_HIP(hipStreamSynchronize(snapshot_.stream()));
    }
    return nullptr;
}

const char* builder_t::adopt(const image_t& image, const build_config_t& config, int device) {
    if (image.connectivity < 2 || image.connectivity > 64 || image.connectivity_base > builder_max_connectivity_base_k)
        return "Connectivity is too large for the device builder (connectivity ≤ 64, base connectivity ≤ 128)";
    if (const char* e = snapshot_.build(image, device))
        return e;
    snapshot_.adopt_for_build();
    release_workspace();
    config_ = config;
    config_.connectivity = (std::uint32_t)image.connectivity;
    config_.connectivity_base = (std::uint32_t)image.connectivity_base;
    config_.batch_divisor = std::max<std::uint32_t>(1, config_.batch_divisor);
    config_.max_batch = std::max<std::uint32_t>(1, config_.max_batch);
    config_.multi = image.multi;
    stats_ = build_stats_t{};
    metric_ = image.metric, scalar_ = image.scalar, dimensions_ = (std::size_t)image.dimensions;
    size_ = image.size, upper_lists_ = snapshot_.upper_lists();
    entry_slot_ = (std::uint32_t)image.entry_slot, max_level_ = (std::uint32_t)image.max_level;
    stats_.max_level = max_level_;
    identity_keys_ = false;
    generator_.seed(config_.seed);
    levels_.resize(size_);
    keys_.resize(size_);
    std::size_t offset = 0; // the node tapes are variable-length: one sequential pass (snapshot_t::build has checked their extent)
    for (std::uint64_t i = 0; i < size_; ++i) {
        levels_[i] = image.level(i);
        keys_[i] = image_t::load<std::uint64_t>(image.tapes + offset);
        offset += image.node_bytes(levels_[i]);
    }
    return nullptr;
}

const char* builder_t::isolate(compact_stats_t* stats) { return snapshot_.isolate(stats); }

const char* builder_t::compact(const compact_config_t& config, std::uint32_t* slot_map, compact_stats_t* stats_out) {
    std::vector<std::uint32_t> own_map;
    if (!slot_map) {
        own_map.resize(size_);
        slot_map = own_map.data();
    }
    compact_stats_t stats{};
    if (const char* e = snapshot_.compact(config, slot_map, &stats))
        return e;
    if (stats.removed_members) {
        std::uint64_t lists = 0;
        for (std::uint64_t i = 0; i < size_; ++i) {
            const std::uint32_t to = slot_map[i];
            if (to == none_slot_k)
                continue;
            levels_[to] = levels_[i]; // to ≤ i: nothing that is still needed is overwritten
            if (!identity_keys_)
                keys_[to] = keys_[i];
            lists += (std::uint64_t)levels_[to];
        }
        size_ = stats.survivors;
        levels_.resize(size_);
        if (!identity_keys_)
            keys_.resize(size_);
        upper_lists_ = lists;
        entry_slot_ = stats.new_entry_slot, max_level_ = stats.new_max_level;
        stats_.max_level = max_level_;
    }
    if (stats_out)
        *stats_out = stats;
    return nullptr;
}

} // namespace usearch_amd
