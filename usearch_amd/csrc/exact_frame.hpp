/**
 *  usearch_amd/csrc/exact_frame.hpp — what the partitioned exact-search routes (the wave kernel, the matrix-unit tiles, the bit tile)
 *  have around their launches: per-partition results, the timed window, the fold of the partitions.
 *
 *  Host code only, and included by those routes' translation units alone: engine.hpp stays free of it, so the per-pair kernel units
 *  do not see it.
 */
#pragma once
#include "device_scratch.hpp"
#include "engine.hpp"
#include "host_util.hpp"

namespace usearch_amd {

/// Where a partitioned launch leaves its lists: [partitions][count][wanted] distances and keys, [partitions][count] counts.
struct exact_partials_t {
    float* distances = nullptr;
    std::uint64_t *keys = nullptr, *counts = nullptr;
};

/**
 *  Runs `launch(partials)` — everything the route enqueues on `call.stream` that belongs to its kernel time; it returns null or a
 *  static message — between the event pair that `call.kernel_ms` asks for, then folds the `partitions` lists of every query into
 *  the call's outputs (the earlier partition in front on a tie: partitions are in slot order) and waits for the stream.
 */
template <typename launch_at>
const char* exact_partitioned(const exact_call_t& call, std::uint64_t partitions, launch_at&& launch) {
    exact_partials_t partials;
    event_pair_t events;
    device_scratch_t scratch(current_device_k); // the caller has selected the device the view lives on
    UA_HIP(scratch.allocate(&partials.distances, partitions * call.count * call.wanted * 4));
    UA_HIP(scratch.allocate(&partials.keys, partitions * call.count * call.wanted * 8));
    UA_HIP(scratch.allocate(&partials.counts, partitions * call.count * 8));
    if (call.kernel_ms) {
        UA_HIP(events.create());
        UA_HIP(hipEventRecord(events.begin, call.stream));
    }
    if (const char* error = launch(partials))
        return error;
    if (call.kernel_ms)
        UA_HIP(hipEventRecord(events.end, call.stream));
    if (const char* error = merge_shards_device(partials.distances, partials.keys, partials.counts, partitions, call.count, call.wanted,
                                                call.distances, call.keys, call.counts, call.stream, false))
        return error;
    if (call.kernel_ms)
        UA_HIP(hipEventElapsedTime(call.kernel_ms, events.begin, events.end));
    return nullptr;
}

} // namespace usearch_amd
