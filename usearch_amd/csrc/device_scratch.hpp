/**
 *  usearch_amd/csrc/device_scratch.hpp — device memory and events that live for one call and leave with its scope.
 *
 *  Long-lived arrays (the snapshot's, a workspace's, a filter's bitmaps, the builder's) stay with their owners; everything a
 *  function allocates for its own duration goes through `device_scratch_t`, so every return path releases it.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "placement.hpp"

namespace usearch_amd {

/// How a holder gives its blocks back: `hipFree`, or `placed_free`, which time-stamps large releases for the settle window
/// (placement.hpp: settle, then allocate).
enum class release_t { hip_free, placed_free };

/// "The calling thread's current device, left alone": for code that has no snapshot to ask.
constexpr int current_device_k = -1;

class device_scratch_t {
    int device_;
    release_t release_;
    std::vector<void*> blocks_;

    hipError_t select() const { return device_ < 0 ? hipSuccess : hipSetDevice(device_); }

  public:
    explicit device_scratch_t(int device, release_t release = release_t::hip_free) : device_(device), release_(release) {}
    device_scratch_t(const device_scratch_t&) = delete;
    device_scratch_t& operator=(const device_scratch_t&) = delete;
    ~device_scratch_t() { release(); }

    /// A block with room for `bytes` bytes, at least 16, on the holder's device; `*out` stays null when that fails.
    template <typename T> hipError_t allocate(T** out, std::size_t bytes) {
        *out = nullptr;
        void* block = nullptr;
        hipError_t e = select();
        if (e == hipSuccess)
            e = hipMalloc(&block, std::max<std::size_t>(bytes, 16));
        if (e != hipSuccess)
            return e;
        blocks_.push_back(block);
        *out = static_cast<T*>(block);
        return hipSuccess;
    }

    /// Frees everything held so far, in the order it was allocated; the destructor does the same.
    void release() {
        if (blocks_.empty())
            return;
        (void)select();
        for (void* block : blocks_)
            if (release_ == release_t::placed_free)
                placed_free(block);
            else
                (void)hipFree(block);
        blocks_.clear();
    }
};

/// The begin / end events around a timed launch, destroyed with their scope.
struct event_pair_t {
    hipEvent_t begin = nullptr, end = nullptr;
    event_pair_t() = default;
    event_pair_t(const event_pair_t&) = delete;
    event_pair_t& operator=(const event_pair_t&) = delete;
    ~event_pair_t() {
        if (begin)
            (void)hipEventDestroy(begin);
        if (end)
            (void)hipEventDestroy(end);
    }
    hipError_t create() {
        const hipError_t e = hipEventCreate(&begin);
        return e == hipSuccess ? hipEventCreate(&end) : e;
    }
};

} // namespace usearch_amd
