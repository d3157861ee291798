/**
 *  usearch_amd/csrc/test_hooks.hip — self-test and micro-benchmark entry points of the device-side containers. NOT part of the
 *  product: built into its own library (`usearch_amd/lib/libusearch_amd_testhooks.so`), which only tests/ and scripts/ load.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "device_scratch.hpp"
#include "engine.hpp"
#include "exact_plan.hpp"
#include "host_util.hpp"
#include "kernels.hpp"
#include "kmeans.hpp"
#include "merge_core.hpp"
#include "placement.hpp"
#include "search_plan.hpp"
#include "sketch.hpp"
#include "usearch_amd.h"

typedef char const* usearch_amd_error_t;
namespace {
void fail(usearch_amd_error_t* error, const char* message) {
    if (error && message)
        *error = message;
}
} // namespace

namespace usearch_amd {
/**
 *  Container self-test: replays a scripted sequence of heap pushes / pops and sorted inserts on the scratch-memory containers
 *  and records what comes out, so the GPU tests can compare the tie behaviour with the oracle's containers directly.
 *  ops[i] = {kind, slot}: kind 0 = push(key = keys[i]), 1 = pop, 2 = sorted_insert(keys[i]) with `limit`.
 *  `global_ak`: heap and buffer live in the device memory behind `memory` (the all-global fallback's accessors), else in LDS.
 *  At the end the heap's cells are read out as they lie.
 */
template <bool global_ak>
__global__ __launch_bounds__(64) void containers_kernel(const std::uint32_t* kinds, const float* keys, const std::uint32_t* slots,
                                                        std::uint32_t count, std::uint32_t limit, std::uint32_t capacity, cand_t* memory,
                                                        std::uint64_t* popped, std::uint32_t* counts, std::uint64_t* top_out,
                                                        std::uint64_t* heap_out) {
    extern __shared__ __attribute__((aligned(16))) std::uint8_t lds[];
    using mem = scratch_gt<global_ak>;
    cand_t* heap = global_ak ? memory : reinterpret_cast<cand_t*>(lds);
    cand_t* top = heap + capacity;
    std::uint32_t heap_size = 0, top_size = 0, pops = 0;
    for (std::uint32_t i = 0; i < count; ++i) {
        const std::uint32_t kind = kinds[i];
        if (kind == 0 && heap_size < capacity)
            heap_push<global_ak>(heap, heap_size, keys[i], slots[i]);
        else if (kind == 1 && heap_size) {
            const cand_t c = heap_pop<global_ak>(heap, heap_size);
            if (lane_id() == 0)
                popped[pops] = c;
            ++pops;
        } else if (kind == 2)
            sorted_insert<global_ak>(top, top_size, limit, keys[i], slots[i]);
    }
    for (std::uint32_t i = lane_id(); i < top_size; i += 64)
        top_out[i] = mem::load(top + i);
    for (std::uint32_t i = lane_id(); i < heap_size; i += 64)
        heap_out[i] = mem::load(heap + i);
    if (lane_id() == 0)
        counts[0] = pops, counts[1] = top_size, counts[2] = heap_size;
}

/**
 *  Self-test of `top` as the search kernels hold it, one wave over one `top_gt` layout. ops[i]: kind 0 = insert {keys[i], slots[i]}
 *  under the traversal's acceptance rule, applied here as `search_one` applies it; 1 = the same with the member closed on arrival
 *  (`slot | closed_bit_k`, the pipelined commit); 2 = `first_open` + `close` (the flagged layouts; elsewhere it does nothing).
 *  records[i] = {accepted or found, size, radius bits, and for kind 2: distance bits, slot, owner_lane · epl + owner_cell — none_slot_k
 *  where there is none}. At the end every cell goes out as it lies (registers: all 64 · epl of them, each lane its own; scratch
 *  memory: the first `size`).
 */
constexpr std::uint32_t top_record_words_k = 6;
template <int epl_ak, bool global_ak, bool flags_ak>
__global__ __launch_bounds__(64) void top_kernel(const std::uint32_t* kinds, const float* keys, const std::uint32_t* slots,
                                                 std::uint32_t count, std::uint32_t limit, cand_t* memory, std::uint32_t* records,
                                                 std::uint32_t* cell_bits, std::uint32_t* cell_slots, std::uint32_t* final_size) {
    extern __shared__ __attribute__((aligned(16))) std::uint8_t lds[];
    top_gt<epl_ak, global_ak, flags_ak> top;
    top.reset(global_ak ? memory : reinterpret_cast<cand_t*>(lds));
    float radius = __builtin_inff();
    for (std::uint32_t i = 0; i < count; ++i) {
        const std::uint32_t kind = uniform_u32(kinds[i]);
        std::uint32_t flag = 0, out_bits = 0, out_slot = none_slot_k, out_cell = none_slot_k;
        if (kind <= 1) {
            const float d = uniform_f32(keys[i]);
            const std::uint32_t slot = uniform_u32(slots[i]);
            if (top.size < limit || d < radius) {
                top.insert(d, flags_ak && kind == 1 ? slot | top.closed_bit_k : slot, limit, radius);
                flag = 1;
            }
        } else if constexpr (flags_ak) {
            float distance = 0.f;
            std::uint32_t slot = 0, owner_lane = 0, owner_cell = 0;
            if (top.first_open(distance, slot, owner_lane, owner_cell)) {
                top.close(owner_lane, owner_cell);
                flag = 1, out_bits = __builtin_bit_cast(std::uint32_t, distance), out_slot = slot;
                out_cell = owner_lane * (std::uint32_t)epl_ak + owner_cell;
            }
        }
        if (lane_id() == 0) {
            std::uint32_t* record = records + (std::uint64_t)i * top_record_words_k;
            record[0] = flag, record[1] = top.size, record[2] = __builtin_bit_cast(std::uint32_t, radius);
            record[3] = out_bits, record[4] = out_slot, record[5] = out_cell;
        }
    }
    if constexpr (epl_ak == 0) {
        for (std::uint32_t i = lane_id(); i < top.size; i += 64) {
            const cand_t c = scratch_gt<global_ak>::load(top.cells + i);
            cell_bits[i] = (std::uint32_t)c, cell_slots[i] = cand_slot(c);
        }
    } else {
#pragma unroll
        for (int i = 0; i < epl_ak; ++i) {
            const std::uint32_t g = lane_id() * epl_ak + i;
            cell_bits[g] = __builtin_bit_cast(std::uint32_t, top.d[i]), cell_slots[g] = top.s[i];
        }
    }
    if (lane_id() == 0)
        *final_size = top.size;
}

/**
 *  Micro-benchmark of the register-resident `top`: every wave inserts `count` pseudo-random distances under the
 *  traversal's acceptance rule and reports its shader-clock ticks and how many were accepted (diagnostic only).
 */
template <int epl_ak>
__global__ __launch_bounds__(64) void top_bench_kernel(std::uint32_t count, std::uint32_t limit, unsigned long long* out) {
    top_gt<epl_ak, false> top;
    top.reset(nullptr);
    std::uint32_t state = 12345u + blockIdx.x * 977u;
    float radius = __builtin_inff();
    std::uint32_t accepted = 0;
    const std::uint64_t begin = __builtin_amdgcn_s_memtime();
    for (std::uint32_t i = 0; i < count; ++i) {
        state = state * 1664525u + 1013904223u;
        const float d = uniform_f32((float)(state >> 8) * (1.0f / 16777216.0f));
        if (top.size < limit || d < radius) {
            top.insert(d, i, limit, radius);
            ++accepted;
        }
    }
    const std::uint64_t end = __builtin_amdgcn_s_memtime();
    float checksum = 0.f; // keeps the buffer alive
#pragma unroll
    for (int r = 0; r < epl_ak; ++r)
        checksum += top.d[r] == __builtin_inff() ? 0.f : top.d[r];
    if (lane_id() == 0) {
        out[2 * blockIdx.x] = end - begin;
        out[2 * blockIdx.x + 1] = ((unsigned long long)accepted << 32) | __builtin_bit_cast(std::uint32_t, checksum);
    }
}

/**
 *  Micro-benchmark of the frontier heap: every wave fills a heap of `fill` pseudo-random keys in LDS, then alternates
 *  `count` pops and pushes (the traversal's steady state) and reports the shader-clock ticks spent in each (diagnostic only).
 *  `serial_ak` selects the one-level-per-round-trip pop of the reference's shape.
 */
template <bool serial_ak>
__global__ __launch_bounds__(64) void heap_bench_kernel(std::uint32_t fill, std::uint32_t count, unsigned long long* out) {
    extern __shared__ __attribute__((aligned(16))) std::uint8_t lds[];
    cand_t* heap = reinterpret_cast<cand_t*>(lds);
    std::uint32_t size = 0, state = 4321u + blockIdx.x * 977u;
    auto next_key = [&]() {
        state = state * 1664525u + 1013904223u;
        return uniform_f32(-(float)(state >> 8) * (1.0f / 16777216.0f));
    };
    for (std::uint32_t i = 0; i < fill; ++i)
        heap_push<false>(heap, size, next_key(), i);
    unsigned long long pop_ticks = 0, push_ticks = 0, checksum = 0;
    for (std::uint32_t i = 0; i < count; ++i) {
        const std::uint64_t t0 = __builtin_amdgcn_s_memtime();
        cand_t popped;
        if constexpr (serial_ak)
            popped = heap_pop_serial<false>(heap, size);
        else
            popped = heap_pop<false>(heap, size);
        const std::uint64_t t1 = __builtin_amdgcn_s_memtime();
        heap_push<false>(heap, size, next_key(), fill + i);
        const std::uint64_t t2 = __builtin_amdgcn_s_memtime();
        pop_ticks += t1 - t0, push_ticks += t2 - t1, checksum += popped;
    }
    if (lane_id() == 0)
        out[3 * blockIdx.x] = pop_ticks, out[3 * blockIdx.x + 1] = push_ticks, out[3 * blockIdx.x + 2] = checksum;
}

} // namespace usearch_amd

using namespace usearch_amd;

extern "C" {

/** Diagnostic: per-wave ticks of `heap_bench_kernel` and a checksum of what was popped (both pops must agree on it). */
__attribute__((visibility("default"))) void usearch_amd_bench_heap(uint32_t serial, uint32_t fill, uint32_t count,
                                                                    uint32_t waves, uint64_t* pop_ticks,
                                                                    uint64_t* push_ticks, uint64_t* checksums,
                                                                    usearch_amd_error_t* error) {
    device_scratch_t scratch(current_device_k);
    unsigned long long* d_out = nullptr;
    if (scratch.allocate(&d_out, (size_t)waves * 24) != hipSuccess)
        return fail(error, "hipMalloc failed");
    const size_t lds = ((size_t)fill + 8) * 8;
    if (serial)
        hipLaunchKernelGGL(heap_bench_kernel<true>, dim3(waves), dim3(64), lds, nullptr, fill, count, d_out);
    else
        hipLaunchKernelGGL(heap_bench_kernel<false>, dim3(waves), dim3(64), lds, nullptr, fill, count, d_out);
    std::vector<unsigned long long> host((size_t)waves * 3);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(host.data(), d_out, host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        fail(error, "heap bench failed");
    for (uint32_t w = 0; w < waves; ++w)
        pop_ticks[w] = host[3 * w], push_ticks[w] = host[3 * w + 1], checksums[w] = host[3 * w + 2];
}

/** Diagnostic: ticks[wave] and accepted[wave] of `top_bench_kernel` (entries per lane 4, 8 or 16). */
__attribute__((visibility("default"))) void usearch_amd_bench_top(uint32_t epl, uint32_t count, uint32_t limit,
                                                                   uint32_t waves, uint64_t* ticks, uint64_t* accepted,
                                                                   usearch_amd_error_t* error) {
    device_scratch_t scratch(current_device_k);
    unsigned long long* d_out = nullptr;
    if (scratch.allocate(&d_out, (size_t)waves * 16) != hipSuccess)
        return fail(error, "hipMalloc failed");
    if (epl == 4)
        hipLaunchKernelGGL(top_bench_kernel<4>, dim3(waves), dim3(64), 0, nullptr, count, limit, d_out);
    else if (epl == 8)
        hipLaunchKernelGGL(top_bench_kernel<8>, dim3(waves), dim3(64), 0, nullptr, count, limit, d_out);
    else
        hipLaunchKernelGGL(top_bench_kernel<16>, dim3(waves), dim3(64), 0, nullptr, count, limit, d_out);
    std::vector<unsigned long long> host((size_t)waves * 2);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(host.data(), d_out, host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
        fail(error, "top bench failed");
    for (uint32_t w = 0; w < waves; ++w)
        ticks[w] = host[2 * w], accepted[w] = host[2 * w + 1] >> 32;
}

/**
 *  Self-test hook: replays `count` scripted operations on the device-side containers (kind 0 = frontier push of
 *  {keys[i], slots[i]}, 1 = frontier pop, 2 = insert {keys[i], slots[i]} into the result buffer limited to `limit`) and
 *  returns what was popped, the final result buffer and what remains in the heap, cell by cell, each entry packed as
 *  (slot << 32 | float bits). `global_memory`: the containers live in device memory (`global_ak = true`), else in LDS.
 *  `heap` needs room for one entry per push.
 */
static const char* test_containers(uint32_t const* kinds, float const* keys, uint32_t const* slots, size_t count, size_t limit,
                                   int global_memory, uint64_t* popped, size_t* popped_count, uint64_t* top, size_t* top_count,
                                   uint64_t* heap, size_t* heap_count) {
    size_t pushes = 0;
    for (size_t i = 0; i < count; ++i)
        pushes += kinds[i] == 0;
    const size_t capacity = pushes + 1; // the heap never holds more than was pushed
    const size_t cells = capacity + limit + 1;
    if (!global_memory && cells * 8 > 64 * 1024)
        return "The script's containers do not fit into LDS";
    uint32_t *d_kinds = nullptr, *d_slots = nullptr, *d_counts = nullptr;
    float* d_keys = nullptr;
    uint64_t *d_popped = nullptr, *d_top = nullptr, *d_heap = nullptr;
    cand_t* d_memory = nullptr;
    device_scratch_t scratch(current_device_k);
    UA_HIP(scratch.allocate(&d_kinds, count * 4 + 4));
    UA_HIP(scratch.allocate(&d_slots, count * 4 + 4));
    UA_HIP(scratch.allocate(&d_keys, count * 4 + 4));
    UA_HIP(scratch.allocate(&d_popped, (count + 1) * 8));
    UA_HIP(scratch.allocate(&d_top, (limit + 1) * 8));
    UA_HIP(scratch.allocate(&d_heap, capacity * 8));
    UA_HIP(scratch.allocate(&d_memory, cells * 8));
    UA_HIP(scratch.allocate(&d_counts, 12));
    UA_HIP(hipMemcpy(d_kinds, kinds, count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_slots, slots, count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_keys, keys, count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemset(d_memory, 0, cells * 8));
    if (global_memory)
        hipLaunchKernelGGL(containers_kernel<true>, dim3(1), dim3(64), 0, nullptr, d_kinds, d_keys, d_slots, (uint32_t)count, (uint32_t)limit,
                           (uint32_t)capacity, d_memory, d_popped, d_counts, d_top, d_heap);
    else
        hipLaunchKernelGGL(containers_kernel<false>, dim3(1), dim3(64), cells * 8, nullptr, d_kinds, d_keys, d_slots, (uint32_t)count,
                           (uint32_t)limit, (uint32_t)capacity, d_memory, d_popped, d_counts, d_top, d_heap);
    UA_HIP(hipGetLastError());
    UA_HIP(hipDeviceSynchronize());
    uint32_t host_counts[3] = {0, 0, 0};
    UA_HIP(hipMemcpy(host_counts, d_counts, 12, hipMemcpyDeviceToHost));
    *popped_count = host_counts[0];
    *top_count = host_counts[1];
    UA_HIP(hipMemcpy(popped, d_popped, host_counts[0] * 8, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(top, d_top, host_counts[1] * 8, hipMemcpyDeviceToHost));
    if (heap_count)
        *heap_count = host_counts[2];
    if (heap)
        UA_HIP(hipMemcpy(heap, d_heap, host_counts[2] * 8, hipMemcpyDeviceToHost));
    return nullptr;
}
__attribute__((visibility("default"))) void usearch_amd_test_containers(uint32_t const* kinds, float const* keys, uint32_t const* slots, size_t count,
                                 size_t limit, int global_memory, uint64_t* popped, size_t* popped_count, uint64_t* top, size_t* top_count,
                                 uint64_t* heap, size_t* heap_count, usearch_amd_error_t* error) {
    fail(error, test_containers(kinds, keys, slots, count, limit, global_memory, popped, popped_count, top, top_count, heap, heap_count));
}

/**
 *  Self-test hook of `top` (`top_kernel` above): replays the script on the layout named by `epl` (1, 2, 4, 8, 16: registers; 0: scratch
 *  memory), `flags` (the frontier flags, registers only) and `global_memory` (epl 0 only: device memory instead of LDS).
 *  → `records` [count][6], `cell_bits` / `cell_slots` [64 · epl, or `limit` for epl 0] and the final size.
 */
static const char* test_top(uint32_t epl, int flags, int global_memory, uint32_t const* kinds, float const* keys, uint32_t const* slots,
                            size_t count, size_t limit, uint32_t* records, uint32_t* cell_bits, uint32_t* cell_slots, uint32_t* final_size) {
    if (epl != 0 && epl != 1 && epl != 2 && epl != 4 && epl != 8 && epl != 16)
        return "No such layout of `top`";
    if (!limit || (epl && limit > 64u * epl) || (!epl && flags) || (epl && global_memory))
        return "The layout cannot hold this script";
    if (!epl && !global_memory && (limit + 1) * 8 > 64 * 1024)
        return "The buffer does not fit into LDS";
    const size_t cells = epl ? 64u * epl : limit;
    uint32_t *d_kinds = nullptr, *d_slots = nullptr, *d_records = nullptr, *d_bits = nullptr, *d_cell_slots = nullptr, *d_size = nullptr;
    float* d_keys = nullptr;
    cand_t* d_memory = nullptr;
    device_scratch_t scratch(current_device_k);
    UA_HIP(scratch.allocate(&d_kinds, count * 4 + 4));
    UA_HIP(scratch.allocate(&d_slots, count * 4 + 4));
    UA_HIP(scratch.allocate(&d_keys, count * 4 + 4));
    UA_HIP(scratch.allocate(&d_records, count * top_record_words_k * 4 + 4));
    UA_HIP(scratch.allocate(&d_bits, cells * 4));
    UA_HIP(scratch.allocate(&d_cell_slots, cells * 4));
    UA_HIP(scratch.allocate(&d_memory, (limit + 1) * 8));
    UA_HIP(scratch.allocate(&d_size, 4));
    UA_HIP(hipMemcpy(d_kinds, kinds, count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_slots, slots, count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_keys, keys, count * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_bits, cell_bits, cells * 4, hipMemcpyHostToDevice)); // the caller's pattern: a cell never written shows
    UA_HIP(hipMemcpy(d_cell_slots, cell_slots, cells * 4, hipMemcpyHostToDevice));
    const size_t lds = epl || global_memory ? 0 : (limit + 1) * 8;
#define USEARCH_AMD_TOP_LAYOUT(E, G, F)                                                                                                       \
    hipLaunchKernelGGL((top_kernel<E, G, F>), dim3(1), dim3(64), lds, nullptr, d_kinds, d_keys, d_slots, (uint32_t)count, (uint32_t)limit,      \
                       d_memory, d_records, d_bits, d_cell_slots, d_size)
#define USEARCH_AMD_TOP_REGISTERS(E)                                                                                                          \
    case E:                                                                                                                                   \
        if (flags)                                                                                                                            \
            USEARCH_AMD_TOP_LAYOUT(E, false, true);                                                                                           \
        else                                                                                                                                  \
            USEARCH_AMD_TOP_LAYOUT(E, false, false);                                                                                          \
        break
    switch (epl) {
        USEARCH_AMD_TOP_REGISTERS(1);
        USEARCH_AMD_TOP_REGISTERS(2);
        USEARCH_AMD_TOP_REGISTERS(4);
        USEARCH_AMD_TOP_REGISTERS(8);
        USEARCH_AMD_TOP_REGISTERS(16);
    default:
        if (global_memory)
            USEARCH_AMD_TOP_LAYOUT(0, true, false);
        else
            USEARCH_AMD_TOP_LAYOUT(0, false, false);
    }
#undef USEARCH_AMD_TOP_REGISTERS
#undef USEARCH_AMD_TOP_LAYOUT
    UA_HIP(hipGetLastError());
    UA_HIP(hipDeviceSynchronize());
    UA_HIP(hipMemcpy(records, d_records, count * top_record_words_k * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(cell_bits, d_bits, cells * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(cell_slots, d_cell_slots, cells * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(final_size, d_size, 4, hipMemcpyDeviceToHost));
    return nullptr;
}
__attribute__((visibility("default"))) void usearch_amd_test_top(uint32_t epl, int flags, int global_memory, uint32_t const* kinds,
                                                                  float const* keys, uint32_t const* slots, size_t count, size_t limit,
                                                                  uint32_t* records, uint32_t* cell_bits, uint32_t* cell_slots,
                                                                  uint32_t* final_size, usearch_amd_error_t* error) {
    fail(error, test_top(epl, flags, global_memory, kinds, keys, slots, count, limit, records, cell_bits, cell_slots, final_size));
}

/**
 *  Self-test hook of the fold of per-shard lists: `distances` / `keys` [shards][queries][wanted] and `counts` [shards][queries] →
 *  [queries][wanted] and [queries], with the order inside a shard the caller names (`later_position_first`, merge_core.hpp).
 *  `on_host` = 0: `merge_kernel` through `merge_shards_device`; 1: `merge_rank` as the host path of the sharded step walks it
 *  (`merge_blocks_host` of sharded.hip: every kept element, cells from `found` on padded). Either way the caller's output buffers are
 *  the memory the merge writes into — on the device a copy of them — so a cell it never writes keeps the caller's pattern.
 */
static const char* test_merge(float const* distances, uint64_t const* keys, uint64_t const* counts, size_t shards, size_t queries, size_t wanted,
                              int later_position_first, int on_host, float* out_distances, uint64_t* out_keys, uint64_t* out_counts) {
    const size_t cells = shards * queries * wanted, rows = shards * queries;
    if (!cells)
        return nullptr;
    if (on_host) {
        std::vector<float> pool(shards * wanted);
        std::vector<std::uint32_t> kept(shards);
        for (size_t q = 0; q < queries; ++q) {
            size_t available = 0;
            for (size_t shard = 0; shard < shards; ++shard) {
                kept[shard] = (std::uint32_t)std::min<std::uint64_t>(counts[shard * queries + q], wanted);
                available += kept[shard];
                std::copy_n(distances + (shard * queries + q) * wanted, wanted, pool.data() + shard * wanted);
            }
            const size_t found = std::min(available, wanted);
            for (size_t shard = 0; shard < shards; ++shard)
                for (std::uint32_t position = 0; position < kept[shard]; ++position) {
                    const std::uint32_t rank = merge_rank(pool.data(), kept.data(), (std::uint32_t)shards, (std::uint32_t)wanted,
                                                          (std::uint32_t)shard, position, later_position_first != 0);
                    if (rank >= wanted)
                        continue;
                    out_distances[q * wanted + rank] = pool[shard * wanted + position];
                    out_keys[q * wanted + rank] = keys[(shard * queries + q) * wanted + position];
                }
            for (size_t i = found; i < wanted; ++i) {
                out_keys[q * wanted + i] = 0;
                std::memcpy(out_distances + q * wanted + i, &signaling_nan_bits_k, 4);
            }
            out_counts[q] = found;
        }
        return nullptr;
    }
    float *d_distances = nullptr, *d_out_distances = nullptr;
    uint64_t *d_keys = nullptr, *d_counts = nullptr, *d_out_keys = nullptr, *d_out_counts = nullptr;
    device_scratch_t scratch(current_device_k);
    UA_HIP(scratch.allocate(&d_distances, cells * 4));
    UA_HIP(scratch.allocate(&d_keys, cells * 8));
    UA_HIP(scratch.allocate(&d_counts, rows * 8));
    UA_HIP(scratch.allocate(&d_out_distances, queries * wanted * 4));
    UA_HIP(scratch.allocate(&d_out_keys, queries * wanted * 8));
    UA_HIP(scratch.allocate(&d_out_counts, queries * 8));
    UA_HIP(hipMemcpy(d_distances, distances, cells * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_keys, keys, cells * 8, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_counts, counts, rows * 8, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_out_distances, out_distances, queries * wanted * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_out_keys, out_keys, queries * wanted * 8, hipMemcpyHostToDevice));
    UA_HIP(hipMemcpy(d_out_counts, out_counts, queries * 8, hipMemcpyHostToDevice));
    if (const char* message = merge_shards_device(d_distances, d_keys, d_counts, shards, queries, wanted, d_out_distances, d_out_keys,
                                                  d_out_counts, nullptr, later_position_first != 0))
        return message;
    UA_HIP(hipMemcpy(out_distances, d_out_distances, queries * wanted * 4, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(out_keys, d_out_keys, queries * wanted * 8, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(out_counts, d_out_counts, queries * 8, hipMemcpyDeviceToHost));
    return nullptr;
}
__attribute__((visibility("default"))) void usearch_amd_test_merge(float const* distances, uint64_t const* keys, uint64_t const* counts,
                                                                    size_t shards, size_t queries, size_t wanted, int later_position_first,
                                                                    int on_host, float* out_distances, uint64_t* out_keys,
                                                                    uint64_t* out_counts, usearch_amd_error_t* error) {
    fail(error, test_merge(distances, keys, counts, shards, queries, wanted, later_position_first, on_host, out_distances, out_keys, out_counts));
}

/**
 *  Self-test hook of `device_scratch_t` (device_scratch.hpp); launches no kernel. Makes `current` the thread's device, opens a holder for
 *  `home`, takes blocks of 0, 1 and 4096 bytes, then asks for 2^60 bytes, which the runtime refuses. Reports, read AFTER that refusal:
 *  `pointers[3]`, the device each block lives on (`devices[3]`) and the room behind each pointer (`room[3]`, bytes); the refused
 *  request's error code (`refused`, a hipError_t) and what it left in its out-pointer (`refused_pointer`). The scope then ends and
 *  the thread's device is put back.
 */
__attribute__((visibility("default"))) void usearch_amd_test_device_scratch(int home, int current, void** pointers, int* devices, size_t* room,
                                                                             int* refused, void** refused_pointer,
                                                                             usearch_amd_error_t* error) {
    int entered = 0;
    fail(error, [&]() -> const char* {
        UA_HIP(hipGetDevice(&entered));
        UA_HIP(hipSetDevice(current));
        device_scratch_t scratch(home);
        const size_t sizes[3] = {0, 1, 4096};
        std::uint8_t* blocks[3] = {nullptr, nullptr, nullptr};
        for (int i = 0; i < 3; ++i)
            UA_HIP(scratch.allocate(&blocks[i], sizes[i]));
        std::uint8_t* huge = reinterpret_cast<std::uint8_t*>(std::uintptr_t(1)); // must come back null
        *refused = (int)scratch.allocate(&huge, std::size_t(1) << 60);
        *refused_pointer = huge;
        (void)hipGetLastError(); // the refusal is expected: leave no error behind for the next launch check of this thread
        for (int i = 0; i < 3; ++i) {
            hipPointerAttribute_t attributes{};
            UA_HIP(hipPointerGetAttributes(&attributes, blocks[i]));
            hipDeviceptr_t base = nullptr;
            size_t extent = 0;
            UA_HIP(hipMemGetAddressRange(&base, &extent, blocks[i]));
            pointers[i] = blocks[i], devices[i] = attributes.device;
            room[i] = extent - (size_t)(blocks[i] - static_cast<std::uint8_t*>(base));
        }
        return nullptr;
    }());
    (void)hipSetDevice(entered);
}

} // extern "C"


// ---- diagnostics of round 3 – 5's placement studies (scripts/placement_study.py, scripts/fragment_study.py): probes over the arrays a
//      snapshot hands out through `usearch_amd_snapshot_arrays` (csrc/placement.hpp). Not product entry points.
extern "C" __attribute__((visibility("default"))) float usearch_amd_test_gather_probe(const void* base, size_t bytes, size_t row_bytes,
                                                                                      usearch_amd_error_t* error) {
    float gbps = 0.f;
    const hipError_t e = usearch_amd::gather_probe(base, bytes, row_bytes, &gbps);
    if (e != hipSuccess)
        fail(error, hipGetErrorString(e));
    return gbps;
}
extern "C" __attribute__((visibility("default"))) float usearch_amd_test_translation_probe(const void* base, size_t bytes,
                                                                                           usearch_amd_error_t* error) {
    float rate = 0.f;
    const hipError_t e = usearch_amd::translation_probe(base, bytes, &rate);
    if (e != hipSuccess)
        fail(error, hipGetErrorString(e));
    return rate;
}
extern "C" __attribute__((visibility("default"))) float usearch_amd_test_latency_probe(const void* base, size_t bytes, size_t row_bytes,
                                                                                       usearch_amd_error_t* error) {
    float nanoseconds = 0.f;
    const hipError_t e = usearch_amd::latency_probe(base, bytes, row_bytes, &nanoseconds);
    if (e != hipSuccess)
        fail(error, hipGetErrorString(e));
    return nanoseconds;
}

// ---- the sketch (sketch.hpp): the host twins of the record builder and of the bound the walk evaluates, for tests/test_sketch_bound.py.
//      `rows` [count][stride] and `queries` [query_count][stride] in the storage kind; the directions are drawn from the rows as the
//      engine draws them. Writes `bounds[query_count][count]` (−∞ where a row or a query is never pruned) and the number of directions.
extern "C" __attribute__((visibility("default"))) void usearch_amd_test_sketch_bounds(const void* rows, size_t count, const void* queries,
                                                                                      size_t query_count, size_t dimensions, int scalar_kind,
                                                                                      size_t stride, float* bounds, uint32_t* rank,
                                                                                      usearch_amd_error_t* error) {
    using namespace usearch_amd;
    const scalar_kind_t scalar = (scalar_kind_t)scalar_kind;
    if (scalar != scalar_f32_k && scalar != scalar_f16_k && scalar != scalar_bf16_k)
        return fail(error, "The sketch covers f32, f16 and bf16 rows");
    const std::uint8_t* row_bytes = static_cast<const std::uint8_t*>(rows);
    const std::uint8_t* query_bytes = static_cast<const std::uint8_t*>(queries);
    const std::uint32_t samples = (std::uint32_t)std::min<std::size_t>(sketch_rank_k, count);
    std::vector<double> wide((std::size_t)samples * dimensions);
    for (std::uint32_t s = 0; s < samples; ++s)
        for (std::size_t i = 0; i < dimensions; ++i)
            wide[(std::size_t)s * dimensions + i] = (double)sketch_scalar(row_bytes + sketch_sample_slot(s, count) * stride, (std::uint32_t)i, scalar);
    const sketch_directions_t directions = sketch_orthonormalise(wide, samples, (std::uint32_t)dimensions);
    if (rank)
        *rank = directions.rank;
    std::vector<std::uint8_t> records(count * sketch_record_bytes_k);
    for (std::size_t r = 0; r < count; ++r)
        sketch_record_host(row_bytes + r * stride, scalar, (std::uint32_t)dimensions, directions, records.data() + r * sketch_record_bytes_k);
    std::vector<float> query(dimensions), coefficients(sketch_columns_k);
    for (std::size_t q = 0; q < query_count; ++q) {
        float a2 = 0.f; // any summation order does: only its sign and finiteness matter here
        for (std::size_t i = 0; i < dimensions; ++i) {
            query[i] = sketch_scalar(query_bytes + q * stride, (std::uint32_t)i, scalar);
            a2 = fmaf(query[i], query[i], a2);
        }
        const bool on = sketch_query_host(query.data(), a2, (std::uint32_t)dimensions, directions, coefficients.data());
        for (std::size_t r = 0; r < count; ++r)
            bounds[q * count + r] = on ? sketch_bound_host(coefficients.data(), records.data() + r * sketch_record_bytes_k, (std::uint32_t)dimensions)
                                       : -INFINITY;
    }
}

// ---- k-means (kmeans.hip): the matrix the loop clusters — the caller's rows after the device cast, for tests/test_gpu_kmeans.py.
//      `scalar_kind` / `quantization_kind`: scalar_kind_t of common.hpp.
extern "C" __attribute__((visibility("default"))) void usearch_amd_test_kmeans_quantize(const void* points, size_t count, size_t stride,
                                                                                        int scalar_kind, size_t dimensions,
                                                                                        int quantization_kind, int device, void* out,
                                                                                        size_t out_stride, usearch_amd_error_t* error) {
    fail(error, kmeans_quantize(static_cast<const std::uint8_t*>(points), count, stride, (scalar_kind_t)scalar_kind, dimensions,
                                (scalar_kind_t)quantization_kind, device, static_cast<std::uint8_t*>(out), out_stride));
}

// ---- the launch planner (search_plan.hpp) on plain values, for tests/test_search_plan.py: what `search_begin` settles for the call
//      described by `shape` and `tuning`, then one rung of the retry ladder per entry of `pending` (the queries that rung runs over: all
//      of them, then those that outgrew their scratch), `escalate` between them, until a rung is the global one. `knobs` null = the
//      environment, read as the engine reads it. → rungs planned (0 and `error` set: the call is refused); `plan->stats` reports what
//      `search_finish` would, as far as that is decided and not measured.
static_assert(sizeof(usearch_amd::search_stats_t) == sizeof(usearch_amd_stats_t), "tests read `search_plan_t::stats` as the C ABI's struct");
extern "C" __attribute__((visibility("default"))) size_t usearch_amd_test_plan_search(const usearch_amd::search_shape_t* shape,
                                                                                      const usearch_amd::search_tuning_t* tuning,
                                                                                      const uint32_t* pending, size_t pending_count,
                                                                                      const usearch_amd::search_knobs_t* knobs,
                                                                                      usearch_amd::search_plan_t* plan,
                                                                                      usearch_amd::search_rung_t* rungs,
                                                                                      usearch_amd_error_t* error) {
    using namespace usearch_amd;
    const search_knobs_t read = knobs ? *knobs : read_search_knobs(shape->lanes);
    if (const char* e = plan_search(*shape, *tuning, read, *plan)) {
        fail(error, e);
        return 0;
    }
    size_t planned = 0;
    for (; planned < pending_count && !(planned && rungs[planned - 1].mode == scratch_global_k); ++planned) {
        if (planned == 1)
            plan->stats.retried_lds = pending[planned];
        if (planned)
            escalate(*shape, read, *plan, (int)planned - 1);
        plan_rung(*shape, read, *plan, pending[planned], rungs[planned]);
        if (rungs[planned].mode == scratch_global_k)
            plan->stats.retried_global = pending[planned];
    }
    plan->stats.passes = (std::uint32_t)planned;
    if (planned)
        plan->stats.mode = (std::uint32_t)rungs[0].mode + 1, plan->stats.grid = rungs[0].grid, plan->stats.lds_bytes = rungs[0].lds_bytes;
    return planned;
}

// ---- the tiled exact search's planner (exact_plan.hpp) on plain values, for tests/test_exact_plan.py and the GPU tests that assert the
//      route they are there for: what `exact_search_tiled_device` settles for `rows` rows of `bytes_per_vector` bytes at pitch
//      `row_stride`, `count` queries and `wanted` results. `forced_tile` < 0 / `global_lists` < 0 = the environment, read as the engine
//      reads it. → 1, or 0 and `error` set: the call is refused.
extern "C" __attribute__((visibility("default"))) int usearch_amd_test_plan_exact(uint64_t rows, uint64_t bytes_per_vector, uint64_t row_stride,
                                                                                  uint64_t count, uint64_t wanted, int64_t forced_tile,
                                                                                  int global_lists, usearch_amd::exact_plan_t* plan,
                                                                                  usearch_amd_error_t* error) {
    using namespace usearch_amd;
    const std::uint64_t tile = forced_tile < 0 ? env_size("USEARCH_AMD_EXACT_TILE", 0) : (std::uint64_t)forced_tile;
    const bool lists = global_lists < 0 ? env_size("USEARCH_AMD_EXACT_GLOBAL_LISTS", 0) != 0 : global_lists != 0;
    if (const char* e = plan_exact(rows, bytes_per_vector, row_stride, count, wanted, tile, lists, *plan)) {
        fail(error, e);
        return 0;
    }
    return 1;
}

// ---- which (metric, scalar kind, result count) has a tiled exact-search kernel at all (`exact_tiled_pair` of exact_plan.hpp, what
//      `exact_tiled_available` answers with), for tests/test_exact_tiled_pairs.py. `metric` / `scalar`: metric_kind_t / scalar_kind_t of
//      common.hpp. → 1 or 0.
extern "C" __attribute__((visibility("default"))) int usearch_amd_test_exact_tiled_pair(int metric, int scalar, uint64_t wanted) {
    return usearch_amd::exact_tiled_pair((usearch_amd::metric_kind_t)metric, (usearch_amd::scalar_kind_t)scalar, wanted) ? 1 : 0;
}

// ---- the same two for the bit tile (exact_bits.hip): its table (`exact_bits_pair`) and its planner (`plan_exact_bits`, one variant:
//      nothing to force, no environment), for tests/test_exact_bits_plan.py and the route checks of tests/test_gpu_exact_bits.py.
extern "C" __attribute__((visibility("default"))) int usearch_amd_test_exact_bits_pair(int metric, int scalar, uint64_t wanted) {
    return usearch_amd::exact_bits_pair((usearch_amd::metric_kind_t)metric, (usearch_amd::scalar_kind_t)scalar, wanted) ? 1 : 0;
}
extern "C" __attribute__((visibility("default"))) int usearch_amd_test_plan_exact_bits(uint64_t rows, uint64_t bytes_per_vector,
                                                                                       uint64_t row_stride, uint64_t count, uint64_t wanted,
                                                                                       usearch_amd::exact_bits_plan_t* plan,
                                                                                       usearch_amd_error_t* error) {
    if (const char* e = usearch_amd::plan_exact_bits(rows, bytes_per_vector, row_stride, count, wanted, *plan)) {
        fail(error, e);
        return 0;
    }
    return 1;
}

// ---- the sketch on the device and its twins piece by piece, for tests/test_gpu_sketch_records.py, tests/test_gpu_sketch_counts.py and
//      tests/test_sketch_truth.py. `scalar_kind`: scalar_kind_t of common.hpp (f32, f16, bf16); `directions`: [dimensions][64] f32.
namespace usearch_amd {
struct sketch_test_access_t {
    static const void* records(const snapshot_t& s) { return s.d_sketch_; }
    static const void* directions(const snapshot_t& s) { return s.d_sketch_directions_; }
    static std::uint64_t rows(const snapshot_t& s) { return s.d_sketch_ && s.d_sketch_directions_ ? s.sketch_rows_ : 0; }
    static double gram_defect(const snapshot_t& s) { return s.sketch_gram_defect_; }
};
} // namespace usearch_amd

namespace {
bool sketch_scalar_kind(int scalar_kind) {
    return scalar_kind == scalar_f32_k || scalar_kind == scalar_f16_k || scalar_kind == scalar_bf16_k;
}
sketch_directions_t sketch_directions_of(const float* transposed, size_t dimensions, double gram_defect) {
    sketch_directions_t d;
    d.transposed.assign(transposed, transposed + dimensions * sketch_columns_k);
    d.rank = sketch_rank_k, d.gram_defect = gram_defect;
    return d;
}
} // namespace

/** `sketch_records_kernel` over rows [first, count) of the caller's `rows` ([count][stride] bytes) under the caller's directions: `records`
 *  ([count][128], the caller's pattern in it) goes to the device, the kernel runs as `make_sketch` runs it, and everything comes back: rows
 *  below `first` must still hold the pattern. */
extern "C" __attribute__((visibility("default"))) void usearch_amd_test_sketch_device_records(const void* rows, size_t count, size_t stride,
                                                                                              size_t dimensions, int scalar_kind, size_t first,
                                                                                              const float* directions, double gram_defect,
                                                                                              void* records, usearch_amd_error_t* error) {
    if (!sketch_scalar_kind(scalar_kind))
        return fail(error, "The sketch covers f32, f16 and bf16 rows");
    fail(error, [&]() -> const char* {
        if (!count || first > count)
            return "No rows, or `first` beyond them";
        if (stride < bytes_per_vector((scalar_kind_t)scalar_kind, dimensions) || stride > 0xFFFFFFFFull)
            return "Rows shorter than their dimensions";
        device_scratch_t scratch(current_device_k);
        std::uint8_t *d_rows = nullptr, *d_records = nullptr;
        float* d_directions = nullptr;
        const size_t directions_bytes = dimensions * sketch_columns_k * sizeof(float);
        UA_HIP(scratch.allocate(&d_rows, count * stride));
        UA_HIP(scratch.allocate(&d_records, count * sketch_record_bytes_k));
        UA_HIP(scratch.allocate(&d_directions, directions_bytes));
        UA_HIP(hipMemcpy(d_rows, rows, count * stride, hipMemcpyHostToDevice));
        UA_HIP(hipMemcpy(d_records, records, count * sketch_record_bytes_k, hipMemcpyHostToDevice));
        UA_HIP(hipMemcpy(d_directions, directions, directions_bytes, hipMemcpyHostToDevice));
        launch_sketch_records(d_rows, (std::uint32_t)stride, (std::uint32_t)dimensions, (scalar_kind_t)scalar_kind, first, count, d_directions,
                              gram_defect, d_records, nullptr);
        UA_HIP(hipGetLastError());
        UA_HIP(hipDeviceSynchronize());
        UA_HIP(hipMemcpy(records, d_records, count * sketch_record_bytes_k, hipMemcpyDeviceToHost));
        return nullptr;
    }());
}

/** The directions `sketch_orthonormalise` draws from `rows` as the engine draws them (up to 62 rows at the seeded slots) → `transposed`
 *  [dimensions][64] f32, the number of directions and the gram defect. */
extern "C" __attribute__((visibility("default"))) void usearch_amd_test_sketch_directions(const void* rows, size_t count, size_t stride,
                                                                                          size_t dimensions, int scalar_kind, float* transposed,
                                                                                          uint32_t* rank, double* gram_defect,
                                                                                          usearch_amd_error_t* error) {
    if (!sketch_scalar_kind(scalar_kind))
        return fail(error, "The sketch covers f32, f16 and bf16 rows");
    const std::uint8_t* row_bytes = static_cast<const std::uint8_t*>(rows);
    const std::uint32_t samples = (std::uint32_t)std::min<std::size_t>(sketch_rank_k, count);
    std::vector<double> wide((std::size_t)samples * dimensions);
    for (std::uint32_t s = 0; s < samples; ++s)
        for (std::size_t i = 0; i < dimensions; ++i)
            wide[(std::size_t)s * dimensions + i] =
                (double)sketch_scalar(row_bytes + sketch_sample_slot(s, count) * stride, (std::uint32_t)i, (scalar_kind_t)scalar_kind);
    const sketch_directions_t directions = sketch_orthonormalise(wide, samples, (std::uint32_t)dimensions);
    std::copy(directions.transposed.begin(), directions.transposed.end(), transposed);
    *rank = directions.rank, *gram_defect = directions.gram_defect;
}

/** `sketch_record_host` for every row of `rows` under the caller's directions → `records` [count][128]. */
extern "C" __attribute__((visibility("default"))) void usearch_amd_test_sketch_twin_records(const void* rows, size_t count, size_t stride,
                                                                                            size_t dimensions, int scalar_kind,
                                                                                            const float* directions, double gram_defect,
                                                                                            void* records, usearch_amd_error_t* error) {
    if (!sketch_scalar_kind(scalar_kind))
        return fail(error, "The sketch covers f32, f16 and bf16 rows");
    const sketch_directions_t d = sketch_directions_of(directions, dimensions, gram_defect);
    for (std::size_t r = 0; r < count; ++r)
        sketch_record_host(static_cast<const std::uint8_t*>(rows) + r * stride, (scalar_kind_t)scalar_kind, (std::uint32_t)dimensions, d,
                           static_cast<std::uint8_t*>(records) + r * sketch_record_bytes_k);
}

/** `sketch_query_host` and `sketch_bound_host`: for query q ([query_count][stride] in the storage kind) with the Σa² the kernel has for it
 *  (`sums_of_squares[q]`) → `used[q]` (0 = the query walks without the sketch) and `bounds[q][r]` against every one of `records`
 *  ([count][128]); a query that does not use the sketch gets −∞ everywhere. */
extern "C" __attribute__((visibility("default"))) void usearch_amd_test_sketch_twin_bounds(const void* queries, size_t query_count, size_t stride,
                                                                                           const float* sums_of_squares, size_t dimensions,
                                                                                           int scalar_kind, const float* directions,
                                                                                           const void* records, size_t count, float* bounds,
                                                                                           uint8_t* used, usearch_amd_error_t* error) {
    if (!sketch_scalar_kind(scalar_kind))
        return fail(error, "The sketch covers f32, f16 and bf16 rows");
    const sketch_directions_t d = sketch_directions_of(directions, dimensions, 0.0); // (the query side does not read the gram defect)
    std::vector<float> query(dimensions), coefficients(sketch_columns_k);
    for (std::size_t q = 0; q < query_count; ++q) {
        for (std::size_t i = 0; i < dimensions; ++i)
            query[i] = sketch_scalar(static_cast<const std::uint8_t*>(queries) + q * stride, (std::uint32_t)i, (scalar_kind_t)scalar_kind);
        const bool on = sketch_query_host(query.data(), sums_of_squares[q], (std::uint32_t)dimensions, d, coefficients.data());
        used[q] = on ? 1 : 0;
        for (std::size_t r = 0; r < count; ++r)
            bounds[q * count + r] = on ? sketch_bound_host(coefficients.data(), static_cast<const std::uint8_t*>(records) + r * sketch_record_bytes_k,
                                                           (std::uint32_t)dimensions)
                                       : -INFINITY;
    }
}

/** A snapshot's sketch read back: → the number of records it holds (0: no sketch); with `records` ([that many][128]), `directions`
 *  ([dimensions][64] f32) and `rows` ([that many][bytes per vector], the stored rows the records were made from) non-null, copies of them;
 *  `gram_defect`: what the records were made with. Call it once for the count, then with room. */
extern "C" __attribute__((visibility("default"))) uint64_t usearch_amd_test_sketch_read_back(const void* snapshot, void* records, float* directions,
                                                                                             void* rows, double* gram_defect,
                                                                                             usearch_amd_error_t* error) {
    const snapshot_t& s = *static_cast<const snapshot_t*>(snapshot);
    const std::uint64_t count = sketch_test_access_t::rows(s);
    fail(error, [&]() -> const char* {
        if (!count)
            return nullptr;
        const snapshot_view_t& view = s.view();
        UA_HIP(hipSetDevice(s.device()));
        UA_HIP(hipDeviceSynchronize());
        if (gram_defect)
            *gram_defect = sketch_test_access_t::gram_defect(s);
        if (records)
            UA_HIP(hipMemcpy(records, sketch_test_access_t::records(s), count * sketch_record_bytes_k, hipMemcpyDeviceToHost));
        if (directions)
            UA_HIP(hipMemcpy(directions, sketch_test_access_t::directions(s), (std::size_t)view.dimensions * sketch_columns_k * sizeof(float),
                             hipMemcpyDeviceToHost));
        if (rows)
            UA_HIP(hipMemcpy2D(rows, view.bytes_per_vector, view.vectors, view.row_stride, view.bytes_per_vector, count, hipMemcpyDeviceToHost));
        return nullptr;
    }());
    return count;
}
