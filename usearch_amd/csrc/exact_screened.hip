/**
 *  usearch_amd/csrc/exact_screened.hip — batched EXACT search of f32 rows with the wave kernel's bits: the matrix units screen,
 *  `exact_kernel`'s arithmetic measures.
 *
 *  `exact_kernel` (kernels.hpp) is bit-exact and reads every row once per query; the f32 tile of exact_tiled.hip reads a row once
 *  per 64 queries, but its sums are added in the matrix unit's order: its distances are within a bound, not those bits, and l2sq
 *  from Σa² + Σb² − 2Σab cancels. Here the tile's sums decide nothing but who CAN be among a query's `wanted` nearest:
 *
 *    1. `screen_kernel` — the 64-query × 128-row tile (`multiply_staged_chunk<scalar_f32_k>`, partitions of the rows as the tiled
 *       kernel has them). Per (query, row) the score s and the error e of screen_math.hpp, with `measure_rows` as the measuring
 *       kernel (`screen_g_lane_groups`).
 *       Per (query, partition) the wave that owns the query keeps the ordered list of the `wanted` lowest upper bounds s + e it has
 *       seen (one lane per entry); τ is the last of them, +inf while the list is filling. A row with s − e ≤ τ is a contender: its
 *       slot and s − e are appended to the (query, partition) buffer. τ only falls, so the buffer is a superset of what the final τ
 *       admits. Only the owning wave appends, tile after tile, lane after lane: a buffer is ascending in slot, its counter a
 *       register — no atomics.
 *    2. `exact_remeasure_kernel` (kernels.hpp, instantiated with `exact_kernel`'s lanes and unroll) — one wave per query drops the
 *       contenders above the query's final bound (the lowest τ of any partition), measures the rest with `measure_rows` and builds
 *       `top` by `exact_kernel`'s inserts in ascending slot order: that kernel's keys, distance bits, counts and padding.
 *    3. Hand-overs. The derivation of e assumes sums that neither overflow nor lose bits to underflow, so a row whose Σb² is outside
 *       [2⁻⁶⁰, 2⁶⁰] other than 0 (a NaN or an infinity in a row makes it so; under cos, whose closing special-cases it, 0 too) is
 *       always a contender and never counts towards τ; a query whose Σa² is (under cos, 0 too), a query one of whose buffers
 *       overflowed and a query that measured a NaN are handed over whole: `exact_search_device` runs for the compacted list of
 *       them and its results are scattered over theirs.
 *  Tombstones and rows the caller's `allow_bits` reject are skipped before they can enter a list or a buffer.
 */
#include <hip/hip_runtime.h>

#include <vector>

#include "common.hpp"
#include "device_math.hpp"
#include "device_scratch.hpp"
#include "engine.hpp"
#include "exact_plan.hpp"
#include "host_util.hpp"
#include "screen_math.hpp"

namespace usearch_amd {

namespace {

constexpr std::uint32_t row_live_k = 1u, row_out_of_band_k = 2u;

constexpr std::uint32_t screen_lds_bytes() {
    return staged_tile_bytes(tile_queries_k, tile_rows_k) + tile_queries_k * max_wanted_k * 4 + tile_queries_k * 4 * 4 + tile_rows_k * 4 * 3;
}

/**
 *  grid = (query tiles, row partitions), 256 threads = 4 waves. Products: wave w multiplies all 64 queries of the tile with rows
 *  [32w, 32w + 32) of every row tile (two 32 × 32 accumulators), the next chunk's global loads in flight meanwhile. Fold: wave w
 *  owns queries [16w, 16w + 16) — their lists, their buffers, their counters.
 *  contender_slots / contender_lows: [query][partition][capacity]; contender_counts / bounds: [query][partition] — the count keeps
 *  counting past `capacity` (nothing is stored there), which is how the overflow shows; handed: [query], zeroed by the caller.
 */
template <int metric_ak>
__global__ __launch_bounds__(256) void screen_kernel(const snapshot_view_t ix, const std::uint8_t* queries, std::uint64_t query_stride,
                                                     std::uint32_t query_count, std::uint32_t wanted, std::uint64_t rows_per_partition,
                                                     std::uint32_t capacity, const std::uint32_t* row_norms,
                                                     const std::uint32_t* query_norms, const std::uint32_t* allow_bits,
                                                     std::uint32_t* contender_slots, float* contender_lows,
                                                     std::uint32_t* contender_counts, float* bounds, std::uint32_t* handed) {
    constexpr int scalar_ak = scalar_f32_k;
    extern __shared__ __attribute__((aligned(16))) std::uint8_t lds[]; // the staged tile first: [64 + 128][pitch]
    float* tile_s = reinterpret_cast<float*>(lds);              // [64][129] scores, aliases the staging area after the products
    float* uppers = reinterpret_cast<float*>(lds + staged_tile_bytes(tile_queries_k, tile_rows_k)); // [64][max_wanted_k], ascending
    std::uint32_t* list_n = reinterpret_cast<std::uint32_t*>(uppers + tile_queries_k * max_wanted_k); // [64] entries of a list
    std::uint32_t* held_q = list_n + tile_queries_k;                       // [64] contenders appended so far
    float* roots_q = reinterpret_cast<float*>(held_q + tile_queries_k);    // [64] √Σa²
    std::uint32_t* given_q = reinterpret_cast<std::uint32_t*>(roots_q + tile_queries_k); // [64] 1 = not screened: outside the batch, or handed over
    float* squares_r = reinterpret_cast<float*>(given_q + tile_queries_k); // [128] Σb² of the tile's rows
    float* roots_r = squares_r + tile_rows_k;                              // [128] √Σb²
    std::uint32_t* flags_r = reinterpret_cast<std::uint32_t*>(roots_r + tile_rows_k); // [128] row_live_k | row_out_of_band_k

    const std::uint32_t thread = threadIdx.x, wave = thread / 64, lane = thread % 64;
    const std::uint32_t first_query = blockIdx.x * tile_queries_k, partition = blockIdx.y, partitions = gridDim.y;
    const std::uint64_t first_row = (std::uint64_t)partition * rows_per_partition;
    const std::uint64_t last_row = first_row + rows_per_partition < ix.size ? first_row + rows_per_partition : ix.size;
    const std::uint32_t bytes = ix.bytes_per_vector;
    const std::uint32_t chunks = (bytes + chunk_bytes_k - 1) / chunk_bytes_k;
    const float g = screen_g_lane_groups(ix.dimensions);
    constexpr bool zero_too = metric_ak == metric_cos_k;

    if (thread < tile_queries_k) {
        const bool inside = first_query + thread < query_count;
        const float a2 = inside ? __builtin_bit_cast(float, query_norms[first_query + thread]) : 0.f;
        const bool given = inside && square_out_of_band(a2, zero_too);
        list_n[thread] = 0, held_q[thread] = 0;
        roots_q[thread] = __builtin_sqrtf(a2);
        given_q[thread] = !inside || given ? 1u : 0u;
        if (given) // (every partition's workgroup stores the same word)
            handed[first_query + thread] = 1u;
    }
    __syncthreads();

    // ---- staging: the staged-tile stream of device_math.hpp, the next chunk's rows in flight while this one is multiplied
    staged_stream_gt stream(query_rows(queries, query_stride, first_query, query_count, bytes), stored_rows(ix, first_row, last_row), lds, thread);
    if (first_row < last_row)
        stream.fetch(first_row, 0);

    for (std::uint64_t tile_row = first_row; tile_row < last_row; tile_row += tile_rows_k) {
        f32x16_t acc[2];
        multiply_staged_tile<scalar_ak>(stream, tile_row, chunks, acc, [&] {
            if (thread < tile_rows_k) { // read after the chunks' barriers; written again after the fold's
                const std::uint64_t row = tile_row + thread;
                const bool inside = row < last_row;
                const float b2 = inside ? __builtin_bit_cast(float, row_norms[row]) : 0.f;
                const bool member = inside && row_is_allowed(ix, allow_bits, row);
                squares_r[thread] = b2, roots_r[thread] = __builtin_sqrtf(b2);
                flags_r[thread] = (member ? row_live_k : 0u) | (square_out_of_band(b2, zero_too) ? row_out_of_band_k : 0u);
            }
        });

        // ---- scores of the tile into LDS (the staging area is free now): S[query][row of the tile]
        store_screen_scores<metric_ak>(acc, squares_r, roots_r, wave, lane, tile_s);
        __syncthreads();

        // ---- fold: wave w owns queries [16w, 16w + 16). Per half tile (lane ↔ row): the uppers that beat τ enter the list in
        //      order, then the rows at or below the new τ are appended — in slot order, the counter is the wave's own.
        for (std::uint32_t local = 0; local < tile_queries_k / 4; ++local) {
            const std::uint32_t i = wave * (tile_queries_k / 4) + local;
            if (given_q[i]) // uniform
                continue;
            const std::uint32_t q = first_query + i;
            const float root_a = roots_q[i];
            float* list = uppers + i * max_wanted_k;
            std::uint32_t size = list_n[i], held = held_q[i];
            const std::uint64_t buffer = ((std::uint64_t)q * partitions + partition) * capacity;
#pragma unroll
            for (std::uint32_t half = 0; half < tile_rows_k / 64; ++half) {
                const std::uint32_t j = half * 64 + lane;
                const std::uint32_t flags = flags_r[j];
                const bool live = (flags & row_live_k) != 0, banded = !(flags & row_out_of_band_k);
                const float s = tile_s[i * (tile_rows_k + 1) + j], e = screen_error<metric_ak>(g, root_a, roots_r[j]);
                const float upper = s + e, lower = banded ? s - e : -__builtin_inff();
                float tau = size == wanted ? list[size - 1] : __builtin_inff();
                std::uint64_t pending = __ballot(live && banded && upper < tau);
                while (pending) {
                    const std::uint32_t source = (std::uint32_t)__ffsll((long long)pending) - 1;
                    pending &= pending - 1;
                    const float u = __shfl(upper, (int)source, 64);
                    if (!(u < tau))
                        continue;
                    // position = entries at or below the newcomer; the ones after it move one cell down
                    const bool mine = lane < size;
                    const float my_u = mine ? list[lane] : 0.f;
                    const std::uint32_t position = (std::uint32_t)__popcll(__ballot(mine && my_u <= u));
                    const std::uint32_t grown = size < wanted ? size + 1 : size;
                    if (mine && lane >= position && lane + 1 < grown)
                        list[lane + 1] = my_u;
                    if (lane == position)
                        list[position] = u;
                    size = grown;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                    tau = size == wanted ? list[size - 1] : __builtin_inff();
                }
                const bool contender = live && !(lower > tau);
                const std::uint64_t contenders = __ballot(contender);
                if (contender) {
                    const std::uint32_t at = held + (std::uint32_t)__popcll(contenders & ((1ull << lane) - 1ull));
                    if (at < capacity) {
                        contender_slots[buffer + at] = (std::uint32_t)(tile_row + j);
                        contender_lows[buffer + at] = lower;
                    }
                }
                held += (std::uint32_t)__popcll(contenders);
            }
            if (lane == 0)
                list_n[i] = size, held_q[i] = held;
        }
        __syncthreads(); // the tile's scores are consumed: the area becomes staging again, the norms the next tile's
    }

    // ---- this partition's count and bound per query; a buffer that overflowed hands its query over
    if (thread < tile_queries_k && !given_q[thread]) {
        const std::uint64_t cell = (std::uint64_t)(first_query + thread) * partitions + partition;
        const std::uint32_t size = list_n[thread], held = held_q[thread];
        contender_counts[cell] = held;
        bounds[cell] = size == wanted ? uppers[thread * max_wanted_k + size - 1] : __builtin_inff();
        if (held > capacity)
            handed[first_query + thread] = 1u;
    }
}

/// The handed-over queries' rows, one after the other: what `exact_search_device` takes as its batch.
__global__ __launch_bounds__(256) void gather_queries_kernel(const std::uint8_t* queries, std::uint64_t stride, std::uint32_t bytes,
                                                             const std::uint32_t* list, std::uint32_t listed, std::uint8_t* out) {
    const std::uint64_t total = (std::uint64_t)listed * bytes;
    for (std::uint64_t cell = (std::uint64_t)blockIdx.x * 256 + threadIdx.x; cell < total; cell += (std::uint64_t)gridDim.x * 256) {
        const std::uint64_t entry = cell / bytes, byte = cell % bytes;
        out[cell] = queries[list[entry] * stride + byte];
    }
}

/// Rows `exact_kernel` measures for a query: the members that are no tombstones and pass `allow_bits`. One integer atomic per wave.
__global__ __launch_bounds__(256) void count_allowed_kernel(const snapshot_view_t ix, const std::uint32_t* allow_bits,
                                                            unsigned long long* out) {
    for (std::uint64_t base = ((std::uint64_t)blockIdx.x * 256 + threadIdx.x) / 64 * 64; base < ix.size; base += (std::uint64_t)gridDim.x * 256) {
        const std::uint64_t row = base + threadIdx.x % 64;
        const std::uint64_t mask = __ballot(row < ix.size && row_is_allowed(ix, allow_bits, row));
        if (threadIdx.x % 64 == 0 && mask)
            atomicAdd(out, (unsigned long long)__popcll(mask));
    }
}

/// The wave kernel's results for the handed-over queries, over whatever the closing pass left in their places.
__global__ __launch_bounds__(256) void scatter_results_kernel(const std::uint32_t* list, std::uint32_t listed, std::uint32_t wanted,
                                                              const std::uint64_t* from_keys, const float* from_distances,
                                                              const std::uint64_t* from_counts, const unsigned long long* allowed,
                                                              std::uint64_t* keys, float* distances, std::uint64_t* counts,
                                                              std::uint64_t* remeasured) {
    const std::uint64_t total = (std::uint64_t)listed * wanted;
    for (std::uint64_t cell = (std::uint64_t)blockIdx.x * 256 + threadIdx.x; cell < total; cell += (std::uint64_t)gridDim.x * 256) {
        const std::uint64_t entry = cell / wanted, position = cell % wanted, out = (std::uint64_t)list[entry] * wanted + position;
        keys[out] = from_keys[cell];
        reinterpret_cast<std::uint32_t*>(distances)[out] = reinterpret_cast<const std::uint32_t*>(from_distances)[cell];
        if (position == 0) {
            counts[list[entry]] = from_counts[entry];
            if (remeasured)
                remeasured[list[entry]] = *allowed;
        }
    }
}

template <int metric_ak>
hipError_t launch_screen(const snapshot_view_t& view, const std::uint8_t* queries, std::uint64_t query_stride, std::uint32_t count,
                         std::uint32_t wanted, const exact_screened_plan_t& plan, const std::uint32_t* row_norms,
                         const std::uint32_t* query_norms, const std::uint32_t* allow_bits, std::uint32_t* contender_slots,
                         float* contender_lows, std::uint32_t* contender_counts, float* bounds, std::uint32_t* handed, hipStream_t stream) {
    auto kernel = screen_kernel<metric_ak>;
    constexpr std::uint32_t lds = screen_lds_bytes();
    static_assert(lds <= 64 * 1024, "the screen's lists and staging fit the LDS a kernel gets unasked");
    hipLaunchKernelGGL(kernel, dim3((std::uint32_t)plan.query_tiles, (std::uint32_t)plan.partitions), dim3(256), lds, stream, view,
                       queries, query_stride, count, wanted, plan.rows_per_partition, (std::uint32_t)plan.capacity, row_norms,
                       query_norms, allow_bits, contender_slots, contender_lows, contender_counts, bounds, handed);
    return hipGetLastError();
}

} // namespace

bool exact_screened_available(metric_kind_t metric, scalar_kind_t scalar, std::size_t wanted) {
    return exact_screened_pair(metric, scalar, wanted); // the table: exact_plan.hpp
}

const char* exact_search_screened_device(const exact_call_t& call) {
    const snapshot_view_t& view = call.view;
    const std::size_t count = call.count, wanted = call.wanted, stride_bytes = call.stride_bytes;
    const std::uint32_t* allow_bits = call.allow_bits;
    std::uint64_t* remeasured = call.remeasured;
    hipStream_t stream = call.stream;
    float* kernel_ms = call.kernel_ms;
    if (!count)
        return nullptr;
    if (count >= none_slot_k || view.size >= none_slot_k)
        return "Batch is too large";
    if (view.size == 0) { // nothing to screen: the wave route's empty results, nothing measured
        if (remeasured)
            UA_HIP(hipMemsetAsync(remeasured, 0, count * 8, stream));
        return exact_search_device(call);
    }
    // partitions, the capacity of a (query, partition) buffer, the scratch in all: exact_plan.hpp
    std::size_t free_bytes = 0, total_bytes = 0;
    UA_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
    exact_screened_plan_t plan;
    if (const char* refusal = plan_exact_screened(view.size, view.bytes_per_vector, view.row_stride, count, wanted, free_bytes / 2, plan))
        return refusal;
    const std::uint64_t cells = count * plan.partitions;

    event_pair_t events;
    device_scratch_t scratch(current_device_k); // the caller has selected the device the view lives on
    std::uint32_t *row_norms = nullptr, *query_norms = nullptr, *contender_slots = nullptr, *contender_counts = nullptr, *handed = nullptr;
    float *contender_lows = nullptr, *bounds = nullptr;
    UA_HIP(scratch.allocate(&row_norms, view.size * 4));
    UA_HIP(scratch.allocate(&query_norms, count * 4));
    UA_HIP(scratch.allocate(&contender_slots, cells * plan.capacity * 4));
    UA_HIP(scratch.allocate(&contender_lows, cells * plan.capacity * 4));
    UA_HIP(scratch.allocate(&contender_counts, cells * 4));
    UA_HIP(scratch.allocate(&bounds, cells * 4));
    UA_HIP(scratch.allocate(&handed, count * 4));
    // (a handed-over query's cells of the two arrays below are never written by the screen and never read by the closing pass)
    UA_HIP(hipMemsetAsync(handed, 0, count * 4, stream));
    if (kernel_ms) {
        UA_HIP(events.create());
        UA_HIP(hipEventRecord(events.begin, stream));
    }
    const std::uint8_t* query_bytes = static_cast<const std::uint8_t*>(call.queries);
    UA_HIP(launch_exact_norms<scalar_f32_k>(view, query_bytes, count, stride_bytes, row_norms, query_norms, stream));
    exact_remeasure_params_t p{};
    p.lanes = call.lanes;
    p.lds_bytes = exact_kernel_lds_bytes(view, call.scalar, wanted);
    p.stream = stream;
    p.queries = query_bytes;
    p.query_stride = stride_bytes;
    p.query_count = (std::uint32_t)count;
    p.wanted = (std::uint32_t)wanted;
    p.partitions = (std::uint32_t)plan.partitions;
    p.capacity = (std::uint32_t)plan.capacity;
    p.contender_slots = contender_slots;
    p.contender_lows = contender_lows;
    p.contender_counts = contender_counts;
    p.bounds = bounds;
    p.map_keys = call.map_keys ? 1u : 0u;
    p.handed = handed;
    p.out_distances = call.distances;
    p.out_keys = call.keys;
    p.out_counts = call.counts;
    p.remeasured = remeasured;
#define UA_SCREENED(m, name)                                                                                                           \
    if (call.metric == m) {                                                                                                            \
        UA_HIP(launch_screen<m>(view, query_bytes, stride_bytes, (std::uint32_t)count, (std::uint32_t)wanted, plan, row_norms,         \
                                query_norms, allow_bits, contender_slots, contender_lows, contender_counts, bounds, handed, stream));  \
        UA_HIP(launch_exact_remeasure_##name(p, view));                                                                                \
    }
    UA_SCREENED(metric_cos_k, cos_f32)
    UA_SCREENED(metric_ip_k, ip_f32)
    UA_SCREENED(metric_l2sq_k, l2sq_f32)
#undef UA_SCREENED
    if (kernel_ms)
        UA_HIP(hipEventRecord(events.end, stream));

    // ---- the handed-over queries, compacted on the host: their number sizes the wave kernel's launch
    std::vector<std::uint32_t> flags(count), list;
    UA_HIP(hipStreamSynchronize(stream));
    UA_HIP(hipMemcpy(flags.data(), handed, count * 4, hipMemcpyDeviceToHost));
    if (kernel_ms)
        UA_HIP(hipEventElapsedTime(kernel_ms, events.begin, events.end));
    for (std::size_t q = 0; q < count; ++q)
        if (flags[q])
            list.push_back((std::uint32_t)q);
    if (list.empty())
        return nullptr;
    const std::size_t listed = list.size(), bytes = view.bytes_per_vector;
    std::uint32_t* d_list = nullptr;
    std::uint8_t* gathered = nullptr;
    unsigned long long* allowed = nullptr;
    float wave_ms = 0.f;
    exact_call_t wave = call; // the same search of the gathered queries, into lists of their own
    UA_HIP(scratch.allocate(&d_list, listed * 4));
    UA_HIP(scratch.allocate(&gathered, listed * bytes));
    UA_HIP(scratch.allocate(&wave.keys, listed * wanted * 8));
    UA_HIP(scratch.allocate(&wave.distances, listed * wanted * 4));
    UA_HIP(scratch.allocate(&wave.counts, listed * 8));
    UA_HIP(scratch.allocate(&allowed, 8));
    UA_HIP(hipMemcpy(d_list, list.data(), listed * 4, hipMemcpyHostToDevice));
    UA_HIP(hipMemsetAsync(allowed, 0, 8, stream));
    hipLaunchKernelGGL(gather_queries_kernel, dim3((unsigned)std::min<std::uint64_t>((listed * bytes + 255) / 256, 1u << 16)), dim3(256), 0,
                       stream, query_bytes, (std::uint64_t)stride_bytes, (std::uint32_t)bytes, (const std::uint32_t*)d_list,
                       (std::uint32_t)listed, gathered);
    UA_HIP(hipGetLastError());
    hipLaunchKernelGGL(count_allowed_kernel, dim3((unsigned)std::min<std::uint64_t>((view.size + 255) / 256, 1u << 16)), dim3(256), 0, stream,
                       view, allow_bits, allowed);
    UA_HIP(hipGetLastError());
    wave.queries = gathered, wave.count = listed, wave.stride_bytes = bytes;
    wave.kernel_ms = kernel_ms ? &wave_ms : nullptr;
    if (const char* error = exact_search_device(wave))
        return error;
    hipLaunchKernelGGL(scatter_results_kernel, dim3((unsigned)std::min<std::uint64_t>((listed * wanted + 255) / 256, 1u << 16)), dim3(256), 0,
                       stream, (const std::uint32_t*)d_list, (std::uint32_t)listed, (std::uint32_t)wanted, (const std::uint64_t*)wave.keys,
                       (const float*)wave.distances, (const std::uint64_t*)wave.counts, (const unsigned long long*)allowed, call.keys,
                       call.distances, call.counts, remeasured);
    UA_HIP(hipGetLastError());
    UA_HIP(hipStreamSynchronize(stream));
    if (kernel_ms)
        *kernel_ms += wave_ms;
    return nullptr;
}

} // namespace usearch_amd
