/**
 *  usearch_amd/csrc/exact_bits.hip — many-to-many EXACT search over bit vectors: hamming, tanimoto (= jaccard) and sorensen over b1.
 *
 *  The same argument that made the float kinds a GEMM (exact_tiled.hip): every query meets every row, so a row is read once for a
 *  whole tile of queries instead of once per query. The inner product is popcount(a ∧ b) on the vector ALU — no matrix unit — and
 *  everything is an integer until one IEEE division closes it, so the results carry the bits of the wave-per-query kernel
 *  (`exact_kernel` of kernels.hpp), NaN (0 / 0, two empty sets) included: `closing_distance` of device_math.hpp closes both.
 *
 *  Shape. A workgroup is four INDEPENDENT waves that meet one partition of the rows together (they share the rows through the
 *  vector cache, nothing else: no barrier in the kernel). A wave owns 64 queries and their lists. Lane ↔ row: per step the lane
 *  fetches a 16-byte piece of its row into registers, and the wave walks its queries, whose words arrive at a wave-uniform address
 *  — from the padded copy of the batch through the scalar cache, so they are scalar operands of the `v_and` / `v_xor` and cost
 *  neither vector registers nor LDS bandwidth (a broadcast `ds_read_b128` per 8 vector instructions on four SIMDs would keep the
 *  LDS array busy all the time). After a query's words the wave holds 64 sums, one per lane: exactly what the fold consumes — a
 *  ballot of the lanes that go before the query's k-th best, then ordered inserts. Rows of any length: a lane holds
 *  `bits_block_k` accumulators, one per query of a block, while the row passes 16 bytes at a time (pieces after a block's first
 *  come back from the vector cache); the accumulators are registers whatever the row's length, there is no second path.
 *
 *  Order. A candidate is ONE 64-bit integer: high word = the rank of its distance (0 for a NaN, else the ordered bits of the float;
 *  for hamming the count itself), low word = ~slot. Integer `<` on it is the total order of `search_exact_` — NaN first, distance ↑,
 *  later slot first among equals — whatever the order of arrival. A query's k-th best lives in the registers of
 *  lane (query mod 64) and is read with `v_readlane`; all ones while the list is filling: everything enters.
 *
 *  hamming takes |a⊕b| directly (xor + bcnt: the same two instructions per word, and no stored popcounts to fetch or to add);
 *  tanimoto and sorensen take |a∧b| and the popcounts of both sides, computed once per call by two small kernels.
 */
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "device_math.hpp"
#include "device_scratch.hpp"
#include "engine.hpp"
#include "exact_plan.hpp"
#include "host_util.hpp"

namespace usearch_amd {

namespace {

/// Read-only for the whole launch and addressed uniformly: the constant address space makes these scalar loads.
using u32x4_t = std::uint32_t __attribute__((ext_vector_type(4))); // (a native vector: `uint4` is a class, whose copies know one address space)
using constant_pieces_t = const __attribute__((address_space(4))) u32x4_t*;
using constant_words_t = const __attribute__((address_space(4))) std::uint32_t*;

/// sum + popcount(a ∧ b) — a ⊕ b for hamming — in two vector instructions: the logic operation with the query's word as its scalar
/// operand, and the accumulating `v_bcnt_u32_b32`. (Spelled out: left to itself the compiler starts every 16-byte piece with three
/// counts from zero and joins them with a three-way add, nine instructions where eight do.)
template <int metric_ak> __device__ __forceinline__ int bits_product(std::uint32_t a, std::uint32_t b, int sum) {
    const std::uint32_t common = metric_ak == metric_hamming_k ? a ^ b : a & b;
    int total;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(total) : "v"(common), "v"(sum));
    return total;
}

/// The high word of a candidate: smaller goes first. A NaN ranks 0; no number does (the ordered bits of a float are all ones for one
/// bit pattern only, itself a NaN, and ≥ 2^31 for everything that is not negative).
template <int metric_ak> __device__ __forceinline__ std::uint32_t distance_rank(int sum, std::uint32_t a_count, std::uint32_t b_count) {
    if constexpr (metric_ak == metric_hamming_k)
        return (std::uint32_t)sum;
    else {
        const float d = closing_distance<metric_ak, scalar_b1x8_k, l2sq_nan_stays_k>(sum, a_count, b_count);
        return d == d ? ordered_bits(d) : 0u;
    }
}

/// … and back. The one NaN there is comes from two empty sets — sums of zero — and is computed again, by the same division on the same
/// hardware, from a zero the compiler cannot see through (`zero`): its bits are the wave kernel's, whatever they are.
template <int metric_ak> __device__ __forceinline__ float distance_of_rank(std::uint32_t rank, int zero) {
    if constexpr (metric_ak == metric_hamming_k)
        return closing_distance<metric_ak, scalar_b1x8_k, l2sq_nan_stays_k>((int)rank, 0u, 0u);
    else
        return rank ? from_ordered_bits(rank)
                    : closing_distance<metric_ak, scalar_b1x8_k, l2sq_nan_stays_k>(zero, (std::uint32_t)zero, (std::uint32_t)zero);
}

/// The batch as the kernel reads it: whole 16-byte pieces of every query, whole waves of 64 queries, zeros where a row or the batch
/// ends — and every query's popcount. Laid out [block of 16 queries][piece][query of the block][4 words]: what a wave needs for one
/// piece of one block of accumulators is 256 consecutive bytes. Byte by byte: a caller's rows have any pitch and any alignment.
/// A thread per query, grid-stride.
__global__ __launch_bounds__(256) void bits_pad_queries_kernel(const std::uint8_t* queries, std::uint64_t stride, std::uint64_t count,
                                                               std::uint32_t bytes, std::uint32_t* padded, std::uint64_t pieces,
                                                               std::uint64_t padded_rows, std::uint32_t* counts) {
    for (std::uint64_t row = (std::uint64_t)blockIdx.x * 256 + threadIdx.x; row < padded_rows; row += (std::uint64_t)gridDim.x * 256) {
        std::uint32_t total = 0;
        for (std::uint64_t w = 0; w < pieces * 4; ++w) {
            std::uint32_t word = 0;
            if (row < count)
                for (std::uint32_t b = 0; b < 4 && w * 4 + b < bytes; ++b)
                    word |= (std::uint32_t)queries[row * stride + w * 4 + b] << (8 * b);
            padded[(((row / bits_block_k) * pieces + w / 4) * bits_block_k + row % bits_block_k) * 4 + w % 4] = word;
            total += (std::uint32_t)__popc(word);
        }
        counts[row] = total;
    }
}

/// popcount of every stored row (zero padded to its pitch, so whole pieces count nothing extra): the b1 analogue of
/// `row_norms_kernel`. A thread per row, grid-stride: 125 M rows are more threads than a launch may have.
__global__ __launch_bounds__(256) void bits_row_counts_kernel(const std::uint8_t* rows, std::uint64_t count, std::uint64_t stride,
                                                              std::uint32_t pieces, std::uint32_t* out) {
    for (std::uint64_t row = (std::uint64_t)blockIdx.x * 256 + threadIdx.x; row < count; row += (std::uint64_t)gridDim.x * 256) {
        const uint4* p = reinterpret_cast<const uint4*>(rows + row * stride);
        std::uint32_t total = 0;
        for (std::uint32_t piece = 0; piece < pieces; ++piece) {
            const uint4 v = p[piece];
            total += (std::uint32_t)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
        }
        out[row] = total;
    }
}

/**
 *  grid = (query tiles of 256, row partitions), 256 threads = 4 waves; wave w of workgroup (x, y) takes queries [256x + 64w, + 64)
 *  through rows [y · rows_per_partition, + rows_per_partition). `padded_queries`: the pad kernel's [blocks of 16][pieces][16] × 16 bytes.
 *  LDS: [4][64][wanted] candidates of 8 bytes, a wave's lists. out_*: [partition][query][wanted], like the other exact kernels'.
 */
template <int metric_ak>
__global__ __launch_bounds__(bits_waves_k * 64) void exact_bits_kernel(const snapshot_view_t ix, const uint4* padded_queries,
                                                                       std::uint32_t pieces, std::uint32_t query_count,
                                                                       std::uint32_t wanted, std::uint64_t rows_per_partition,
                                                                       const std::uint32_t* row_counts, const std::uint32_t* query_counts,
                                                                       std::uint32_t map_keys, const std::uint32_t* allow_bits,
                                                                       float* out_distances, std::uint64_t* out_keys,
                                                                       std::uint64_t* out_counts) {
    constexpr bool counted = metric_ak != metric_hamming_k; // the closing arithmetic wants |a| and |b|
    extern __shared__ __attribute__((aligned(16))) std::uint8_t lds[];
    const std::uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64), lane = threadIdx.x % 64;
    const std::uint64_t first_query = ((std::uint64_t)blockIdx.x * bits_waves_k + wave) * bits_wave_queries_k;
    if (first_query >= query_count) // the batch ends before this wave's queries; the waves never meet, so it may leave
        return;
    std::uint64_t* lists = reinterpret_cast<std::uint64_t*>(lds) + (std::uint64_t)wave * bits_wave_queries_k * wanted;
    const std::uint32_t partition = blockIdx.y;
    const std::uint64_t first_row = (std::uint64_t)partition * rows_per_partition;
    const std::uint64_t last_row = first_row + rows_per_partition < ix.size ? first_row + rows_per_partition : ix.size;
    const constant_pieces_t query_pieces = (constant_pieces_t)(padded_queries + first_query * pieces); // (whole blocks: see the pad kernel)
    const constant_words_t a_counts = (constant_words_t)(query_counts + first_query);

    // lane i: the state of the wave's query i — its k-th best (all ones while the list is filling) and the entries its list holds
    std::uint32_t kth_rank = 0xFFFFFFFFu, kth_low = 0xFFFFFFFFu, filled = 0;

    /// Offers the candidates of the lanes in `pending` to the list of the wave's query `query`, lowest lane first; the whole wave
    /// calls it together. An ordered insert, one lane per entry.
    auto offer = [&](std::uint32_t query, std::uint32_t rank, std::uint32_t low, std::uint64_t pending) {
        std::uint64_t* list = lists + (std::uint64_t)query * wanted;
        std::uint32_t size = (std::uint32_t)__builtin_amdgcn_readlane((int)filled, (int)query);
        std::uint64_t kth = ((std::uint64_t)(std::uint32_t)__builtin_amdgcn_readlane((int)kth_rank, (int)query) << 32) |
                            (std::uint32_t)__builtin_amdgcn_readlane((int)kth_low, (int)query);
        while (pending) {
            const int source = __ffsll((long long)pending) - 1;
            pending &= pending - 1;
            const std::uint64_t newcomer = ((std::uint64_t)(std::uint32_t)__builtin_amdgcn_readlane((int)rank, source) << 32) |
                                           (std::uint32_t)__builtin_amdgcn_readlane((int)low, source);
            if (!(newcomer < kth)) // an earlier one of this step has moved the k-th best in front of it
                continue;
            const bool mine = lane < size;
            const std::uint64_t entry = mine ? list[lane] : ~0ull;
            // position = entries that go before the newcomer; the ones at and after it move one cell down
            const std::uint32_t position = (std::uint32_t)__popcll(__builtin_amdgcn_ballot_w64(mine && entry < newcomer));
            const std::uint32_t grown = size < wanted ? size + 1 : size;
            if (mine && lane >= position && lane + 1 < grown)
                list[lane + 1] = entry;
            if (lane == position)
                list[position] = newcomer;
            size = grown;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            if (size == wanted)
                kth = list[wanted - 1];
        }
        if (lane == query)
            filled = size, kth_rank = (std::uint32_t)(kth >> 32), kth_low = (std::uint32_t)kth;
    };

    for (std::uint64_t base = first_row; base < last_row; base += bits_rows_k) {
        const std::uint64_t row = base + lane;
        const bool inside = row < last_row;
        // the `allow` predicate as `exact_kernel` has it: tombstones, then the caller's one bit per slot
        bool member = inside && (!ix.has_tombstones || ix.keys[row] != free_key_k);
        if (allow_bits && member)
            member = ((allow_bits[row >> 5] >> (row & 31)) & 1u) != 0;
        const std::uint64_t members = __ballot(member);
        if (!members)
            continue;
        const std::uint64_t fetched = inside ? row : first_row; // a lane past the end reads a row that exists, and is never a member
        const uint4* row_pieces = reinterpret_cast<const uint4*>(ix.vectors + fetched * ix.row_stride);
        const std::uint32_t b_count = counted ? row_counts[fetched] : 0u;
        const std::uint32_t low = ~(std::uint32_t)row;
        const uint4 head = row_pieces[0];
        for (std::uint32_t block = 0; block < bits_wave_queries_k / bits_block_k; ++block) {
            int sums[bits_block_k];
#pragma unroll
            for (int j = 0; j < bits_block_k; ++j)
                sums[j] = 0;
            for (std::uint32_t piece = 0; piece < pieces; ++piece) {
                const uint4 b = piece ? row_pieces[piece] : head;
#pragma unroll
                for (int j = 0; j < bits_block_k; ++j) {
                    // the block's 16 queries lie next to each other for every piece: 256 bytes at constant offsets from one address
                    const u32x4_t a = query_pieces[((std::uint64_t)block * pieces + piece) * bits_block_k + j];
                    sums[j] = bits_product<metric_ak>(a[0], b.x, sums[j]);
                    sums[j] = bits_product<metric_ak>(a[1], b.y, sums[j]);
                    sums[j] = bits_product<metric_ak>(a[2], b.z, sums[j]);
                    sums[j] = bits_product<metric_ak>(a[3], b.w, sums[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < bits_block_k; ++j) {
                const std::uint32_t query = block * bits_block_k + j;
                const std::uint32_t rank = distance_rank<metric_ak>(sums[j], counted ? a_counts[query] : 0u, b_count);
                const std::uint64_t bar = ((std::uint64_t)(std::uint32_t)__builtin_amdgcn_readlane((int)kth_rank, (int)query) << 32) |
                                          (std::uint32_t)__builtin_amdgcn_readlane((int)kth_low, (int)query);
                // two lane reads and one 64-bit compare per query and 64 rows; the members' mask is scalar arithmetic
                const std::uint64_t pending = __builtin_amdgcn_ballot_w64((((std::uint64_t)rank << 32) | low) < bar) & members;
                if (pending)
                    offer(query, rank, low, pending);
            }
        }
    }

    // ---- this partition's lists, [partition][query][wanted]; cells past a list's end: key 0 and the signalling NaN
    int zero = 0;
    asm volatile("" : "+v"(zero));
    for (std::uint32_t query = 0; query < bits_wave_queries_k && first_query + query < query_count; ++query) {
        const std::uint32_t size = (std::uint32_t)__builtin_amdgcn_readlane((int)filled, (int)query);
        const std::uint64_t cells = (std::uint64_t)partition * query_count + first_query + query;
        if (lane < wanted) {
            std::uint64_t key = 0;
            std::uint32_t bits = signaling_nan_bits_k;
            if (lane < size) {
                const std::uint64_t entry = lists[(std::uint64_t)query * wanted + lane];
                const std::uint32_t slot = ~(std::uint32_t)entry;
                key = map_keys ? ix.keys[slot] : (std::uint64_t)slot;
                bits = __builtin_bit_cast(std::uint32_t, distance_of_rank<metric_ak>((std::uint32_t)(entry >> 32), zero));
            }
            out_keys[cells * wanted + lane] = key;
            reinterpret_cast<std::uint32_t*>(out_distances)[cells * wanted + lane] = bits;
        }
        if (lane == 0)
            out_counts[cells] = size;
    }
}

constexpr std::uint32_t bits_count_blocks_k = 1u << 16; ///< the grid of the two popcount launches at most (both are grid-stride)

template <int metric_ak>
hipError_t launch_bits(const snapshot_view_t& view, const std::uint8_t* queries, std::uint64_t query_stride, std::uint32_t query_count,
                       std::uint32_t wanted, const exact_bits_plan_t& plan, std::uint32_t* padded, std::uint32_t* row_counts,
                       std::uint32_t* query_counts, bool map_keys, const std::uint32_t* allow_bits, float* out_distances,
                       std::uint64_t* out_keys, std::uint64_t* out_counts, hipStream_t stream) {
    const std::uint32_t pieces = (std::uint32_t)(plan.padded_query_bytes / 16);
    hipLaunchKernelGGL(bits_pad_queries_kernel, dim3((unsigned)std::min<std::uint64_t>((plan.padded_queries + 255) / 256, bits_count_blocks_k)),
                       dim3(256), 0, stream, queries, query_stride, (std::uint64_t)query_count, view.bytes_per_vector, padded,
                       (std::uint64_t)pieces, plan.padded_queries, query_counts);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && metric_ak != metric_hamming_k) {
        hipLaunchKernelGGL(bits_row_counts_kernel, dim3((unsigned)std::min<std::uint64_t>((view.size + 255) / 256, bits_count_blocks_k)),
                           dim3(256), 0, stream, view.vectors, view.size, (std::uint64_t)view.row_stride, pieces, row_counts);
        e = hipGetLastError();
    }
    if (e != hipSuccess)
        return e;
    auto kernel = exact_bits_kernel<metric_ak>;
    if (plan.lds_bytes > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)plan.query_tiles, (unsigned)plan.partitions), dim3(bits_waves_k * 64),
                       (std::uint32_t)plan.lds_bytes, stream, view, reinterpret_cast<const uint4*>(padded), pieces, query_count, wanted,
                       plan.rows_per_partition, (const std::uint32_t*)row_counts, (const std::uint32_t*)query_counts,
                       map_keys ? 1u : 0u, allow_bits, out_distances, out_keys, out_counts);
    return hipGetLastError();
}

} // namespace

const char* exact_search_bits_device(metric_kind_t metric, const snapshot_view_t& view, const void* queries, std::size_t count,
                                     std::size_t stride_bytes, std::size_t wanted, bool map_keys, std::uint64_t* keys, float* distances,
                                     std::uint64_t* counts, hipStream_t stream, float* kernel_ms, const std::uint32_t* allow_bits) {
    if (kernel_ms)
        *kernel_ms = 0.f;
    if (!exact_bits_pair(metric, scalar_b1x8_k, wanted))
        return "No tiled exact-search kernel for this metric / scalar kind / result count";
    if (!count)
        return nullptr;
    if (count >= none_slot_k || view.size >= none_slot_k)
        return "Batch is too large";
    exact_bits_plan_t plan; // how many partitions, which workgroup takes which (query tile, partition): exact_plan.hpp
    if (const char* refusal = plan_exact_bits(view.size, view.bytes_per_vector, view.row_stride, count, wanted, plan))
        return refusal;
    const bool counted = metric != metric_hamming_k;

    event_pair_t events;
    device_scratch_t scratch(current_device_k); // the caller has selected the device the view lives on
    std::uint32_t *padded = nullptr, *row_counts = nullptr, *query_counts = nullptr;
    float* partial_distances = nullptr;
    std::uint64_t *partial_keys = nullptr, *partial_counts = nullptr;
    UA_HIP(scratch.allocate(&padded, plan.padded_queries * plan.padded_query_bytes));
    UA_HIP(scratch.allocate(&query_counts, plan.padded_queries * 4));
    if (counted)
        UA_HIP(scratch.allocate(&row_counts, view.size * 4));
    UA_HIP(scratch.allocate(&partial_distances, plan.partitions * count * wanted * 4));
    UA_HIP(scratch.allocate(&partial_keys, plan.partitions * count * wanted * 8));
    UA_HIP(scratch.allocate(&partial_counts, plan.partitions * count * 8));
    if (kernel_ms) {
        UA_HIP(events.create());
        UA_HIP(hipEventRecord(events.begin, stream));
    }
    const std::uint8_t* query_bytes = static_cast<const std::uint8_t*>(queries);
    hipError_t e = hipErrorInvalidValue;
#define UA_BITS(m)                                                                                                                     \
    e = launch_bits<m>(view, query_bytes, stride_bytes, (std::uint32_t)count, (std::uint32_t)wanted, plan, padded, row_counts,        \
                       query_counts, map_keys, allow_bits, partial_distances, partial_keys, partial_counts, stream)
    if (metric == metric_hamming_k)
        UA_BITS(metric_hamming_k);
    else if (metric == metric_sorensen_k)
        UA_BITS(metric_sorensen_k);
    else // tanimoto, and jaccard, which is tanimoto over bit sets (index_plugins.hpp:2003-2004)
        UA_BITS(metric_tanimoto_k);
#undef UA_BITS
    if (e != hipSuccess)
        return hip_message(e);
    if (kernel_ms)
        UA_HIP(hipEventRecord(events.end, stream));
    if (const char* error = merge_shards_device(partial_distances, partial_keys, partial_counts, plan.partitions, count, wanted, distances,
                                                keys, counts, stream, false))
        return error;
    if (kernel_ms)
        UA_HIP(hipEventElapsedTime(kernel_ms, events.begin, events.end));
    return nullptr;
}

} // namespace usearch_amd
