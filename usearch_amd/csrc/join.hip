/**
 *  usearch_amd/csrc/join.hip — semantic join (join.hpp): preference lists from the existing walk / exact kernels, then the
 *  matching as rounds of three plain launches over compact lists of free men and touched women:
 *
 *    propose  every free man with list entries left offers to his next woman: one 64-bit atomicMin on
 *             offer[w] = (order-preserving bits of d) << 32 | man, so the nearest offer wins and the lowest man among equals;
 *    resolve  every touched woman compares that offer with her husband's distance and switches only when it is strictly
 *             nearer (index.hpp:4502); the displaced husband goes onto the next free list; offer[w] is reset;
 *    requeue  a proposer who did not win goes onto the next free list.
 *
 *  The host reads one counter per round (the next free list's length) and stops when it is zero. The women's distance to her
 *  husband is the winning proposal's own d(man, woman), as the walk computed it; the reference recomputes it with the arguments
 *  swapped (index.hpp:4497-4498) — tests/test_join_model.py checks that the two agree bit for bit.
 */
#include "join.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>

#include "device_math.hpp" // ordered_bits: the unsigned order of the result = the float order of d (negative ip distances included)
#include "device_scratch.hpp"
#include "host_util.hpp"

namespace usearch_amd {

namespace {

constexpr unsigned join_threads_k = 256;
constexpr std::uint64_t no_offer_k = ~0ull;
constexpr std::size_t list_chunk_k = std::size_t(1) << 20; ///< men per list search call
constexpr std::uint64_t exact_width_limit_k = 4096;         ///< `exact_search_device`'s largest `wanted`

enum : unsigned { touched_k = 0, lazy_k = 1, next_free_k = 2, counters_k = 4 };
enum : unsigned { proposals_k = 0, engagements_k = 1, sum_visited_k = 2, sum_computed_k = 3, totals_k = 4 };

/// Appends `value` for every lane with `take` to `list`: one atomic per wave (ballot + rank among the taking lanes). Every lane of
/// the wave must reach it. Returns the lane's position in `list` (meaningless where `take` is false).
__device__ inline std::uint32_t wave_append(bool take, std::uint32_t value, std::uint32_t* list, std::uint32_t* counter) {
    const std::uint64_t mask = __ballot(take);
    if (!mask)
        return 0;
    const std::uint32_t leader = (std::uint32_t)__ffsll((unsigned long long)mask) - 1u;
    const std::uint32_t lane = threadIdx.x & 63u;
    std::uint32_t base = 0;
    if (lane == leader)
        base = atomicAdd(counter, (std::uint32_t)__popcll(mask));
    base = (std::uint32_t)__shfl((int)base, (int)leader, 64);
    const std::uint32_t position = base + __builtin_amdgcn_mbcnt_hi((std::uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((std::uint32_t)mask, 0u));
    if (take)
        list[position] = value;
    return position;
}

/// Adds the wave's count of `p` to `total`: one atomic per wave.
__device__ inline void wave_count(bool p, unsigned long long* total) {
    const std::uint64_t mask = __ballot(p);
    if (mask && (threadIdx.x & 63u) == (std::uint32_t)__ffsll((unsigned long long)mask) - 1u)
        atomicAdd(total, (unsigned long long)__popcll(mask));
}

__device__ inline void offer(std::uint32_t man, std::uint32_t woman, float d, std::uint64_t* offers, std::uint32_t* proposed_to,
                             bool& first) {
    const std::uint64_t bid = ((std::uint64_t)ordered_bits(d) << 32) | man;
    first = atomicMin(reinterpret_cast<unsigned long long*>(offers + woman), (unsigned long long)bid) == no_offer_k;
    proposed_to[man] = woman;
}

/// Free men take their next list entry. Men whose next proposal lies beyond the list (`width`) but within P go onto the lazy list
/// (with the k of their search) instead; men past P or past the end of a list the walk could not fill are retired.
__global__ __launch_bounds__(join_threads_k) void propose_kernel(const std::uint32_t* free_list, std::uint32_t free_count,
                                                                 std::uint32_t* next, std::uint32_t max_proposals, std::uint32_t width,
                                                                 const std::uint64_t* pref_slots, const float* pref_distances,
                                                                 const std::uint64_t* pref_counts, std::uint64_t women,
                                                                 std::uint64_t* offers, std::uint32_t* proposed_to, std::uint32_t* touched,
                                                                 std::uint32_t* lazy, std::uint32_t* lazy_k_of, std::uint32_t* counters,
                                                                 unsigned long long* totals) {
    const std::uint64_t i = (std::uint64_t)blockIdx.x * join_threads_k + threadIdx.x;
    bool proposes = false, needs_search = false, first = false;
    std::uint32_t man = 0, woman = none_slot_k, c = 0;
    if (i < free_count) {
        man = free_list[i];
        c = next[man];
        proposed_to[man] = none_slot_k;
        if (c < max_proposals) {
            if (c >= width) {
                needs_search = true;
            } else if (c < pref_counts[man]) {
                const std::uint64_t cell = (std::uint64_t)man * width + c;
                const std::uint64_t slot = pref_slots[cell];
                next[man] = c + 1;
                if (slot < women) { // always true for a found entry; guards the offer array
                    woman = (std::uint32_t)slot;
                    proposes = true;
                    offer(man, woman, pref_distances[cell], offers, proposed_to, first);
                }
            }
        }
    }
    wave_append(first, woman, touched, counters + touched_k);
    const std::uint32_t at = wave_append(needs_search, man, lazy, counters + lazy_k);
    if (needs_search)
        lazy_k_of[at] = c + 1;
    wave_count(proposes, totals + proposals_k);
}

/// Proposals number k of the men in `men[0 .. count)`, each from his own search with k results: result k - 1 when the search
/// found k members; otherwise he is retired (the reference would re-propose to a woman who has refused him already).
__global__ __launch_bounds__(join_threads_k) void propose_searched_kernel(const std::uint32_t* men, std::uint32_t count, std::uint32_t k,
                                                                          std::uint32_t* next, const std::uint64_t* slots,
                                                                          const float* distances, const std::uint64_t* counts,
                                                                          std::uint64_t women, std::uint64_t* offers,
                                                                          std::uint32_t* proposed_to, std::uint32_t* touched,
                                                                          std::uint32_t* counters, unsigned long long* totals) {
    const std::uint64_t i = (std::uint64_t)blockIdx.x * join_threads_k + threadIdx.x;
    bool proposes = false, first = false;
    std::uint32_t woman = none_slot_k;
    if (i < count) {
        const std::uint32_t man = men[i];
        next[man] = k;
        const std::uint64_t cell = i * k + (k - 1);
        if (counts[i] >= k && slots[cell] < women) {
            woman = (std::uint32_t)slots[cell];
            proposes = true;
            offer(man, woman, distances[cell], offers, proposed_to, first);
        }
    }
    wave_append(first, woman, touched, counters + touched_k);
    wave_count(proposes, totals + proposals_k);
}

/// Touched women keep the best offer when it is strictly nearer than their husband (index.hpp:4482-4510).
__global__ __launch_bounds__(join_threads_k) void resolve_kernel(const std::uint32_t* touched, std::uint32_t* counters,
                                                                 std::uint64_t* offers, std::uint32_t* husband, float* husband_distance,
                                                                 std::uint32_t* next_free, unsigned long long* totals) {
    const std::uint64_t i = (std::uint64_t)blockIdx.x * join_threads_k + threadIdx.x;
    bool accepted = false;
    std::uint32_t displaced = none_slot_k;
    if (i < counters[touched_k]) {
        const std::uint32_t woman = touched[i];
        const std::uint64_t best = offers[woman];
        offers[woman] = no_offer_k;
        const std::uint32_t man = (std::uint32_t)best;
        const float d = from_ordered_bits((std::uint32_t)(best >> 32));
        const std::uint32_t current = husband[woman];
        if (current == none_slot_k || husband_distance[woman] > d) {
            husband[woman] = man;
            husband_distance[woman] = d;
            displaced = current;
            accepted = true;
        }
    }
    wave_append(displaced != none_slot_k, displaced, next_free, counters + next_free_k);
    wave_count(accepted, totals + engagements_k);
}

/// Proposers of this round who are not their woman's husband now go back onto the free list.
__global__ __launch_bounds__(join_threads_k) void requeue_kernel(const std::uint32_t* free_list, std::uint32_t free_count,
                                                                 const std::uint32_t* proposed_to, const std::uint32_t* husband,
                                                                 std::uint32_t* next_free, std::uint32_t* counters) {
    const std::uint64_t i = (std::uint64_t)blockIdx.x * join_threads_k + threadIdx.x;
    bool lost = false;
    std::uint32_t man = 0;
    if (i < free_count) {
        man = free_list[i];
        const std::uint32_t woman = proposed_to[man];
        lost = woman != none_slot_k && husband[woman] != man;
    }
    wave_append(lost, man, next_free, counters + next_free_k);
}

__global__ __launch_bounds__(join_threads_k) void sum_kernel(const std::uint64_t* values, std::uint64_t count, unsigned long long* total) {
    unsigned long long sum = 0;
    for (std::uint64_t i = (std::uint64_t)blockIdx.x * join_threads_k + threadIdx.x; i < count; i += (std::uint64_t)gridDim.x * join_threads_k)
        sum += values[i];
    if (sum)
        atomicAdd(total, sum);
}

unsigned blocks_for(std::uint64_t n) { return (unsigned)std::max<std::uint64_t>(1, (n + join_threads_k - 1) / join_threads_k); }
unsigned strided_blocks(std::uint64_t n) { return (unsigned)std::min<std::uint64_t>(4096, blocks_for(n)); }

/// Room for `count` elements out of one of the join's arenas, or the join's own out-of-memory message.
template <typename T> const char* get(device_scratch_t& arena, T*& out, std::uint64_t count) {
    if (arena.allocate(&out, count * sizeof(T)) == hipSuccess)
        return nullptr;
    (void)hipGetLastError();
    return "The preference lists do not fit in free HBM";
}

/// Joins run one at a time in a process. A join holds a lease of its proposers' snapshot while every list search leases one of the
/// other snapshot; two joins in opposite directions over snapshots of one workspace each would otherwise each hold what the other
/// waits for. A plain search leases one snapshot only, so it can wait behind a join but never closes a cycle with it.
std::mutex join_mutex;

double seconds_since(std::chrono::steady_clock::time_point start) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
}

} // namespace

const char* join_snapshots(snapshot_t& a, snapshot_t& b, const join_config_t& config, std::vector<std::uint64_t>& a_keys,
                           std::vector<std::uint64_t>& b_keys, join_stats_t* stats) {
    join_stats_t s;
    a_keys.clear(), b_keys.clear();
    if (stats)
        *stats = s;
    if (&a == &b)
        return "Can't join with itself, consider copying"; // index.hpp:4388
    if (a.device() != b.device())
        return "Can't join snapshots on different devices";
    if (a.metric() != b.metric() || a.scalar() != b.scalar() || a.view().dimensions != b.view().dimensions)
        return "Can't join indexes of different metrics, scalar kinds or dimensions";
    // the smaller side proposes; on equal sizes `a` does (index.hpp:4373-4385)
    const bool a_proposes = !(b.view().size < a.view().size);
    snapshot_t& men = a_proposes ? a : b;
    snapshot_t& women = a_proposes ? b : a;
    const std::uint64_t n_men = men.view().size, n_women = women.view().size;
    s.a_proposes = a_proposes ? 1u : 0u;
    s.expansion = config.expansion ? config.expansion : 64;
    std::uint64_t p = config.max_proposals;
    if (p == 0 && n_men) // index.hpp:4390-4391: a double assigned to a size_t
        p = (std::uint64_t)(std::log((double)n_men) + (double)std::max<std::uint64_t>(1, config.threads));
    p = std::min<std::uint64_t>(p, n_men); // index.hpp:4394
    if (p > 0xFFFFu)
        return "Too many proposals per member: the proposal counter holds at most 65535";
    s.max_proposals = p;
    const std::uint64_t width = config.exact ? p : std::min<std::uint64_t>(p, s.expansion);
    s.list_width = width;
    if (stats)
        *stats = s;
    if (!n_men || !n_women || !p)
        return nullptr;
    if (n_men >= none_slot_k || n_women >= none_slot_k)
        return "Can't join more than 2^32 - 1 members per side";
    if (config.exact && width > exact_width_limit_k) // the brute-force kernel keeps at most 4096 results per query
        return "Exact join lists hold at most 4096 proposals per member: lower max_proposals";

    std::lock_guard<std::mutex> one_join_at_a_time(join_mutex);
    UA_HIP(hipSetDevice(men.device()));
    // the men's stored rows are the queries: hold a lease of their snapshot, as every search entry point does, so that no
    // placement trial moves the matrix meanwhile
    snapshot_t::lease_t men_lease(men);
    if (const char* e = men_lease.take())
        return e;
    const hipStream_t stream = men_lease.workspace->stream;

    // ---- room: the lists and the matching state, on top of what a list search needs for itself
    const std::uint64_t chunk = std::min<std::uint64_t>(n_men, list_chunk_k);
    const std::uint64_t list_bytes = n_men * (width * 12 + 24);
    const std::uint64_t state_bytes = n_men * 20 + n_women * 16 + 4096;
    // the exact scan's own partial results per chunk: its partitions (engine.hip `exact_search_device`) × the chunk's cells
    std::uint64_t exact_bytes = 0;
    if (config.exact) {
        std::uint64_t partitions = std::max<std::uint64_t>(1, (8192 + chunk - 1) / chunk);
        partitions = std::min<std::uint64_t>(partitions, std::max<std::uint64_t>(1, 8192 / width));
        partitions = std::min<std::uint64_t>(partitions, std::max<std::uint64_t>(1, n_women / 256));
        exact_bytes = partitions * chunk * (width * 12 + 8);
    }
    {
        std::size_t free_bytes = 0, total_bytes = 0;
        UA_HIP(hipMemGetInfo(&free_bytes, &total_bytes));
        const std::uint64_t search_reserve = (std::uint64_t)256 << 20;
        if (list_bytes + state_bytes + exact_bytes + search_reserve > free_bytes)
            return "The preference lists do not fit in free HBM";
    }

    std::vector<std::uint64_t> men_keys(n_men), women_keys(n_women);
    UA_HIP(hipMemcpy(men_keys.data(), men.view().keys, n_men * 8, hipMemcpyDeviceToHost));
    UA_HIP(hipMemcpy(women_keys.data(), women.view().keys, n_women * 8, hipMemcpyDeviceToHost));

    device_scratch_t arena(men.device());
    std::uint64_t *pref_slots, *pref_counts, *visited, *computed, *offers;
    float *pref_distances, *husband_distance;
    std::uint32_t *next, *proposed_to, *husband, *free_a, *free_b, *touched, *lazy, *lazy_k_of, *counters;
    unsigned long long* totals;
    for (const char* e : {get(arena, pref_slots, n_men * width), get(arena, pref_distances, n_men * width), get(arena, pref_counts, n_men),
                          get(arena, visited, chunk), get(arena, computed, chunk), get(arena, offers, n_women),
                          get(arena, husband_distance, n_women), get(arena, next, n_men), get(arena, proposed_to, n_men),
                          get(arena, husband, n_women), get(arena, free_a, n_men), get(arena, free_b, n_men), get(arena, touched, n_men),
                          get(arena, lazy, n_men), get(arena, lazy_k_of, n_men), get(arena, counters, counters_k),
                          get(arena, totals, totals_k)})
        if (e)
            return e;
    UA_HIP(hipMemsetAsync(totals, 0, totals_k * 8, stream));
    UA_HIP(hipMemsetAsync(next, 0, n_men * 4, stream));
    UA_HIP(hipMemsetAsync(offers, 0xFF, n_women * 8, stream));
    UA_HIP(hipMemsetAsync(husband, 0xFF, n_women * 4, stream));
    UA_HIP(hipMemsetAsync(husband_distance, 0, n_women * 4, stream));
    UA_HIP(hipStreamSynchronize(stream));

    // ---- preference lists: the men's own rows as queries, slots out
    const auto started = std::chrono::steady_clock::now();
    const snapshot_view_t& men_view = men.view();
    search_extras_t extras;
    extras.emit_slots = true;
    for (std::uint64_t first = 0; first < n_men; first += chunk) {
        const std::uint64_t count = std::min<std::uint64_t>(chunk, n_men - first);
        const std::uint8_t* queries = men_view.vectors + first * men_view.row_stride;
        if (config.exact) {
            snapshot_t::lease_t women_lease(women);
            if (const char* e = women_lease.take())
                return e;
            if (const char* e = exact_search_device(women.metric(), women.scalar(), women.lanes_per_row(), women.view(), queries, count,
                                                    men_view.row_stride, width, false, pref_slots + first * width,
                                                    pref_distances + first * width, pref_counts + first, women_lease.workspace->stream,
                                                    nullptr))
                return e;
            s.computed_distances += count * n_women;
        } else {
            search_stats_t search_stats;
            if (const char* e = women.search_device(queries, count, men_view.row_stride, width, s.expansion, pref_slots + first * width,
                                                    pref_distances + first * width, pref_counts + first, visited, computed, nullptr,
                                                    search_tuning_t{}, &search_stats, false, &extras))
                return e;
            if (!first)
                s.frontier = search_stats.frontier;
            hipLaunchKernelGGL(sum_kernel, dim3(strided_blocks(count)), dim3(join_threads_k), 0, stream, visited, count,
                               totals + sum_visited_k);
            hipLaunchKernelGGL(sum_kernel, dim3(strided_blocks(count)), dim3(join_threads_k), 0, stream, computed, count,
                               totals + sum_computed_k);
            UA_HIP(hipGetLastError());
            UA_HIP(hipStreamSynchronize(stream)); // `visited` / `computed` are reused by the next chunk
        }
    }
    s.seconds_lists = seconds_since(started);

    // ---- matching rounds
    std::vector<std::uint32_t> initial;
    initial.reserve(n_men);
    for (std::uint64_t m = 0; m < n_men; ++m)
        if (men_keys[m] != free_key_k) // tombstoned men do not propose
            initial.push_back((std::uint32_t)m);
    std::uint32_t free_count = (std::uint32_t)initial.size();
    if (free_count)
        UA_HIP(hipMemcpy(free_a, initial.data(), free_count * 4ull, hipMemcpyHostToDevice));
    std::uint32_t* pinned = nullptr;
    UA_HIP(hipHostMalloc((void**)&pinned, 16, hipHostMallocDefault));
    struct pinned_t {
        std::uint32_t* p;
        ~pinned_t() { (void)hipHostFree(p); }
    } pinned_guard{pinned};

    // searches for proposals beyond the first list (k = i > expansion): buffers grown on demand
    std::uint64_t* lazy_slots = nullptr;
    float* lazy_distances = nullptr;
    std::uint64_t *lazy_counts = nullptr, *lazy_visited = nullptr, *lazy_computed = nullptr;
    std::uint32_t* lazy_ids = nullptr;
    std::uint64_t lazy_cells = 0, lazy_rows = 0;
    device_scratch_t lazy_arena(men.device()); // replaced, not added to, when a larger group comes
    std::vector<std::uint32_t> lazy_men, lazy_wanted;

    while (free_count) {
        ++s.rounds;
        UA_HIP(hipMemsetAsync(counters, 0, counters_k * 4, stream));
        hipLaunchKernelGGL(propose_kernel, dim3(blocks_for(free_count)), dim3(join_threads_k), 0, stream, free_a, free_count, next,
                           (std::uint32_t)p, (std::uint32_t)width, pref_slots, pref_distances, pref_counts, n_women, offers, proposed_to,
                           touched, lazy, lazy_k_of, counters, totals);
        UA_HIP(hipGetLastError());
        if (p > width) {
            UA_HIP(hipMemcpyAsync(pinned, counters, 16, hipMemcpyDeviceToHost, stream));
            UA_HIP(hipStreamSynchronize(stream));
            const std::uint32_t lazy_count = pinned[lazy_k];
            if (lazy_count) {
                const auto lazy_started = std::chrono::steady_clock::now();
                lazy_men.resize(lazy_count), lazy_wanted.resize(lazy_count);
                UA_HIP(hipMemcpy(lazy_men.data(), lazy, lazy_count * 4ull, hipMemcpyDeviceToHost));
                UA_HIP(hipMemcpy(lazy_wanted.data(), lazy_k_of, lazy_count * 4ull, hipMemcpyDeviceToHost));
                std::map<std::uint32_t, std::vector<std::uint32_t>> by_k;
                for (std::uint32_t j = 0; j < lazy_count; ++j)
                    by_k[lazy_wanted[j]].push_back(lazy_men[j]);
                for (auto& [k, group] : by_k) {
                    const std::uint64_t rows = group.size(), cells = rows * k;
                    if (cells > lazy_cells || rows > lazy_rows) {
                        lazy_cells = std::max(lazy_cells, cells), lazy_rows = std::max(lazy_rows, rows);
                        lazy_arena.release(); // nothing in flight reads them: every group ends in a synchronize
                        for (const char* e : {get(lazy_arena, lazy_slots, lazy_cells), get(lazy_arena, lazy_distances, lazy_cells),
                                              get(lazy_arena, lazy_counts, lazy_rows), get(lazy_arena, lazy_visited, lazy_rows),
                                              get(lazy_arena, lazy_computed, lazy_rows), get(lazy_arena, lazy_ids, lazy_rows)})
                            if (e)
                                return e;
                    }
                    UA_HIP(hipMemcpy(lazy_ids, group.data(), rows * 4, hipMemcpyHostToDevice));
                    search_extras_t lazy_extras;
                    lazy_extras.emit_slots = true;
                    lazy_extras.query_ids = lazy_ids;
                    if (const char* e = women.search_device(men_view.vectors, rows, men_view.row_stride, k, s.expansion, lazy_slots,
                                                            lazy_distances, lazy_counts, lazy_visited, lazy_computed, nullptr,
                                                            search_tuning_t{}, nullptr, false, &lazy_extras))
                        return e;
                    ++s.lazy_searches;
                    hipLaunchKernelGGL(sum_kernel, dim3(strided_blocks(rows)), dim3(join_threads_k), 0, stream, lazy_visited, rows,
                                       totals + sum_visited_k);
                    hipLaunchKernelGGL(sum_kernel, dim3(strided_blocks(rows)), dim3(join_threads_k), 0, stream, lazy_computed, rows,
                                       totals + sum_computed_k);
                    hipLaunchKernelGGL(propose_searched_kernel, dim3(blocks_for(rows)), dim3(join_threads_k), 0, stream, lazy_ids,
                                       (std::uint32_t)rows, k, next, lazy_slots, lazy_distances, lazy_counts, n_women, offers,
                                       proposed_to, touched, counters, totals);
                    UA_HIP(hipGetLastError());
                    UA_HIP(hipStreamSynchronize(stream)); // the buffers serve the next group
                }
                s.seconds_lists += seconds_since(lazy_started);
            }
        }
        // touched women and this round's proposers both number at most `free_count`
        hipLaunchKernelGGL(resolve_kernel, dim3(blocks_for(free_count)), dim3(join_threads_k), 0, stream, touched, counters, offers,
                           husband, husband_distance, free_b, totals);
        hipLaunchKernelGGL(requeue_kernel, dim3(blocks_for(free_count)), dim3(join_threads_k), 0, stream, free_a, free_count, proposed_to,
                           husband, free_b, counters);
        UA_HIP(hipGetLastError());
        UA_HIP(hipMemcpyAsync(pinned, counters, 16, hipMemcpyDeviceToHost, stream));
        UA_HIP(hipStreamSynchronize(stream));
        free_count = pinned[next_free_k];
        std::swap(free_a, free_b);
    }

    // ---- export in ascending order of `a`'s slots (index.hpp:4524-4545)
    std::vector<std::uint32_t> husband_host(n_women);
    UA_HIP(hipMemcpy(husband_host.data(), husband, n_women * 4, hipMemcpyDeviceToHost));
    unsigned long long totals_host[totals_k] = {};
    UA_HIP(hipMemcpy(totals_host, totals, sizeof(totals_host), hipMemcpyDeviceToHost));
    if (a_proposes) {
        std::vector<std::uint32_t> wife(n_men, none_slot_k);
        for (std::uint64_t w = 0; w < n_women; ++w)
            if (husband_host[w] < n_men)
                wife[husband_host[w]] = (std::uint32_t)w;
        for (std::uint64_t m = 0; m < n_men; ++m)
            if (wife[m] != none_slot_k)
                a_keys.push_back(men_keys[m]), b_keys.push_back(women_keys[wife[m]]);
    } else {
        for (std::uint64_t w = 0; w < n_women; ++w)
            if (husband_host[w] < n_men)
                a_keys.push_back(women_keys[w]), b_keys.push_back(men_keys[husband_host[w]]);
    }
    s.pairs = a_keys.size();
    s.proposals = totals_host[proposals_k];
    s.engagements = totals_host[engagements_k];
    if (!config.exact) {
        s.visited_members = totals_host[sum_visited_k];
        s.computed_distances = totals_host[sum_computed_k];
    }
    s.seconds_matching = seconds_since(started) - s.seconds_lists;
    if (stats)
        *stats = s;
    return nullptr;
}

} // namespace usearch_amd
