/**
 *  usearch_amd/csrc/engine.hpp — host side of the MI355X search engine: an immutable HBM snapshot of one index and the
 *  batched search over it.
 *
 *  Replaces, for the search path only, what `index_dense_gt` owns on the CPU (/root/reference/include/usearch/
 *  index_dense.hpp:419-460 `metric_proxy_t` + `vectors_lookup_`, index.hpp:2280 `nodes_`) and what its callers loop over
 *  (`cpp/bench.cpp:352-377`, `python/lib.cpp:261-319`): one call = one batch of independent queries.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "image.hpp"
#include "placement.hpp"

namespace usearch_amd {

struct compact_config_t; // compact.hpp
struct compact_stats_t;
struct clustering_config_t; // clustering.hpp
struct clustering_stats_t;

/// Tunables of one search launch; zeros mean "choose for me".
struct search_tuning_t {
    std::uint32_t hash_cap = 0;     ///< visited-set cells per query (power of two)
    std::uint32_t next_cap = 0;     ///< frontier capacity per query
    std::uint32_t variant = 0;      ///< 0 = auto, else 1 + kernel_variant_t (loads in flight per lane vs waves per SIMD)
    std::uint32_t mode = 0;         ///< 0 = auto, 1 = visited set in LDS, 2 = visited set in a global hash, 3 = all-global fallback
    std::uint32_t waves_per_cu = 0; ///< persistent waves per compute unit (0 = as many as LDS / registers admit)
    std::uint32_t top_in_memory = 0; ///< 1 = keep `top` in scratch memory even when it would fit registers
    std::uint32_t frontier = 0;     ///< 0 = auto, 1 = the reference's heap (its pop order among equal distances), 2 = the open
                                    ///< cells of `top` (kernels.hpp frontier_top_k; refused where it does not apply)
    std::uint32_t wave_clock = 0;   ///< 1 = record every persistent wave's start / exit time (batch-tail telemetry)
    std::uint32_t sketch = 0;       ///< 0 = auto (use the snapshot's sketch until it proves useless), 1 = off, 2 = on where eligible
};

struct search_stats_t {
    std::uint32_t passes = 0;            ///< launches needed (1 = every query fit its LDS scratch)
    std::uint32_t retried_lds = 0;       ///< queries rerun with the enlarged LDS scratch
    std::uint32_t retried_global = 0;    ///< queries rerun with the global-memory scratch
    float kernel_ms = 0.f;               ///< HIP-event time of the search launches of this call (when `timed`)
    std::uint32_t mode = 0;              ///< scratch mode of the last launch (1 = LDS, 2 = global hash, 3 = all global)
    std::uint32_t grid = 0;              ///< persistent waves of the last launch
    std::uint32_t lds_bytes = 0;         ///< LDS per wave of the last launch
    std::uint32_t frontier = 0;          ///< 1 = heap, 2 = open cells of `top` (first launch)
    std::uint32_t variant = 0;           ///< 1 + kernel_variant_t of the first launch
    float tail_idle = 0.f;               ///< with `wave_clock`: share of wave-time between the first start and the last exit
                                         ///< that waves spent gone (the drain phase of the batch), first launch
    float span_ms = 0.f;                 ///< with `wave_clock`: first start → last exit on the device's 100-MHz clock
    std::uint32_t top_cells = 0;         ///< `top` cells per lane in registers of the first launch (0 = scratch memory)
    std::uint32_t probe_mode = 0;        ///< always 0, kept for layout (the slab is probed by compare-and-swap: DESIGN.md §3.2)
    std::uint32_t seen_cells = 0;        ///< short rows over a global slab: the `seen` cells in LDS of the last launch
    std::uint32_t claim_bits = 0;        ///< always 0, kept for layout
    std::uint32_t early_rows = 0;        ///< rows of ≤ 128 bytes: 1 = gathered next to the probe of the visited set, not behind it
    std::uint32_t plain = 0;             ///< short rows: 1 = the last launch ran the build cut for plain batches (kernels.hpp `plain_ak`)
    std::uint32_t aside_cells = 0;       ///< … and its LDS cells for the members whose home cell in the slab was taken
    std::uint64_t sketch_tested = 0;     ///< candidates of this call tested against the sketch (sketch.hpp) …
    std::uint64_t sketch_pruned = 0;     ///< … and how many of them it proved too far: their rows were not fetched
};

/// What index construction asks of the search on top of a plain query batch (see search_args_t).
struct search_extras_t {
    const std::uint32_t* query_ids = nullptr; ///< device: query q is row query_ids[q] of `queries`
    std::uint32_t beam_level = 0;             ///< level the beam runs on
    bool emit_slots = false;                  ///< slots instead of keys in the `keys` output
    bool descent_only = false;                ///< `cluster`: the greedy descent to `beam_level` alone, one result per query
    const std::uint32_t* allow_bits = nullptr; ///< device: one bit per slot, 0 = rejected by the caller's predicate
    // a predicate evaluated lazily by the host (search_args_t::known_bits): all device pointers
    const std::uint32_t* known_bits = nullptr;
    std::uint32_t* ask_slots = nullptr;
    std::uint64_t* ask_keys = nullptr;
    std::uint32_t* ask_cursor = nullptr;
    std::uint32_t ask_cap = 0;
    std::uint32_t guess_threshold = 0xFFFFFFFFu;
    bool reference_frontier = false;          ///< keep the reference's heap whatever the pair (index construction does)
    bool exclude_own = false;                 ///< `search_to_update_`: a query's own stored row routes, never becomes a candidate
};

/// Whether an instantiation of the search kernel also exists in the cut for plain batches (kernels.hpp `plain_ak`; launch_impl.hpp
/// instantiates exactly these): rows of ≤ 128 bytes of the common pairs, 4 loads in flight, the visited set in the global hash, `top` of
/// one or two cells per lane, the reference's heap.
inline constexpr bool plain_build_exists(metric_kind_t metric, scalar_kind_t scalar, int lanes, bool four_deep, bool global_hash,
                                         int top_cells, bool heap) {
    return all_kernel_builds(metric, scalar) && lanes <= 2 && four_deep && global_hash && (top_cells == 1 || top_cells == 2) && heap;
}

// ---- the launch planner's plain values (search_plan.hpp holds the functions that fill them: the ONE place that chooses a build)

/// Every USEARCH_AMD_<NAME> override the planner looks at, read once per search call by `read_search_knobs` (0 = not set, unless
/// noted). Numbers stay as wide as the environment gave them: the planner narrows them where it always did.
struct search_knobs_t {
    std::size_t lds_budget = 160 * 1024; ///< LDS_BUDGET: bytes of a compute unit's LDS the resident waves may share
    std::size_t hash_cap = 0, hash_load_pct = 50; ///< HASH_LOAD_PCT: 10 … 75, by default 50 for rows of 8 lanes and 75 below
    std::size_t next_cap = 0, mode = 0, top_in_memory = 0, no_two_cells = 0, frontier = 0, variant = 0, no_team = 0, no_plain = 0;
    std::size_t waves_per_cu = 32, no_small_batch_lds = 0, early_rows = 1, aside_cells = 0, plain_whatever_the_room = 0;
    std::size_t seen_cells = (std::size_t)-1; ///< SEEN_CELLS: −1 = as many as cost no resident wave, 0 = none
};

/// What the planner needs to know about the index and the call.
struct search_shape_t {
    std::uint64_t size = 0, count = 0, wanted = 0, expansion = 0;
    std::int32_t metric = 0, scalar = 0; ///< `kernel_metric` of the index's metric_kind_t; its scalar_kind_t
    std::uint32_t lanes = 0, chunks = 0, m0 = 0, compute_units = 0;
    std::uint32_t has_tombstones = 0, nbr0 = 0, nbr0_rows = 0, sketch = 0; ///< flags: which arrays of the view are there
    std::uint32_t query_ids = 0, beam_level = 0, descent_only = 0, allow_bits = 0, exclude_own = 0, reference_frontier = 0; ///< search_extras_t
};

/// What `plan_search` settles for the whole call; `plan_rung` and `escalate` revise it on the way up the retry ladder.
struct search_plan_t {
    std::uint32_t ef = 0, query_lds = 0, entries_per_lane = 0, waves_cap = 0, hash_cap = 0, next_cap = 0;
    std::int32_t mode = 0, variant = 0, frontier = 0; ///< scratch_mode_t, kernel_variant_t, frontier_mode_t of kernels.hpp
    std::uint32_t team = 0;           ///< five waves per query (kernels.hpp team_search_kernel)
    std::uint32_t plain_possible = 0; ///< short rows: nothing known before the first rung rules the build cut for plain batches out
    std::uint32_t sketch = 0;         ///< the walk tests candidates against the sketch, until a rung finds no LDS for its coefficients
    /// The decisions as `search_stats_t` reports them — `plan_search`: frontier, variant, top_cells; `plan_rung`: early_rows, plain,
    /// aside_cells, over short rows seen_cells, and variant again when a team is demoted — next to which
    /// the engine writes what the device did.
    search_stats_t stats{};
};

/// One launch of the ladder as `plan_rung` shapes it: what goes into `launch_params_t` and `search_args_t`.
struct search_rung_t {
    std::int32_t mode = 0, frontier = 0;
    std::uint32_t team = 0, plain = 0, entries_per_lane = 0, grid = 0, lds_bytes = 0, hash_cap = 0, next_cap = 0;
    std::uint32_t early_rows = 0, aside_offset = 0, aside_cells = 0, seen_offset = 0,
        seen_cells = 0, sketch_offset = 0, team_offset = 0;
    std::uint64_t slab = 0;                            ///< bytes of global scratch per wave
    std::uint64_t visits_offset = 0, bitmap_bytes = 0; ///< the global rung: where in a slab the bitmap sits, which the host zeroes
};

/// Per-scalar-kind launchers, one translation unit each (compile time): defined in search_<kind>.hip.
struct launch_params_t {
    metric_kind_t metric;
    std::uint32_t lanes;
    int variant; ///< kernel_variant_t of kernels.hpp
    int mode;    ///< scratch_mode_t of kernels.hpp
    std::uint32_t entries_per_lane; ///< `top` in registers: 1, 4, 8 or 16 entries per lane; 0 = in scratch memory
    int frontier;                   ///< frontier_mode_t of kernels.hpp
    std::uint32_t grid;
    std::uint32_t lds_bytes;
    hipStream_t stream;
    std::uint32_t team = 0;       ///< 1 = five waves per query (team_search_kernel): small batches over long rows
    std::uint32_t plain = 0;      ///< 1 = the short-row build cut for a plain `search` batch (kernels.hpp `plain_ak`): the engine vouches
                                  ///< for level 0, no predicate / tombstones / own row, lists of ≤ 64 cells, `seen` cells, rows inline or early
};

/**
 *  Everything ONE in-flight batch needs besides the immutable snapshot: a stream, the ticket counter, per-query status,
 *  scratch slabs, and the device + pinned-host staging of the host-buffer entry points. A snapshot keeps a small pool of
 *  these, so that concurrent callers (the reference leases one `context_t` per thread, index_dense.hpp:1984-2000) run
 *  side by side instead of queueing on one mutex.
 */
struct workspace_t {
    hipStream_t stream = nullptr;
    hipEvent_t event_begin = nullptr, event_end = nullptr;
    std::uint32_t* d_status = nullptr;
    std::uint32_t* d_todo = nullptr;
    std::uint32_t* d_queue = nullptr; ///< 256-byte block: [0] ticket counter, [1] overflowed queries, [16…] phase clock
    std::uint32_t* d_peaks = nullptr;
    std::uint32_t* h_status = nullptr; ///< pinned: [0..1] copy of the queue block's counters, then per-query status
    std::size_t queries = 0;
    std::uint8_t* d_scratch = nullptr;
    std::size_t scratch_bytes = 0;
    unsigned long long* d_wave_clock = nullptr;
    std::size_t wave_clock_waves = 0;
    std::uint8_t* d_stage = nullptr; ///< host-buffer API: queries | keys | distances | counts | visited | computed [| allow bits]
    std::uint8_t* h_stage = nullptr; ///< pinned mirror of the result part
    std::size_t stage_bytes = 0, host_stage_bytes = 0;
    std::size_t last_count = 0;

    const char* create();
    const char* reserve(std::size_t queries_wanted, std::size_t scratch_wanted);
    const char* reserve_stage(std::size_t device_bytes, std::size_t host_bytes);
    const char* reserve_wave_clock(std::size_t waves);
    void destroy();
};

/// Launches the sketch's record builder (sketch.hip) over rows [first, size) of `vectors` on `stream`: records[row][128] for those rows,
/// rows below `first` untouched. `directions`: [dimensions][64] f32 on the device, `gram_defect` as `sketch_orthonormalise` reports it.
void launch_sketch_records(const std::uint8_t* vectors, std::uint32_t row_stride, std::uint32_t dimensions, scalar_kind_t scalar,
                           std::uint64_t first, std::uint64_t size, const float* directions, double gram_defect, std::uint8_t* records,
                           hipStream_t stream);

class snapshot_t {
  public:
    friend struct sketch_test_access_t; ///< test_hooks.hip: reads the sketch back for tests/test_gpu_sketch_records.py
    snapshot_t() = default;
    ~snapshot_t();
    snapshot_t(const snapshot_t&) = delete;
    snapshot_t& operator=(const snapshot_t&) = delete;

    /// Flattens `image` into the HBM layout of `snapshot_view_t` on `device`. Returns nullptr or a static message.
    const char* build(const image_t& image, int device);

    const snapshot_view_t& view() const { return view_; }
    metric_kind_t metric() const { return metric_; }
    scalar_kind_t scalar() const { return scalar_; }
    std::uint32_t lanes_per_row() const { return lanes_; }
    int device() const { return device_; }
    std::size_t device_bytes() const { return device_bytes_; }
    std::uint64_t count_present() const { return count_present_; }
    std::uint64_t upper_lists() const { return upper_lists_; }
    float last_distances_ms() const { return last_distances_ms_; }
    /// How the matrix of stored rows was placed in HBM (placement.hpp): draws, their gather rates, which one was kept.
    const placement_t& placement() const { return placement_; }

    /**
     *  Batched search, all pointers device-resident, queries already in the storage scalar kind.
     *  Enqueues on `stream` (the leased workspace's own when null) and waits for it: the retry ladder needs to know
     *  whether any query outgrew its scratch (one 8-byte read-back).
     */
    const char* search_device(const void* queries, std::size_t count, std::size_t stride_bytes, std::size_t wanted,
                              std::size_t expansion, std::uint64_t* keys, float* distances, std::uint64_t* counts,
                              std::uint64_t* visited, std::uint64_t* computed, hipStream_t stream,
                              const search_tuning_t& tuning, search_stats_t* stats, bool timed,
                              const search_extras_t* extras = nullptr);

    /**
     *  TUNES WHERE THE MATRIX SITS, on the caller's own sample batch (round 6; `usearch_amd_snapshot_tune`). Which frames of HBM the
     *  matrix of stored rows received decides how fast the walk runs over it — 44.4 … 51.4 ms for the headline batch over the same
     *  bytes, per box and per what the process allocated before (profiles/r06_settled/) — and nothing but the walk itself tells the
     *  placements apart. So a host that is about to serve one shape of batch hands over a sample of it: up to `max_trials` times a
     *  fresh device-to-device copy of the matrix is placed and timed against the incumbent on the sample's first queries (one per
     *  resident wave, at the sample's expansion: `try_matrix_placement`), the faster stays, the other is freed — and because the
     *  driver hands freed frames back late, consecutive copies land on different frames. Three wins of the incumbent in a row end
     *  it early. EXPLICIT and synchronous: nothing of it ever happens inside a search call (round 5 ran these trials there; the
     *  advisor's finding), a second copy of the matrix exists in HBM only during this call, and the matrix does not move afterwards.
     *  Arrays under 1 GiB, inline-row snapshots and samples that do not fill the chip are left alone (returns 0 trials).
     */
    const char* tune(const void* queries, std::size_t count, std::size_t stride_bytes, std::size_t wanted, std::size_t expansion,
                     std::uint32_t max_trials, std::uint32_t* trials_made);

    /**
     *  The same search in two halves, for callers that append their own work to the stream before anybody waits (the
     *  sharded step: search → all-gather → merge, one stream, one wait): `search_begin` sizes the scratch, leases a
     *  workspace and launches; `search_finish` waits, and re-runs what outgrew its scratch (`reran` tells the caller that
     *  outputs changed after its appended work read them). A call object is used once.
     */
    struct search_call_t {
        workspace_t* workspace = nullptr;
        hipStream_t stream = nullptr;
        search_args_t args{};
        launch_params_t params{};
        std::size_t count = 0;
        search_shape_t shape{}; ///< what the planner (search_plan.hpp) was told, …
        search_knobs_t knobs{}; ///< … the environment's overrides as they stood when the call began, …
        search_plan_t plan{};   ///< … and what it decided; `plan.stats` is the call's statistics
        bool timed = false, want_phases = false, want_clock = false, done = false, reran = false;
        bool sketch_auto = false;    ///< this call used the sketch in auto mode: its counters judge it (`judge_sketch`)
        bool keep_workspace = false; ///< search_finish leaves the workspace with the caller (who gives it back)
        float total_ms = 0.f;
        std::uint32_t passes = 0;
        std::vector<std::uint32_t> todo;
        bool have_todo = false;
    };
    const char* search_begin(search_call_t& call, const void* queries, std::size_t count, std::size_t stride_bytes,
                             std::size_t wanted, std::size_t expansion, std::uint64_t* keys, float* distances,
                             std::uint64_t* counts, std::uint64_t* visited, std::uint64_t* computed, hipStream_t stream,
                             const search_tuning_t& tuning, bool timed, const search_extras_t* extras = nullptr);
    const char* search_finish(search_call_t& call, search_stats_t* stats);

    /**
     *  Construction support (build.hip): allocates the HBM arrays of an index with room for `capacity` members and
     *  `lists_capacity` upper-level lists, every list empty; `append_for_build` uploads members, `grow_for_build` makes room
     *  for more. The graph arrays are filled in place by the link kernels while `set_frontier` tells the search how much of
     *  the graph exists.
     */
    const char* allocate_for_build(metric_kind_t metric, scalar_kind_t scalar, std::size_t dimensions,
                                   std::uint64_t capacity, std::uint64_t lists_capacity, std::uint32_t m, std::uint32_t m0,
                                   int device);
    /// Re-allocates the build arrays for `capacity` members / `lists_capacity` upper-level lists, keeping what is linked.
    const char* grow_for_build(std::uint64_t capacity, std::uint64_t lists_capacity);
    /// Uploads members [first, first + count): rows (re-pitched), keys (null = the slot number), upper-list references.
    const char* append_for_build(std::uint64_t first, std::uint64_t count, const std::uint32_t* upper_refs,
                                 const void* vectors, std::size_t stride, bool vectors_on_device, const std::uint64_t* keys);
    /// Overwrites one member's stored row (host memory, storage kind) and key in HBM: a recycled slot (builder_t::update).
    const char* overwrite_member(std::uint64_t slot, const void* vector, std::uint64_t key);
    /// Overwrites one member's key in HBM (rename; `free_key_k` = tombstone).
    const char* set_key(std::uint64_t slot, std::uint64_t key);
    /// Counts what changes WHO the members are without necessarily changing how many there are (`append_for_build`,
    /// `overwrite_member`, `set_key`): a `filter_t` made before is a bitmap of the keys as they were (filter.hpp: `check`).
    std::uint64_t mutations() const { return mutations_; }
    std::uint64_t build_capacity() const { return build_capacity_; }
    std::uint64_t build_lists_capacity() const { return build_lists_capacity_; }
    /// A snapshot loaded from an image becomes the arrays of an index under construction (builder_t::adopt): they are exactly
    /// full, which is what `grow_for_build` has to know to keep what is linked when more members arrive.
    void adopt_for_build() { build_capacity_ = view_.size, build_lists_capacity_ = upper_lists_ > 1 ? upper_lists_ : 1; }
    void set_upper_lists(std::uint64_t lists) { upper_lists_ = lists; }
    void set_frontier(std::uint64_t size, std::uint32_t entry_slot, std::uint32_t max_level) {
        view_.size = size, view_.entry_slot = entry_slot, view_.max_level = max_level;
    }
    void set_tombstones(bool any) { view_.has_tombstones = any ? 1u : 0u; }
    /// Once the graph no longer changes: lays the stored rows of every node's level-0 neighbours next to each other
    /// (`snapshot_view_t::nbr0_rows`) when rows are a single 16-byte chunk — b1 × 128, haversine … — so that a hop reads one
    /// contiguous block. Costs size × M0 × 16 bytes of HBM; USEARCH_AMD_INLINE_ROWS=0 turns it off.
    const char* finalize_layout();
    void suspend_layout() { view_.nbr0_rows = nullptr, view_.sketch = nullptr; } ///< while the lists are being rewritten (construction)
    /// The sketch of the stored rows (sketch.hpp), made or extended for the members the snapshot holds now: called by `finalize_layout`.
    /// Members appended since get records under the same directions; an overwritten row makes everything anew. Not eligible: none.
    const char* finalize_sketch();
    const char* make_sketch();
    bool has_sketch() const { return view_.sketch != nullptr; }
    std::uint32_t* mutable_nbr0() { return static_cast<std::uint32_t*>(d_nbr0_); }
    std::uint32_t* mutable_upper() { return static_cast<std::uint32_t*>(d_upper_); }
    hipStream_t stream() const { return stream_; }
    int compute_units() const { return compute_units_; }

    /// How many batches may be in flight at once (`usearch_change_threads_search`): the size of the workspace pool.
    void set_concurrency(std::size_t workspaces);
    std::size_t concurrency() const { return max_workspaces_; }

    /// Same with host buffers and a query scalar kind that may differ from the storage kind (cast first).
    const char* search_host(const void* queries, scalar_kind_t query_kind, std::size_t count, std::size_t stride_bytes,
                            std::size_t wanted, std::size_t expansion, std::uint64_t* keys, float* distances,
                            std::uint64_t* counts, std::uint64_t* visited, std::uint64_t* computed,
                            const search_tuning_t& tuning, search_stats_t* stats,
                            const std::uint32_t* allow_bits_host = nullptr, const search_extras_t* more = nullptr);

    /// `index_dense_gt::cluster(query, level)` for a batch (index_dense.hpp:788-793 → index.hpp:3089-3125): host buffers, any
    /// query scalar kind; keys / distances / visited / computed are [count] arrays.
    const char* cluster_host(const void* queries, scalar_kind_t query_kind, std::size_t count, std::size_t stride_bytes,
                             std::size_t level, std::uint64_t* keys, float* distances, std::uint64_t* visited,
                             std::uint64_t* computed);

    /// Telemetry of the last search_device call: per query {peak frontier size, visited-set size}; host copy.
    const char* last_peaks(std::uint32_t* out, std::size_t queries);

    /// `search(…, exact = true)` for a batch (index_dense.hpp:767-772 with exact, index.hpp:3046-3049): device buffers,
    /// queries in the storage kind. `allow_bits` (device, one bit per slot): the caller's predicate, which the brute-force scan
    /// applies too (index.hpp:4260-4263).
    const char* exact_device(const void* queries, std::size_t count, std::size_t stride_bytes, std::size_t wanted,
                             std::uint64_t* keys, float* distances, std::uint64_t* counts, hipStream_t stream,
                             float* kernel_ms, bool tiled = false, const std::uint32_t* allow_bits = nullptr);
    /// Same with host buffers and any query scalar kind. `tiled`: the matrix-unit kernel where one exists for the pair
    /// (exact_tiled.hip; an error otherwise) instead of the bit-exact wave-per-query one.
    const char* exact_host(const void* queries, scalar_kind_t query_kind, std::size_t count, std::size_t stride_bytes,
                           std::size_t wanted, std::uint64_t* keys, float* distances, std::uint64_t* counts,
                           float* kernel_ms, bool tiled = false, const std::uint32_t* allow_bits = nullptr);

    /// out[q][j] = metric(query q, stored row slots[q][j]); host buffers, queries in storage kind.
    const char* distances_host(const void* queries, std::size_t count, std::size_t stride_bytes,
                               const std::uint32_t* slots, std::size_t slots_per_query, float* out);

    /**
     *  `index_dense_gt::isolate` (index_dense.hpp:1709-1720 → index.hpp:3700-3728) on the device: every neighbour whose key is
     *  `free_key_k` leaves every list of every member, the rest of a list keeps its order. Nothing else moves. Refused while search
     *  workspaces are leased. compact.hip.
     */
    const char* isolate(compact_stats_t* stats);
    /**
     *  `isolate`, then the removed members leave for good: survivors are renumbered by their rank (stable), lists, keys and rows
     *  follow, `has_tombstones` is cleared (compact.hpp has the rules). `slot_map` (host, optional): [old size] old slot → new slot,
     *  `none_slot_k` for removed members. Refused while search workspaces are leased.
     */
    const char* compact(const compact_config_t& config, std::uint32_t* slot_map, compact_stats_t* stats);

    /**
     *  `index_dense_gt::cluster(begin, end, config, keys, distances)` (index_dense.hpp:1819-1981) for a batch: level choice, descent,
     *  popularity count, refinement, merges and trace, everything between the first descent and the copy-out in HBM (clustering.hpp
     *  has the rules, clustering.hip the kernels). `queries` (host, `query_kind`, `stride_bytes` apart) or, when null, members as
     *  queries: `member_slots` (host, [count]) names them, null = every member whose key is not `free_key_k` in slot order (`count`
     *  must be their number). `keys` / `distances`: host, [count]. Refused while search workspaces are leased.
     */
    const char* clustering(const void* queries, scalar_kind_t query_kind, std::size_t count, std::size_t stride_bytes,
                           const std::uint32_t* member_slots, const clustering_config_t& config, std::uint64_t* keys,
                           float* distances, clustering_stats_t* stats);
    /// Several members may share a key (the image's head says so; a builder's configuration does).
    bool multi() const { return multi_; }
    void set_multi(bool multi) { multi_ = multi; }

    /// Leases a workspace (waits while `concurrency()` of them are out); `give_back` returns it. RAII: `lease_t`.
    const char* take(workspace_t*& out);
    void give_back(workspace_t* workspace);
    struct lease_t {
        snapshot_t& owner;
        workspace_t* workspace = nullptr;
        explicit lease_t(snapshot_t& s) : owner(s) {}
        ~lease_t() {
            if (workspace)
                owner.give_back(workspace);
        }
        const char* take() { return owner.take(workspace); }
    };

  private:
    const char* run_ladder(search_call_t& call);
    /// One placement trial of the matrix of stored rows inside a launch that fills the chip (placement.hpp): a fresh device-to-device
    /// copy, incumbent and candidate timed alternately over the launch's first `grid` queries (`launch(view, ms)` runs them once and
    /// times them), the faster one stays. Needs the matrix to itself (no other batch in flight); does nothing otherwise.
    const char* try_matrix_placement(std::uint32_t expansion, const std::function<const char*(const snapshot_view_t&, float&)>& launch, hipStream_t stream);
    void release();
    void drop_sketch();
    /// Auto mode: the first call of at least 1 024 queries that has the snapshot to itself judges the sketch; if it pruned less than a
    /// quarter of what it tested, the snapshot frees the sketch and walks without one from then on.
    void judge_sketch(std::uint64_t tested, std::uint64_t pruned);

    snapshot_view_t view_{};
    metric_kind_t metric_ = metric_unknown_k;
    scalar_kind_t scalar_ = scalar_unknown_k;
    std::uint32_t lanes_ = 1;
    int device_ = 0;
    bool multi_ = false;
    std::size_t device_bytes_ = 0;
    std::uint64_t count_present_ = 0, upper_lists_ = 0, mutations_ = 0;

    void* d_vectors_ = nullptr;
    void* d_nbr0_ = nullptr;
    void* d_upper_ref_ = nullptr;
    void* d_upper_ = nullptr;
    void* d_keys_ = nullptr;
    void* d_nbr0_rows_ = nullptr;
    void* d_sketch_ = nullptr;            ///< [sketch_capacity_][128] records, the first sketch_rows_ of them filled
    void* d_sketch_directions_ = nullptr; ///< [dimensions][64] f32
    std::uint64_t sketch_rows_ = 0, sketch_capacity_ = 0;
    double sketch_gram_defect_ = 0.0;
    bool sketch_stale_ = false;   ///< a stored row was overwritten: its record no longer bounds it
    bool sketch_refused_ = false; ///< auto mode found the sketch useless on this snapshot's data
    bool sketch_judged_ = false;  ///< auto mode has passed its verdict on the sketch this snapshot holds (guarded by pool_mutex_)
    std::uint64_t build_capacity_ = 0, build_lists_capacity_ = 0; ///< room in the arrays above while an index is under construction

    placement_t placement_{};
    std::uint32_t placement_trials_left_ = placement_max_draws_k; ///< trials `try_matrix_placement` may still make
    std::uint32_t placement_losses_ = 0;                          ///< trials in a row the incumbent has won
    std::uint32_t placement_last_ef_ = 0, placement_reopens_ = 0; ///< the expansion of the last trial; how often a wider regime reopened the search
    bool placing_ = false;            ///< a trial owns the matrix: `take` waits (guarded by pool_mutex_)
    std::uint32_t tuning_trials_ = 0; ///< > 0 only inside `tune`: the trials `run_ladder` may make there (0: the environment decides)
    std::size_t vectors_bytes_ = 0;   ///< bytes allocated behind d_vectors_
    int compute_units_ = 256;
    float last_distances_ms_ = 0.f;
    hipStream_t stream_ = nullptr; ///< the snapshot's own stream: construction and one-off kernels

    std::mutex pool_mutex_; ///< guards the pool below, never held while a batch runs
    std::condition_variable pool_ready_;
    std::vector<std::unique_ptr<workspace_t>> workspaces_;
    std::vector<workspace_t*> idle_;
    workspace_t* last_used_ = nullptr;
    std::size_t max_workspaces_ = 16;
};

#define USEARCH_AMD_DECLARE_LAUNCHERS(name)                                                                            \
    hipError_t launch_search_##name(const launch_params_t&, const snapshot_view_t&, const search_args_t&);            \
    hipError_t launch_distances_##name(const struct distances_params_t&, const snapshot_view_t&);                     \
    hipError_t launch_exact_##name(const struct exact_params_t&, const snapshot_view_t&);                             \
    hipError_t launch_build_##name(const struct build_params_t&, const snapshot_view_t&, const struct build_args_t&);
/// Every (metric, scalar) pair with a HIP kernel — the reference's own dispatch table, `configure_with_autovec`
/// (index_plugins.hpp:1930-2008); jaccard over bit sets is tanimoto there (2003-2004) and is mapped onto it at the boundary.
#define USEARCH_AMD_FOR_EACH_PAIR(X) \
    X(metric_ip_k, scalar_f32_k, ip_f32)\
    X(metric_cos_k, scalar_f32_k, cos_f32)\
    X(metric_l2sq_k, scalar_f32_k, l2sq_f32)\
    X(metric_pearson_k, scalar_f32_k, pearson_f32)\
    X(metric_ip_k, scalar_f16_k, ip_f16)\
    X(metric_cos_k, scalar_f16_k, cos_f16)\
    X(metric_l2sq_k, scalar_f16_k, l2sq_f16)\
    X(metric_pearson_k, scalar_f16_k, pearson_f16)\
    X(metric_ip_k, scalar_bf16_k, ip_bf16)\
    X(metric_cos_k, scalar_bf16_k, cos_bf16)\
    X(metric_l2sq_k, scalar_bf16_k, l2sq_bf16)\
    X(metric_pearson_k, scalar_bf16_k, pearson_bf16)\
    X(metric_ip_k, scalar_f64_k, ip_f64)\
    X(metric_cos_k, scalar_f64_k, cos_f64)\
    X(metric_l2sq_k, scalar_f64_k, l2sq_f64)\
    X(metric_pearson_k, scalar_f64_k, pearson_f64)\
    X(metric_ip_k, scalar_i8_k, ip_i8)\
    X(metric_cos_k, scalar_i8_k, cos_i8)\
    X(metric_l2sq_k, scalar_i8_k, l2sq_i8)\
    X(metric_pearson_k, scalar_i8_k, pearson_i8)\
    X(metric_divergence_k, scalar_f32_k, divergence_f32)\
    X(metric_divergence_k, scalar_f16_k, divergence_f16)\
    X(metric_divergence_k, scalar_bf16_k, divergence_bf16)\
    X(metric_divergence_k, scalar_f64_k, divergence_f64)\
    X(metric_haversine_k, scalar_f32_k, haversine_f32)\
    X(metric_haversine_k, scalar_f64_k, haversine_f64)\
    X(metric_hamming_k, scalar_b1x8_k, hamming_b1)\
    X(metric_tanimoto_k, scalar_b1x8_k, tanimoto_b1)\
    X(metric_sorensen_k, scalar_b1x8_k, sorensen_b1)
#define USEARCH_AMD_DECLARE_PAIR(metric_kind, scalar_kind, name) USEARCH_AMD_DECLARE_LAUNCHERS(name)
USEARCH_AMD_FOR_EACH_PAIR(USEARCH_AMD_DECLARE_PAIR)

/// Launch shape of one construction linking kernel (build_kernels.hpp): `reverse` = 0 select, 1 reverse links.
struct build_params_t {
    std::uint32_t lanes;
    std::uint32_t grid;
    int reverse;
    hipStream_t stream;
};

struct distances_params_t {
    metric_kind_t metric;
    std::uint32_t lanes;
    std::uint32_t lds_bytes;
    hipStream_t stream;
    const std::uint8_t* queries;
    std::uint64_t query_stride;
    const std::uint32_t* slots;
    std::uint32_t slots_per_query;
    std::uint32_t count;
    float* out;
};
struct exact_params_t {
    std::uint32_t lanes;
    std::uint32_t lds_bytes;
    hipStream_t stream;
    const std::uint8_t* queries;
    std::uint64_t query_stride;
    std::uint32_t query_count;
    std::uint32_t wanted;
    std::uint32_t partitions;
    std::uint64_t rows_per_partition;
    std::uint32_t map_keys;
    const std::uint32_t* allow_bits; ///< optional, device: one bit per slot, 0 = the caller's predicate rejects that member
    float* out_distances;      ///< [partitions][queries][wanted]
    std::uint64_t* out_keys;
    std::uint64_t* out_counts; ///< [partitions][queries]
};

/// One launch of the distance kernel behind `usearch_amd_distances` for the index's (metric, scalar) pair (engine.hip): `count` waves,
/// `slots_per_query` rows each. Also what the merges and the closing distances of clustering.hip run.
hipError_t launch_distances(metric_kind_t metric, scalar_kind_t scalar, const distances_params_t& p, const snapshot_view_t& view);

/// starts[r] = 1 where upper-level list r is a member's first (compact.hip): lists of one member are consecutive and members own
/// them in slot order, so the run of lists up to the next start is the member's level. `starts` ([lists], device) is zeroed first.
const char* mark_list_starts(const std::uint32_t* upper_ref, std::uint64_t members, std::uint64_t lists, std::uint8_t* starts,
                             hipStream_t stream);

/**
 *  Exact search over the rows of `view` (device pointers everywhere; `view` needs `vectors`, sizes and — when
 *  `map_keys` — `keys`): partition scan + fold. Results as `index_gt::search_exact_` gives them: top-`wanted` under
 *  (distance ↑, slot ↓), padded with key 0 / signalling NaN.
 */
const char* exact_search_device(metric_kind_t metric, scalar_kind_t scalar, std::uint32_t lanes,
                                const snapshot_view_t& view, const void* queries, std::size_t count,
                                std::size_t stride_bytes, std::size_t wanted, bool map_keys, std::uint64_t* keys,
                                float* distances, std::uint64_t* counts, hipStream_t stream, float* kernel_ms,
                                const std::uint32_t* allow_bits = nullptr);

/// Is there a tiled (matrix-unit) exact-search kernel for this pair and result count? (exact_tiled.hip: cos / ip / l2sq over f16
/// and bf16 — float tolerance —, cos / ip over f32 — a derived bound, not bit equality; l2sq over f32 stays refused — and over i8 — bit-identical to the wave-per-query
/// kernel. The table itself: `exact_tiled_pair` of exact_plan.hpp.) Or a bit tile (exact_bits.hip: hamming, tanimoto / jaccard and
/// sorensen over b1, no matrix unit, bit-identical to the wave-per-query kernel, NaN included; its table: `exact_bits_pair`)? Either
/// one makes the tiled routes available: `exact_search_tiled_device` runs whichever the pair has.
bool exact_tiled_available(metric_kind_t metric, scalar_kind_t scalar, std::size_t wanted);

/// Many-to-many exact search as a tiled matrix product (index_plugins.hpp:2071-2164): rows are read once per 64 queries — or, for the
/// b1 pairs of `exact_bits_pair`, the bit tile below. Same contract as `exact_search_device`.
const char* exact_search_tiled_device(metric_kind_t metric, scalar_kind_t scalar, const snapshot_view_t& view,
                                      const void* queries, std::size_t count, std::size_t stride_bytes, std::size_t wanted,
                                      bool map_keys, std::uint64_t* keys, float* distances, std::uint64_t* counts,
                                      hipStream_t stream, float* kernel_ms, const std::uint32_t* allow_bits = nullptr);

/// The bit tile (exact_bits.hip): rows are read once per 256 queries, popcount(a ∧ b) on the vector ALU. `metric`: hamming, tanimoto,
/// jaccard or sorensen; the view's rows are b1. Same contract and the same refusals as `exact_search_tiled_device`, which is its
/// one caller.
const char* exact_search_bits_device(metric_kind_t metric, const snapshot_view_t& view, const void* queries, std::size_t count,
                                     std::size_t stride_bytes, std::size_t wanted, bool map_keys, std::uint64_t* keys, float* distances,
                                     std::uint64_t* counts, hipStream_t stream, float* kernel_ms, const std::uint32_t* allow_bits = nullptr);

/// Host-buffer exact search of a raw dataset — `usearch_exact_search` (c/usearch.h:467-474): keys are dataset offsets.
/// `tiled`: the matrix-unit kernel (or the bit tile) over the uploaded rows for any pair that has one (`exact_tiled_available`; refused otherwise)
/// instead of the bit-exact wave-per-query one, which stays what the float kinds get unasked.
const char* exact_search_dataset_host(metric_kind_t metric, scalar_kind_t scalar, std::size_t dimensions,
                                      const void* dataset, std::size_t dataset_count, std::size_t dataset_stride,
                                      const void* queries, std::size_t queries_count, std::size_t queries_stride,
                                      std::size_t wanted, std::uint64_t* keys, std::size_t keys_stride,
                                      float* distances, std::size_t distances_stride, bool tiled = false);

/// Lanes per stored row, the row pitch and the 16-byte chunks the kernels read of a row of `bytes` bytes (the summation layout
/// of DESIGN.md §3.3; the pitch may exceed chunks × 16 so that short rows never straddle a 128-byte line).
void row_geometry(std::size_t bytes, std::uint32_t& lanes, std::uint32_t& row_stride, std::uint32_t& chunks);

/// Exchange step of sharded search (merge.hip): [shards][queries][wanted] per-shard results → [queries][wanted], device
/// pointers, `merge_into` tie rule with shards merged in index order. Returns after the stream has drained.
const char* merge_shards_device(const float* distances, const std::uint64_t* keys, const std::uint64_t* counts,
                                std::size_t shards, std::size_t queries, std::size_t wanted, float* out_distances,
                                std::uint64_t* out_keys, std::uint64_t* out_counts, hipStream_t stream,
                                bool later_position_first = true);

/// The same merge without the wait, shards `*_stride` ELEMENTS apart (a packed all-gather block keeps the three arrays of one
/// shard together, so the strides differ from the dense [shards][queries][wanted] case).
const char* merge_shards_enqueue(const float* distances, const std::uint64_t* keys, const std::uint64_t* counts,
                                 std::uint64_t distances_stride, std::uint64_t keys_stride, std::uint64_t counts_stride,
                                 std::size_t shards, std::size_t queries, std::size_t wanted, float* out_distances,
                                 std::uint64_t* out_keys, std::uint64_t* out_counts, hipStream_t stream,
                                 bool later_position_first = true);

/// Is there a HIP kernel for this (metric, scalar) pair?
bool kernel_available(metric_kind_t metric, scalar_kind_t scalar);

} // namespace usearch_amd
