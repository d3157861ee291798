/**
 *  usearch_amd/csrc/search_plan.hpp — the ONE place that chooses how a search batch is launched: the kernel instantiation (variant,
 *  `top` cells per lane, frontier, team, plain cut, scratch mode), the capacities of the visited set and the frontier, how a wave's LDS
 *  is carved up, the residency and the grid — and how all of that grows when a query outgrows its scratch. Pure integer arithmetic
 *  over the plain structs of engine.hpp: no HIP runtime call, no snapshot, no workspace, no look at the environment outside
 *  `read_search_knobs` (once per search call). engine.hip does the device work; tests/test_search_plan.py replays recorded calls here.
 */
#pragma once
#include <algorithm>

#include "engine.hpp"
#include "host_util.hpp"
#include "kernels.hpp"

namespace usearch_amd {

/// Rows of ≤ 128 bytes gathered next to the probe of the visited set (USEARCH_AMD_EARLY_ROWS = 0 | 1 overrides).
static constexpr std::size_t default_early_rows_k = 1; // 20M x 96 i8: +6.4 % at ef 80, +5.1 % at ef 64, same keys / bits / counters (profiles/r06_short_rows/early_rows.log)

/// gfx950 hands LDS out in blocks of 320 dwords (160 KB = 128 of them). Round 6 measured it the hard way: a wave of 8 160 bytes "fits" 20
/// times by a 1 024-byte count and runs as 18 (i8 × 96 at expansion 80 with 1 024 `seen` cells: 10.99 ms against 9.97 with 512).
constexpr std::uint64_t lds_granule_k = 1280;

/// Jaccard over bit sets IS Tanimoto in the reference's dispatch (index_plugins.hpp:2003-2004): one kernel serves both.
inline metric_kind_t kernel_metric(metric_kind_t metric) { return metric == metric_jaccard_k ? metric_tanimoto_k : metric; }

/// The float-valued pairs may keep their frontier as the open cells of a register `top` (kernels.hpp frontier_top_k).
inline bool frontier_in_top_capable(scalar_kind_t scalar) { return scalar != scalar_b1x8_k && scalar != scalar_i8_k; }

/// The environment's overrides for one search call over rows of `lanes` lanes.
inline search_knobs_t read_search_knobs(std::uint32_t lanes) {
    search_knobs_t k;
    k.lds_budget = env_size("USEARCH_AMD_LDS_BUDGET", 160 * 1024), k.hash_cap = env_size("USEARCH_AMD_HASH_CAP", 0);
    k.hash_load_pct = std::min<std::size_t>(75, std::max<std::size_t>(10, env_size("USEARCH_AMD_HASH_LOAD_PCT", lanes >= 8 ? 50 : 75)));
    k.next_cap = env_size("USEARCH_AMD_NEXT_CAP", 0), k.mode = env_size("USEARCH_AMD_MODE", 0);
    k.top_in_memory = env_size("USEARCH_AMD_TOP_IN_MEMORY", 0), k.no_two_cells = env_size("USEARCH_AMD_NO_TWO_CELLS", 0);
    k.frontier = env_size("USEARCH_AMD_FRONTIER", 0), k.variant = env_size("USEARCH_AMD_VARIANT", 0);
    k.no_team = env_size("USEARCH_AMD_NO_TEAM", 0), k.no_plain = env_size("USEARCH_AMD_NO_PLAIN", 0);
    k.waves_per_cu = env_size("USEARCH_AMD_WAVES_PER_CU", 32), k.no_small_batch_lds = env_size("USEARCH_AMD_NO_SMALL_BATCH_LDS", 0);
    k.early_rows = env_size("USEARCH_AMD_EARLY_ROWS", default_early_rows_k);
    k.aside_cells = env_size("USEARCH_AMD_ASIDE_CELLS", 0), k.plain_whatever_the_room = env_size("USEARCH_AMD_PLAIN_WHATEVER_THE_ROOM", 0);
    k.seen_cells = env_size("USEARCH_AMD_SEEN_CELLS", (std::size_t)-1);
    return k;
}

/// A visited set is never larger than the index could possibly need.
inline std::uint32_t hash_cap_ceiling(std::uint64_t size) { return pow2_ceil((std::uint32_t)std::min<std::uint64_t>(size * 2 + 128, 1u << 30)); }

/// LDS of one wave: its query, `top` (unless in registers), the frontier and — `scratch_lds_k` — the visited set. `with_sketch` adds
/// the room of the sketch's coefficients where the plan uses the sketch. `plan_search` counts it while it chooses the mode and trims
/// `next_cap`; `plan_rung` and `escalate` do not, and append the coefficients behind the other areas only where they still fit
/// (DESIGN.md §3.1 keeps that asymmetry as an open question).
inline std::uint64_t wave_lds_bytes(const search_plan_t& plan, int mode, std::uint32_t next_cap, std::uint32_t hash_cap, bool with_sketch) {
    if (mode == scratch_global_k)
        return plan.query_lds;
    const scratch_layout_t l = scratch_layout(plan.entries_per_lane ? 0 : plan.ef, next_cap, mode == scratch_lds_k ? (std::uint64_t)hash_cap * 4 : 0);
    return plan.query_lds + l.total + (with_sketch && plan.sketch ? sketch_columns_k * 4 + 16 : 0);
}

/// Waves of `lds_bytes` each that one compute unit keeps resident.
inline std::uint32_t waves_per_cu(const search_plan_t& plan, const search_knobs_t& knobs, std::uint64_t lds_bytes) {
    const std::uint64_t granule = (lds_bytes + lds_granule_k - 1) / lds_granule_k * lds_granule_k; // LDS is allocated in coarse granules
    return (std::uint32_t)std::max<std::uint64_t>(1, std::min<std::uint64_t>(plan.waves_cap, (std::uint32_t)knobs.lds_budget / std::max<std::uint64_t>(granule, 1)));
}

/// What the build cut for plain batches (kernels.hpp `plain_ak`) takes for granted, as far as a rung over short rows and the global
/// hash knows it before it looks for LDS cells: the engine vouches for all of it (USEARCH_AMD_NO_PLAIN=1 keeps the general build).
inline bool plain_wanted(const search_shape_t& shape, const search_plan_t& plan, const search_rung_t& rung) {
    return plan.plain_possible && !shape.query_ids && !shape.beam_level && !shape.descent_only && !shape.allow_bits && !shape.exclude_own &&
           (shape.lanes == 1 || rung.early_rows != 0);
}

/// Everything settled before the first launch. → nullptr, or why the call is refused.
inline const char* plan_search(const search_shape_t& shape, const search_tuning_t& tuning, const search_knobs_t& knobs, search_plan_t& plan) {
    plan = search_plan_t{};
    const metric_kind_t metric = (metric_kind_t)shape.metric;
    const scalar_kind_t scalar = (scalar_kind_t)shape.scalar;
    const std::uint32_t lanes = shape.lanes;
    const std::uint64_t count = shape.count;
    const std::uint32_t ef = plan.ef = (std::uint32_t)std::max(shape.expansion ? shape.expansion : default_expansion_search_k, shape.wanted); // index.hpp:3052

    // ---- scratch sizing, from measurements with the reference's own traversal (DESIGN.md "scratch sizing"): the frontier
    // peaks at 2.4-3.9 × ef; the visited set ends at 18-30 × ef entries plus what the first hops of a big index cost
    // whatever the expansion (10M × 768, ef = 64: 3 137 entries = 49 × ef) — hence the constant term. Outliers go through
    // the retry ladder.
    plan.query_lds = shape.chunks * (query_chunk_bytes_of(scalar));
    const std::uint32_t lds_budget = (std::uint32_t)knobs.lds_budget;
    std::uint32_t hash_cap = tuning.hash_cap ? tuning.hash_cap : (std::uint32_t)knobs.hash_cap;
    if (!hash_cap) {
        // entries expected ÷ the load the set is sized for: 75 % (the kernel's limit) for short rows, whose slabs must stay
        // cache-resident (profiles/r02_visited_set.log); 50 % for rows of ≥ 128 bytes — every probe round is a two-microsecond trip
        // to the memory side for the whole wave, and the headline batch runs 1.9 % faster with 65 536 cells than with 32 768
        // (46.2 against 47.1 ms on fresh blocks, profiles/r04_placement/scratch_footprint.log); USEARCH_AMD_HASH_LOAD_PCT overrides
        const std::uint32_t load_pct = (std::uint32_t)knobs.hash_load_pct;
        hash_cap = std::max<std::uint32_t>(1024, (std::uint32_t)((std::uint64_t)(ef * 30 + 1600) * 100 / load_pct));
    }
    hash_cap = pow2_ceil(hash_cap);
    std::uint32_t next_cap = tuning.next_cap ? tuning.next_cap : (std::uint32_t)knobs.next_cap;
    if (!next_cap) // (peaks measured on 20M-vector slices, 100 000 queries: b1 × 128 at 64: median 158, maximum 317; i8 × 96 at 80: 220 / 360)
        next_cap = std::max<std::uint32_t>(448, ef * 3 + 256);
    hash_cap = std::min<std::uint32_t>(hash_cap, hash_cap_ceiling(shape.size));
    next_cap = (std::uint32_t)std::min<std::uint64_t>(next_cap, shape.size + 64);

    const std::uint32_t mode_request = tuning.mode ? tuning.mode : (std::uint32_t)knobs.mode;
    if (mode_request > 3)
        return "Unknown scratch mode";
    // `top` lives in registers (1 / 4 / 8 / 16 entries per lane) while the expansion allows it
    const bool top_in_memory = tuning.top_in_memory || knobs.top_in_memory != 0;
    const bool two_cells = lanes <= 2 && ef <= 128 && !knobs.no_two_cells; // short rows: see kernel_waves()
    const std::uint32_t entries_per_lane = top_in_memory ? 0u : ef <= 64 ? 1u : two_cells ? 2u : ef <= 256 ? 4u : ef <= 512 ? 8u : ef <= 1024 ? 16u : 0u;
    plan.entries_per_lane = entries_per_lane;

    // ---- who holds the frontier (kernels.hpp frontier_mode_t): the open cells of `top` wherever that is exact up to ties —
    // float-valued pair, `top` in registers, every member a result candidate, slots below 2^31 — else the reference's heap
    const std::uint32_t frontier_request = tuning.frontier ? tuning.frontier : (std::uint32_t)knobs.frontier;
    const bool filtered = shape.has_tombstones || shape.allow_bits || shape.exclude_own;
    const bool in_top_possible = frontier_in_top_capable(scalar) && entries_per_lane && !filtered && mode_request != 3 &&
                                 shape.size < 0x80000000ull && !(shape.reference_frontier || shape.descent_only);
    if (frontier_request == 2 && !in_top_possible)
        return "The frontier cannot ride in `top` for this search (integer-valued pair, filter, tombstones or expansion > 1024)";
    const int frontier = (frontier_request == 1 || !in_top_possible) ? frontier_heap_k : frontier_top_k;
    if (frontier == frontier_top_k)
        next_cap = 0;

    // register/latency trade-off of the kernel (kernels.hpp kernel_variant_t); rows shorter than 8 chunks per lane have
    // nothing to unroll
    const std::uint32_t chunks_per_lane = shape.chunks / lanes;
    const std::uint32_t variant_request = tuning.variant ? tuning.variant : (std::uint32_t)knobs.variant;
    int variant = variant_u4_w4_k;
    const bool every_build = lanes == 8 && all_kernel_builds(metric, scalar);
    if (every_build && chunks_per_lane >= 8) {
        // measured on 10M x 768 f16 (profiles/): a whole row per round trip (12 loads per lane, 8 waves per CU) beats 8 loads
        // at 12 waves per CU at every expansion — the traversal is latency-bound, fewer round trips per hop win
        variant = chunks_per_lane >= 12 ? variant_u12_w2_k : variant_u8_w3_k;
        // Without the heap (profiles/r02_sweep_variants.log, ef = 608): every build lands within 3 % of the others — the
        // kernel moves 4.6-4.9 TB/s of rows plus the visited-set traffic, which is what random 1.5-KB gathers reach on this
        // memory system at all — and what separates them is the DRAIN of the batch: with one wave per query the last queries
        // run alone, for about 0.65 × waves / queries of the launch. Few waves with many bytes in flight each (two rows per
        // lane group per round, 8 waves per CU) win while that matters; 16 waves per CU win once the batch is long enough.
        if (frontier == frontier_top_k && chunks_per_lane >= 12)
            variant = count >= 40000 ? variant_u4_w4_k : variant_u12x2_w2_k;
    }
    if (variant_request && variant_request - 1 < (std::uint32_t)variant_count_k && every_build) {
        const int requested = (int)variant_request - 1;
        if (requested == variant_u12x2_w2_k && frontier != frontier_top_k)
            return "That kernel build exists for the in-`top` frontier only";
        variant = requested;
    }
    // A batch that cannot give every CU two queries to walk (a `usearch_search` caller's single query above all) over long rows: four
    // helper waves per query take the rows of every hop, the leader walks and commits (kernels.hpp team_search_kernel)
    const bool team = every_build && chunks_per_lane >= 8 && !variant_request && mode_request != 3 &&
                      count <= 2ull * shape.compute_units && !shape.descent_only && !knobs.no_team && !tuning.waves_per_cu;
    if (team)
        variant = variant_u12_w2_k;
    // whether this call can run the short-row build cut for plain batches (kernels.hpp `plain_ak`) as far as that is known here; the
    // scratch mode, the `seen` cells and the early rows are settled per rung in plan_rung, which has the last word (`rung.plain`)
    plan.plain_possible = !team && !shape.has_tombstones && shape.m0 <= 64 && shape.nbr0 &&
                          !(shape.query_ids || shape.beam_level || shape.descent_only || shape.allow_bits || shape.exclude_own) &&
                          (lanes == 1 ? shape.nbr0_rows && shape.chunks == 1 : lanes == 2) &&
                          plain_build_exists(metric, scalar, (int)lanes, variant == variant_u4_w4_k, true, (int)entries_per_lane,
                                             frontier == frontier_heap_k) &&
                          !knobs.no_plain;
    const std::uint32_t variant_waves_per_cu =
        4u * (std::uint32_t)kernel_waves(variant, (int)entries_per_lane, frontier, (int)lanes, plan.plain_possible);
    const std::uint32_t waves_cap = tuning.waves_per_cu ? tuning.waves_per_cu : (std::uint32_t)knobs.waves_per_cu;
    plan.waves_cap = std::min(waves_cap, variant_waves_per_cu);

    // the sketch (sketch.hpp): plain and filtered searches of the finished graph walked by one wave per query in a build with twelve
    // loads in flight (the others have no registers to spare: kernels.hpp); `tuning.sketch` = 1 turns it off for this call, 2 keeps
    // auto mode from judging it by this call. Its 256 bytes of LDS per wave (plus alignment) count in every residency decision below.
    if (tuning.sketch > 2)
        return "Unknown sketch mode";
    plan.sketch = shape.sketch && tuning.sketch != 1 && !team && mode_request != 3 &&
                  (variant == variant_u12_w2_k || variant == variant_u12x2_w2_k) &&
                  !(shape.query_ids || shape.beam_level || shape.descent_only || shape.reference_frontier);
    auto lds_bytes_for = [&](int mode, std::uint32_t cap_next, std::uint32_t cap_hash) { return wave_lds_bytes(plan, mode, cap_next, cap_hash, true); };
    auto waves_for = [&](std::uint64_t lds_bytes) { return waves_per_cu(plan, knobs, lds_bytes); };
    // the frontier's default room has 256 cells of slack; when giving up to half of it back lets one more wave share the
    // compute unit's LDS, do (the retry ladder still catches a query that would have needed them)
    const bool default_next_cap = !tuning.next_cap && !knobs.next_cap;
    if (default_next_cap && next_cap && mode_request != 1 && mode_request != 3) {
        const std::uint32_t now = waves_for(lds_bytes_for(scratch_hash_k, next_cap, hash_cap));
        if (now < plan.waves_cap) {
            const std::uint64_t room = lds_budget / (now + 1) / lds_granule_k * lds_granule_k;
            const std::uint64_t fixed = lds_bytes_for(scratch_hash_k, 0, hash_cap);
            if (room > fixed) {
                const std::uint32_t trimmed = (std::uint32_t)((room - fixed) / 8 / 2 * 2);
                if (trimmed < next_cap && trimmed + 128 >= next_cap)
                    next_cap = trimmed;
            }
        }
    }
    // auto: keep the visited set in LDS only while that does not cost a resident wave; otherwise move it to the global hash. A batch
    // so small that every query gets a wave of its own even at the LDS residency (a `usearch_search` caller's single query above
    // all) also takes LDS: residency buys it nothing, and every probe round of the global hash is a two-microsecond trip to the
    // memory side — half of such a query's latency (profiles/r03_short_rows/README.md §1)
    std::uint64_t lds_mode_bytes = lds_bytes_for(scratch_lds_k, next_cap, hash_cap);
    // a set sized for half load that does not fit LDS where the one sized for 75 % would (expansion 608 over long rows: 256 KB
    // against 128 KB): a small batch takes the smaller set in LDS rather than the larger one in global memory — a lone query walks
    // 3.1 ms that way and 3.5 ms the other
    if (!tuning.hash_cap && !knobs.hash_cap && mode_request == 0 && lds_mode_bytes > lds_budget) {
        const std::uint32_t tighter = std::min<std::uint32_t>(pow2_ceil(std::max<std::uint32_t>(1024, (ef * 30 + 1600) / 3 * 4)), hash_cap_ceiling(shape.size));
        const std::uint64_t tighter_bytes = lds_bytes_for(scratch_lds_k, next_cap, tighter);
        if (tighter < hash_cap && tighter_bytes <= lds_budget && count <= (std::uint64_t)waves_for(tighter_bytes) * shape.compute_units &&
            !knobs.no_small_batch_lds) {
            hash_cap = tighter;
            lds_mode_bytes = tighter_bytes;
        }
    }
    const bool small_batch = lds_mode_bytes <= lds_budget && count <= (std::uint64_t)waves_for(lds_mode_bytes) * shape.compute_units &&
                             !knobs.no_small_batch_lds;
    plan.mode = mode_request == 1 ? scratch_lds_k : mode_request == 2 ? scratch_hash_k : mode_request == 3 ? scratch_global_k
                : (small_batch || waves_for(lds_mode_bytes) >= std::min<std::uint32_t>(8, plan.waves_cap) ? scratch_lds_k : scratch_hash_k);
    plan.hash_cap = hash_cap, plan.next_cap = next_cap, plan.variant = variant, plan.frontier = frontier, plan.team = team ? 1u : 0u;
    plan.stats.frontier = frontier == frontier_top_k ? 2u : 1u, plan.stats.top_cells = entries_per_lane;
    plan.stats.variant = team ? 5u : (std::uint32_t)variant + 1; // 5 = the team build (five waves per query)
    return nullptr;
}

/// One rung of the ladder over `pending` queries: the team's demotion, the mode and `next_cap` that fit the budget, and — unless that
/// ends in `scratch_global_k` — the areas behind the wave's heaps, the residency and the grid. Revises `plan`, shapes `rung`.
inline void plan_rung(const search_shape_t& shape, const search_knobs_t& knobs, search_plan_t& plan, std::uint32_t pending, search_rung_t& rung) {
    rung = search_rung_t{};
    const std::uint32_t lanes = shape.lanes;
    const std::uint32_t lds_budget = (std::uint32_t)knobs.lds_budget;
    auto lds_bytes_now = [&]() { return wave_lds_bytes(plan, plan.mode, plan.next_cap, plan.hash_cap, false); };
    auto waves_for = [&](std::uint64_t lds_bytes) { return waves_per_cu(plan, knobs, lds_bytes); };
    // a team's workgroup adds its shared control block (16-byte alignment + 64 bytes) to the leader's areas: a size that only just
    // fits the budget alone must not become a launch failure — such a batch walks with one wave per query
    if (plan.team && plan.mode != scratch_global_k && align16(lds_bytes_now()) + team_block_bytes_k > lds_budget) {
        plan.team = 0;
        plan.stats.variant = (std::uint32_t)plan.variant + 1;
    }
    if (plan.mode != scratch_global_k && lds_bytes_now() > lds_budget) {
        if (plan.mode == scratch_lds_k)
            plan.mode = scratch_hash_k;
        while (plan.next_cap > 64 && lds_bytes_now() > lds_budget)
            plan.next_cap /= 2;
        if (lds_bytes_now() > lds_budget)
            plan.mode = scratch_global_k; // `top` alone does not fit LDS: straight to the global fallback
    }
    rung.mode = plan.mode;
    if (plan.mode == scratch_global_k) {
        // ---- last rung: global-memory scratch — exact sizes (one bit per slot, one frontier cell per slot), cannot overflow;
        //      the reference's heap (a frontier in `top` needs `top` in registers)
        rung.bitmap_bytes = ((shape.size + 31) / 32) * 4;
        rung.next_cap = (std::uint32_t)std::min<std::uint64_t>(shape.size + 64, 0xFFFFFFF0u);
        const scratch_layout_t layout = scratch_layout(plan.ef, rung.next_cap, rung.bitmap_bytes);
        rung.visits_offset = layout.visits, rung.slab = (layout.total + 255) & ~(std::uint64_t)255;
        rung.frontier = frontier_heap_k, rung.lds_bytes = plan.query_lds, plan.sketch = 0;
        rung.grid = pending; // one wave per query; the engine cuts the rung into chunks where its memory budget asks for that
        return;
    }
    // a team's workgroup carries the leader's LDS areas plus the shared block; one workgroup per query of the small batch
    std::uint64_t wave_bytes = lds_bytes_now();
    rung.team = plan.team, rung.frontier = plan.frontier, rung.entries_per_lane = plan.entries_per_lane;
    rung.hash_cap = plan.hash_cap, rung.next_cap = plan.next_cap;
    // rows of ≤ 128 bytes gathered next to the probe of the visited set instead of behind it (kernels.hpp, the hop loop)
    rung.early_rows = plan.mode == scratch_hash_k && !plan.team && lanes == 2 && knobs.early_rows ? 1u : 0u;
    plan.stats.early_rows = rung.early_rows;
    // short rows over a global visited set: `seen` cells in LDS in front of it (kernels.hpp `search_one`) — as many as cost no
    // resident wave (the walk lives on its residency), at most 2 048; USEARCH_AMD_SEEN_CELLS forces a number (0 = none)
    const bool short_rows_over_hash = plan.mode == scratch_hash_k && !plan.team && lanes <= 2;
    if (short_rows_over_hash) {
        // a plain `search` batch runs the build without the features it never uses (kernels.hpp `plain_ak`, `plain_wanted` above). That
        // build never probes the slab past a member's home cell and sets what collides aside in LDS: about visits² / (2 · cells of the
        // slab) members, visits ≈ 20 · expansion + 800 on the measured shapes (20M × 128 b1 at 64: median 1 521, maximum 2 225 of
        // 100 000 queries; 20M × 96 i8 at 80: 1 742 / 2 281) — 512 cells at three quarters' load must take them, and must cost no
        // resident wave; a query that outgrows them all the same is run again by the retry ladder
        const bool aside_wanted = plain_wanted(shape, plan, rung) && lanes == 2; // (rows that travel with the lists gain nothing from it: kernels.hpp)
        if (aside_wanted) {
            std::uint32_t aside_cells = 512;
            if (const std::size_t forced_cells = knobs.aside_cells) // tests: a table that is sure to fill up
                for (aside_cells = 64; aside_cells * 2 <= forced_cells && aside_cells < 2048; aside_cells *= 2) {}
            const std::uint64_t expected_visits = std::min<std::uint64_t>((std::uint64_t)plan.ef * 20 + 800, shape.size);
            const bool room = expected_visits * expected_visits / (2ull * plan.hash_cap) <= aside_cells * 3ull / 4 ||
                              knobs.plain_whatever_the_room; // tests: a query that outgrows `aside` goes up the retry ladder
            const std::uint64_t with_aside = align16(wave_bytes) + aside_cells * 4ull;
            if (room && waves_for(with_aside) >= waves_for(wave_bytes) && with_aside <= lds_budget) {
                rung.aside_offset = (std::uint32_t)align16(wave_bytes);
                rung.aside_cells = aside_cells;
                wave_bytes = with_aside;
            }
        }
        const std::size_t forced = knobs.seen_cells;
        std::uint32_t cells = 0;
        if (forced != (std::size_t)-1) {
            for (cells = 1; cells * 2 <= forced && cells < 8192; cells *= 2) {}
            cells = forced ? cells : 0;
        } else {
            for (std::uint32_t candidate = 2048; candidate >= 128 && !cells; candidate /= 2)
                if (waves_for(align16(wave_bytes) + candidate * 4ull) >= waves_for(wave_bytes))
                    cells = candidate;
        }
        if (cells && align16(wave_bytes) + cells * 4ull <= lds_budget) {
            rung.seen_offset = (std::uint32_t)align16(wave_bytes);
            rung.seen_cells = cells;
            wave_bytes = rung.seen_offset + cells * 4ull;
        }
        plan.stats.seen_cells = rung.seen_cells;
        // decided with the LDS areas above: what the instantiation takes for granted must be there
        if (plain_wanted(shape, plan, rung))
            rung.plain = (lanes == 2 ? rung.aside_cells : rung.seen_cells) ? 1u : 0u;
    }
    plan.stats.plain = rung.plain, plan.stats.aside_cells = rung.aside_cells;
    // the query's 64 coefficients on the sketch's directions: 256 bytes behind the wave's other areas
    if (plan.sketch) {
        const std::uint64_t offset = align16(wave_bytes);
        if (!plan.team && offset + sketch_columns_k * 4 <= lds_budget) {
            rung.sketch_offset = (std::uint32_t)offset;
            wave_bytes = offset + sketch_columns_k * 4;
        } else {
            plan.sketch = 0;
        }
    }
    const std::uint64_t lds_bytes = plan.team ? align16(wave_bytes) + team_block_bytes_k : wave_bytes;
    rung.team_offset = plan.team ? (std::uint32_t)align16(wave_bytes) : 0u, rung.lds_bytes = (std::uint32_t)lds_bytes;
    rung.grid = plan.team ? pending : (std::uint32_t)std::min<std::uint64_t>(pending, (std::uint64_t)waves_for(lds_bytes) * shape.compute_units);
    rung.slab = plan.mode == scratch_hash_k ? (std::uint64_t)plan.hash_cap * 4 : 0;
}

/// What the rung after rung `rung_index` runs with, for the queries that outgrew their scratch there. Second rung: visited set in the
/// global hash, 4× the room for both structures (the frontier's as far as LDS takes it). Third rung: global-memory scratch.
inline void escalate(const search_shape_t& shape, const search_knobs_t& knobs, search_plan_t& plan, int rung_index) {
    plan.mode = rung_index == 0 ? scratch_hash_k : scratch_global_k;
    if (rung_index != 0)
        return;
    plan.hash_cap = std::min<std::uint32_t>(plan.hash_cap * 4, hash_cap_ceiling(shape.size));
    if (plan.next_cap) {
        plan.next_cap = (std::uint32_t)std::min<std::uint64_t>((std::uint64_t)plan.next_cap * 4, shape.size + 64);
        while (plan.next_cap > 64 && wave_lds_bytes(plan, scratch_hash_k, plan.next_cap, 0, false) > (std::uint32_t)knobs.lds_budget)
            plan.next_cap = plan.next_cap * 3 / 4;
    }
}

} // namespace usearch_amd
