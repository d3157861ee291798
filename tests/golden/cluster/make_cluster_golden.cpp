// tests/golden/cluster/make_cluster_golden.cpp — one-off driver that recorded tests/golden/cluster/*.npz: the reference builds a
// small index on one thread (member i gets key 1000 + i), saves it, and runs its own
// `index_dense_gt::cluster(begin, end, config, keys, distances)` (index_dense.hpp:1819-1981) over vector queries or member keys.
// make_cluster_golden.py next to it feeds it and packs the fixtures. Not built by the project, not run by a test. Built like
// tests/golden/compact/make_compact_golden.cpp:
//
//   clang++ -std=c++17 -O2 -DUSEARCH_USE_SIMSIMD=0 -DUSEARCH_USE_FP16LIB=0 -DUSEARCH_USE_OPENMP=0 -I<reference>/include \
//       make_cluster_golden.cpp -o make_cluster_golden -lpthread
//
//   make_cluster_golden metric scalar X.bin N dims connectivity vectors|keys Q.bin Q min max image.usearch results.bin [repeats]
//
// X.bin: [N] rows in the storage kind (b1: dims / 8 bytes a row). Q.bin: [Q] rows in the storage kind, or [Q] u64 keys.
// results.bin: u64 keys[Q], f32 distances[Q], u64 clusters, visited_members, computed_distances. `repeats` > 0 prints the best
// wall time of that many runs of `cluster` as one JSON line (the yardstick of profiles/r10_clustering/); the index is then built
// on every core (nothing is recorded from such a run: the graph depends on the threads' timing) and `cluster` maps on every core.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <usearch/index_dense.hpp>

using namespace unum::usearch;

static std::vector<char> read_all(const char* path) {
    std::vector<char> bytes;
    std::FILE* in = std::fopen(path, "rb");
    if (!in)
        std::fprintf(stderr, "cannot read %s\n", path), std::exit(1);
    std::fseek(in, 0, SEEK_END);
    bytes.resize((std::size_t)std::ftell(in));
    std::fseek(in, 0, SEEK_SET);
    if (bytes.size() && std::fread(bytes.data(), 1, bytes.size(), in) != bytes.size())
        std::fprintf(stderr, "cannot read %s\n", path), std::exit(1);
    std::fclose(in);
    return bytes;
}

/// An iterator over rows of `stride` bytes that dereferences to `scalar const*`, as `cluster` asks.
template <typename scalar_at> struct rows_iterator_t {
    const char* base;
    std::size_t stride;
    scalar_at const* operator[](std::size_t i) const { return reinterpret_cast<scalar_at const*>(base + i * stride); }
    std::ptrdiff_t operator-(rows_iterator_t const& other) const { return (base - other.base) / (std::ptrdiff_t)stride; }
};

template <typename scalar_at> int run(int argc, char** argv, metric_kind_t metric_kind, scalar_kind_t scalar_kind) {
    const std::size_t count = std::strtoull(argv[4], nullptr, 10), dimensions = std::strtoull(argv[5], nullptr, 10);
    const std::size_t connectivity = std::strtoull(argv[6], nullptr, 10), queries_count = std::strtoull(argv[9], nullptr, 10);
    const bool by_keys = std::string(argv[7]) == "keys";
    index_dense_clustering_config_t clustering;
    clustering.min_clusters = std::strtoull(argv[10], nullptr, 10), clustering.max_clusters = std::strtoull(argv[11], nullptr, 10);
    const std::size_t repeats = argc > 14 ? std::strtoull(argv[14], nullptr, 10) : 0;

    metric_punned_t metric(dimensions, metric_kind, scalar_kind);
    const std::size_t row_bytes = metric.bytes_per_vector();
    std::vector<char> points = read_all(argv[3]), queries = read_all(argv[8]);
    if (points.size() != count * row_bytes || queries.size() != queries_count * (by_keys ? 8 : row_bytes))
        return std::fprintf(stderr, "input sizes do not match\n"), 1;

    index_dense_config_t config(connectivity);
    index_dense_t index = index_dense_t::make(metric, config);
    executor_default_t executor(repeats ? std::thread::hardware_concurrency() : 1);
    if (!index.try_reserve(index_limits_t(count, executor.size())))
        return std::fprintf(stderr, "cannot reserve\n"), 1;
    if (repeats) {
        executor.fixed(count, [&](std::size_t thread, std::size_t i) {
            index.add(1000 + i, reinterpret_cast<scalar_at const*>(points.data() + i * row_bytes), thread);
        });
        if (index.size() != count)
            return std::fprintf(stderr, "cannot add\n"), 1;
    } else {
        for (std::size_t i = 0; i < count; ++i)
            if (!index.add(1000 + i, reinterpret_cast<scalar_at const*>(points.data() + i * row_bytes)))
                return std::fprintf(stderr, "cannot add\n"), 1;
    }
    if (!index.save(argv[12]))
        return std::fprintf(stderr, "cannot save\n"), 1;

    std::vector<index_dense_t::vector_key_t> keys(queries_count);
    std::vector<index_dense_t::distance_t> distances(queries_count);
    index_dense_t::clustering_result_t result;
    double best = 1e30;
    for (std::size_t round = 0; round < (repeats ? repeats : 1); ++round) {
        const auto started = std::chrono::steady_clock::now();
        if (by_keys) {
            auto* begin = reinterpret_cast<index_dense_t::vector_key_t const*>(queries.data());
            result = index.cluster(begin, begin + queries_count, clustering, keys.data(), distances.data(), executor);
        } else {
            rows_iterator_t<scalar_at> begin{queries.data(), row_bytes}, end{queries.data() + queries_count * row_bytes, row_bytes};
            result = index.cluster(begin, end, clustering, keys.data(), distances.data(), executor);
        }
        best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count());
        if (!result)
            return std::fprintf(stderr, "cluster failed: %s\n", result.error.release()), 1;
    }
    std::FILE* out = std::fopen(argv[13], "wb");
    if (!out)
        return std::fprintf(stderr, "cannot write %s\n", argv[13]), 1;
    const unsigned long long tail[3] = {result.clusters, result.visited_members, result.computed_distances};
    std::fwrite(keys.data(), 8, keys.size(), out), std::fwrite(distances.data(), 4, distances.size(), out), std::fwrite(tail, 8, 3, out);
    std::fclose(out);
    if (repeats)
        std::printf("{\"reference_cluster_seconds\": %.6f, \"threads\": %zu, \"members\": %zu, \"queries\": %zu, \"clusters\": %llu}\n", best,
                    executor.size(), count, queries_count, tail[0]);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 14)
        return std::fprintf(stderr, "usage: see the header of make_cluster_golden.cpp\n"), 2;
    const std::string metric = argv[1], scalar = argv[2];
    const metric_kind_t metric_kind = metric == "cos"       ? metric_kind_t::cos_k
                                      : metric == "l2sq"    ? metric_kind_t::l2sq_k
                                      : metric == "ip"      ? metric_kind_t::ip_k
                                      : metric == "hamming" ? metric_kind_t::hamming_k
                                                            : metric_kind_t::unknown_k;
    if (metric_kind == metric_kind_t::unknown_k)
        return std::fprintf(stderr, "unknown metric\n"), 2;
    if (scalar == "f32")
        return run<f32_t>(argc, argv, metric_kind, scalar_kind_t::f32_k);
    if (scalar == "i8")
        return run<i8_t>(argc, argv, metric_kind, scalar_kind_t::i8_k);
    if (scalar == "b1")
        return run<b1x8_t>(argc, argv, metric_kind, scalar_kind_t::b1x8_k);
    return std::fprintf(stderr, "unknown scalar kind\n"), 2;
}
