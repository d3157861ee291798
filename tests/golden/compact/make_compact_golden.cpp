// tests/golden/compact/make_compact_golden.cpp — one-off driver that recorded tests/golden/compact/*.npz: the reference builds a
// small index on one thread, removes a set of keys, saves (image "before"), calls `index_dense_gt::isolate()`
// (index_dense.hpp:1709-1720) and saves again (image "after"). make_compact_golden.py next to it feeds it and packs the
// fixtures. Not built by the project, not run by a test.
//
//   clang++ -std=c++17 -O2 -DUSEARCH_USE_SIMSIMD=0 -DUSEARCH_USE_FP16LIB=0 -DUSEARCH_USE_OPENMP=0 -I<reference>/include \
//       make_compact_golden.cpp -o make_compact_golden -lpthread
//
//   make_compact_golden X.bin N dims connectivity removed.bin removed_count before.usearch after.usearch
//
// X.bin: f32 [N][dims]; member i gets key 1000 + i. removed.bin: u64 keys.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <usearch/index_dense.hpp>

using namespace unum::usearch;

int main(int argc, char** argv) {
    if (argc != 9)
        return std::fprintf(stderr, "usage: see the header of make_compact_golden.cpp\n"), 2;
    const std::size_t count = std::strtoull(argv[2], nullptr, 10), dimensions = std::strtoull(argv[3], nullptr, 10);
    const std::size_t connectivity = std::strtoull(argv[4], nullptr, 10), removed_count = std::strtoull(argv[6], nullptr, 10);
    std::vector<float> points(count * dimensions);
    std::vector<unsigned long long> removed(removed_count);
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in || std::fread(points.data(), 4, points.size(), in) != points.size())
        return std::fprintf(stderr, "cannot read %s\n", argv[1]), 1;
    std::fclose(in);
    in = std::fopen(argv[5], "rb");
    if (!in || std::fread(removed.data(), 8, removed.size(), in) != removed.size())
        return std::fprintf(stderr, "cannot read %s\n", argv[5]), 1;
    std::fclose(in);

    metric_punned_t metric(dimensions, metric_kind_t::cos_k, scalar_kind_t::f32_k);
    index_dense_config_t config(connectivity);
    index_dense_t index = index_dense_t::make(metric, config);
    if (!index.try_reserve(count))
        return std::fprintf(stderr, "cannot reserve\n"), 1;
    for (std::size_t i = 0; i < count; ++i)
        if (!index.add(1000 + i, points.data() + i * dimensions))
            return std::fprintf(stderr, "cannot add\n"), 1;
    for (unsigned long long key : removed)
        if (!index.remove(key))
            return std::fprintf(stderr, "cannot remove %llu\n", key), 1;
    if (!index.save(argv[7]))
        return std::fprintf(stderr, "cannot save\n"), 1;
    auto result = index.isolate();
    if (!result)
        return std::fprintf(stderr, "isolate failed\n"), 1;
    if (!index.save(argv[8]))
        return std::fprintf(stderr, "cannot save\n"), 1;
    return 0;
}
