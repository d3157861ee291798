// tests/cpp/compact_surface.cpp — `isolate()` and `compact()` through the C++ class surface (include/usearch/index_dense.hpp), called
// the way the reference's cpp/test.cpp:1147-1180 (`test_isolate`) calls them. `compact_surface link` proves that it compiles and
// links (no GPU); `compact_surface run` runs that scenario: 16 members, the even keys removed, `isolate()`, every search returns
// 8; then `compact()` and `size() == 8`.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include <usearch/index_dense.hpp>

using namespace unum::usearch;

#define EXPECT(condition)                                                                                              \
    do {                                                                                                               \
        if (!(condition)) {                                                                                            \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #condition);                                         \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main(int argc, char** argv) {
    std::printf("isolate and compact through index_dense_t\n");
    if (argc < 2 || std::strcmp(argv[1], "run") != 0)
        return 0;
    constexpr std::size_t dataset_count = 16, dimensions = 32;
    metric_punned_t metric(dimensions, metric_kind_t::cos_k);
    std::mt19937 generator(7);
    std::uniform_real_distribution<float> distribution(0.0, 1.0);
    std::vector<std::vector<float>> vectors(dataset_count, std::vector<float>(dimensions));
    for (auto& vector : vectors)
        for (float& x : vector)
            x = distribution(generator);

    index_dense_t index = index_dense_t::make(metric);
    index.reserve(dataset_count);
    for (std::size_t idx = 0; idx < dataset_count; ++idx)
        index.add(idx, vectors[idx].data());
    EXPECT(index.size() == dataset_count);
    for (std::size_t idx = 0; idx < dataset_count; idx += 2)
        EXPECT(index.remove(idx));

    index_dense_t::compaction_result_t isolated = index.isolate();
    EXPECT(isolated);
    EXPECT(isolated.pruned_edges > 0);
    for (std::size_t idx = 0; idx < dataset_count; ++idx) {
        auto result = index.search(vectors[idx].data(), 16);
        EXPECT(result.size() == dataset_count / 2);
    }

    std::size_t told = 0;
    auto compacted = index.compact(executor_default_t(4), [&](std::size_t progress, std::size_t total) {
        told = total;
        return progress == total;
    });
    EXPECT(compacted);
    EXPECT(index.size() == dataset_count / 2 && told == dataset_count / 2);
    for (std::size_t idx = 0; idx < dataset_count; ++idx) {
        EXPECT(index.contains(idx) == (idx % 2 == 1));
        auto result = index.search(vectors[idx].data(), 16);
        EXPECT(result.size() == dataset_count / 2);
        if (idx % 2)
            EXPECT(result[0].member.key == idx);
    }
    std::printf("ok\n");
    return 0;
}
