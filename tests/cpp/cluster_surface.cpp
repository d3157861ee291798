// tests/cpp/cluster_surface.cpp — `cluster(begin, end, config, keys, distances)` through the C++ class surface
// (include/usearch/index_dense.hpp), called the way the reference's own callers do (python/lib.cpp:662-777): once with an iterator
// over `i8_t const*` rows, once with an iterator over member keys. `cluster_surface link` proves that it compiles and links (no
// GPU); `cluster_surface run image.usearch Q.bin Q dims min max out.bin` loads a saved i8 index, clusters the Q rows of Q.bin and
// then the members 1000 … 1000 + Q − 1, and writes for each: u64 keys[Q], f32 distances[Q], u64 clusters, visited, computed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct rows_t {
    i8_t const* base;
    std::size_t dimensions;
    i8_t const* operator[](std::size_t i) const { return base + i * dimensions; }
    std::ptrdiff_t operator-(rows_t const& other) const { return (base - other.base) / (std::ptrdiff_t)dimensions; }
};

static void write_result(std::FILE* out, std::vector<index_dense_t::vector_key_t> const& keys, std::vector<float> const& distances,
                         index_dense_t::clustering_result_t const& result) {
    std::vector<unsigned long long> wide(keys.begin(), keys.end());
    unsigned long long const tail[3] = {result.clusters, result.visited_members, result.computed_distances};
    std::fwrite(wide.data(), 8, wide.size(), out), std::fwrite(distances.data(), 4, distances.size(), out), std::fwrite(tail, 8, 3, out);
}

int main(int argc, char** argv) {
    std::printf("cluster through index_dense_t\n");
    if (argc < 9 || std::strcmp(argv[1], "run") != 0)
        return 0;
    std::size_t const count = std::strtoull(argv[4], nullptr, 10), dimensions = std::strtoull(argv[5], nullptr, 10);
    index_dense_clustering_config_t config;
    config.min_clusters = std::strtoull(argv[6], nullptr, 10), config.max_clusters = std::strtoull(argv[7], nullptr, 10);
    std::vector<i8_t> queries(count * dimensions);
    std::FILE* in = std::fopen(argv[3], "rb");
    EXPECT(in && std::fread(queries.data(), 1, queries.size(), in) == queries.size());
    std::fclose(in);

    index_dense_t index = index_dense_t::make(argv[2]);
    EXPECT(index);
    EXPECT(index.dimensions() == dimensions);
    std::vector<index_dense_t::vector_key_t> keys(count);
    std::vector<float> distances(count);
    std::FILE* out = std::fopen(argv[8], "wb");
    EXPECT(out);

    rows_t begin{queries.data(), dimensions}, end{queries.data() + count * dimensions, dimensions};
    auto by_vectors = index.cluster(begin, end, config, keys.data(), distances.data());
    EXPECT(by_vectors);
    write_result(out, keys, distances, by_vectors);

    std::vector<index_dense_t::vector_key_t> members(count);
    for (std::size_t i = 0; i != count; ++i)
        members[i] = 1000 + i;
    auto by_keys = index.cluster(members.data(), members.data() + count, config, keys.data(), distances.data(), executor_default_t(2));
    EXPECT(by_keys);
    write_result(out, keys, distances, by_keys);
    std::fclose(out);

    index_dense_clustering_config_t endless;
    endless.min_clusters = 3; // … and max_clusters == 0: refused by name instead of never returning
    auto refused = index.cluster(begin, end, endless, keys.data(), distances.data());
    EXPECT(!refused);
    std::printf("ok\n");
    return 0;
}
