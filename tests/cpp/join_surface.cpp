// tests/cpp/join_surface.cpp — the semantic join through the C++ class surface (include/usearch/index_dense.hpp), called the way the
// reference's cpp/bench.cpp:412-445 calls it: the free `join(men, women, index_join_config_t{executor.size()}, raw key arrays,
// executor, progress)`, then the member `men.join(women, config, unordered_map, unordered_map, executor)`.
// `join_surface link` proves that it compiles and links (no GPU); `join_surface run MEN WOMEN` builds two indexes, saves them to
// MEN and WOMEN, joins them both ways and prints the member call's pairs as "pair <man> <woman>" lines.
#include <cstdio>
#include <cstring>
#include <random>
#include <unordered_map>
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

static index_dense_t make_index(std::size_t count, std::size_t dims, unsigned seed) {
    metric_punned_t metric(dims, metric_kind_t::cos_k, scalar_kind_t::f32_k);
    index_dense_t index = index_dense_t::make(metric, index_dense_config_t(16, 128, 64));
    index.reserve(index_limits_t(count, 1));
    std::mt19937 generator(seed);
    std::normal_distribution<float> normal;
    std::vector<float> row(dims);
    for (std::size_t i = 0; i < count; ++i) {
        for (float& x : row)
            x = normal(generator);
        index.add(static_cast<default_key_t>(i), row.data());
    }
    return index;
}

int main(int argc, char** argv) {
    std::printf("join through index_dense_t\n");
    if (argc < 4 || std::strcmp(argv[1], "run") != 0)
        return 0;
    const std::size_t dims = 32, men_count = 1500, women_count = 1800;
    index_dense_t men = make_index(men_count, dims, 5);
    index_dense_t women = make_index(women_count, dims, 6);
    EXPECT(men && women && men.size() == men_count && women.size() == women_count);
    EXPECT(men.save(argv[2]) && women.save(argv[3]));

    // cpp/bench.cpp:418-437: raw key arrays, indexed by key, `missing_key` where nothing was matched
    const default_key_t missing_key = static_cast<default_key_t>(-1);
    std::vector<default_key_t> man_to_woman(women_count, missing_key), woman_to_man(women_count, missing_key);
    executor_default_t executor(4);
    std::size_t reported = 0;
    join_result_t result = join(men, women, index_join_config_t{executor.size()}, man_to_woman.data(), woman_to_man.data(), executor,
                                [&](std::size_t progress, std::size_t total) {
                                    reported = total;
                                    return progress <= total;
                                });
    EXPECT(result);
    EXPECT(result.intersection_size > men_count / 4 && result.intersection_size <= men_count && reported == result.intersection_size);

    // the member call with hash maps and the default P of the same executor
    std::unordered_map<default_key_t, default_key_t> m2w, w2m;
    index_join_config_t config;
    config.max_proposals = executor.size(); // as above: index_join_config_t{executor.size()}
    join_result_t again = men.join(women, config, m2w, w2m, executor);
    EXPECT(again && again.intersection_size == result.intersection_size && m2w.size() == again.intersection_size);
    // the free function hands its maps over crossed, as the reference's does (index_dense.hpp:2254-2270): `woman_to_man` got
    // man → woman and `man_to_woman` woman → man
    std::size_t agree = 0;
    for (auto const& pair : m2w) {
        EXPECT(w2m.at(pair.second) == pair.first);
        EXPECT(woman_to_man[pair.first] == pair.second && man_to_woman[pair.second] == pair.first);
        ++agree;
    }
    EXPECT(agree == result.intersection_size);
    // refused by name
    join_result_t self = men.join(men);
    EXPECT(!self && std::strstr(self.error.what(), "Can't join with itself"));
    for (auto const& pair : m2w)
        std::printf("pair %llu %llu\n", (unsigned long long)pair.first, (unsigned long long)pair.second);
    return 0;
}
