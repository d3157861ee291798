// scripts/compact_reference_driver.cpp — times the reference's `index_dense_gt::isolate()` (index_dense.hpp:1709-1720) on host
// threads for scripts/compact_bench.py. Compiled OUTSIDE the repository against the reference's headers, the binary handed to
// the script:
//
//   clang++ -std=c++17 -O2 -march=x86-64-v3 -DUSEARCH_USE_SIMSIMD=0 -DUSEARCH_USE_FP16LIB=0 -I<reference>/include \
//           compact_reference_driver.cpp -pthread -o compact_reference
//
//   compact_reference image.usearch threads   → one line: seconds of `isolate()`, members, the count it reports
//
// image.usearch: an index with removed members, as `BuiltIndex.save` writes it after `remove`.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include <usearch/index_dense.hpp>

using namespace unum::usearch;

int main(int argc, char** argv) {
    if (argc != 3)
        return std::fprintf(stderr, "usage: compact_reference image.usearch threads\n"), 2;
    const std::size_t threads = std::strtoull(argv[2], nullptr, 10);
    auto made = index_dense_t::make(argv[1]);
    if (!made)
        return std::fprintf(stderr, "cannot load %s: %s\n", argv[1], made.error.release()), 1;
    index_dense_t& index = made.index;
    executor_default_t executor(threads);
    const auto begin = std::chrono::steady_clock::now();
    auto result = index.isolate(executor);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
    if (!result)
        return std::fprintf(stderr, "isolate failed\n"), 1;
    std::printf("%.6f %zu %zu\n", seconds, index.size(), (std::size_t)result.pruned_edges);
    return 0;
}
