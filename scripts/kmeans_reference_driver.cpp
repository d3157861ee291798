// scripts/kmeans_reference_driver.cpp — times the reference's `kmeans_clustering_t` (index_plugins.hpp:2199-2500) on host threads
// for scripts/kmeans_bench.py. Compiled OUTSIDE the repository against the reference's headers, the binary handed to the script:
//
//   clang++ -std=c++17 -O2 -march=x86-64-v3 -DUSEARCH_USE_SIMSIMD=0 -DUSEARCH_USE_FP16LIB=0 -I<reference>/include \
//           kmeans_reference_driver.cpp -pthread -o kmeans_reference
//
//   kmeans_reference X.f16 N dims k iterations threads   → one line: seconds of the call, iterations run, aggregate distance
//
// X.f16: N rows of `dims` IEEE half floats. l2sq, quantised to bf16 (the class's defaults), every early exit switched off.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <usearch/index_plugins.hpp>

using namespace unum::usearch;

int main(int argc, char** argv) {
    if (argc != 7)
        return std::fprintf(stderr, "usage: kmeans_reference X.f16 N dims k iterations threads\n"), 2;
    const std::size_t count = std::strtoull(argv[2], nullptr, 10), dimensions = std::strtoull(argv[3], nullptr, 10);
    const std::size_t clusters = std::strtoull(argv[4], nullptr, 10), threads = std::strtoull(argv[6], nullptr, 10);
    std::vector<std::uint16_t> points(count * dimensions), centroids(clusters * dimensions);
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in || std::fread(points.data(), 2, points.size(), in) != points.size())
        return std::fprintf(stderr, "cannot read %s\n", argv[1]), 1;
    std::fclose(in);
    kmeans_clustering_t engine(42);
    engine.max_iterations = std::strtoull(argv[5], nullptr, 10);
    engine.inertia_threshold = 0, engine.max_seconds = 0, engine.min_shifts = 0;
    std::vector<std::size_t> assignments(count);
    std::vector<distance_punned_t> distances(count);
    executor_default_t executor(threads);
    const auto begin = std::chrono::steady_clock::now();
    kmeans_clustering_result_t result = engine(
        reinterpret_cast<byte_t const*>(points.data()), count, dimensions * 2, reinterpret_cast<byte_t*>(centroids.data()), clusters,
        dimensions * 2, assignments.data(), distances.data(), scalar_kind_t::f16_k, dimensions, executor);
    const std::chrono::duration<double> seconds = std::chrono::steady_clock::now() - begin;
    if (!result)
        return std::fprintf(stderr, "refused: %s\n", result.error.release()), 1;
    std::printf("%.6f %zu %.9g\n", seconds.count(), result.iterations, result.aggregate_distance);
    return 0;
}
