// tests/golden/kmeans/make_kmeans_golden.cpp — one-off driver that recorded tests/golden/kmeans/*.npz: runs the reference's
// `kmeans_clustering_t` (index_plugins.hpp:2199-2500) on one thread (its default `dummy_executor_t`) over an f32 matrix and dumps
// what it returns. make_kmeans_golden.py next to it feeds it and packs the fixtures. Not built by the project, not run by a test.
//
//   clang++ -std=c++17 -O2 -march=x86-64-v3 -ffp-contract=off -mllvm -force-vector-width=1 -mllvm -force-vector-interleave=1 \
//           -DUSEARCH_USE_SIMSIMD=0 -DUSEARCH_USE_FP16LIB=0 -DUSEARCH_USE_OPENMP=0 -I<reference>/include make_kmeans_golden.cpp \
//           -o make_kmeans_golden
//
// The float flags pin the sums the source spells out, which is what the Python model (and the oracle's serial loops) restate:
// no fused multiply-add, and no vector lanes — the metric loops carry `#pragma clang loop vectorize(enable)`, under which clang
// deals a float sum over lanes and the last bits then depend on the compiler's choice of width.
//
//   make_kmeans_golden X.bin N dims k metric(l2sq|cos|ip) kind(bf16|f16|i8|f32) max_iterations inertia_threshold max_seconds min_shifts seed out.bin
//
// out.bin: u64 assignments[N], f32 distances[N], f32 centroids[k][dims], u64 iterations, u64 last_iteration_points_shifted,
//          u64 computed_distances, f64 last_iteration_inertia, f64 aggregate_distance
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <usearch/index_plugins.hpp>

using namespace unum::usearch;

int main(int argc, char** argv) {
    if (argc != 13)
        return std::fprintf(stderr, "usage: see the header of make_kmeans_golden.cpp\n"), 2;
    const std::size_t count = std::strtoull(argv[2], nullptr, 10), dimensions = std::strtoull(argv[3], nullptr, 10);
    const std::size_t clusters = std::strtoull(argv[4], nullptr, 10);
    const std::string metric = argv[5], kind = argv[6];
    std::vector<float> points(count * dimensions), centroids(clusters * dimensions);
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in || std::fread(points.data(), 4, points.size(), in) != points.size())
        return std::fprintf(stderr, "cannot read %s\n", argv[1]), 1;
    std::fclose(in);

    kmeans_clustering_t engine(std::strtoull(argv[11], nullptr, 10));
    engine.metric_kind = metric == "cos" ? metric_kind_t::cos_k : metric == "ip" ? metric_kind_t::ip_k : metric_kind_t::l2sq_k;
    engine.quantization_kind = kind == "bf16" ? scalar_kind_t::bf16_k
                               : kind == "f16" ? scalar_kind_t::f16_k
                               : kind == "i8"  ? scalar_kind_t::i8_k
                                               : scalar_kind_t::f32_k;
    engine.max_iterations = std::strtoull(argv[7], nullptr, 10);
    engine.inertia_threshold = std::strtod(argv[8], nullptr);
    engine.max_seconds = std::strtod(argv[9], nullptr);
    engine.min_shifts = std::strtod(argv[10], nullptr);

    std::vector<std::size_t> assignments(count);
    std::vector<distance_punned_t> distances(count);
    kmeans_clustering_result_t result = engine(
        reinterpret_cast<byte_t const*>(points.data()), count, dimensions * sizeof(float), reinterpret_cast<byte_t*>(centroids.data()),
        clusters, dimensions * sizeof(float), assignments.data(), distances.data(), scalar_kind_t::f32_k, dimensions);
    if (!result)
        return std::fprintf(stderr, "refused: %s\n", result.error.release()), 1;

    std::FILE* out = std::fopen(argv[12], "wb");
    if (!out)
        return 1;
    static_assert(sizeof(std::size_t) == 8 && sizeof(distance_punned_t) == 4, "the layout of out.bin");
    std::fwrite(assignments.data(), 8, count, out);
    std::fwrite(distances.data(), 4, count, out);
    std::fwrite(centroids.data(), 4, centroids.size(), out);
    const unsigned long long integers[3] = {result.iterations, result.last_iteration_points_shifted, result.computed_distances};
    const double reals[2] = {result.last_iteration_inertia, result.aggregate_distance};
    std::fwrite(integers, 8, 3, out);
    std::fwrite(reals, 8, 2, out);
    std::fclose(out);
    std::printf("iterations=%llu shifted=%llu inertia=%.17g aggregate=%.17g\n", integers[0], integers[1], reals[0], reals[1]);
    return 0;
}
