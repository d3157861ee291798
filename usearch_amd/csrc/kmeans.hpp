/**
 *  usearch_amd/csrc/kmeans.hpp — k-means clustering on the device (kmeans.hip): the reference's `kmeans_clustering_gt`
 *  (/root/reference/include/usearch/index_plugins.hpp:2199-2500) with its observable behaviour, quirks included.
 */
#pragma once
#include <cstddef>
#include <cstdint>

#include "common.hpp"

namespace usearch_amd {

struct kmeans_config_t {
    metric_kind_t metric = metric_l2sq_k;          ///< index_plugins.hpp:2203
    scalar_kind_t quantization = scalar_bf16_k;    ///< 2204
    std::uint64_t max_iterations = 300;            ///< 2206
    double inertia_threshold = 1e-4;               ///< 2207
    double max_seconds = 60.0;                     ///< 2208
    double min_shifts = 0.01;                      ///< 2209
    std::uint64_t seed = 0;
    int device = 0;
};

struct kmeans_stats_t {
    std::uint64_t iterations = 0, last_iteration_points_shifted = 0, computed_distances = 0;
    double last_iteration_inertia = 0, aggregate_distance = 0, runtime_seconds = 0;
    float assign_ms = 0, update_ms = 0; ///< HIP-event time of the assignment / update kernels, summed over the iterations
};

/// The whole loop. `points`: host rows of `kind`, `stride` bytes apart. Writes `clusters` centroid rows of `kind`
/// (`centroids_stride` bytes apart), and per point its centroid and the distance to it. Returns an error message or null.
const char* kmeans_run(const std::uint8_t* points, std::size_t count, std::size_t stride, scalar_kind_t kind,
                       std::size_t dimensions, std::size_t clusters, const kmeans_config_t& config, std::uint8_t* centroids,
                       std::size_t centroids_stride, std::uint64_t* assignments, float* distances, kmeans_stats_t* stats);

/// The assignment step alone: the nearest of `clusters` centroid rows per point (lowest index among equals) after both were
/// cast from `kind` to `quantization` on the device.
const char* kmeans_assign(const std::uint8_t* points, std::size_t count, std::size_t stride, const std::uint8_t* centroids,
                          std::size_t clusters, std::size_t centroids_stride, scalar_kind_t kind, std::size_t dimensions,
                          metric_kind_t metric, scalar_kind_t quantization, int device, std::uint64_t* assignments,
                          float* distances);

/// The device cast alone (what the loop clusters): `count` rows of `kind` → rows of `quantization`, `out_stride` bytes apart.
const char* kmeans_quantize(const std::uint8_t* points, std::size_t count, std::size_t stride, scalar_kind_t kind,
                            std::size_t dimensions, scalar_kind_t quantization, int device, std::uint8_t* out,
                            std::size_t out_stride);

} // namespace usearch_amd
