/**
 *  usearch_amd/csrc/sketch.hip — builds the low-rank sketch of a snapshot (sketch.hpp): the directions on the host, once per
 *  snapshot, and one 128-byte record per member in one pass over the matrix of stored rows.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>

#include "engine.hpp"
#include "host_util.hpp"
#include "sketch.hpp"

namespace usearch_amd {

/**
 *  Records of rows [first, size): a tile of 256 rows × 64 directions per workgroup of 256 threads, 16 dimensions per step through
 *  LDS, every thread 8 rows × 8 directions in f64 (sketch.hpp: the sums behind ρ must not lose what f32 chains of 768 terms lose).
 *  Thread t stages row t of the tile and keeps that row's Σb²; threads 8g … 8g + 7 finish rows 8g … 8g + 7, 16 bytes of a record each.
 */
template <int scalar_ak>
__global__ __launch_bounds__(256) void sketch_records_kernel(const std::uint8_t* vectors, std::uint32_t row_stride, std::uint32_t dimensions,
                                                             std::uint64_t first, std::uint64_t size, const float* directions,
                                                             double gram_defect, std::uint8_t* records) {
    constexpr scalar_kind_t scalar = (scalar_kind_t)scalar_ak;
    __shared__ float rows_lds[16][256];
    __shared__ __attribute__((aligned(16))) float directions_lds[16][sketch_columns_k];
    __shared__ double norms_lds[256];
    const std::uint32_t t = threadIdx.x, tx = t & 7u, ty = t >> 3;
    const std::uint64_t tile = first + (std::uint64_t)blockIdx.x * 256;
    const std::uint64_t my_row = tile + t;
    const std::uint8_t* row = my_row < size ? vectors + my_row * row_stride : nullptr;
    double acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int d = 0; d < 8; ++d)
            acc[r][d] = 0.0;
    double n2 = 0.0;
    for (std::uint32_t k0 = 0; k0 < dimensions; k0 += 16) {
#pragma unroll
        for (std::uint32_t kk = 0; kk < 16; ++kk) {
            const std::uint32_t i = k0 + kk;
            const float b = row && i < dimensions ? sketch_scalar(row, i, scalar) : 0.f;
            rows_lds[kk][t] = b;
            n2 = fma((double)b, (double)b, n2);
        }
        {
            const std::uint32_t kk = t >> 4, column = (t & 15u) * 4;
            float4 d = {0.f, 0.f, 0.f, 0.f};
            if (k0 + kk < dimensions)
                d = *reinterpret_cast<const float4*>(directions + (std::size_t)(k0 + kk) * sketch_columns_k + column);
            *reinterpret_cast<float4*>(&directions_lds[kk][column]) = d;
        }
        __syncthreads();
#pragma unroll 4
        for (std::uint32_t kk = 0; kk < 16; ++kk) {
            double b[8], d[8];
#pragma unroll
            for (int r = 0; r < 8; ++r)
                b[r] = (double)rows_lds[kk][ty * 8 + r];
#pragma unroll
            for (int e = 0; e < 8; ++e)
                d[e] = (double)directions_lds[kk][tx * 8 + e];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    acc[r][e] = fma(b[r], d[e], acc[r][e]);
        }
        __syncthreads();
    }
    norms_lds[t] = n2;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const std::uint64_t out_row = tile + ty * 8 + r;
        const double row_n2 = norms_lds[ty * 8 + r];
        bool never = !sketch_norm_in_range(row_n2);
        const double inverse = never ? 0.0 : 1.0 / sqrt(row_n2);
        _Float16 halves[8];
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double c = acc[r][e] * inverse;
            halves[e] = (_Float16)c;
            const double stored = (double)halves[e];
            never |= !(fabs(stored) < INFINITY);
            s1 = fma(c, stored, s1), s2 = fma(stored, stored, s2);
        }
        // the eight threads of a row are neighbouring lanes of one wave
#pragma unroll
        for (int offset = 1; offset < 8; offset <<= 1) {
            s1 += __shfl_xor(s1, offset, 64);
            s2 += __shfl_xor(s2, offset, 64);
            never |= __shfl_xor((int)never, offset, 64) != 0;
        }
        float residual = sketch_residual(s1, s2, gram_defect);
        if (never || !(residual < INFINITY)) {
            residual = INFINITY;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                halves[e] = (_Float16)0.f;
        }
        uint4 out;
        memcpy(&out, halves, 16);
        if (tx == 7)
            out.w = __builtin_bit_cast(std::uint32_t, residual);
        if (out_row < size)
            *reinterpret_cast<uint4*>(records + out_row * sketch_record_bytes_k + tx * 16) = out;
    }
}

/// Records of rows [first, size) of `vectors` into `records` ([size][128], rows below `first` are left alone), on `stream`: the one place
/// that launches `sketch_records_kernel` (`make_sketch`, and the test hooks on a caller's rows). The launch's error is the caller's to read.
void launch_sketch_records(const std::uint8_t* vectors, std::uint32_t row_stride, std::uint32_t dimensions, scalar_kind_t scalar,
                           std::uint64_t first, std::uint64_t size, const float* directions, double gram_defect, std::uint8_t* records,
                           hipStream_t stream) {
    if (first >= size)
        return;
    const std::uint64_t blocks = (size - first + 255) / 256;
    if (scalar == scalar_f32_k)
        hipLaunchKernelGGL(sketch_records_kernel<scalar_f32_k>, dim3((unsigned)blocks), dim3(256), 0, stream, vectors, row_stride, dimensions,
                           first, size, directions, gram_defect, records);
    else if (scalar == scalar_f16_k)
        hipLaunchKernelGGL(sketch_records_kernel<scalar_f16_k>, dim3((unsigned)blocks), dim3(256), 0, stream, vectors, row_stride, dimensions,
                           first, size, directions, gram_defect, records);
    else
        hipLaunchKernelGGL(sketch_records_kernel<scalar_bf16_k>, dim3((unsigned)blocks), dim3(256), 0, stream, vectors, row_stride, dimensions,
                           first, size, directions, gram_defect, records);
}

void snapshot_t::drop_sketch() {
    view_.sketch = nullptr;
    view_.sketch_directions = nullptr;
    for (void** p : {&d_sketch_, &d_sketch_directions_}) {
        if (*p)
            placed_free(*p);
        *p = nullptr;
    }
    device_bytes_ -= std::min<std::size_t>(device_bytes_, (std::size_t)sketch_capacity_ * sketch_record_bytes_k);
    sketch_rows_ = sketch_capacity_ = 0;
    sketch_stale_ = false;
    sketch_judged_ = false;
}

const char* snapshot_t::finalize_sketch() {
    // a snapshot that cannot have its sketch (no memory for the records, a failed copy) walks without one, as it always could
    if (make_sketch() != nullptr) {
        (void)hipGetLastError();
        drop_sketch();
    }
    return nullptr;
}

const char* snapshot_t::make_sketch() {
    const bool wanted = view_.size && sketch_eligible(metric_, scalar_, view_.bytes_per_vector) && !sketch_refused_;
    if (!wanted || sketch_stale_ || sketch_rows_ > view_.size)
        drop_sketch(); // an overwritten row, a shrunken index: records and directions are made anew
    if (!wanted)
        return nullptr;
    UA_HIP(hipSetDevice(device_));
    const std::uint32_t dimensions = view_.dimensions, row_stride = view_.row_stride;
    if (!d_sketch_directions_) {
        // the directions: up to 62 stored rows at seeded slots, orthonormalised on the host in f64
        const std::uint32_t samples = (std::uint32_t)std::min<std::uint64_t>(sketch_rank_k, view_.size);
        std::vector<std::uint8_t> row(row_stride);
        std::vector<double> wide((std::size_t)samples * dimensions);
        for (std::uint32_t s = 0; s < samples; ++s) {
            const std::uint64_t slot = sketch_sample_slot(s, view_.size);
            UA_HIP(hipMemcpy(row.data(), static_cast<const std::uint8_t*>(d_vectors_) + slot * row_stride, row_stride, hipMemcpyDeviceToHost));
            for (std::uint32_t i = 0; i < dimensions; ++i)
                wide[(std::size_t)s * dimensions + i] = (double)sketch_scalar(row.data(), i, scalar_);
        }
        const sketch_directions_t directions = sketch_orthonormalise(wide, samples, dimensions);
        sketch_gram_defect_ = directions.gram_defect;
        UA_HIP(hipMalloc(&d_sketch_directions_, directions.transposed.size() * sizeof(float)));
        UA_HIP(hipMemcpy(d_sketch_directions_, directions.transposed.data(), directions.transposed.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (sketch_capacity_ < view_.size) { // members were appended: room for their records, the old ones move over
        void* fresh = nullptr;
        // as much room as the build arrays have (they double: `grow_for_build`), so that a run of small additions moves the records as
        // rarely as it moves the rows; a loaded index has no spare room and gets the exact size.
        // a plain block: 1.28 GB at the headline, and nothing the settle window of the matrix (placement.hpp) should wait for
        const std::uint64_t capacity = std::max<std::uint64_t>(view_.size, build_capacity_);
        UA_HIP(block_malloc(&fresh, (std::size_t)capacity * sketch_record_bytes_k));
        if (d_sketch_) {
            UA_HIP(hipMemcpy(fresh, d_sketch_, (std::size_t)sketch_rows_ * sketch_record_bytes_k, hipMemcpyDeviceToDevice));
            placed_free(d_sketch_);
        }
        device_bytes_ += (std::size_t)(capacity - sketch_capacity_) * sketch_record_bytes_k;
        d_sketch_ = fresh;
        sketch_capacity_ = capacity;
    }
    if (sketch_rows_ < view_.size) {
        launch_sketch_records(static_cast<const std::uint8_t*>(d_vectors_), row_stride, dimensions, scalar_, sketch_rows_, view_.size,
                              static_cast<const float*>(d_sketch_directions_), sketch_gram_defect_, static_cast<std::uint8_t*>(d_sketch_), stream_);
        UA_HIP(hipGetLastError());
        UA_HIP(hipStreamSynchronize(stream_));
        sketch_rows_ = view_.size;
    }
    view_.sketch = static_cast<const std::uint8_t*>(d_sketch_);
    view_.sketch_directions = static_cast<const float*>(d_sketch_directions_);
    return nullptr;
}

void snapshot_t::judge_sketch(std::uint64_t tested, std::uint64_t pruned) {
    // Auto mode: a sketch that prunes less than a quarter of what it tests costs more than it saves — the bytes break even at
    // 128 / 1536 = 0.083 for the headline's rows, and every hop pays one more dependent round trip
    // The verdict is passed once per sketch, by the first such call that has the snapshot to itself — the gate of
    // `try_matrix_placement`: this call's workspace is the only one out and `take` admits nobody until the records are gone, so no
    // other batch holds, or can pick up, a view with the pointer in it. A call that finds company leaves the verdict to a later one.
    {
        std::lock_guard<std::mutex> lock(pool_mutex_);
        if (!view_.sketch || sketch_judged_ || placing_ || workspaces_.size() - idle_.size() != 1)
            return;
        sketch_judged_ = true;
        if (tested == 0 || pruned * 4 >= tested)
            return;
        placing_ = true;
    }
    // readers without a workspace lease (exact search on a caller's stream) never touch the records, but this call's own launches
    // did: nothing of this device may be running when their memory goes back
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    drop_sketch();
    {
        std::lock_guard<std::mutex> lock(pool_mutex_);
        sketch_refused_ = true;
        placing_ = false;
    }
    pool_ready_.notify_all();
}

} // namespace usearch_amd
