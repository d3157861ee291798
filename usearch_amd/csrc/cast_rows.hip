/**
 *  usearch_amd/csrc/cast_rows.hip — a whole matrix cast on the device: f32, f16, bf16 or f64 rows → f8 (OCP e4m3fn) codes.
 *
 *  Users hold f32 embeddings, not codes, and `usearch_amd_cast` is one vector at a time on the host. The rules are casts.hpp's —
 *  the kernel calls the very functions the host cast does (nearest finite code, ties to the even code, ±448 beyond it, NaN → 0x7F
 *  with its sign, −0 kept, subnormal codes produced), so both give the same bytes for every input.
 *
 *  The work is cut into PIECES of 16 scalars of one row: a lane takes a piece, loads it with 16-byte loads (four for f32, two for
 *  the 16-bit kinds, eight for f64), converts the sixteen values in registers and packs the sixteen codes into ONE 16-byte store.
 *  A workgroup of 256 lanes takes 256 consecutive pieces — a block of 256 / ⌈ndim / 16⌉ rows — and the grid strides over the
 *  blocks. Two dense matrices (pitch = row bytes on both sides) are one long row to the kernel: pieces then run over the row ends
 *  and every one of them but the very last is whole and aligned, whatever `ndim` is (130-d f32 rows are 520 bytes: not a multiple
 *  of 16, yet piece g of the flat matrix begins at byte 64·g). A piece that is short (the end of a row) or whose source or target
 *  is not 16-byte aligned (a caller's pitch) goes scalar by scalar. The kernel is bound by its reads: 5 bytes move per f32 scalar.
 */
#include <hip/hip_runtime.h>

#include "casts.hpp"
#include "common.hpp"
#include "device_scratch.hpp"
#include "engine.hpp"
#include "host_util.hpp"

namespace usearch_amd {

namespace {

constexpr std::uint32_t piece_scalars_k = 16; ///< codes of one 16-byte store

/// Scalar `i` of a piece whose 16-byte words are `words` → the f8 code.
template <int from_ak> __device__ __forceinline__ std::uint8_t piece_code(const uint4* words, std::uint32_t i) {
    if constexpr (from_ak == scalar_f32_k) {
        const uint4 w = words[i / 4];
        const std::uint32_t bits = i % 4 == 0 ? w.x : i % 4 == 1 ? w.y : i % 4 == 2 ? w.z : w.w;
        return f32_to_f8_bits(__builtin_bit_cast(float, bits));
    } else if constexpr (from_ak == scalar_f64_k) {
        const uint4 w = words[i / 2];
        const std::uint64_t bits = i % 2 == 0 ? ((std::uint64_t)w.y << 32) | w.x : ((std::uint64_t)w.w << 32) | w.z;
        return f64_to_f8_bits(__builtin_bit_cast(double, bits));
    } else {
        const uint4 w = words[i / 8];
        const std::uint32_t pair = i % 8 / 2 == 0 ? w.x : i % 8 / 2 == 1 ? w.y : i % 8 / 2 == 2 ? w.z : w.w;
        const std::uint16_t bits = (std::uint16_t)(i % 2 ? pair >> 16 : pair);
        return f32_to_f8_bits(from_ak == scalar_bf16_k ? bf16_bits_to_f32(bits) : f16_bits_to_f32(bits));
    }
}

/// One scalar at `p` (aligned to its own size at most) → the f8 code.
template <int from_ak> __device__ __forceinline__ std::uint8_t scalar_code(const std::uint8_t* p) {
    constexpr std::uint32_t width = from_ak == scalar_f64_k ? 8 : from_ak == scalar_f32_k ? 4 : 2;
    std::uint64_t bits = 0;
#pragma unroll
    for (std::uint32_t b = 0; b < width; ++b)
        bits |= (std::uint64_t)p[b] << (8 * b);
    if constexpr (from_ak == scalar_f64_k)
        return f64_to_f8_bits(__builtin_bit_cast(double, bits));
    else if constexpr (from_ak == scalar_f32_k)
        return f32_to_f8_bits(__builtin_bit_cast(float, (std::uint32_t)bits));
    else
        return f32_to_f8_bits(from_ak == scalar_bf16_k ? bf16_bits_to_f32((std::uint16_t)bits) : f16_bits_to_f32((std::uint16_t)bits));
}

template <int from_ak>
__global__ __launch_bounds__(256) void cast_rows_to_f8_kernel(const std::uint8_t* input, std::uint64_t rows, std::uint64_t input_stride,
                                                              std::uint64_t dimensions, std::uint8_t* output,
                                                              std::uint64_t output_stride) {
    constexpr std::uint32_t width = from_ak == scalar_f64_k ? 8 : from_ak == scalar_f32_k ? 4 : 2;
    constexpr std::uint32_t words = piece_scalars_k * width / 16; // 16-byte loads of a piece
    const std::uint64_t pieces_per_row = (dimensions + piece_scalars_k - 1) / piece_scalars_k, pieces = rows * pieces_per_row;
    for (std::uint64_t piece = (std::uint64_t)blockIdx.x * 256 + threadIdx.x; piece < pieces; piece += (std::uint64_t)gridDim.x * 256) {
        const std::uint64_t row = piece / pieces_per_row, first = piece % pieces_per_row * piece_scalars_k;
        const std::uint8_t* source = input + row * input_stride + first * width;
        std::uint8_t* target = output + row * output_stride + first;
        const std::uint64_t left = dimensions - first;
        if (left >= piece_scalars_k && (std::uintptr_t)source % 16 == 0 && (std::uintptr_t)target % 16 == 0) {
            uint4 loaded[words];
#pragma unroll
            for (std::uint32_t w = 0; w < words; ++w)
                loaded[w] = reinterpret_cast<const uint4*>(source)[w];
            std::uint32_t packed[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (std::uint32_t i = 0; i < piece_scalars_k; ++i)
                packed[i / 4] |= (std::uint32_t)piece_code<from_ak>(loaded, i) << (8 * (i % 4));
            *reinterpret_cast<uint4*>(target) = uint4{packed[0], packed[1], packed[2], packed[3]};
        } else {
            const std::uint32_t here = left < piece_scalars_k ? (std::uint32_t)left : piece_scalars_k;
            for (std::uint32_t i = 0; i < here; ++i)
                target[i] = scalar_code<from_ak>(source + i * width);
        }
    }
}

template <int from_ak>
hipError_t launch_cast_rows_to_f8(const std::uint8_t* input, std::uint64_t rows, std::uint64_t input_stride, std::uint64_t dimensions,
                                  std::uint8_t* output, std::uint64_t output_stride, hipStream_t stream) {
    const std::uint64_t pieces = rows * ((dimensions + piece_scalars_k - 1) / piece_scalars_k);
    hipLaunchKernelGGL(cast_rows_to_f8_kernel<from_ak>, dim3((unsigned)std::min<std::uint64_t>((pieces + 255) / 256, 1u << 20)), dim3(256), 0,
                       stream, input, rows, input_stride, dimensions, output, output_stride);
    return hipGetLastError();
}

} // namespace

const char* cast_rows_device(scalar_kind_t from, scalar_kind_t to, const void* input, std::size_t count, std::size_t input_stride,
                             std::size_t dimensions, void* output, std::size_t output_stride, hipStream_t stream) {
    if (to != scalar_f8_k || (from != scalar_f32_k && from != scalar_f16_k && from != scalar_bf16_k && from != scalar_f64_k))
        return "No MI355X kernel for this cast: rows of f32, f16, bf16 or f64 to f8";
    const std::size_t row_bytes = bytes_per_vector(from, dimensions);
    if (input_stride < row_bytes || output_stride < dimensions)
        return "Stride is smaller than one vector";
    if (!count || !dimensions)
        return nullptr;
    std::uint64_t rows = count, scalars = dimensions;
    if (input_stride == row_bytes && output_stride == dimensions) // two dense matrices: one long row
        scalars = rows * scalars, rows = 1;
    const std::uint8_t* source = static_cast<const std::uint8_t*>(input);
    std::uint8_t* target = static_cast<std::uint8_t*>(output);
    hipError_t e = hipSuccess;
    switch (from) {
    case scalar_f32_k: e = launch_cast_rows_to_f8<scalar_f32_k>(source, rows, input_stride, scalars, target, output_stride, stream); break;
    case scalar_f16_k: e = launch_cast_rows_to_f8<scalar_f16_k>(source, rows, input_stride, scalars, target, output_stride, stream); break;
    case scalar_bf16_k: e = launch_cast_rows_to_f8<scalar_bf16_k>(source, rows, input_stride, scalars, target, output_stride, stream); break;
    default: e = launch_cast_rows_to_f8<scalar_f64_k>(source, rows, input_stride, scalars, target, output_stride, stream); break;
    }
    return e == hipSuccess ? nullptr : hip_message(e);
}

const char* cast_rows_host(scalar_kind_t from, scalar_kind_t to, const void* input, std::size_t count, std::size_t input_stride,
                           std::size_t dimensions, void* output, std::size_t output_stride) {
    if (to != scalar_f8_k || (from != scalar_f32_k && from != scalar_f16_k && from != scalar_bf16_k && from != scalar_f64_k))
        return "No MI355X kernel for this cast: rows of f32, f16, bf16 or f64 to f8";
    const std::size_t row_bytes = bytes_per_vector(from, dimensions);
    if (input_stride < row_bytes || output_stride < dimensions)
        return "Stride is smaller than one vector";
    if (!count || !dimensions)
        return nullptr;
    device_scratch_t scratch(current_device_k); // no snapshot here: the matrix goes to the caller's device
    std::uint8_t *d_input = nullptr, *d_output = nullptr;
    // the caller's matrix as it lies, pitch and all (one copy; the kernel takes any pitch), the codes dense
    const std::size_t input_bytes = (count - 1) * input_stride + row_bytes;
    UA_HIP(scratch.allocate(&d_input, input_bytes));
    UA_HIP(scratch.allocate(&d_output, count * dimensions));
    UA_HIP(hipMemcpy(d_input, input, input_bytes, hipMemcpyHostToDevice));
    if (const char* error = cast_rows_device(from, to, d_input, count, input_stride, dimensions, d_output, dimensions, nullptr))
        return error;
    UA_HIP(hipStreamSynchronize(nullptr));
    UA_HIP(hipMemcpy2D(output, output_stride, d_output, dimensions, dimensions, count, hipMemcpyDeviceToHost));
    return nullptr;
}

} // namespace usearch_amd
