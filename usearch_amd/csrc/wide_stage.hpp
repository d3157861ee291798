/**
 *  usearch_amd/csrc/wide_stage.hpp — how the 256 × 256 tile stages its operands, stated once for its two users: exact search
 *  (`exact_wide_kernel`, exact_tiled.hip) and the k-means assignment (`assign_wide_kernel`, kmeans.hip). A workgroup of 8 waves
 *  holds two buffers of [256 A rows + 256 B rows][128 bytes] in LDS, one being multiplied while the other is filled; both operands
 *  go global → LDS by LDS-DMA (`buffer_load_dwordx4 … lds`: no staging registers, no `ds_write`), and a row's eight 16-byte pieces
 *  are XOR-swizzled so that fragment reads meet no bank conflict. Everything else — what is multiplied with what, the pipeline
 *  around the fills, the epilogue — is the kernels' own.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"

namespace usearch_amd {

constexpr int wide_tile_k = 256;    ///< rows of either operand per tile
constexpr int wide_threads_k = 512; ///< 8 waves; wave w multiplies A rows [32w, 32w + 32) with the tile's 256 B rows
constexpr int wide_blocks_k = wide_tile_k / 32; ///< 32-row blocks of a tile = accumulators of a wave
constexpr int wide_buffers_k = 2;   ///< staging buffers: one being multiplied, one being filled
constexpr int wide_stage_rows_k = 2 * wide_tile_k;
constexpr std::uint32_t wide_stage_bytes_k = wide_stage_rows_k * chunk_bytes_k; ///< a buffer: [512][128] bytes, no padding
constexpr int wide_resource_flags_k = 0x00020000; ///< raw buffer, 32-bit data format: what the range check needs on gfx94x / gfx950

using global_bytes_t = const __attribute__((address_space(1))) void*;
using lds_bytes_t = __attribute__((address_space(3))) void*;

/// Where the 16-byte piece `piece` of staged row `row` sits inside the row's 128 bytes. A `ds_read_b128` is served in groups of 16
/// lanes — 16 different rows at one piece index — and rows 128 bytes apart fall on the same banks every second row; XOR-ing the
/// piece index with bits 1…3 of the row spreads each group over all sixteen 16-byte bank slots (no conflict). The DMA writes lanes
/// linearly, so the swizzle is applied to the SOURCE: lane i of a fill instruction fetches the piece that belongs in slot i.
__device__ __forceinline__ std::uint32_t wide_swizzle(std::uint32_t row, std::uint32_t piece) { return piece ^ ((row >> 1) & 7u); }

/// One fill step of a wave: 64 lanes × 16 bytes = 8 staged rows, written to the 1 024 consecutive LDS bytes at `stage_rows` (wave
/// w fills rows 64·pass + 8w … + 8 of an operand). `lane_offset` is the lane's share of the source address — its row inside the
/// 64-row pass times the row pitch, plus its swizzled piece — and never changes; pass and chunk travel in `scalar_offset`. A source
/// outside `resource` reads as zeros.
__device__ __forceinline__ void wide_fill(__amdgpu_buffer_rsrc_t resource, std::uint8_t* stage_rows, std::uint32_t lane_offset,
                                          std::uint32_t scalar_offset) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(resource, (lds_bytes_t)stage_rows, 16, (int)lane_offset, (int)scalar_offset, 0, 0);
}

} // namespace usearch_amd
