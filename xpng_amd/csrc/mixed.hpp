// mixed.hpp -- mixed-size batches: what a batch of images of DIFFERENT sizes needs beside the ordinary codec kernels.
//
// A mixed context (xpnghip_ctx_create_mixed) concatenates the tile tables of its images into one table of M entries; a decode
// (xpnghip_decode_mixed_device_batch) runs the ordinary decode kernels once over all M tiles as an explicit work list
// (TileSel::list, common.hpp), and an encode (xpnghip_encode_varsize_device_batch) runs the ordinary encode kernels once over
// the table enumerated as ONE image of M tiles.  What "every image has N tiles" meant on the device is in four kernels:
//   k_dec_offsets_mixed  (m1_decode.hpp, beside k_dec_offsets) the serial size walk, one lane per image, over that image's own
//                        span of the table;
//   k_mixed_copy         (here) staging raster (one pitch for the launch) -> tight rasters, a destination pitch per image;
//   k_tile_offsets_seg   (tile_container.hpp, beside k_tile_offsets) the scan of the encoded tile sizes, segmented per image;
//   k_mixed_pack         (here) tight rasters, a source pitch per image -> staging raster: the mirror of k_mixed_copy.
#pragma once
#include <stdint.h>

#include "common.hpp"
#include "m1_decode.hpp"

namespace xpng {

// one image's way out of the staging raster: `rows` rows of `row_bytes` bytes from stage + src (the launch's pitch) to dst, rows
// back to back (the destination pitch IS row_bytes)
struct MixedCopy {
    uint64_t src;
    uint8_t *dst;
    uint32_t row_bytes, rows;
};

constexpr uint32_t MC_ROWS = 8;  // rows per workgroup of k_mixed_copy

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads.  A tight RGB row is w * 3 bytes, so the destination rows of one image
// start at every alignment: each row is written as a head of up to 3 bytes, whole ALIGNED dwords (each assembled from the source
// by ld32u: two aligned loads and a shift when the source sits at another alignment), and a tail of up to 3 bytes.  Exactly
// rows * row_bytes bytes of dst are written.  ld32u may read the aligned dword behind the last source byte: the staging raster
// keeps 256 spare bytes behind its last slot.
__global__ __launch_bounds__(256) void k_mixed_copy(const MixedCopy *__restrict__ mc, const uint8_t *__restrict__ stage, uint64_t stage_bpr) {
    const MixedCopy r = mc[blockIdx.y];
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= r.rows) return;
    for (uint32_t y = y0; y < y0 + MC_ROWS && y < r.rows; y++) {
        const uint8_t *s = stage + r.src + (uint64_t)y * stage_bpr;
        uint8_t *d = r.dst + (uint64_t)y * r.row_bytes;
        uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;
        if (head > r.row_bytes) head = r.row_bytes;
        const uint32_t nw = (r.row_bytes - head) / 4, tail0 = head + 4 * nw;
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        uint32_t *d4 = reinterpret_cast<uint32_t *>(d + head);
        for (uint32_t k = threadIdx.x; k < nw; k += 256) d4[k] = ld32u(s + head + 4 * k);
        if (tail0 + threadIdx.x < r.row_bytes) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
    }
}

// one image's way INTO the staging raster: `rows` rows of `row_bytes` bytes from src, rows back to back, to stage + dst at the
// launch's pitch
struct MixedPack {
    uint64_t dst;
    const uint8_t *src;
    uint32_t row_bytes, rows;
};

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads.  The mirror of k_mixed_copy: the rows of a tight raster start at every
// alignment (w * 3 bytes each) and the staging rows are 16-byte aligned, so each row is written as whole aligned dwords (each
// assembled by ld32u: its two aligned loads both hold a byte of the row, so nothing outside the dwords the source occupies is
// read) and a tail of up to 3 single bytes.  Exactly row_bytes bytes of each of the `rows` staging rows are written; the bytes of
// a staging row behind them keep whatever they held (no encode kernel lets them reach the output).
__global__ __launch_bounds__(256) void k_mixed_pack(const MixedPack *__restrict__ mp, uint8_t *__restrict__ stage, uint64_t stage_bpr) {
    const MixedPack r = mp[blockIdx.y];
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= r.rows) return;
    const uint32_t nw = r.row_bytes / 4, tail0 = 4 * nw;
    for (uint32_t y = y0; y < y0 + MC_ROWS && y < r.rows; y++) {
        const uint8_t *s = r.src + (uint64_t)y * r.row_bytes;
        uint8_t *d = stage + r.dst + (uint64_t)y * stage_bpr;
        uint32_t *d4 = reinterpret_cast<uint32_t *>(d);
        for (uint32_t k = threadIdx.x; k < nw; k += 256) d4[k] = ld32u(s + 4 * k);
        if (tail0 + threadIdx.x < r.row_bytes) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
    }
}

}  // namespace xpng
