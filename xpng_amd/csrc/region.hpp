// region.hpp -- region decode: which tiles a crop rectangle touches, and the copy of the crop out of the staging raster.
//
// A region decode (xpnghip_decode_region_device_batch) runs the ordinary decode kernels over an explicit work list of tiles
// (TileSel::list, common.hpp) and points their reconstruction at a per-context staging raster: image i's tile-aligned bounding
// box of the selected tiles, at the batch's largest box pitch, behind a virtual base pointer (base - Y0 * bpr - X0 * pxsz, the
// form the multi-device shards use for their bands).  k_region_copy then moves each image's rectangle from staging into the
// caller's buffer at the caller's row pitch.
#pragma once
#include <stdint.h>

#include <vector>

#include "common.hpp"

namespace xpng {

// rect = {x, y, w, h}: non-empty and inside a W x H image (no overflow: x <= W and w <= W - x)
inline bool region_valid(uint64_t W, uint64_t H, const uint64_t *rect) {
    return rect[2] && rect[3] && rect[0] <= W && rect[2] <= W - rect[0] && rect[1] <= H && rect[3] <= H - rect[1];
}

// indices of the tiles that rect intersects, ascending (tiles of one image, row-major)
inline void region_select(const std::vector<TileDesc> &tiles, const uint64_t *rect, std::vector<uint32_t> &out) {
    out.clear();
    const uint64_t x0 = rect[0], y0 = rect[1], x1 = rect[0] + rect[2], y1 = rect[1] + rect[3];
    for (size_t i = 0; i < tiles.size(); i++) {
        const TileDesc &t = tiles[i];
        if (t.x < x1 && x0 < (uint64_t)t.x + t.w && t.y < y1 && y0 < (uint64_t)t.y + t.h) out.push_back((uint32_t)i);
    }
}

// one image's crop: `rows` rows of `row_bytes` bytes from stage + src (row pitch stage_bpr) to dst (row pitch out_bpr)
struct RegionCopy {
    uint64_t src;
    uint8_t *dst;
    uint32_t row_bytes, rows;
};

constexpr uint32_t RC_ROWS = 4;  // rows per workgroup of k_region_copy

// grid (ceil(max rows / RC_ROWS), nimg), 256 threads.  Consecutive threads move consecutive bytes (or dwords, when the image's
// source, destination, pitches and row length all allow them) of a row; nothing outside [0, row_bytes) of a destination row
// is touched, so pitch padding and whatever lies behind the last row stay as they were.
__global__ __launch_bounds__(256) void k_region_copy(const RegionCopy *__restrict__ rc, const uint8_t *__restrict__ stage,
                                                     uint64_t stage_bpr, uint64_t out_bpr) {
    const RegionCopy r = rc[blockIdx.y];
    const uint32_t y0 = blockIdx.x * RC_ROWS;
    const bool words = ((r.src | (uint64_t)(uintptr_t)r.dst | stage_bpr | out_bpr | r.row_bytes) & 3) == 0;
    for (uint32_t y = y0; y < y0 + RC_ROWS && y < r.rows; y++) {
        const uint8_t *s = stage + r.src + (uint64_t)y * stage_bpr;
        uint8_t *d = r.dst + (uint64_t)y * out_bpr;
        if (words) {
            const uint32_t *s4 = reinterpret_cast<const uint32_t *>(s);
            uint32_t *d4 = reinterpret_cast<uint32_t *>(d);
            for (uint32_t i = threadIdx.x; i < r.row_bytes / 4; i += 256) d4[i] = s4[i];
        } else {
            for (uint32_t i = threadIdx.x; i < r.row_bytes; i += 256) d[i] = s[i];
        }
    }
}

}  // namespace xpng
