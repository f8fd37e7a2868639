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
// Two more kernels stand in for the last two when the caller's buffers have another LAYOUT than the file's interleaved R,G,B[,A]
// (xpnghip_decode_varsize_device_batch_as / xpnghip_encode_varsize_device_batch_from):
//   k_mixed_copy_as      (here) staging raster -> planar or interleaved, RGB or BGR, 3 or 4 channels;
//   k_mixed_pack_from    (here) planar or BGR rasters of the context's own channel count -> staging raster.
// All of them (and k_mixed_copy_as_float, mixed_float.hpp) read the same per-image record, MixedLayout: one table of B records per
// direction, whatever the form of the call ("The record table").
#pragma once
#include <stdint.h>

#include "common.hpp"
#include "m1_decode.hpp"

namespace xpng {

// one image of a mixed batch at the staging raster, either direction and every form: its slot of the staging raster (the launch's
// pitch), the caller's tight buffer at any alignment, and the image's size in pixels.  What a row of the buffer is - w * px bytes,
// w bytes of a plane, w * C elements - is the kernel's business, so the record depends on nothing but the buffers
struct MixedLayout {
    uint64_t stage;
    uint8_t *buf;
    uint32_t w, h;
};

constexpr uint32_t MC_ROWS = 8;  // rows per workgroup of every staging copy kernel (here and mixed_float.hpp)

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads.  A tight RGB row is w * 3 bytes, so the destination rows of one image
// start at every alignment: each row is written as a head of up to 3 bytes, whole ALIGNED dwords (each assembled from the source
// by ld32u: two aligned loads and a shift when the source sits at another alignment), and a tail of up to 3 bytes.  Exactly
// rows * row_bytes bytes of dst are written.  ld32u may read the aligned dword behind the last source byte: the staging raster
// keeps 256 spare bytes behind its last slot.  px = bytes per pixel of the context: a row is w * px bytes, and the destination
// pitch IS that.
__global__ __launch_bounds__(256) void k_mixed_copy(const MixedLayout *__restrict__ ml, const uint8_t *__restrict__ stage, uint64_t stage_bpr, uint32_t px) {
    const MixedLayout r = ml[blockIdx.y];
    const uint32_t row_bytes = r.w * px, rows = r.h;
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= rows) return;
    for (uint32_t y = y0; y < y0 + MC_ROWS && y < rows; y++) {
        const uint8_t *s = stage + r.stage + (uint64_t)y * stage_bpr;
        uint8_t *d = r.buf + (uint64_t)y * row_bytes;
        uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;
        if (head > row_bytes) head = row_bytes;
        const uint32_t nw = (row_bytes - head) / 4, tail0 = head + 4 * nw;
        if (threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
        uint32_t *d4 = reinterpret_cast<uint32_t *>(d + head);
        for (uint32_t k = threadIdx.x; k < nw; k += 256) d4[k] = ld32u(s + head + 4 * k);
        if (tail0 + threadIdx.x < row_bytes) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
    }
}

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads.  The mirror of k_mixed_copy: the rows of a tight raster start at every
// alignment (w * 3 bytes each) and the staging rows are 16-byte aligned, so each row is written as whole aligned dwords (each
// assembled by ld32u: its two aligned loads both hold a byte of the row, so nothing outside the dwords the source occupies is
// read) and a tail of up to 3 single bytes.  Exactly row_bytes bytes of each of the `rows` staging rows are written; the bytes of
// a staging row behind them keep whatever they held (no encode kernel lets them reach the output).  px as in k_mixed_copy.
__global__ __launch_bounds__(256) void k_mixed_pack(const MixedLayout *__restrict__ ml, uint8_t *__restrict__ stage, uint64_t stage_bpr, uint32_t px) {
    const MixedLayout r = ml[blockIdx.y];
    const uint32_t row_bytes = r.w * px, rows = r.h;
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= rows) return;
    const uint32_t nw = row_bytes / 4, tail0 = 4 * nw;
    for (uint32_t y = y0; y < y0 + MC_ROWS && y < rows; y++) {
        const uint8_t *s = r.buf + (uint64_t)y * row_bytes;
        uint8_t *d = stage + r.stage + (uint64_t)y * stage_bpr;
        uint32_t *d4 = reinterpret_cast<uint32_t *>(d);
        for (uint32_t k = threadIdx.x; k < nw; k += 256) d4[k] = ld32u(s + 4 * k);
        if (tail0 + threadIdx.x < row_bytes) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
    }
}

// ---- layouts (include/xpng_hip.h XPNGHIP_LAYOUT_*) ------------------------------------------------------------
// 16 bytes at a dword-aligned address (staging rows are 16-byte aligned, so every pixel group of a row starts on a dword)
struct __attribute__((aligned(4))) Dw4 {
    uint32_t x, y, z, w;
};

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads; PX = bytes per pixel of the staging raster (the context's), C = channels
// of the caller's buffer.  C == PX passes the channels through, C == 4 on PX == 3 adds alpha 255, C == 3 on PX == 4 drops alpha;
// bgr != 0 exchanges the first and the third colour (alpha stays last).  Each of the block's four waves takes whole rows
// (interleaved) or whole plane rows (planar), so everything a row depends on is wave-uniform:
//   planar       row y of plane c is w bytes at buf + c * w * h + y * w (64-bit offsets), at every alignment: a head of up to 3
//                bytes, whole ALIGNED dwords - each the channel's byte of four neighbouring pixels, gathered from one 16-byte load
//                of the staging row (RGB: the 12 bytes are first shifted into place with v_alignbyte, as ld32u does) by two or
//                three v_perm - and a tail of up to 3 bytes.  The alpha plane of an RGB context is filled with 255.
//   interleaved  row y is w * C bytes at buf + y * w * C: head, aligned dwords, tail as in k_mixed_copy; a dword takes its bytes
//                from two neighbouring pixels, each loaded as a dword (RGB: ld32u) and put into the caller's order by one v_perm,
//                and v_alignbyte cuts the dword out of the pair.
// Exactly C * w * h bytes of buf are written.  The loads may reach up to 7 bytes behind a staging row's last pixel: the pitch's
// padding, the next row, or the 256 spare bytes behind the last slot.
template <int PX, int C, bool PLANAR>
__global__ __launch_bounds__(256) void k_mixed_copy_as(const MixedLayout *__restrict__ ml, const uint8_t *__restrict__ stage, uint64_t stage_bpr, uint32_t bgr) {
    const MixedLayout r = ml[blockIdx.y];
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= r.h) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = r.h - y0 < MC_ROWS ? r.h - y0 : MC_ROWS;
    if constexpr (PLANAR) {
        const uint64_t plane = (uint64_t)r.w * r.h;
        for (uint32_t it = wv; it < rows * C; it += 4) {
            const uint32_t y = y0 + it / C, c = it % C;
            const uint8_t *s = stage + r.stage + (uint64_t)y * stage_bpr;
            uint8_t *d = r.buf + (uint64_t)c * plane + (uint64_t)y * r.w;
            uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;
            if (head > r.w) head = r.w;
            const uint32_t nw = (r.w - head) / 4, tail0 = head + 4 * nw;
            uint32_t *d4 = reinterpret_cast<uint32_t *>(d + head);
            if (PX == 3 && c == 3) {  // the alpha an RGB file does not store
                if (lane < head) d[lane] = 0xFF;
                for (uint32_t k = lane; k < nw; k += 64) d4[k] = 0xFFFFFFFFu;
                if (tail0 + lane < r.w) d[tail0 + lane] = 0xFF;
                continue;
            }
            const uint32_t sc = bgr && c < 3 ? 2 - c : c;  // the channel's byte inside a staging pixel
            if (lane < head) d[lane] = s[lane * PX + sc];
            if (tail0 + lane < r.w) d[tail0 + lane] = s[(tail0 + lane) * PX + sc];
            if constexpr (PX == 4) {
                const uint32_t sel = sc | ((4 + sc) << 8);  // byte sc of the low and of the high operand
                const uint8_t *g = s + 4 * head;
                for (uint32_t k = lane; k < nw; k += 64) {
                    const Dw4 v = *reinterpret_cast<const Dw4 *>(g + 16 * k);
                    const uint32_t lo = __builtin_amdgcn_perm(v.y, v.x, sel), hi = __builtin_amdgcn_perm(v.w, v.z, sel);
                    d4[k] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                }
            } else {
                // four pixels = bytes 0..11 of D0 D1 D2; the channel sits at sc, sc + 3, sc + 6, sc + 9.  12 bytes per group keep
                // the alignment of the first group for the whole row
                const uint8_t *g = s + 3 * head;
                const uint32_t sh = (uint32_t)((uintptr_t)g & 3);
                g -= sh;
                const uint32_t selA = sc == 0 ? 0x00060300u : sc == 1 ? 0x00070401u : 0x00000502u;  // of D1:D0 -> bytes 0, 1 (, 2)
                const uint32_t selB = sc == 0 ? 0x05020100u : sc == 1 ? 0x06020100u : 0x07040100u;  // of D2:that -> the dword
                for (uint32_t k = lane; k < nw; k += 64) {
                    const Dw4 v = *reinterpret_cast<const Dw4 *>(g + 12 * k);
                    const uint32_t D0 = __builtin_amdgcn_alignbyte(v.y, v.x, sh), D1 = __builtin_amdgcn_alignbyte(v.z, v.y, sh),
                                   D2 = __builtin_amdgcn_alignbyte(v.w, v.z, sh);
                    d4[k] = __builtin_amdgcn_perm(D2, __builtin_amdgcn_perm(D1, D0, selA), selB);
                }
            }
        }
    } else {
        // a staging pixel as the caller's pixel T: bytes 0..2 the colours in the caller's order, byte 3 the alpha of an RGBA
        // context, 255 (C == 4 on RGB: selector 0x0d) or 0 (C == 3: selector 0x0c)
        const uint32_t sel = (bgr ? 0x00000102u : 0x00020100u) | (C == 3 ? 0x0c000000u : PX == 4 ? 0x03000000u : 0x0d000000u);
        const uint32_t row_bytes = r.w * C;
        for (uint32_t it = wv; it < rows; it += 4) {
            const uint32_t y = y0 + it;
            const uint8_t *s = stage + r.stage + (uint64_t)y * stage_bpr;
            uint8_t *d = r.buf + (uint64_t)y * row_bytes;
            auto T = [&](uint32_t p) {
                const uint32_t P = PX == 4 ? reinterpret_cast<const uint32_t *>(s)[p] : ld32u(s + 3 * p);
                return __builtin_amdgcn_perm(0u, P, sel);
            };
            uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3)) & 3u;
            if (head > row_bytes) head = row_bytes;
            const uint32_t nw = (row_bytes - head) / 4, tail0 = head + 4 * nw;
            uint32_t *d4 = reinterpret_cast<uint32_t *>(d + head);
            if (lane < head) d[lane] = (uint8_t)(T(lane / C) >> (8 * (lane % C)));
            if (tail0 + lane < row_bytes) d[tail0 + lane] = (uint8_t)(T((tail0 + lane) / C) >> (8 * ((tail0 + lane) % C)));
            for (uint32_t k = lane; k < nw; k += 64) {
                const uint32_t j = head + 4 * k, p = j / C, rr = j - p * C;  // the dword starts at byte rr of pixel p
                const uint32_t t0 = T(p), t1 = T(p + 1);
                if constexpr (C == 4) d4[k] = __builtin_amdgcn_alignbyte(t1, t0, rr);
                else d4[k] = __builtin_amdgcn_alignbyte(t1 >> 8, t0 | (t1 << 24), rr);
            }
        }
    }
}

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads; PX = bytes per pixel of the context = channels of the caller's buffer.
// The mirror of k_mixed_copy_as: the staging rows are 16-byte aligned, so each wave writes its rows as whole groups of four pixels
// (12 or 16 bytes at a dword-aligned offset) and a tail of up to 3 pixels written byte by byte.
//   planar       a group is one ld32u per plane (the channel's byte of four pixels) and a 4 x PX byte transpose by v_perm; bgr != 0
//                reads the first colour from the third plane and the third from the first.
//   interleaved  a group is PX ld32u of the caller's row and v_perm by selectors that either exchange the first and third colour
//                of every pixel (bgr != 0) or pass the bytes through.
// READS: every ld32u covers four bytes of the image itself, so its two aligned loads both hold a byte of the caller's C * w * h
// bytes: nothing outside the aligned dwords that buffer occupies is read, and every other access is a single byte of it.
// Exactly w * PX bytes of each of the h staging rows are written; the bytes of a staging row behind them keep whatever they held.
template <int PX, bool PLANAR>
__global__ __launch_bounds__(256) void k_mixed_pack_from(const MixedLayout *__restrict__ ml, uint8_t *__restrict__ stage, uint64_t stage_bpr, uint32_t bgr) {
    const MixedLayout r = ml[blockIdx.y];
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= r.h) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = r.h - y0 < MC_ROWS ? r.h - y0 : MC_ROWS;
    const uint32_t ng = r.w / 4, tail0 = 4 * ng, tail_bytes = (r.w - tail0) * PX;
    const uint64_t plane = (uint64_t)r.w * r.h;
    for (uint32_t it = wv; it < rows; it += 4) {
        const uint32_t y = y0 + it;
        uint8_t *d = stage + r.stage + (uint64_t)y * stage_bpr;
        if constexpr (PLANAR) {
            const uint8_t *row = r.buf + (uint64_t)y * r.w;  // of plane 0
            const uint8_t *p0 = row + (bgr ? 2 * plane : 0), *p1 = row + plane, *p2 = row + (bgr ? 0 : 2 * plane);
            for (uint32_t g = lane; g < ng; g += 64) {
                const uint32_t R = ld32u(p0 + 4 * g), G = ld32u(p1 + 4 * g), B = ld32u(p2 + 4 * g);
                if constexpr (PX == 4) {
                    const uint32_t A = ld32u(row + 3 * plane + 4 * g);
                    const uint32_t t01lo = __builtin_amdgcn_perm(G, R, 0x05010400u), t01hi = __builtin_amdgcn_perm(G, R, 0x07030602u);  // R0 G0 R1 G1, R2 G2 R3 G3
                    const uint32_t t23lo = __builtin_amdgcn_perm(A, B, 0x05010400u), t23hi = __builtin_amdgcn_perm(A, B, 0x07030602u);
                    uint4 o;
                    o.x = __builtin_amdgcn_perm(t23lo, t01lo, 0x05040100u);
                    o.y = __builtin_amdgcn_perm(t23lo, t01lo, 0x07060302u);
                    o.z = __builtin_amdgcn_perm(t23hi, t01hi, 0x05040100u);
                    o.w = __builtin_amdgcn_perm(t23hi, t01hi, 0x07060302u);
                    reinterpret_cast<uint4 *>(d)[g] = o;
                } else {
                    uint32_t *o = reinterpret_cast<uint32_t *>(d) + 3 * g;
                    o[0] = __builtin_amdgcn_perm(B, __builtin_amdgcn_perm(G, R, 0x01000400u), 0x03040100u);  // R0 G0 B0 R1
                    o[1] = __builtin_amdgcn_perm(B, __builtin_amdgcn_perm(G, R, 0x06020005u), 0x03020500u);  // G1 B1 R2 G2
                    o[2] = __builtin_amdgcn_perm(B, __builtin_amdgcn_perm(G, R, 0x00070300u), 0x07020106u);  // B2 R3 G3 B3
                }
            }
            if (lane < tail_bytes) {
                const uint32_t p = tail0 + lane / PX, c = lane % PX;
                d[p * PX + c] = row[(uint64_t)(bgr && c < 3 ? 2 - c : c) * plane + p];
            }
        } else {
            const uint8_t *s = r.buf + (uint64_t)y * r.w * PX;
            if constexpr (PX == 4) {
                const uint32_t sel = bgr ? 0x03000102u : 0x03020100u;
                for (uint32_t g = lane; g < ng; g += 64) {
                    uint4 o;
                    o.x = __builtin_amdgcn_perm(0u, ld32u(s + 16 * g), sel);
                    o.y = __builtin_amdgcn_perm(0u, ld32u(s + 16 * g + 4), sel);
                    o.z = __builtin_amdgcn_perm(0u, ld32u(s + 16 * g + 8), sel);
                    o.w = __builtin_amdgcn_perm(0u, ld32u(s + 16 * g + 12), sel);
                    reinterpret_cast<uint4 *>(d)[g] = o;
                }
            } else {
                // source bytes 0..11 of D0 D1 D2 -> B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3 (bgr), or themselves
                const uint32_t s0 = bgr ? 0x05000102u : 0x03020100u, s1a = bgr ? 0x07000304u : 0x07060504u, s1b = bgr ? 0x03040100u : 0x03020100u,
                               s2 = bgr ? 0x05060702u : 0x07060504u;
                for (uint32_t g = lane; g < ng; g += 64) {
                    const uint32_t D0 = ld32u(s + 12 * g), D1 = ld32u(s + 12 * g + 4), D2 = ld32u(s + 12 * g + 8);
                    uint32_t *o = reinterpret_cast<uint32_t *>(d) + 3 * g;
                    o[0] = __builtin_amdgcn_perm(D1, D0, s0);
                    o[1] = __builtin_amdgcn_perm(D2, __builtin_amdgcn_perm(D1, D0, s1a), s1b);
                    o[2] = __builtin_amdgcn_perm(D2, D1, s2);
                }
            }
            if (lane < tail_bytes) {
                const uint32_t p = tail0 + lane / PX, c = lane % PX;
                d[p * PX + c] = s[p * PX + (bgr && c < 3 ? 2 - c : c)];
            }
        }
    }
}

}  // namespace xpng
