// mixed_views_colour.hpp -- the copy-out pass of a views call with a COLOUR MATRIX per view: mixed_views.hpp's pass, and between
// the resampling and the constants every output pixel's three colours go through the view's own 3 x 4 matrix and a clamp to
// 0 .. 255 (xpnghip_decode_varsize_device_batch_views_colour).
//
// The rule.  vR, vG, vB are the fp32 values mixed_views.hpp's rule gives for the three colour bytes of an output pixel (its v,
// before the constants), m the view's matrix, row-major, row k the output colour k in the order R, G, B, columns R, G, B, 1:
//     t_k = fmaf(m[k][0], vR, fmaf(m[k][1], vG, fmaf(m[k][2], vB, m[k][3])))
//     t_k = t_k < 0.0f ? 0.0f : t_k > 255.0f ? 255.0f : t_k
//     y   = fmaf(t_k, scale[c], bias[c])      out = (T)y
// c is the position in the caller's buffer; with the BGR bit position c < 3 holds colour k = 2 - c.  Alpha - stored, or the 255 an
// RGB context lacks - does not pass through the matrix.  xpnghip_resample_colour_host (xpng_hip.hip) is the same arithmetic on
// the host, bit for bit, per view.
//
// What differs from mixed_views.hpp is the shape of the work: an output element needs all three source colours of its pixel, so
// the unit is the PIXEL.  The taps, the windows and the weights of a pixel are the same for its colour bytes and only the byte
// offset differs, so they are computed once and every source byte is read once per output pixel; the sums W are the same
// sequence of additions for every byte, so the values are bit for bit what a loop per byte gives.
#pragma once
#include <stdint.h>

#include "mixed_views.hpp"

namespace xpng {

// ---- views colour ----------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_colour_kernels_host.cpp compiles)
// a view's matrix as the table holds it: 48 bytes, beside the view's ViewRec and with its index
struct ViewColour {
    float m[12];
};
static_assert(sizeof(ViewColour) == 48, "xpng_hip.h states the size of a view's matrix");

// one colour through a row of the matrix and the clamp
__device__ __forceinline__ float colour_row(const float *m, float r, float g, float b) {
    const float t = fma_f32(m[0], r, fma_f32(m[1], g, fma_f32(m[2], b, m[3])));
    return t < 0.0f ? 0.0f : t > 255.0f ? 255.0f : t;
}

// grid (ceil(max oh / MC_ROWS), nviews), 256 threads; the template axes, the early return of a short view's blocks, the head, the
// aligned 16-byte stores and the tail are k_mixed_views_as_float's, and exactly C * oh * ow * sizeof(T) bytes of the view's buf are
// written.  Each of the block's four waves takes whole output ROWS in both layouts, so the y taps and the y window are
// wave-uniform, and the branch an axis takes depends on the view alone.  The view's matrix is 12 uniform loads per block.
//   interleaved  a 16-byte store covers the elements of two to four neighbouring pixels: each of them is resampled once, put
//                through the matrix, and the store's E elements are cut out of the pixels' values at the store's first channel rr
//                (uniform for C == 4, per lane for C == 3: a select between C candidates, never an indexed array).
//   planar       every pixel of the row is resampled once and its values go into EVERY plane.  When all planes' rows start at one
//                offset modulo 16 - oh * ow * sizeof(T) is a multiple of 16: oh * ow a multiple of 8 for the 2-byte types, of 4
//                for f32; 224 x 224 and 96 x 96 are, 14 x 14 and 37 x 5 are not - a lane resamples E neighbouring pixels and
//                writes them into the 16-byte store of every plane (the f16 store holds 8 pixels, 24 colour values).  Otherwise
//                no 16-byte store serves every plane from one lane's pixels: a lane takes one pixel at a time and stores its C
//                elements one by one, and a wave's stores are 64 neighbouring elements of each plane's row.
// Everything is unrolled over compile-time indices: no LDS and no scratch.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_views_colour(const ViewRec *__restrict__ vr, const ViewColour *__restrict__ vm, const uint8_t *__restrict__ stage,
                                                            uint64_t stage_bpr, uint32_t bgr, uint32_t filter, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T), E = 16 / ES;
    constexpr uint32_t NS = PX == 4 && C == 4 ? 4 : 3;  // source bytes of a pixel that are read: the colours, and a stored alpha that is asked for
    const ViewRec z = vr[blockIdx.y];
    const uint32_t OW = z.ow, OH = z.oh;
    const uint32_t oy0 = blockIdx.x * MC_ROWS;
    if (oy0 >= OH) return;
    float m[12];
#pragma unroll
    for (uint32_t i = 0; i < 12; i++) m[i] = vm[blockIdx.y].m[i];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = OH - oy0 < MC_ROWS ? OH - oy0 : MC_ROWS;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    const bool aax = filter && z.kx > 1.0f, aay = filter && z.ky > 1.0f;
    const uint8_t *rect0 = stage + z.stage + (uint64_t)z.ry * stage_bpr + (uint64_t)z.rx * PX;  // the rectangle's first pixel
    const bool same = !PLANAR || (((uint64_t)OH * OW * ES) & 15u) == 0;  // every plane's row oy starts at one offset modulo 16
    for (uint32_t it = wv; it < rows; it += 4) {
        const uint32_t oy = oy0 + it;
        const ResizeTap ty = resize_tap(oy, z.ky, z.rh);
        const ResampleWin wy = resample_win(oy, z.ky, z.rh);
        // output pixel ox of the row: o[c] is the value of channel position c of the caller's buffer before the constants
        auto pixel = [&](uint32_t ox, float (&o)[4]) {
            const uint32_t u = z.flip ? OW - 1 - ox : ox;
            const ResizeTap tx = resize_tap(u, z.kx, z.rw);
            const ResampleWin wx = resample_win(u, z.kx, z.rw);
            auto H = [&](uint32_t s, float (&h)[NS]) {  // the x-axis operation over source row s of the rectangle, every byte of the pixel
                const uint8_t *p = rect0 + (uint64_t)s * stage_bpr;
                if (!aax) {
#pragma unroll
                    for (uint32_t b = 0; b < NS; b++) {
                        const float q0 = (float)stage_ld8(p + tx.i0 * PX + b), q1 = (float)stage_ld8(p + tx.i1 * PX + b);
                        h[b] = fma_f32(tx.l, q1 - q0, q0);
                    }
                    return;
                }
                float W = 0.0f, A[NS] = {};
                for (uint32_t j = wx.j0; j <= wx.j1; j++) {
                    const float w = resample_weight(j, wx.f, z.ikx);
                    W = W + w;
#pragma unroll
                    for (uint32_t b = 0; b < NS; b++) A[b] = fma_f32(w, (float)stage_ld8(p + j * PX + b), A[b]);
                }
#pragma unroll
                for (uint32_t b = 0; b < NS; b++) h[b] = resample_div(A[b], W);
            };
            float v[NS];
            if (!aay) {
                float a[NS], b[NS];
                H(ty.i0, a); H(ty.i1, b);
#pragma unroll
                for (uint32_t i = 0; i < NS; i++) v[i] = fma_f32(ty.l, b[i] - a[i], a[i]);
            } else {
                float W = 0.0f, A[NS] = {};
                for (uint32_t s = wy.j0; s <= wy.j1; s++) {
                    const float w = resample_weight(s, wy.f, z.iky);
                    W = W + w;
                    float h[NS];
                    H(s, h);
#pragma unroll
                    for (uint32_t i = 0; i < NS; i++) A[i] = fma_f32(w, h[i], A[i]);
                }
#pragma unroll
                for (uint32_t i = 0; i < NS; i++) v[i] = resample_div(A[i], W);
            }
            const float tr = colour_row(m, v[0], v[1], v[2]), tg = colour_row(m + 4, v[0], v[1], v[2]), tb = colour_row(m + 8, v[0], v[1], v[2]);
            o[0] = bgr ? tb : tr; o[1] = tg; o[2] = bgr ? tr : tb;
            o[3] = NS == 4 ? v[NS - 1] : 255.0f;  // a stored alpha, or the alpha an RGB file does not store
        };
        if constexpr (PLANAR) {
            uint8_t *d = z.buf + (uint64_t)oy * row_el * ES;  // row oy of plane 0
            const uint64_t plane = (uint64_t)OH * OW * ES;
            auto single = [&](uint32_t j) {
                float o[4];
                pixel(j, o);
#pragma unroll
                for (uint32_t c = 0; c < (uint32_t)C; c++) store1<T>(d + c * plane, j, fma_f32(o[c], pick4(k.scale, c), pick4(k.bias, c)));
            };
            if (!same) {  // a pixel per lane: a wave's stores are 64 neighbouring elements of each plane's row
                for (uint32_t j = lane; j < row_el; j += 64) single(j);
                continue;
            }
            uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
            if (head > row_el) head = row_el;
            const uint32_t nq = (row_el - head) / E, tail0 = head + E * nq;
            if (lane < head) single(lane);
            if (tail0 + lane < row_el) single(tail0 + lane);
            uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned, in every plane
            for (uint32_t q = lane; q < nq; q += 64) {
                const uint32_t j = head + E * q;
                float o[8][4];
#pragma unroll
                for (uint32_t i = 0; i < E; i++) pixel(j + i, o[i]);
#pragma unroll
                for (uint32_t c = 0; c < (uint32_t)C; c++) {
                    float v[8] = {}, sa[4] = {}, ba[4] = {};
                    sa[0] = pick4(k.scale, c); ba[0] = pick4(k.bias, c);
#pragma unroll
                    for (uint32_t i = 0; i < E; i++) v[i] = o[i][c];
                    out_st128(d16 + c * plane + 16ull * q, float_chunk<T, 1>(v, sa, ba));
                }
            }
        } else {
            constexpr uint32_t NP = (C - 1 + E - 1) / C + 1;  // pixels a store can touch
            uint8_t *d = z.buf + (uint64_t)oy * row_el * ES;
            uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
            if (head > row_el) head = row_el;
            const uint32_t nq = (row_el - head) / E, tail0 = head + E * nq;
            auto single = [&](uint32_t j) {
                const uint32_t ox = j / C, c = j - ox * C;
                float o[4];
                pixel(ox, o);
                store1<T>(d, j, fma_f32(pick4(o, c), pick4(k.scale, c), pick4(k.bias, c)));
            };
            if (lane < head) single(lane);
            if (tail0 + lane < row_el) single(tail0 + lane);
            uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned
            for (uint32_t q = lane; q < nq; q += 64) {
                const uint32_t j = head + E * q, p = j / C, rr = j - p * C;  // the store starts at channel rr of pixel p
                float f[NP * C] = {}, sa[4] = {}, ba[4] = {};  // the pixels' values in the caller's order, pixel after pixel
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)C; i++) {
                    const uint32_t c = rr + i < (uint32_t)C ? rr + i : rr + i - C;
                    sa[i] = pick4(k.scale, c); ba[i] = pick4(k.bias, c);
                }
#pragma unroll
                for (uint32_t dq = 0; dq < NP; dq++) {
                    if (dq * C >= rr + E) continue;  // (the store ends in front of this pixel; it may lie behind the row)
                    float o[4];
                    pixel(p + dq, o);
#pragma unroll
                    for (uint32_t c = 0; c < (uint32_t)C; c++) f[dq * C + c] = o[c];
                }
                float v[8] = {};
#pragma unroll
                for (uint32_t i = 0; i < E; i++) {
                    if constexpr (C == 3) v[i] = rr == 0 ? f[i] : rr == 1 ? f[i + 1] : f[i + 2];
                    else v[i] = rr == 0 ? f[i] : rr == 1 ? f[i + 1] : rr == 2 ? f[i + 2] : f[i + 3];
                }
                out_st128(d16 + 16ull * q, float_chunk<T, C>(v, sa, ba));
            }
        }
    }
}

}  // namespace xpng
