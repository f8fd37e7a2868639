// mixed_views_pixel.hpp -- what the PIXEL-unit kernels of the views calls share: the end of a pixel's value and the stores of an
// output row.  k_mixed_views_colour, k_mixed_views_cubic and k_mixed_views_affine resample a pixel's source bytes once into v[NS]
// and hand a callable pixel(ox, o[4]) to a row writer; k_mixed_views_blur stores the pixels it kept in registers.  A kernel of this
// family supplies how its record is read, its row loop and the pixel callable up to v[NS]; everything behind v is here, once.
// (The element-unit kernel k_mixed_views_as_float has another unit of work and keeps its own stores: mixed_views.hpp.)
//
// The end of a pixel.  v[0 .. 2] are the fp32 values of the file's R, G, B, v[3] a stored alpha that is asked for.  Where the call
// has matrices, t_k = clamp(fmaf(m[k][0], vR, fmaf(m[k][1], vG, fmaf(m[k][2], vB, m[k][3]))), 0, 255) for the three rows k of the
// view's matrix, else t = v; o[c] is the value of channel position c of the caller's buffer: with the BGR bit position c < 3 holds
// colour 2 - c, and o[3] is the stored alpha or the 255 an RGB context lacks (it does not pass through the matrix).  The element
// is fmaf(o[c], scale[c], bias[c]) narrowed to T.
//
// The stores of a row.  Exactly C * ow elements of T are written per output row, and the bytes do not depend on the form:
//   narrow       a lane takes one pixel at a time and stores its C elements one by one: a wave's stores are neighbouring
//                elements of each plane's row, or C times as many neighbouring elements of the interleaved row.  The form of a
//                kernel whose pixel costs hundreds of taps (cubic), beside which the stores are nothing, and no pixel is
//                resampled twice.
//   wide         a head of single elements up to the first 16-byte boundary, aligned 16-byte stores, a tail of single elements
//                (k_mixed_views_as_float's scheme).
//     interleaved  a 16-byte store covers the elements of two to four neighbouring pixels: each of them is resampled once, put
//                  through the end of a pixel, and the store's E elements are cut out of the pixels' values at the store's first
//                  channel rr (uniform for C == 4, per lane for C == 3: a select between C candidates, never an indexed array).
//     planar       every pixel of the row is resampled once and its values go into EVERY plane.  When all planes' rows start at
//                  one offset modulo 16 - oh * ow * sizeof(T) is a multiple of 16: oh * ow a multiple of 8 for the 2-byte types,
//                  of 4 for f32; 224 x 224 and 96 x 96 are, 14 x 14 and 37 x 5 are not - a lane resamples E neighbouring pixels
//                  and writes them into the 16-byte store of every plane (the f16 store holds 8 pixels, 24 colour values).
//                  Otherwise no 16-byte store serves every plane from one lane's pixels, and the row takes the narrow form.
// A row is walked by LR lanes, lane lc of them: a whole wave (lane, 64) where a wave takes one row, 64 / PR lanes where it takes a
// patch of PR rows (mixed_views_affine.hpp); a head and a tail of up to 7 elements need LR >= 8.
// Everything is unrolled over compile-time indices: no LDS and no scratch.
#pragma once
#include <stdint.h>

#include "mixed_views.hpp"

namespace xpng {

// ---- views pixel -----------------------------------------------------------------------------------------------------------
// (the text from here on is what the host programs of the four kernels compile in front of them: tests/views_*_kernels_host.cpp)
// one colour through a row of the matrix and the clamp
__device__ __forceinline__ float colour_row(const float *m, float r, float g, float b) {
    const float t = fma_f32(m[0], r, fma_f32(m[1], g, fma_f32(m[2], b, m[3])));
    return t < 0.0f ? 0.0f : t > 255.0f ? 255.0f : t;
}

// the end of a pixel: the NS resampled values v, the view's matrix m where `mat` says the call has one, the BGR exchange, alpha last
template <uint32_t NS> __device__ __forceinline__ void pixel_finish(const float (&v)[NS], const float *m, bool mat, uint32_t bgr, float (&o)[4]) {
    float tr = v[0], tg = v[1], tb = v[2];
    if (mat) { tr = colour_row(m, v[0], v[1], v[2]); tg = colour_row(m + 4, v[0], v[1], v[2]); tb = colour_row(m + 8, v[0], v[1], v[2]); }
    o[0] = bgr ? tb : tr; o[1] = tg; o[2] = bgr ? tr : tb;
    o[3] = NS == 4 ? v[NS - 1] : 255.0f;  // a stored alpha, or the alpha an RGB file does not store
}

// the C elements of output pixel ox of the row at d (row oy of plane 0, the planes `plane` bytes apart; or the interleaved row)
template <int C, bool PLANAR, class T>
__device__ __forceinline__ void pixel_store(uint8_t *d, uint64_t plane, uint32_t ox, const float (&o)[4], const FloatConsts &k) {
#pragma unroll
    for (uint32_t c = 0; c < (uint32_t)C; c++) {
        const float y = fma_f32(o[c], pick4(k.scale, c), pick4(k.bias, c));
        if constexpr (PLANAR) store1<T>(d + c * plane, ox, y);
        else store1<T>(d, ox * C + c, y);
    }
}

// the narrow form of a row of OW pixels: a PIXEL per lane, its C elements stored one by one
template <int C, bool PLANAR, class T, class P>
__device__ __forceinline__ void row_narrow(uint8_t *d, uint32_t OW, uint64_t plane, uint32_t lc, uint32_t LR, const FloatConsts &k, const P &pixel) {
    for (uint32_t ox = lc; ox < OW; ox += LR) {
        float o[4];
        pixel(ox, o);
        pixel_store<C, PLANAR, T>(d, plane, ox, o, k);
    }
}

// the wide form of a row of OW pixels: the head, the aligned 16-byte stores and the tail of either layout
template <int C, bool PLANAR, class T, class P>
__device__ __forceinline__ void row_wide(uint8_t *d, uint32_t OW, uint64_t plane, uint32_t lc, uint32_t LR, const FloatConsts &k, const P &pixel) {
    constexpr uint32_t ES = sizeof(T), E = 16 / ES;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    if constexpr (PLANAR) {
        if ((plane & 15u) != 0) {  // the planes' rows do not start at one offset modulo 16
            row_narrow<C, true, T>(d, OW, plane, lc, LR, k, pixel);
            return;
        }
        auto single = [&](uint32_t j) {
            float o[4];
            pixel(j, o);
            pixel_store<C, true, T>(d, plane, j, o, k);
        };
        uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
        if (head > row_el) head = row_el;
        const uint32_t nq = (row_el - head) / E, tail0 = head + E * nq;
        if (lc < head) single(lc);
        if (tail0 + lc < row_el) single(tail0 + lc);
        uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned, in every plane
        for (uint32_t q = lc; q < nq; q += LR) {
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
        uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
        if (head > row_el) head = row_el;
        const uint32_t nq = (row_el - head) / E, tail0 = head + E * nq;
        auto single = [&](uint32_t j) {
            const uint32_t ox = j / C, c = j - ox * C;
            float o[4];
            pixel(ox, o);
            store1<T>(d, j, fma_f32(pick4(o, c), pick4(k.scale, c), pick4(k.bias, c)));
        };
        if (lc < head) single(lc);
        if (tail0 + lc < row_el) single(tail0 + lc);
        uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned
        for (uint32_t q = lc; q < nq; q += LR) {
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

}  // namespace xpng
