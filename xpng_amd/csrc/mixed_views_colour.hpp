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

#include "mixed_views_pixel.hpp"

namespace xpng {

// ---- views colour ----------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_colour_kernels_host.cpp compiles)
// a view's matrix as the table holds it: 48 bytes, beside the view's ViewRec and with its index
struct ViewColour {
    float m[12];
};
static_assert(sizeof(ViewColour) == 48, "xpng_hip.h states the size of a view's matrix");

// grid (ceil(max oh / MC_ROWS), nviews), 256 threads; the template axes and the early return of a short view's blocks are
// k_mixed_views_as_float's, the stores are the wide row writer's (mixed_views_pixel.hpp), and exactly C * oh * ow * sizeof(T) bytes
// of the view's buf are written.  Each of the block's four waves takes whole output ROWS in both layouts, so the y taps and the y
// window are wave-uniform, and the branch an axis takes depends on the view alone.  The view's matrix is 12 uniform loads per block.
// Everything is unrolled over compile-time indices: no LDS and no scratch.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_views_colour(const ViewRec *__restrict__ vr, const ViewColour *__restrict__ vm, const uint8_t *__restrict__ stage,
                                                            uint64_t stage_bpr, uint32_t bgr, uint32_t filter, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T);
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
    const uint64_t plane = (uint64_t)OH * OW * ES;  // bytes from a plane's row oy to the next plane's
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
            pixel_finish(v, m, true, bgr, o);
        };
        row_wide<C, PLANAR, T>(z.buf + (uint64_t)oy * row_el * ES, OW, plane, lane, 64, k, pixel);
    }
}

}  // namespace xpng
