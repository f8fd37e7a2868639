// mixed_views_cubic.hpp -- the copy-out pass of a views call that resamples with an ANTIALIASED BICUBIC: mixed_views_colour.hpp's
// pass with Keys' cubic (a = -0.5) on both axes, stretched by the ratio where an axis shrinks, and a clamp of every resampled value
// to 0 .. 255 (xpnghip_decode_varsize_device_batch_views_cubic).
//
// The rule.  An axis operation maps q(0 .. n-1), fp32, to one fp32 value; n is the RECTANGLE's extent on the axis, k the ratio and
// ik its inverse, both from the view's record.  For output index u
//     f  = fmaf((float)u + 0.5f, k, -0.5f)
//     s  = k > 1.0f ? k : 1.0f     is = k > 1.0f ? ik : 1.0f     r = s + s
//     lo = f - r   j0 = lo > 0 ? (uint32_t)lo : 0   j1 = min((uint32_t)(f + r), n - 1)
//     W = 0, A = 0, then for j = j0 .. j1 ascending:
//         d = fabsf((float)j - f)   t = fmaf(d, is, 0.0f)
//         w = t < 1 ? fmaf(fmaf(fmaf( 1.5f, t, -2.5f), t,  0.0f), t, 1.0f)
//           : t < 2 ? fmaf(fmaf(fmaf(-0.5f, t,  2.5f), t, -4.0f), t, 2.0f) : 0.0f
//         W = W + w   A = fmaf(w, q(j), A)
//     result A / W, one IEEE fp32 division
// There is no two-tap branch: an axis with k <= 1 takes the same window with s = 1.  H(s) is the x-axis operation over source row s
// of the rectangle, u = flip ? OW-1-ox : ox; the y-axis operation runs over H(.); then v = clamp(result, 0.0f, 255.0f) - a cubic
// overshoots - then the view's matrix where the call has matrices (colour_row, on these clamped v), then
// y = fmaf(v_or_t, scale[c], bias[c]) and out = (T)y.  Channel choice, the BGR exchange, alpha last and the 255 an RGB context
// lacks are the views-colour call's.  xpnghip_resample_cubic_host (xpng_hip.hip) is the same arithmetic on the host, bit for bit.
// Consequences: (a) a rectangle of the output's size is a pure crop (k = 1: f is an integer, the weights are exactly 1, 0, 0);
// (b) a flip is a mirror on the bits; (c) no tap leaves the rectangle; (d) an identity matrix gives the bits of no matrix, because
// v already lies in 0 .. 255.  W > 0 always.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "mixed_views_colour.hpp"

namespace xpng {

// ---- views cubic -----------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_cubic_kernels_host.cpp compiles)
// the window of one axis: the first and the last tap and the centre.  is is the inverse of the stretch, 1 where the axis grows
__device__ __forceinline__ ResampleWin cubic_win(uint32_t u, float k, uint32_t n) {
    const float c = (float)u + 0.5f;  // exact: u < 2^23
    ResampleWin r;
    r.f = fma_f32(c, k, -0.5f);
    const float s = k > 1.0f ? k : 1.0f;
    const float rad = s + s;
    const float lo = r.f - rad, hi = r.f + rad;
    r.j0 = lo > 0.0f ? (uint32_t)lo : 0u;
    const uint32_t t = (uint32_t)hi;  // (hi > 0: f >= -0.5 and rad >= 2)
    r.j1 = t < n - 1 ? t : n - 1;
    return r;
}
// the weight of tap j of a window centred at f: both pieces of the cubic, then the choice (no branch)
__device__ __forceinline__ float cubic_weight(uint32_t j, float f, float is) {
    const float d = __builtin_fabsf((float)j - f);
    const float t = fma_f32(d, is, 0.0f);
    const float a = fma_f32(fma_f32(fma_f32(1.5f, t, -2.5f), t, 0.0f), t, 1.0f);
    const float b = fma_f32(fma_f32(fma_f32(-0.5f, t, 2.5f), t, -4.0f), t, 2.0f);
    return t < 1.0f ? a : t < 2.0f ? b : 0.0f;
}

// source rows whose x-axis operations a lane runs together, sharing the x weights (R * 4 accumulators in registers)
constexpr uint32_t CUBIC_ROWS = 4;

// grid (ceil(max oh / MC_ROWS), nviews), 256 threads; the template axes, the unit (the output PIXEL: windows and weights once for a
// pixel's bytes), the wave-uniform rows and the early return of a short view's blocks are k_mixed_views_colour's, and exactly
// C * oh * ow * sizeof(T) bytes of the view's buf are written.  What is not taken from that kernel is the 16-byte store: there a
// lane resamples the two to eight pixels one store covers, one after another, and a 224-wide planar f16 row keeps 28 of a wave's 64
// lanes busy; here a pixel costs hundreds of taps and its C stores nothing beside them, so a lane takes ONE pixel and stores its
// elements one by one (the narrow row writer of mixed_views_pixel.hpp), and no pixel is resampled twice.
// vm may be null - no matrices in this call, uniform for the launch - and then no matrix is read.  The source side is a
// loop per output pixel over the rows of its y window, CUBIC_ROWS at a time, and the taps of its x window: reads of single bytes (PX
// 3) or of one whole pixel as an aligned dword (PX 4: the staging slots and rows are 16-byte aligned) inside the view's rectangle,
// an x weight computed once for the rows that run together, no LDS and no scratch.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_views_cubic(const ViewRec *__restrict__ vr, const ViewColour *__restrict__ vm, const uint8_t *__restrict__ stage,
                                                           uint64_t stage_bpr, uint32_t bgr, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T);
    constexpr uint32_t NS = PX == 4 && C == 4 ? 4 : 3;  // source bytes of a pixel that are read: the colours, and a stored alpha that is asked for
    const ViewRec z = vr[blockIdx.y];
    const uint32_t OW = z.ow, OH = z.oh;
    const uint32_t oy0 = blockIdx.x * MC_ROWS;
    if (oy0 >= OH) return;
    const bool mat = vm != nullptr;
    float m[12] = {};
    if (mat) {
#pragma unroll
        for (uint32_t i = 0; i < 12; i++) m[i] = vm[blockIdx.y].m[i];
    }
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = OH - oy0 < MC_ROWS ? OH - oy0 : MC_ROWS;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    const float isx = z.kx > 1.0f ? z.ikx : 1.0f, isy = z.ky > 1.0f ? z.iky : 1.0f;
    const uint8_t *rect0 = stage + z.stage + (uint64_t)z.ry * stage_bpr + (uint64_t)z.rx * PX;  // the rectangle's first pixel
    const uint64_t plane = (uint64_t)OH * OW * ES;  // bytes from a plane's row oy to the next plane's
    for (uint32_t it = wv; it < rows; it += 4) {
        const uint32_t oy = oy0 + it;
        const ResampleWin wy = cubic_win(oy, z.ky, z.rh);
        // output pixel ox of the row: o[c] is the value of channel position c of the caller's buffer before the constants
        auto pixel = [&](uint32_t ox, float (&o)[4]) {
            const uint32_t u = z.flip ? OW - 1 - ox : ox;
            const ResampleWin wx = cubic_win(u, z.kx, z.rw);
            float W = 0.0f, A[NS] = {};
            // H(s) .. H(s + R - 1), the x-axis operation over R source rows at once, every byte of the pixel: the x weights and
            // their sum are the same sequence for every row, so they are computed once for the R rows and every row's sum takes
            // its taps in ascending j; then the rows enter the y sums in ascending s.  The bits are the plain loop's
            auto rows_of = [&](uint32_t s, auto Rc) {
                constexpr uint32_t R = decltype(Rc)::value;
                const uint8_t *p = rect0 + (uint64_t)s * stage_bpr;
                float Wx = 0.0f, Ax[R][NS] = {};
                for (uint32_t j = wx.j0; j <= wx.j1; j++) {
                    const float wj = cubic_weight(j, wx.f, isx);
                    Wx = Wx + wj;
#pragma unroll
                    for (uint32_t r = 0; r < R; r++) {
                        const uint8_t *t = p + r * stage_bpr + j * PX;  // tap j of row s + r
                        if constexpr (PX == 4) {  // one aligned dword is the pixel; its bytes are v_cvt_f32_ubyte<b>
                            const uint32_t q = stage_ld32(t);
#pragma unroll
                            for (uint32_t b = 0; b < NS; b++) Ax[r][b] = fma_f32(wj, (float)((q >> (8 * b)) & 0xffu), Ax[r][b]);
                        } else {
#pragma unroll
                            for (uint32_t b = 0; b < NS; b++) Ax[r][b] = fma_f32(wj, (float)stage_ld8(t + b), Ax[r][b]);
                        }
                    }
                }
#pragma unroll
                for (uint32_t r = 0; r < R; r++) {
                    const float w = cubic_weight(s + r, wy.f, isy);
                    W = W + w;
#pragma unroll
                    for (uint32_t b = 0; b < NS; b++) A[b] = fma_f32(w, resample_div(Ax[r][b], Wx), A[b]);
                }
            };
            uint32_t s = wy.j0;
            for (; s + CUBIC_ROWS <= wy.j1 + 1; s += CUBIC_ROWS) rows_of(s, std::integral_constant<uint32_t, CUBIC_ROWS>{});
            for (; s <= wy.j1; s++) rows_of(s, std::integral_constant<uint32_t, 1>{});
            float v[NS];
#pragma unroll
            for (uint32_t i = 0; i < NS; i++) {
                const float x = resample_div(A[i], W);
                v[i] = x < 0.0f ? 0.0f : x > 255.0f ? 255.0f : x;
            }
            pixel_finish(v, m, mat, bgr, o);
        };
        row_narrow<C, PLANAR, T>(z.buf + (uint64_t)oy * row_el * ES, OW, plane, lane, 64, k, pixel);
    }
}

}  // namespace xpng
