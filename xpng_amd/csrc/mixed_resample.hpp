// mixed_resample.hpp -- the copy-out pass of a mixed-size decode that crops, resamples with an ANTIALIASED downscale and flips while
// it converts: mixed_resize.hpp's pass with a triangle filter wherever an axis shrinks
// (xpnghip_decode_varsize_device_batch_resampled with XPNGHIP_FILTER_TRIANGLE_AA).
//
// The rule.  Per image, on the host: kx = (float)rw / (float)OW and ky, one fp32 division each (as in mixed_resize.hpp), and
// ikx = 1.0f / kx, iky = 1.0f / ky, one fp32 division each.  An axis operation maps a sequence q(0 .. n-1) of fp32 values to one
// fp32 value; n is the extent of the RECTANGLE on that axis, O the output extent, k the ratio, ik its inverse.  For output index u
//     f = fmaf((float)u + 0.5f, k, -0.5f)
//   k <= 1.0f (or filter 0): the two taps of mixed_resize.hpp, unchanged
//     s = max(f, 0)   i0 = min((uint32_t)s, n-1)   i1 = min(i0+1, n-1)   l = s - (float)i0
//     result fmaf(l, q(i1) - q(i0), q(i0))
//   k > 1.0f with filter 1: a triangle of half-width k, clamped to the rectangle and renormalised
//     lo = f - k   j0 = lo > 0 ? (uint32_t)lo : 0   j1 = min((uint32_t)(f + k), n - 1)
//     W = 0, A = 0, then for j = j0 .. j1 ascending:
//         d = fabsf((float)j - f)   w = max(fmaf(-d, ik, 1.0f), 0.0f)   W = W + w   A = fmaf(w, q(j), A)
//     result A / W, one IEEE fp32 division
// H(s) is the x-axis operation over the channel's bytes of source row s as floats, u = flip ? OW-1-ox : ox; v is the y-axis
// operation over H(.); then y = fmaf(v, scale[c], bias[c]), out = (T)y, round to nearest even.  Each axis chooses its branch on its
// own k.  Channel choice, the BGR exchange, alpha last, the alpha an RGB context lacks (v = 255 exactly, no read), the constants,
// the layouts and the dtypes are the float and resized calls'.
// Consequences: (a) an image with kx <= 1 and ky <= 1 gives bit for bit what filter 0 gives; (b) a flip is a mirror on the bits;
// (c) no tap leaves the rectangle - the window is clamped to it, not to the image.
// W > 0 always: the pixel nearest to f lies inside [0, n-1] and its distance is below k, and where f is large enough for fp32 to
// round the distance by up to 1, k is at least 512 because O <= 16384.
// Every multiplication is inside an explicit fmaf (fma_f32), sums and the division are single operations, and the order of
// accumulation - ascending j within a row, ascending s over rows - is part of the rule.  xpnghip_resample_host (xpng_hip.hip) is
// the same arithmetic on the host, bit for bit.
#pragma once
#include <stdint.h>

#include "mixed_resize.hpp"

namespace xpng {

// ---- resample --------------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/resample_kernels_host.cpp compiles)
// one image of a resampled call with filter 1, beside its MixedLayout record: ResizeRec's fields and the two inverses.  Uploaded
// on every call and never cached, as the ResizeRec table is.
struct ResampleRec {
    uint32_t rx, ry, rw, rh;
    float kx, ky, ikx, iky;
    uint32_t flip, pad[3];
};

// the window of the triangle branch of one axis: the first and the last tap and the centre
struct ResampleWin {
    uint32_t j0, j1;
    float f;
};
__device__ __forceinline__ ResampleWin resample_win(uint32_t u, float k, uint32_t n) {
    const float c = (float)u + 0.5f;  // exact: u < 2^23
    ResampleWin r;
    r.f = fma_f32(c, k, -0.5f);
    const float lo = r.f - k, hi = r.f + k;
    r.j0 = lo > 0.0f ? (uint32_t)lo : 0u;
    const uint32_t t = (uint32_t)hi;  // (hi > 0: f > -0.5 + 0.5 k and k > 1)
    r.j1 = t < n - 1 ? t : n - 1;
    return r;
}
// the weight of tap j of a window centred at f
__device__ __forceinline__ float resample_weight(uint32_t j, float f, float ik) {
    const float d = __builtin_fabsf((float)j - f);
    const float w = fma_f32(-d, ik, 1.0f);
    return w > 0.0f ? w : 0.0f;
}
// the quotient of the rule as a value of its own: one correctly rounded fp32 division (the v_div_scale / v_rcp / v_fma /
// v_div_fmas / v_div_fixup sequence; the library is built without any fast-math flag)
__device__ __forceinline__ float resample_div(float a, float w) { return a / w; }

// grid (ceil(OH / MC_ROWS), nimg), 256 threads; the template axes, the grid, the wave-uniform rows, the head, the aligned 16-byte
// stores and the tail are k_mixed_resize_as_float's, and exactly C * OH * OW * sizeof(T) bytes of buf are written.  The source
// side is a loop per output element over its rows and its taps: single-byte reads of the staging rows, so no read leaves the
// pixels of the rectangle; the weights are recomputed in registers and nothing is kept in LDS.  Which branch an axis takes depends
// on the image alone, so it is uniform for the block; the rows of the y window are uniform for the wave, the taps of the x window
// differ between lanes by the few pixels that neighbouring output columns are apart.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_resample_as_float(const MixedLayout *__restrict__ ml, const ResampleRec *__restrict__ rz,
                                                                 const uint8_t *__restrict__ stage, uint64_t stage_bpr, uint32_t bgr, uint32_t OW,
                                                                 uint32_t OH, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T), E = 16 / ES;
    const MixedLayout r = ml[blockIdx.y];
    const ResampleRec z = rz[blockIdx.y];
    const uint32_t oy0 = blockIdx.x * MC_ROWS;
    if (oy0 >= OH) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = OH - oy0 < MC_ROWS ? OH - oy0 : MC_ROWS;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    const bool aax = z.kx > 1.0f, aay = z.ky > 1.0f;
    const uint8_t *rect0 = stage + r.stage + (uint64_t)z.ry * stage_bpr + (uint64_t)z.rx * PX;  // the rectangle's first pixel
    for (uint32_t it = wv; it < (PLANAR ? rows * C : rows); it += 4) {
        const uint32_t oy = oy0 + (PLANAR ? it / C : it), pc = PLANAR ? it % C : 0;
        const ResizeTap ty = resize_tap(oy, z.ky, z.rh);
        const ResampleWin wy = resample_win(oy, z.ky, z.rh);
        uint8_t *d = r.buf + (PLANAR ? (uint64_t)pc * OH + oy : (uint64_t)oy) * row_el * ES;
        // the value of the rule before the constants, for output column ox and channel position c of the caller's buffer
        auto val = [&](uint32_t ox, uint32_t c) {
            if (PX == 3 && c == 3) return 255.0f;                        // the alpha an RGB file does not store
            const uint32_t sc = bgr && c < 3 ? 2 - c : c;                // the channel's byte inside a staging pixel
            const uint32_t u = z.flip ? OW - 1 - ox : ox;
            const ResizeTap tx = resize_tap(u, z.kx, z.rw);
            const ResampleWin wx = resample_win(u, z.kx, z.rw);
            auto H = [&](uint32_t s) {  // the x-axis operation over source row s of the rectangle
                const uint8_t *p = rect0 + (uint64_t)s * stage_bpr + sc;
                if (!aax) {
                    const float q0 = (float)stage_ld8(p + tx.i0 * PX), q1 = (float)stage_ld8(p + tx.i1 * PX);
                    return fma_f32(tx.l, q1 - q0, q0);
                }
                float W = 0.0f, A = 0.0f;
                for (uint32_t j = wx.j0; j <= wx.j1; j++) {
                    const float w = resample_weight(j, wx.f, z.ikx);
                    W = W + w;
                    A = fma_f32(w, (float)stage_ld8(p + j * PX), A);
                }
                return resample_div(A, W);
            };
            if (!aay) {
                const float a = H(ty.i0), b = H(ty.i1);
                return fma_f32(ty.l, b - a, a);
            }
            float W = 0.0f, A = 0.0f;
            for (uint32_t s = wy.j0; s <= wy.j1; s++) {
                const float w = resample_weight(s, wy.f, z.iky);
                W = W + w;
                A = fma_f32(w, H(s), A);
            }
            return resample_div(A, W);
        };
        auto one = [&](uint32_t j) {  // element j of the row
            const uint32_t ox = PLANAR ? j : j / C, c = PLANAR ? pc : j - ox * C;
            return fma_f32(val(ox, c), pick4(k.scale, c), pick4(k.bias, c));
        };
        uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
        if (head > row_el) head = row_el;
        const uint32_t nq = (row_el - head) / E, tail0 = head + E * nq;
        uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned
        if (lane < head) store1<T>(d, lane, one(lane));
        if (tail0 + lane < row_el) store1<T>(d, tail0 + lane, one(tail0 + lane));
        for (uint32_t q = lane; q < nq; q += 64) {
            const uint32_t j = head + E * q;
            float v[8] = {}, sa[4] = {}, ba[4] = {};
            if constexpr (PLANAR) {
                sa[0] = pick4(k.scale, pc); ba[0] = pick4(k.bias, pc);
#pragma unroll
                for (uint32_t i = 0; i < E; i++) v[i] = val(j + i, pc);
                out_st128(d16 + 16ull * q, float_chunk<T, 1>(v, sa, ba));
            } else {
                const uint32_t p = j / C, rr = j - p * C;  // the store starts at channel rr of pixel p
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)C; i++) {
                    const uint32_t c = rr + i < (uint32_t)C ? rr + i : rr + i - C;
                    sa[i] = pick4(k.scale, c); ba[i] = pick4(k.bias, c);
                }
#pragma unroll
                for (uint32_t i = 0; i < E; i++) {
                    const uint32_t t = rr + i, dq = t >= 3u * C ? 3u : t >= 2u * C ? 2u : t >= (uint32_t)C ? 1u : 0u;
                    v[i] = val(p + dq, t - dq * C);
                }
                out_st128(d16 + 16ull * q, float_chunk<T, C>(v, sa, ba));
            }
        }
    }
}

}  // namespace xpng
