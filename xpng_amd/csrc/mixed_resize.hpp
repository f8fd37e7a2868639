// mixed_resize.hpp -- the copy-out pass of a mixed-size decode that crops, resizes and flips while it converts: a rectangle of every
// image of the staging raster -> ONE output size OH x OW per call, planar or interleaved, RGB or BGR, 3 or 4 channels of f16, bf16
// or f32 (xpnghip_decode_varsize_device_batch_resized).
//
// The rule, for output column ox of image i (rows alike with ky, rh and no flip), u = flip ? OW - 1 - ox : ox:
//     sx = max(fmaf((float)u + 0.5f, kx, -0.5f), 0)      kx = (float)rw / (float)OW, one fp32 division on the host
//     x0 = min((uint32_t)sx, rw - 1)    x1 = min(x0 + 1, rw - 1)    lx = sx - (float)x0
//     a = fmaf(lx, p01 - p00, p00)      b = fmaf(lx, p11 - p10, p10)      v = fmaf(ly, b - a, a)
//     y = fmaf(v, scale[c], bias[c])    out = (T)y                        round to nearest even
// p00 p01 / p10 p11 the four taps at (ry + y0|y1, rx + x0|x1) as floats, the byte chosen as in mixed_float.hpp (BGR exchange, alpha
// last, the alpha an RGB context lacks is 255).  Every fmaf is a value of its own (fma_f32); no other operation of the rule is a
// multiplication, so there is nothing a compiler could contract.  xpnghip_resize_host (xpng_hip.hip) is the same arithmetic on the
// host, bit for bit.
#pragma once
#include <stdint.h>

#include "mixed_float.hpp"

namespace xpng {

// ---- resize ----------------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/resize_kernels_host.cpp compiles)
// one image of a resized call, beside its MixedLayout record (which keeps the buffer and the staging slot): the source rectangle
// in pixels of the image, the two ratios and the flip.  Uploaded on every call - rectangles change with every batch of a training
// run - and never cached.
struct ResizeRec {
    uint32_t rx, ry, rw, rh;
    float kx, ky;
    uint32_t flip, pad;
};

// one axis of the rule: output index u of the axis, ratio k, n source pixels -> the two taps and the weight of the second
struct ResizeTap {
    uint32_t i0, i1;
    float l;
};
__device__ __forceinline__ ResizeTap resize_tap(uint32_t u, float k, uint32_t n) {
    const float c = (float)u + 0.5f;  // exact: u < 2^23
    const float f = fma_f32(c, k, -0.5f);
    const float s = f > 0.0f ? f : 0.0f;
    const uint32_t t = (uint32_t)s;
    ResizeTap r;
    r.i0 = t < n - 1 ? t : n - 1;
    r.i1 = r.i0 + 1 < n - 1 ? r.i0 + 1 : n - 1;
    r.l = s - (float)r.i0;  // exact
    return r;
}

// grid (ceil(OH / MC_ROWS), nimg), 256 threads; PX, C, PLANAR, bgr, T and E as in k_mixed_copy_as_float.  Each of the block's four
// waves takes whole output rows (interleaved) or plane rows (planar), so y0, y1, ly, the two staging row pointers, the head and the
// alignment are wave-uniform.  The caller's side is the float kernel's: a head of fewer than E single elements, whole ALIGNED
// 16-byte stores (lane k of a pass takes store k) and a tail of fewer than E elements.  The source side is a gather: every element
// reads its four taps as single bytes of the two staging rows, so no read leaves the pixels of its row (the read rule of the
// staging raster holds with nothing to spare needed), and the rows were written by the kernels just before, so they come from L2.
// The alpha of an RGB context is 255 at every tap and the rule then gives v = 255 exactly, so no byte is read for it.
// Exactly C * OH * OW * sizeof(T) bytes of buf are written.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_resize_as_float(const MixedLayout *__restrict__ ml, const ResizeRec *__restrict__ rz,
                                                               const uint8_t *__restrict__ stage, uint64_t stage_bpr, uint32_t bgr, uint32_t OW,
                                                               uint32_t OH, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T), E = 16 / ES;
    const MixedLayout r = ml[blockIdx.y];
    const ResizeRec z = rz[blockIdx.y];
    const uint32_t oy0 = blockIdx.x * MC_ROWS;
    if (oy0 >= OH) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = OH - oy0 < MC_ROWS ? OH - oy0 : MC_ROWS;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    for (uint32_t it = wv; it < (PLANAR ? rows * C : rows); it += 4) {
        const uint32_t oy = oy0 + (PLANAR ? it / C : it), pc = PLANAR ? it % C : 0;
        const ResizeTap ty = resize_tap(oy, z.ky, z.rh);
        const uint8_t *s0 = stage + r.stage + (uint64_t)(z.ry + ty.i0) * stage_bpr + (uint64_t)z.rx * PX;
        const uint8_t *s1 = stage + r.stage + (uint64_t)(z.ry + ty.i1) * stage_bpr + (uint64_t)z.rx * PX;
        uint8_t *d = r.buf + (PLANAR ? (uint64_t)pc * OH + oy : (uint64_t)oy) * row_el * ES;
        // the value of the rule before the constants, for output column ox and channel position c of the caller's buffer
        auto val = [&](uint32_t ox, uint32_t c) {
            const bool fill = PX == 3 && c == 3;                         // the alpha an RGB file does not store
            const uint32_t sc = fill ? 0 : bgr && c < 3 ? 2 - c : c;     // the channel's byte inside a staging pixel
            const ResizeTap tx = resize_tap(z.flip ? OW - 1 - ox : ox, z.kx, z.rw);
            const uint32_t o0 = tx.i0 * PX + sc, o1 = tx.i1 * PX + sc;
            const float p00 = (float)stage_ld8(s0 + o0), p01 = (float)stage_ld8(s0 + o1);
            const float p10 = (float)stage_ld8(s1 + o0), p11 = (float)stage_ld8(s1 + o1);
            const float a = fma_f32(tx.l, p01 - p00, p00), b = fma_f32(tx.l, p11 - p10, p10);
            const float v = fma_f32(ty.l, b - a, a);
            return fill ? 255.0f : v;
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
