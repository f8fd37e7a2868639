// mixed_views.hpp -- the copy-out pass of a views call: ANY number of outputs per image of a mixed-size decode, every one with a
// rectangle, a flip and an output size of its own (xpnghip_decode_varsize_device_batch_views).
//
// The rule is mixed_resample.hpp's, word for word, with everything that call keeps per image taken from the view's record instead:
// the staging slot of the view's image, the output buffer, the rectangle, the four ratios, the flip and OW x OH.  With filter 0 both
// axes take the two-tap branch whatever their ratio, which is the resized call's rule; with filter 1 an axis takes the triangle
// where its own k > 1.  xpnghip_resample_host (xpng_hip.hip) is the same arithmetic on the host, bit for bit, per view.
//
// Only the tiles that some view of their image touches were reconstructed before this pass runs (view_select, xpng_hip.hip): the
// rest of the staging raster holds whatever earlier calls left.  No tap reads it - every window and both taps are clamped to the
// rectangle, not to the image - so consequence (c) of the resampled call is what makes skipping tiles safe.
#pragma once
#include <stdint.h>

#include "mixed_resample.hpp"

namespace xpng {

// ---- views -----------------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_kernels_host.cpp compiles)
// one view of a views call, 64 bytes: where its image lies in the staging raster, the caller's buffer, the source rectangle in
// pixels of the image, the output size, the two ratios and their inverses (one fp32 division each on the host, as ResizeRec's and
// ResampleRec's) and the flip.  Uploaded on every call and never cached.
struct ViewRec {
    uint64_t stage;  // byte offset of the image's slot in the staging raster
    uint8_t *buf;    // C * oh * ow elements
    uint32_t rx, ry, rw, rh;
    uint32_t ow, oh;
    float kx, ky, ikx, iky;
    uint32_t flip, pad;
};
static_assert(sizeof(ViewRec) == 64, "xpng_hip.h states the size of a view's record");

// grid (ceil(max oh / MC_ROWS), nviews), 256 threads; the template axes, the wave-uniform rows, the head, the aligned 16-byte stores
// and the tail are k_mixed_resample_as_float's, and exactly C * oh * ow * sizeof(T) bytes of the view's buf are written.  The grid's
// x extent is the tallest view's: a block whose first row is at or past its own view's oh returns at once.  The source side is the
// resampled kernel's loop per output element over its rows and its taps: single-byte reads of the staging rows inside the view's
// rectangle, weights recomputed in registers, no LDS.  Which branch an axis takes depends on the view alone, so it is uniform for
// the block.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_views_as_float(const ViewRec *__restrict__ vr, const uint8_t *__restrict__ stage, uint64_t stage_bpr,
                                                              uint32_t bgr, uint32_t filter, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T), E = 16 / ES;
    const ViewRec z = vr[blockIdx.y];
    const uint32_t OW = z.ow, OH = z.oh;
    const uint32_t oy0 = blockIdx.x * MC_ROWS;
    if (oy0 >= OH) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = OH - oy0 < MC_ROWS ? OH - oy0 : MC_ROWS;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    const bool aax = filter && z.kx > 1.0f, aay = filter && z.ky > 1.0f;
    const uint8_t *rect0 = stage + z.stage + (uint64_t)z.ry * stage_bpr + (uint64_t)z.rx * PX;  // the rectangle's first pixel
    for (uint32_t it = wv; it < (PLANAR ? rows * C : rows); it += 4) {
        const uint32_t oy = oy0 + (PLANAR ? it / C : it), pc = PLANAR ? it % C : 0;
        const ResizeTap ty = resize_tap(oy, z.ky, z.rh);
        const ResampleWin wy = resample_win(oy, z.ky, z.rh);
        uint8_t *d = z.buf + (PLANAR ? (uint64_t)pc * OH + oy : (uint64_t)oy) * row_el * ES;
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
