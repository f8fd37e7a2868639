// mixed_views_blur.hpp -- the SECOND pass of a views call with a Gaussian blur and a solarise per view
// (xpnghip_decode_varsize_device_batch_views_blur).  A blur reads its neighbours' finished values, so it cannot live in
// the copy-out pass: the views that blur or solarise are first written by the existing copy-out kernel of the call's filter as C
// planes of fp32 in byte units into the context's scratch (the intermediate T), and this kernel turns T into the caller's buffer.
//
// The rule, per colour plane q of T (OH x OW; alpha, or the 255 an RGB context lacks, passes through untouched), R the view's
// radius, w[0 .. R] its weights (xpnghip_blur_weights, computed on the host), refl(i, n) = i < 0 ? -i : i >= n ? 2 (n - 1) - i : i:
//     A = 0.0f;  for d = R down to 1:  A = fmaf(w[d], q(y, refl(x - d, OW)) + q(y, refl(x + d, OW)), A);  A = fmaf(w[0], q(y, x), A)
// is the horizontal operation; the vertical one is the same over the horizontal results with OH; then b = clamp(A, 0.0f, 255.0f).
// With R == 0 the blur is skipped, b = q.  Solarise, where it is on: b = b >= thr ? 255.0f - b : b.  Last y = fmaf(b, scale[c],
// bias[c]) and out = (T)y, c the position in the caller's buffer (with the BGR bit position c < 3 holds colour 2 - c).
// xpnghip_resample_blur_host (xpng_hip.hip) is the same arithmetic on the host, bit for bit.
#pragma once
#include <stdint.h>

#include "mixed_views_cubic.hpp"

namespace xpng {

// the kernel's reads of the scratch planes and its barrier: the host program checks every read against the view's own slice
__device__ __forceinline__ float scratch_ld(const float *p) { return *p; }
__device__ __forceinline__ void blur_sync() { __syncthreads(); }

// ---- views blur ------------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_blur_kernels_host.cpp compiles)
// the tile of one workgroup: BLUR_TW output columns, so that a wave's 64 lanes walk one row of LDS or of global memory with stride
// one (no bank conflict in either axis operation, whole-row coalesced reads and stores), and BLUR_TH output rows, the most whose
// tile plus halo (s_in) and horizontal results (s_mid) stay under 64 KB at the largest radius: (16 + 62) * (126 + 64) * 4 = 59280
// bytes, two workgroups on a compute unit's 160 KB
constexpr uint32_t BLUR_TW = 64, BLUR_TH = 16, BLUR_RMAX = 31;
constexpr uint32_t BLUR_IN_W = BLUR_TW + 2 * BLUR_RMAX, BLUR_IN_H = BLUR_TH + 2 * BLUR_RMAX;
static_assert((BLUR_IN_H * BLUR_IN_W + BLUR_IN_H * BLUR_TW) * 4 <= 65536, "two workgroups must fit a compute unit's LDS");

// one second-pass view, 160 bytes, in a table of its own: where its planes lie in the scratch, the caller's buffer, the output
// size, the radius, the solarise threshold (256.0f: off) and the weights
struct BlurRec {
    uint64_t src;    // offset of the view's slice in the scratch, in floats: C planes of oh * ow
    uint8_t *buf;    // C * oh * ow elements
    uint32_t ow, oh;
    uint32_t radius;
    float thr;
    float w[32];
};
static_assert(sizeof(BlurRec) == 160, "DESIGN.md 23 states the size of a blurred view's record");

__device__ __forceinline__ uint32_t blur_refl(int32_t i, uint32_t n) {
    return i < 0 ? (uint32_t)-i : i >= (int32_t)n ? 2u * (n - 1) - (uint32_t)i : (uint32_t)i;
}

// grid (the most tiles of any view, second-pass views), 256 threads: block x of view y takes tile x of the view's ceil(ow / 64) *
// ceil(oh / 16) tiles, row-major, and returns at once when the view has fewer.  C is the caller's channel count - the scratch holds
// C planes -, PLANAR and T the caller's layout and element.  Per colour plane: the tile and its halo of R on every side go from the
// scratch into s_in, each wave taking whole rows with the reflection resolved at the load; the horizontal operation of every row of
// s_in goes into s_mid; the vertical operation runs over s_mid.  A lane owns column `lane` of rows wv, wv + 4, .. of the tile and
// keeps its pixels' three colours in registers until the last plane is through, then stores the C elements of each pixel
// (pixel_store, mixed_views_pixel.hpp): a wave's stores are 64 neighbouring elements of a plane's row, or 64 * C neighbouring
// elements of an interleaved row.  Exactly C * oh * ow * sizeof(T) bytes of the view's buf are written and no read leaves the
// view's slice.  R == 0 (solarise alone) skips the LDS and the barriers; R is uniform for the block.
template <int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_views_blur(const BlurRec *__restrict__ br, const float *__restrict__ scratch, uint32_t bgr, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T), NIT = BLUR_TH / 4;
    __shared__ float s_in[BLUR_IN_H * BLUR_IN_W];
    __shared__ float s_mid[BLUR_IN_H * BLUR_TW];
    const BlurRec &z = br[blockIdx.y];
    const uint32_t OW = z.ow, OH = z.oh, R = z.radius;
    const uint32_t ntx = (OW + BLUR_TW - 1) / BLUR_TW, nty = (OH + BLUR_TH - 1) / BLUR_TH;
    if (blockIdx.x >= ntx * nty) return;
    const uint32_t tyi = blockIdx.x / ntx, y0 = tyi * BLUR_TH, x0 = (blockIdx.x - tyi * ntx) * BLUR_TW;
    const uint32_t tw = OW - x0 < BLUR_TW ? OW - x0 : BLUR_TW, th = OH - y0 < BLUR_TH ? OH - y0 : BLUR_TH;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t plane = (uint64_t)OH * OW;
    const float *src = scratch + z.src;
    const bool mine = lane < tw;
    float v[NIT][3] = {};
#pragma unroll
    for (uint32_t q = 0; q < 3; q++) {
        const float *pl = src + q * plane;
        if (R == 0) {
#pragma unroll
            for (uint32_t it = 0; it < NIT; it++) {
                const uint32_t y = wv + 4 * it;
                if (mine && y < th) v[it][q] = scratch_ld(pl + (uint64_t)(y0 + y) * OW + x0 + lane);
            }
            continue;
        }
        const uint32_t rows = th + 2 * R, cols = tw + 2 * R;
        for (uint32_t ry = wv; ry < rows; ry += 4) {
            const float *row = pl + (uint64_t)blur_refl((int32_t)(y0 + ry) - (int32_t)R, OH) * OW;
            for (uint32_t cx = lane; cx < cols; cx += 64) s_in[ry * BLUR_IN_W + cx] = scratch_ld(row + blur_refl((int32_t)(x0 + cx) - (int32_t)R, OW));
        }
        blur_sync();
        for (uint32_t ry = wv; ry < rows; ry += 4) {
            if (!mine) continue;
            const float *p = s_in + ry * BLUR_IN_W + R + lane;
            float A = 0.0f;
            for (uint32_t d = R; d >= 1; d--) A = fma_f32(z.w[d], p[-(int32_t)d] + p[d], A);
            s_mid[ry * BLUR_TW + lane] = fma_f32(z.w[0], p[0], A);
        }
        blur_sync();
#pragma unroll
        for (uint32_t it = 0; it < NIT; it++) {
            const uint32_t y = wv + 4 * it;
            if (!mine || y >= th) continue;
            const float *p = s_mid + (R + y) * BLUR_TW + lane;
            float A = 0.0f;
            for (uint32_t d = R; d >= 1; d--) A = fma_f32(z.w[d], p[-(int32_t)(d * BLUR_TW)] + p[d * BLUR_TW], A);
            A = fma_f32(z.w[0], p[0], A);
            v[it][q] = A < 0.0f ? 0.0f : A > 255.0f ? 255.0f : A;
        }
        // (the next plane's load writes s_in, which nobody reads any more; its barrier stands between these reads of s_mid and the
        // next writes of it)
    }
    const bool sol = z.thr < 256.0f;
#pragma unroll
    for (uint32_t it = 0; it < NIT; it++) {
        const uint32_t y = wv + 4 * it;
        if (!mine || y >= th) continue;
        const uint64_t e = (uint64_t)(y0 + y) * OW + x0;  // the row's first pixel of the tile, in pixels of a plane
        float o[4];
#pragma unroll
        for (uint32_t q = 0; q < 3; q++) {
            const float b = v[it][q];
            o[q] = sol && b >= z.thr ? 255.0f - b : b;
        }
        if (bgr) { const float t = o[0]; o[0] = o[2]; o[2] = t; }
        o[3] = 0.0f;
        if constexpr (C == 4) o[3] = scratch_ld(src + 3 * plane + e + lane);  // stored, or the 255 the first pass wrote
        pixel_store<C, PLANAR, T>(z.buf + e * (PLANAR ? 1 : C) * ES, plane * ES, lane, o, k);
    }
}

}  // namespace xpng
