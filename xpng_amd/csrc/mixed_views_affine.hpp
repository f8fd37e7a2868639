// mixed_views_affine.hpp -- the copy-out pass of a views call under an AFFINE MAP per view: rotation, shear, scale and translation,
// bilinear or nearest, with a fill for what lies outside (xpnghip_decode_varsize_device_batch_views_affine).
//
// The rule.  m is the view's inverse matrix, row-major 2 x 3, from continuous output coordinates to continuous source coordinates
// of the whole image, pixel (j, i) centred at (j + 0.5, i + 0.5).  For output pixel (ox, oy), X = (float)ox + 0.5f, Y = (float)oy + 0.5f:
//     sx = fmaf(m[0], X, fmaf(m[1], Y, m[2])) - 0.5f        sy = fmaf(m[3], X, fmaf(m[4], Y, m[5])) - 0.5f
// A tap q(j, i, c) is the staging byte as fp32 where (j, i) lies inside the view's FOOTPRINT F (the host's rectangle around the
// warped output, clipped to the image: xpnghip_affine_footprint) and fill[colour of c] everywhere else.
//     filter 0   x0 = floorf(sx), lx = sx - x0, y0 = floorf(sy), ly = sy - y0
//                t = fmaf(lx, q(x0+1, y0) - q(x0, y0), q(x0, y0))      u = fmaf(lx, q(x0+1, y0+1) - q(x0, y0+1), q(x0, y0+1))
//                v = fmaf(ly, u - t, t)
//     filter 3   v = q((int)rintf(sx), (int)rintf(sy)), ties to even
// Behind v everything is mixed_views_colour.hpp's: the optional matrix and its clamp, the constants, the BGR exchange, alpha last
// (255 exactly, with no read, for the alpha an RGB context lacks).  xpnghip_resample_affine_host (xpng_hip.hip) is the same
// arithmetic on the host, bit for bit, per view.
//
// Only the tiles that intersect some view's footprint were reconstructed before this pass runs.  No tap reads anything else: the
// inside-F test is made on the integer tap itself, so consequence (c) holds by construction and needs no rounding argument.
#pragma once
#include <stdint.h>

#include "mixed_views_colour.hpp"

namespace xpng {

// ---- views affine ----------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_affine_kernels_host.cpp compiles)
// one view of an affine views call, 64 bytes: where its image lies in the staging raster, the caller's buffer, the inverse matrix,
// the output size and the footprint [fx0, fx1) x [fy0, fy1) in pixels of the image (all four 0: empty).  Uploaded on every call.
struct AffineRec {
    uint64_t stage;  // byte offset of the image's slot in the staging raster
    uint8_t *buf;    // C * oh * ow elements
    float m[6];
    uint32_t ow, oh;
    int32_t fx0, fy0, fx1, fy1;
};
static_assert(sizeof(AffineRec) == 64, "xpng_hip.h states the size of an affine view's record");
// the fill of a call in byte units, R, G, B, A: it travels in the kernel's arguments
struct AffineFill {
    float v[4];
};
constexpr uint32_t AF_NEAREST = 3;  // XPNGHIP_FILTER_NEAREST
constexpr uint32_t AF_ROWS = 16;    // output rows per workgroup

// grid (ceil(max oh / AF_ROWS), nviews), 256 threads; the template axes and the early return of a short view's blocks are
// k_mixed_views_colour's, the stores are the wide row writer's (mixed_views_pixel.hpp), and exactly C * oh * ow * sizeof(T) bytes of
// the view's buf are written.  The unit is the pixel: its coordinates, its taps and their inside-F tests are computed once and
// every source byte is read once per output pixel.  vm == nullptr: no colour matrix.
// PR is the lane mapping: a wave covers PR neighbouring output rows with 64 / PR lanes each in one pass.  Under a rotation a wave
// walking one output row reads a slanted line of the staging raster, every few lanes a cache line of their own; a patch of PR rows
// keeps the source footprint of a wave compact in both directions (DESIGN.md 24 has the measurement that chose PR).
// Everything is unrolled over compile-time indices: no LDS and no scratch.
template <int PX, int C, bool PLANAR, class T, int PR = 4>
__global__ __launch_bounds__(256) void k_mixed_views_affine(const AffineRec *__restrict__ vr, const ViewColour *__restrict__ vm, const uint8_t *__restrict__ stage,
                                                            uint64_t stage_bpr, uint32_t bgr, uint32_t filter, AffineFill fill, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T);
    constexpr uint32_t NS = PX == 4 && C == 4 ? 4 : 3;  // source bytes of a pixel that are read: the colours, and a stored alpha that is asked for
    constexpr uint32_t LR = 64 / PR;                    // lanes of a wave on one output row
    static_assert(PR == 1 || PR == 2 || PR == 4, "a head and a tail of up to 7 elements need at least 8 lanes on a row");
    const AffineRec z = vr[blockIdx.y];
    const uint32_t OW = z.ow, OH = z.oh;
    const uint32_t oy0 = blockIdx.x * AF_ROWS;
    if (oy0 >= OH) return;
    float m[12] = {};
    if (vm) {
#pragma unroll
        for (uint32_t i = 0; i < 12; i++) m[i] = vm[blockIdx.y].m[i];
    }
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t lr = lane / LR, lc = lane - lr * LR;  // the lane's row of the patch and its place on that row
    const uint32_t rows = OH - oy0 < AF_ROWS ? OH - oy0 : AF_ROWS;
    const uint32_t row_el = PLANAR ? OW : OW * C;  // elements of one row of the caller's buffer
    const uint8_t *img = stage + z.stage;          // the image's first pixel
    const uint32_t fw = (uint32_t)(z.fx1 - z.fx0), fh = (uint32_t)(z.fy1 - z.fy0);
    const uint64_t plane = (uint64_t)OH * OW * ES;  // bytes from a plane's row oy to the next plane's
    for (uint32_t it = wv * PR + lr; it < rows; it += 4 * PR) {
        const uint32_t oy = oy0 + it;
        const float Y = (float)oy + 0.5f;
        const float cx = fma_f32(z.m[1], Y, z.m[2]), cy = fma_f32(z.m[4], Y, z.m[5]);
        // output pixel ox of the row: o[c] is the value of channel position c of the caller's buffer before the constants
        auto pixel = [&](uint32_t ox, float (&o)[4]) {
            const float X = (float)ox + 0.5f;
            const float sx = fma_f32(z.m[0], X, cx) - 0.5f, sy = fma_f32(z.m[3], X, cy) - 0.5f;
            // the tap (j, i): inside F the staging bytes of the pixel, outside it the fill
            auto tap = [&](int32_t j, int32_t i, float (&q)[NS]) {
                const bool in = (uint32_t)(j - z.fx0) < fw && (uint32_t)(i - z.fy0) < fh;
                if (in) {
                    const uint8_t *p = img + (uint64_t)(uint32_t)i * stage_bpr + (uint64_t)(uint32_t)j * PX;
#pragma unroll
                    for (uint32_t b = 0; b < NS; b++) q[b] = (float)stage_ld8(p + b);
                } else {
#pragma unroll
                    for (uint32_t b = 0; b < NS; b++) q[b] = fill.v[b];
                }
            };
            float v[NS];
            if (filter == AF_NEAREST) {
                tap((int32_t)rintf(sx), (int32_t)rintf(sy), v);
            } else {
                const float x0 = floorf(sx), y0 = floorf(sy);
                const float lx = sx - x0, ly = sy - y0;
                const int32_t j = (int32_t)x0, i = (int32_t)y0;
                float q00[NS], q10[NS], q01[NS], q11[NS];
                tap(j, i, q00); tap(j + 1, i, q10); tap(j, i + 1, q01); tap(j + 1, i + 1, q11);
#pragma unroll
                for (uint32_t b = 0; b < NS; b++) {
                    const float t = fma_f32(lx, q10[b] - q00[b], q00[b]), u = fma_f32(lx, q11[b] - q01[b], q01[b]);
                    v[b] = fma_f32(ly, u - t, t);
                }
            }
            pixel_finish(v, m, vm != nullptr, bgr, o);
        };
        row_wide<C, PLANAR, T>(z.buf + (uint64_t)oy * row_el * ES, OW, plane, lc, LR, k, pixel);
    }
}

}  // namespace xpng
