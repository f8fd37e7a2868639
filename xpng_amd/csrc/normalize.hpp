// normalize.hpp -- normalize_RGBA (libxpng.c:688-721) and the whole-image single-colour test (libxpng.c:741-753) on the
// device, so that xpng_store uploads the caller's raster once and never walks it on the host.
//
//   hidden      = exists px: alpha == 0 and (r | g | b) != 0   -> rewrite: those pixels become 0 (stays RGBA)
//   translucent = exists px: alpha != 255                      -> else if none: repack to RGB
// (the reference's early-break loop is equivalent to these two ORs: SURVEY.md §8(a) row E)
#pragma once
#include "common.hpp"

namespace xpng {

// flags[0] |= hidden, flags[1] |= translucent.  One uint4 (4 pixels) per thread per iteration; px needs only its natural 4-byte
// alignment (a band of a raster starts at any pixel): the pixels in front of the first 16-byte boundary and behind the last whole
// group are looked at one by one.
__global__ __launch_bounds__(256) void k_norm_flags(const uint32_t *__restrict__ px, uint64_t n, uint32_t *__restrict__ flags) {
    uint32_t hidden = 0, transl = 0;
    const uint64_t head = min(n, (uint64_t)(((16u - (uint32_t)((uintptr_t)px & 15u)) & 15u) >> 2));
    const uint32_t *body = px + head;
    const uint64_t nb = n - head, stride = (uint64_t)gridDim.x * blockDim.x, n4 = nb / 4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(body)[i];
        const uint32_t p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t a = p[k] >> 24;
            hidden |= (a == 0 && (p[k] & 0xFFFFFFu)) ? 1u : 0u;
            transl |= a != 255 ? 1u : 0u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {  // head pixels (threads 0..2) and tail pixels (threads 4..6)
        const uint32_t t = threadIdx.x & 3u;
        const bool tail = threadIdx.x >= 4;
        if (t < (tail ? (nb & 3) : head)) {
            const uint32_t v = tail ? body[n4 * 4 + t] : px[t], a = v >> 24;
            hidden |= (a == 0 && (v & 0xFFFFFFu)) ? 1u : 0u;
            transl |= a != 255 ? 1u : 0u;
        }
    }
    if (__ballot(hidden) && (threadIdx.x & 63) == 0) atomicOr(&flags[0], 1u);
    if (__ballot(transl) && (threadIdx.x & 63) == 0) atomicOr(&flags[1], 1u);
}

// the rewrite of the "hidden" case IN PLACE on a raster this library owns, and only when flags[0] says there is something to
// rewrite (the kernel is launched behind k_norm_flags on the same stream without the host looking at the flag in between): pixels
// with alpha 0 become 0 (libxpng.c:699-707), everything else is left alone - nothing is written for a pixel that does not change
__global__ __launch_bounds__(256) void k_norm_zero_hidden_if(const uint32_t *__restrict__ flags, uint32_t *__restrict__ px, uint64_t n) {
    if (!flags[0]) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t v = px[i];
        if ((v >> 24) == 0 && v) px[i] = 0u;
    }
}

__global__ __launch_bounds__(256) void k_norm_zero_hidden(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t v = in[i];
        out[i] = (v >> 24) ? v : 0u;
    }
}

// RGBA -> RGB: 4 pixels (one uint4) in, 3 dwords out per thread
__global__ __launch_bounds__(256) void k_norm_to_rgb(const uint32_t *__restrict__ in, uint8_t *__restrict__ out, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n4 = n / 4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(in)[i];
        const uint32_t a = v.x & 0xFFFFFFu, b = v.y & 0xFFFFFFu, c = v.z & 0xFFFFFFu, d = v.w & 0xFFFFFFu;
        uint32_t *o = reinterpret_cast<uint32_t *>(out) + 3 * i;
        o[0] = a | (b << 24); o[1] = (b >> 8) | (c << 16); o[2] = (c >> 16) | (d << 8);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const uint64_t i = n4 * 4 + threadIdx.x;
        const uint32_t v = in[i];
        out[3 * i] = (uint8_t)v; out[3 * i + 1] = (uint8_t)(v >> 8); out[3 * i + 2] = (uint8_t)(v >> 16);
    }
}

// flag[0] |= 1 if some pixel differs from pixel 0
template <int PXSZ>
__global__ __launch_bounds__(256) void k_any_differs(const uint8_t *__restrict__ p, uint64_t n, uint32_t *__restrict__ flag) {
    const uint32_t first = load_px<PXSZ>(p) & (PXSZ == 4 ? 0xFFFFFFFFu : 0xFFFFFFu);
    uint32_t diff = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t v;
        if (PXSZ == 4) v = reinterpret_cast<const uint32_t *>(p)[i];
        else v = (uint32_t)p[3 * i] | ((uint32_t)p[3 * i + 1] << 8) | ((uint32_t)p[3 * i + 2] << 16);
        diff |= v != first ? 1u : 0u;
    }
    if (__ballot(diff) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---- a list of images (xpnghip_images_*, wrappers.hpp): the same rules with the image index in blockIdx.y -------------------------
// One record per image; the flags of image i are flags[IMG_FLAGS * i + 0..2] = hidden, translucent, "some pixel differs from the
// first", and [3] = the first pixel of the normalised raster (k_any_differs_batch).
struct ImgRec {
    uint8_t *in;     // the uploaded raster, tight, 16-byte aligned; hidden colours are zeroed in place
    uint8_t *norm;   // RGBA inputs: room for the repack to RGB (npx * 3 bytes, 16-byte aligned)
    uint64_t npx;
    uint32_t pxsz_in, spare;
};
constexpr uint32_t IMG_FLAGS = 4;

// the staged (normalised) raster of an image and its bytes per pixel, from the flags k_norm_flags_batch left
__device__ __forceinline__ const uint8_t *img_cur(const ImgRec &r, const uint32_t *__restrict__ f, uint32_t &pxsz) {
    const bool repacked = r.pxsz_in == 4 && !f[0] && !f[1];
    pxsz = (r.pxsz_in == 4 && !repacked) ? 4u : 3u;
    return repacked ? r.norm : r.in;
}

// grid (blocks, nimg): k_norm_flags for every RGBA image of the list in one launch (an RGB image's workgroups return at once)
__global__ __launch_bounds__(256) void k_norm_flags_batch(const ImgRec *__restrict__ rec, uint32_t *__restrict__ flags_all) {
    const ImgRec r = rec[blockIdx.y];
    if (r.pxsz_in != 4) return;
    uint32_t *flags = flags_all + IMG_FLAGS * blockIdx.y;
    const uint32_t *px = reinterpret_cast<const uint32_t *>(r.in);
    const uint64_t n = r.npx;
    uint32_t hidden = 0, transl = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n4 = n / 4;  // (the rasters are 16-byte aligned: no head pixels)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const uint4 v = reinterpret_cast<const uint4 *>(px)[i];
        const uint32_t p[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t a = p[k] >> 24;
            hidden |= (a == 0 && (p[k] & 0xFFFFFFu)) ? 1u : 0u;
            transl |= a != 255 ? 1u : 0u;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail pixels
        const uint32_t v = px[n4 * 4 + threadIdx.x], a = v >> 24;
        hidden |= (a == 0 && (v & 0xFFFFFFu)) ? 1u : 0u;
        transl |= a != 255 ? 1u : 0u;
    }
    if (__ballot(hidden) && (threadIdx.x & 63) == 0) atomicOr(&flags[0], 1u);
    if (__ballot(transl) && (threadIdx.x & 63) == 0) atomicOr(&flags[1], 1u);
}

// grid (blocks, nimg), launched behind k_norm_flags_batch on the same stream: the rewrite each image's flags ask for, decided on
// the device (the host reads the flags once, for the whole list, and only to learn the pixel sizes).  hidden: pixels with alpha 0
// become 0 in place (k_norm_zero_hidden_if); no translucent pixel: repack to RGB into norm (k_norm_to_rgb); else nothing.
__global__ __launch_bounds__(256) void k_norm_rewrite_batch(const ImgRec *__restrict__ rec, const uint32_t *__restrict__ flags_all) {
    const ImgRec r = rec[blockIdx.y];
    if (r.pxsz_in != 4) return;
    const uint32_t *flags = flags_all + IMG_FLAGS * blockIdx.y;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, n = r.npx, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t *px = reinterpret_cast<uint32_t *>(r.in);
    if (flags[0]) {
        for (uint64_t i = first; i < n; i += stride) {
            const uint32_t v = px[i];
            if ((v >> 24) == 0 && v) px[i] = 0u;
        }
    } else if (!flags[1]) {
        const uint64_t n4 = n / 4;
        for (uint64_t i = first; i < n4; i += stride) {
            const uint4 v = reinterpret_cast<const uint4 *>(px)[i];
            const uint32_t a = v.x & 0xFFFFFFu, b = v.y & 0xFFFFFFu, c = v.z & 0xFFFFFFu, d = v.w & 0xFFFFFFu;
            uint32_t *o = reinterpret_cast<uint32_t *>(r.norm) + 3 * i;
            o[0] = a | (b << 24); o[1] = (b >> 8) | (c << 16); o[2] = (c >> 16) | (d << 8);
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
            const uint64_t i = n4 * 4 + threadIdx.x;
            const uint32_t v = px[i];
            r.norm[3 * i] = (uint8_t)v; r.norm[3 * i + 1] = (uint8_t)(v >> 8); r.norm[3 * i + 2] = (uint8_t)(v >> 16);
        }
    }
}

// grid (blocks, nimg): the whole-image single-colour test (k_any_differs) of every normalised raster of the list
__global__ __launch_bounds__(256) void k_any_differs_batch(const ImgRec *__restrict__ rec, uint32_t *__restrict__ flags_all) {
    const ImgRec r = rec[blockIdx.y];
    uint32_t *flags = flags_all + IMG_FLAGS * blockIdx.y;
    uint32_t pxsz;
    const uint8_t *p = img_cur(r, flags, pxsz);
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t diff = 0;
    if (pxsz == 4) {
        const uint32_t v0 = reinterpret_cast<const uint32_t *>(p)[0];
        for (uint64_t i = first; i < r.npx; i += stride) diff |= reinterpret_cast<const uint32_t *>(p)[i] != v0 ? 1u : 0u;
    } else {
        const uint32_t v0 = load_px<3>(p);
        for (uint64_t i = first; i < r.npx; i += stride) diff |= load_px<3>(p + 3 * i) != v0 ? 1u : 0u;
    }
    if (__ballot(diff) && (threadIdx.x & 63) == 0) atomicOr(&flags[2], 1u);
    // the first pixel travels with the flags: a single-colour file holds nothing else, so the host never fetches that raster
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[3] = pxsz == 4 ? reinterpret_cast<const uint32_t *>(p)[0] : load_px<3>(p);
}

}  // namespace xpng
