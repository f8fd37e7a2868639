// stage_from.hpp -- fills the rasters of a staged batch (xpnghip_images_begin_device, wrappers.hpp) from the caller's device tensors:
// planar or interleaved, RGB or BGR, uint8, f16, bf16 or f32 -> the interleaved R,G,B[,A] bytes the batch normalises and encodes
// (DESIGN.md 18).  The mirror of mixed_float.hpp.
//
// For every element x of the caller's buffer, with c the channel's position in that buffer (alpha last; with bgr scale[0] belongs
// to blue):
//     y = fmaf((float)x, scale[c], bias[c])      f16 / bf16 widened exactly; one fp32 fused multiply-add, subnormals kept
//     v = 0 if y is NaN or y <= 0,  255 if y >= 255,  else (uint8_t)rintf(y)      round half to even
// A uint8 buffer holds v itself.  xpnghip_quantize_host (xpng_hip.hip) is the same arithmetic on the host.
#pragma once
#include <stdint.h>

#include "mixed_float.hpp"
#include "normalize.hpp"

namespace xpng {

// ---- the device operations of the kernel below, each behind a small named function: tests/quant_kernels_host.cpp replaces every
// ---- one of them with a host shim that also checks it (the text from "staging from tensors" on is what that program compiles;
// ---- fma_f32 is mixed_float.hpp's)
// the kernel's reads of the caller's buffer, which is global memory (a pointer read from a table is a flat one to the compiler).
// The wide ones need only dword alignment: global_load_dwordx4 / _dwordx2 / _dword, _ushort, _ubyte
typedef u32x4_t u32x4_a4_t __attribute__((aligned(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef u32x2_t u32x2_a4_t __attribute__((aligned(4)));
__device__ __forceinline__ uint4 src_ld128(const uint8_t *p) {
    const u32x4_t v = *(const __attribute__((address_space(1))) u32x4_a4_t *)p;
    return uint4{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ uint2 src_ld64(const uint8_t *p) {
    const u32x2_t v = *(const __attribute__((address_space(1))) u32x2_a4_t *)p;
    return uint2{v.x, v.y};
}
__device__ __forceinline__ uint32_t src_ld32(const uint8_t *p) { return *(const __attribute__((address_space(1))) uint32_t *)p; }
__device__ __forceinline__ uint32_t src_ld16(const uint8_t *p) { return *(const __attribute__((address_space(1))) uint16_t *)p; }
__device__ __forceinline__ uint32_t src_ld8(const uint8_t *p) { return *(const __attribute__((address_space(1))) uint8_t *)p; }
// ... and its writes of the staged raster: 16 and 12 bytes at a dword-aligned address, single bytes for the last npx & 3 pixels
__device__ __forceinline__ void stg_st128(uint8_t *p, uint4 v) { *(__attribute__((address_space(1))) u32x4_t *)p = u32x4_t{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void stg_st96(uint8_t *p, uint32_t a, uint32_t b, uint32_t c) {
    __attribute__((address_space(1))) uint32_t *o = (__attribute__((address_space(1))) uint32_t *)p;
    o[0] = a; o[1] = b; o[2] = c;
}
__device__ __forceinline__ void stg_st8(uint8_t *p, uint32_t v) { *(__attribute__((address_space(1))) uint8_t *)p = (uint8_t)v; }
// the bits of an f16 / a bf16 (in bits 0..15) widened to fp32: exact, subnormals kept (v_cvt_f32_f16; a shift)
__device__ __forceinline__ float cvt_f32_f16(uint32_t bits) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits); }
__device__ __forceinline__ float cvt_f32_bf16(uint32_t bits) { return __builtin_bit_cast(float, bits << 16); }
// the quantisation of the rule.  Two ordered compares, so a NaN fails both and leaves as 0 with -0 and -inf; v_rndne_f32 rounds
// half to even whatever the rounding mode of the conversion that follows
__device__ __forceinline__ uint32_t quant_u8(float y) {
    const float hi = y >= 255.0f ? 255.0f : y;
    const float c = hi > 0.0f ? hi : 0.0f;
    return (uint32_t)__builtin_rintf(c);
}

// ---- staging from tensors ---------------------------------------------------------------------------------------------------
// ND dwords from the dword-aligned q: the widest loads first
template <int ND> __device__ __forceinline__ void src_dwords(const uint8_t *q, uint32_t *w) {
    if constexpr (ND >= 4) {
        const uint4 v = src_ld128(q);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        src_dwords<ND - 4>(q + 16, w + 4);
    } else if constexpr (ND >= 2) {
        const uint2 v = src_ld64(q);
        w[0] = v.x; w[1] = v.y;
        src_dwords<ND - 2>(q + 8, w + 2);
    } else if constexpr (ND == 1) {
        w[0] = src_ld32(q);
    }
}
// the 4 * ND bytes at a, which is aligned to the ES bytes of an element only: the aligned dwords that hold them - ND of them, one
// more when a is not dword-aligned, and then that one holds a byte of the window too - and v_alignbyte puts the first byte at
// byte 0.  So nothing outside the aligned dwords the caller's buffer occupies is read.  (a & 3 is the same for every group of an
// image's plane, so the branch is uniform.)
template <int ND, int ES> __device__ __forceinline__ void src_window(const uint8_t *a, uint32_t (&d)[ND]) {
    if constexpr (ES == 4) {
        src_dwords<ND>(a, d);
    } else {
        const uint32_t sh = (uint32_t)((uintptr_t)a & 3u);
        const uint8_t *q = a - sh;
        uint32_t w[ND + 1];
        src_dwords<ND>(q, w);
        w[ND] = sh ? src_ld32(q + 4 * ND) : 0u;
#pragma unroll
        for (int i = 0; i < ND; i++) d[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
    }
}
// the stored byte for the element x of a float buffer
__device__ __forceinline__ uint32_t quant_x(float x, float s, float b) { return quant_u8(fma_f32(x, s, b)); }
// ... for element j of a window (a uint8 buffer holds the byte itself)
template <class T> __device__ __forceinline__ uint32_t quant_at(const uint32_t *d, int j, float s, float b) {
    if constexpr (sizeof(T) == 1) return (d[j / 4] >> (8 * (j % 4))) & 0xffu;
    else if constexpr (FloatElem<T>::KIND == 1) return quant_x(cvt_f32_f16((d[j / 2] >> (16 * (j % 2))) & 0xffffu), s, b);
    else if constexpr (FloatElem<T>::KIND == 2) return quant_x(cvt_f32_bf16((d[j / 2] >> (16 * (j % 2))) & 0xffffu), s, b);
    else return quant_x(__builtin_bit_cast(float, d[j]), s, b);
}
// ... for the single element at p
template <class T> __device__ __forceinline__ uint32_t quant_one(const uint8_t *p, float s, float b) {
    if constexpr (sizeof(T) == 1) return src_ld8(p);
    else if constexpr (FloatElem<T>::KIND == 1) return quant_x(cvt_f32_f16(src_ld16(p)), s, b);
    else if constexpr (FloatElem<T>::KIND == 2) return quant_x(cvt_f32_bf16(src_ld16(p)), s, b);
    else return quant_x(__builtin_bit_cast(float, src_ld32(p)), s, b);
}

// grid (blocks, nimg), 256 threads, grid-stride, the image in blockIdx.y as in k_norm_flags_batch; C = 3 | 4 channels of the
// caller's buffer = bytes per pixel of the staged raster (a workgroup of an image of the other kind returns at once), PLANAR as in
// k_mixed_pack_from, T = uint8_t | f16_t | bf16_t | float the element of the caller's buffer.  Source and destination are both
// tight, so rows do not matter: image i is a flat transform of npx pixels from srcs[i] (C * npx elements, aligned to the element)
// to rec[i].in (npx * C bytes, 16-byte aligned).  A lane takes groups of four pixels - one 12- or 16-byte store at a dword-aligned
// offset - and the npx & 3 pixels behind the last group are written byte by byte.
//   planar       plane c is npx elements at src + c * npx * sizeof(T); a group is one window of four neighbouring elements per plane
//   interleaved  a group is one window of 4 * C consecutive elements
// READS: windows (src_window) and single elements of the buffer.  WRITES: exactly npx * C bytes of the image's raster.
template <int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_images_stage_from(const ImgRec *__restrict__ rec, const uint8_t *const *__restrict__ srcs, uint32_t bgr, FloatConsts k) {
    constexpr int ES = sizeof(T);
    const ImgRec r = rec[blockIdx.y];
    if (r.pxsz_in != (uint32_t)C) return;
    const uint8_t *src = srcs[blockIdx.y];
    const uint64_t n = r.npx, n4 = n / 4, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += stride) {
        uint32_t q[4][C];  // [pixel of the group][channel position in the caller's buffer]
        if constexpr (PLANAR) {
#pragma unroll
            for (int c = 0; c < C; c++) {
                uint32_t d[ES];
                src_window<ES, ES>(src + ((uint64_t)c * n + 4 * g) * ES, d);
#pragma unroll
                for (int p = 0; p < 4; p++) q[p][c] = quant_at<T>(d, p, k.scale[c], k.bias[c]);
            }
        } else {
            uint32_t d[C * ES];
            src_window<C * ES, ES>(src + g * (uint64_t)(4 * C * ES), d);
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int c = 0; c < C; c++) q[p][c] = quant_at<T>(d, p * C + c, k.scale[c], k.bias[c]);
        }
        uint32_t P[4];  // the pixels as R | G << 8 | B << 16 [| A << 24]
#pragma unroll
        for (int p = 0; p < 4; p++) {
            P[p] = (bgr ? q[p][2] : q[p][0]) | (q[p][1] << 8) | ((bgr ? q[p][0] : q[p][2]) << 16);
            if constexpr (C == 4) P[p] |= q[p][3] << 24;
        }
        uint8_t *o = r.in + g * (uint64_t)(4 * C);
        if constexpr (C == 4) stg_st128(o, uint4{P[0], P[1], P[2], P[3]});
        else stg_st96(o, P[0] | (P[1] << 24), (P[1] >> 8) | (P[2] << 16), (P[2] >> 16) | (P[3] << 8));
    }
    if (blockIdx.x == 0 && threadIdx.x < (uint32_t)(n & 3) * C) {  // tail pixels, a byte per lane
        const uint32_t c = threadIdx.x % C, cc = bgr && c < 3 ? 2 - c : c;  // cc: the channel's position in the caller's buffer
        const uint64_t p = 4 * n4 + threadIdx.x / C, e = PLANAR ? (uint64_t)cc * n + p : p * C + cc;
        stg_st8(r.in + p * C + c, quant_one<T>(src + e * ES, pick4(k.scale, cc), pick4(k.bias, cc)));
    }
}

}  // namespace xpng
