// mixed_float.hpp -- the copy-out pass of a mixed-size decode that converts while it rearranges: staging raster -> planar or
// interleaved, RGB or BGR, 3 or 4 channels of f16, bf16 or f32 (xpnghip_decode_varsize_device_batch_as_float).
//
// For every output element, with v the stored byte and c the channel's position in the caller's buffer:
//     y = fmaf((float)v, scale[c], bias[c])      one fp32 fused multiply-add, subnormals kept
//     out = (T)y                                 round to nearest even (f32: y itself)
// The alpha an RGB context does not store is v = 255 through the same formula with c = 3.  The arithmetic of the host's table
// (xpnghip_float_table in xpng_hip.hip) is the same, so a byte answered from that table is bit for bit what this kernel writes.
#pragma once
#include <stdint.h>

#include "mixed.hpp"

namespace xpng {

// ---- the device operations of the kernel below, each behind a small named function: tests/float_kernels_host.cpp replaces every
// ---- one of them with a host shim that also checks it (the text from "float layouts" on is what that program compiles)
// fmaf as a value of its own: one v_fma_f32 (or half a v_pk_fma_f32).  The empty asm keeps the compiler from fusing the multiply-add
// with the narrowing that follows into v_fma_mixlo_f16; the rule is an fp32 result, then a conversion.
__device__ __forceinline__ float fma_f32(float v, float s, float b) {
    float y = __builtin_fmaf(v, s, b);
    asm("" : "+v"(y));
    return y;
}
// two floats -> two halves / two bfloat16 in one dword (lo in bits 0..15), each rounded to nearest even.  NOT v_cvt_pkrtz_f16_f32,
// which rounds toward zero.
__device__ __forceinline__ uint32_t cvt_pk_f16_rne(float lo, float hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = {(_Float16)lo, (_Float16)hi};  // fptrunc: v_cvt_f16_f32 / v_cvt_pk_f16_f32
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint32_t cvt_pk_bf16_rne(float lo, float hi) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));  // (no builtin)
    return r;
}

// 12 and 16 bytes at a dword-aligned address
struct __attribute__((aligned(4))) Dw3 {
    uint32_t x, y, z;
};
// the kernel's own reads of the staging raster (ld32u beside them): the host program checks every one against the read rule
__device__ __forceinline__ Dw4 stage_ld128(const uint8_t *p) { return *reinterpret_cast<const Dw4 *>(p); }
__device__ __forceinline__ Dw3 stage_ld96(const uint8_t *p) { return *reinterpret_cast<const Dw3 *>(p); }
__device__ __forceinline__ uint32_t stage_ld32(const uint8_t *p) { return *reinterpret_cast<const uint32_t *>(p); }
__device__ __forceinline__ uint32_t stage_ld8(const uint8_t *p) { return *p; }
// ... and its writes of the caller's buffer, which is global memory (a pointer read from a record is a flat one to the compiler):
// global_store_dwordx4, _dword, _short
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void out_st128(uint8_t *p, uint4 v) { *(__attribute__((address_space(1))) u32x4_t *)p = u32x4_t{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ void out_st32(uint8_t *p, uint32_t v) { *(__attribute__((address_space(1))) uint32_t *)p = v; }
__device__ __forceinline__ void out_st16(uint8_t *p, uint32_t v) { *(__attribute__((address_space(1))) uint16_t *)p = (uint16_t)v; }

// ---- float layouts ----------------------------------------------------------------------------------------------------------
// the constants of a call, by value in the kernel's arguments: scale[c], bias[c] for channel position c of the caller's buffer
struct FloatConsts {
    float scale[4], bias[4];
};
// the element types of the caller's buffer: f16 and bf16 by their bits, f32 as itself
struct f16_t {
    uint16_t bits;
};
struct bf16_t {
    uint16_t bits;
};
template <class T> struct FloatElem { static constexpr int KIND = 3; };
template <> struct FloatElem<f16_t> { static constexpr int KIND = 1; };
template <> struct FloatElem<bf16_t> { static constexpr int KIND = 2; };

// a[i] for a run-time i without indexing memory (the constants live in SGPRs; a lane-varying i becomes v_cndmask)
__device__ __forceinline__ float pick4(const float (&a)[4], uint32_t i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }
// byte i of x as a float: v_cvt_f32_ubyte<i>
template <int I> __device__ __forceinline__ float ubf(uint32_t x) { return (float)((x >> (8 * I)) & 0xffu); }

template <class T> __device__ __forceinline__ uint32_t narrow2(float lo, float hi) {
    if constexpr (FloatElem<T>::KIND == 1) return cvt_pk_f16_rne(lo, hi);
    else return cvt_pk_bf16_rne(lo, hi);
}
// element j of the row at d
template <class T> __device__ __forceinline__ void store1(uint8_t *d, uint32_t j, float y) {
    if constexpr (sizeof(T) == 4) out_st32(d + 4ull * j, __builtin_bit_cast(uint32_t, y));
    else out_st16(d + 2ull * j, narrow2<T>(y, 0.0f));
}
// the 16 / sizeof(T) elements of one aligned 16-byte store: element i is fmaf(v[i], sa[i % P], ba[i % P]) (P = 1: one channel,
// planar; P = C: interleaved, sa / ba already rotated to the chunk's first element)
template <class T, int P> __device__ __forceinline__ uint4 float_chunk(const float (&v)[8], const float (&sa)[4], const float (&ba)[4]) {
    constexpr int N = 16 / sizeof(T);
    float y[8];
#pragma unroll
    for (int i = 0; i < N; i++) y[i] = fma_f32(v[i], sa[i % P], ba[i % P]);
    uint4 o;
    if constexpr (sizeof(T) == 4) {
        o.x = __builtin_bit_cast(uint32_t, y[0]); o.y = __builtin_bit_cast(uint32_t, y[1]);
        o.z = __builtin_bit_cast(uint32_t, y[2]); o.w = __builtin_bit_cast(uint32_t, y[3]);
    } else {
        o.x = narrow2<T>(y[0], y[1]); o.y = narrow2<T>(y[2], y[3]);
        o.z = narrow2<T>(y[4], y[5]); o.w = narrow2<T>(y[6], y[7]);
    }
    return o;
}

// grid (ceil(tallest image / MC_ROWS), nimg), 256 threads; PX, C, PLANAR and bgr as in k_mixed_copy_as, T = f16_t | bf16_t | float the
// element of the caller's buffer, E = 16 / sizeof(T) elements per aligned 16-byte store.  Each of the block's four waves takes
// whole rows (interleaved) or whole plane rows (planar), so head, alignment and constants are wave-uniform.  The caller's rows
// start at every multiple of sizeof(T): a row is written as a head of fewer than E single elements, whole ALIGNED 16-byte stores
// (global_store_dwordx4; lane k of a pass takes store k, so a wave writes 1 KiB back to back) and a tail of fewer than E elements.
//   planar       row y of plane c is w elements at buf + ((c * h + y) * w) * sizeof(T).  A store takes the channel's byte of E
//                neighbouring pixels.  RGBA: one or two 16-byte loads, the byte cut out by a shift.  RGB: the E * 3 bytes start at
//                any byte, so the 4 or 7 dwords around them are loaded and v_alignbyte puts the channel's byte of the first pixel at
//                byte 0 - the bytes are then at the fixed places 0, 3, 6 .. and each is one v_cvt_f32_ubyte<n>.  The alpha plane of
//                an RGB context is a fill with T(fmaf(255, scale[3], bias[3])).
//   interleaved  row y is w * C elements at buf + y * w * C * sizeof(T).  A store starts at byte rr of pixel p of the caller's
//                byte stream; the two to four pixels it covers are loaded as in k_mixed_copy_as (a dword each, RGB: ld32u, put into
//                the caller's order by one v_perm) and v_alignbyte cuts the E bytes out of them.  The constants are rotated by rr:
//                wave-uniform for C == 4, per lane for C == 3.
// Exactly C * w * h * sizeof(T) bytes of buf are written.  The loads reach at most 7 bytes behind a staging row's last pixel: the
// pitch's padding, the next row, or the 256 spare bytes behind the last slot.
template <int PX, int C, bool PLANAR, class T>
__global__ __launch_bounds__(256) void k_mixed_copy_as_float(const MixedLayout *__restrict__ ml, const uint8_t *__restrict__ stage, uint64_t stage_bpr,
                                                             uint32_t bgr, FloatConsts k) {
    constexpr uint32_t ES = sizeof(T), E = 16 / ES;
    const MixedLayout r = ml[blockIdx.y];
    const uint32_t y0 = blockIdx.x * MC_ROWS;
    if (y0 >= r.h) return;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t rows = r.h - y0 < MC_ROWS ? r.h - y0 : MC_ROWS;
    if constexpr (PLANAR) {
        const uint64_t plane = (uint64_t)r.w * r.h;
        for (uint32_t it = wv; it < rows * C; it += 4) {
            const uint32_t y = y0 + it / C, c = it % C;
            const uint8_t *s = stage + r.stage + (uint64_t)y * stage_bpr;
            uint8_t *d = r.buf + ((uint64_t)c * plane + (uint64_t)y * r.w) * ES;
            uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
            if (head > r.w) head = r.w;
            const uint32_t nq = (r.w - head) / E, tail0 = head + E * nq;
            uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned
            const float sa[4] = {pick4(k.scale, c), 0, 0, 0}, ba[4] = {pick4(k.bias, c), 0, 0, 0};
            if (PX == 3 && c == 3) {  // the alpha an RGB file does not store
                const float v[8] = {255.0f, 255.0f, 255.0f, 255.0f, 255.0f, 255.0f, 255.0f, 255.0f};
                const uint4 o = float_chunk<T, 1>(v, sa, ba);
                const float a = fma_f32(255.0f, sa[0], ba[0]);
                if (lane < head) store1<T>(d, lane, a);
                for (uint32_t q = lane; q < nq; q += 64) out_st128(d16 + 16ull * q, o);
                if (tail0 + lane < r.w) store1<T>(d, tail0 + lane, a);
                continue;
            }
            const uint32_t sc = bgr && c < 3 ? 2 - c : c;  // the channel's byte inside a staging pixel
            if (lane < head) store1<T>(d, lane, fma_f32((float)stage_ld8(s + lane * PX + sc), sa[0], ba[0]));
            if (tail0 + lane < r.w) store1<T>(d, tail0 + lane, fma_f32((float)stage_ld8(s + (tail0 + lane) * PX + sc), sa[0], ba[0]));
            if constexpr (PX == 4) {
                const uint8_t *g = s + 4 * head;
                const uint32_t sh8 = 8 * sc;
                for (uint32_t q = lane; q < nq; q += 64) {
                    float v[8] = {};
                    const Dw4 a = stage_ld128(g + (uint64_t)(4 * E) * q);
                    v[0] = ubf<0>(a.x >> sh8); v[1] = ubf<0>(a.y >> sh8); v[2] = ubf<0>(a.z >> sh8); v[3] = ubf<0>(a.w >> sh8);
                    if constexpr (E == 8) {
                        const Dw4 b = stage_ld128(g + (uint64_t)(4 * E) * q + 16);
                        v[4] = ubf<0>(b.x >> sh8); v[5] = ubf<0>(b.y >> sh8); v[6] = ubf<0>(b.z >> sh8); v[7] = ubf<0>(b.w >> sh8);
                    }
                    out_st128(d16 + 16ull * q, float_chunk<T, 1>(v, sa, ba));
                }
            } else {
                // E pixels = 3 * E bytes with the channel at sc, sc + 3, ..: start the window AT the channel's first byte, so that
                // after v_alignbyte the bytes sit at 0, 3, 6, .. of D0 D1 ..  3 * E bytes per store keep the alignment for the row.
                // The window ends 4 - sh + sc <= 6 bytes behind the store's last pixel.
                const uint8_t *g = s + 3 * head + sc;
                const uint32_t sh = (uint32_t)((uintptr_t)g & 3);
                g -= sh;
                for (uint32_t q = lane; q < nq; q += 64) {
                    float v[8] = {};
                    const Dw4 a = stage_ld128(g + (uint64_t)(3 * E) * q);
                    const uint32_t D0 = __builtin_amdgcn_alignbyte(a.y, a.x, sh), D1 = __builtin_amdgcn_alignbyte(a.z, a.y, sh),
                                   D2 = __builtin_amdgcn_alignbyte(a.w, a.z, sh);
                    v[0] = ubf<0>(D0); v[1] = ubf<3>(D0); v[2] = ubf<2>(D1); v[3] = ubf<1>(D2);
                    if constexpr (E == 8) {
                        const Dw3 b = stage_ld96(g + (uint64_t)(3 * E) * q + 16);
                        const uint32_t D3 = __builtin_amdgcn_alignbyte(b.x, a.w, sh), D4 = __builtin_amdgcn_alignbyte(b.y, b.x, sh),
                                       D5 = __builtin_amdgcn_alignbyte(b.z, b.y, sh);
                        v[4] = ubf<0>(D3); v[5] = ubf<3>(D3); v[6] = ubf<2>(D4); v[7] = ubf<1>(D5);
                    }
                    out_st128(d16 + 16ull * q, float_chunk<T, 1>(v, sa, ba));
                }
            }
        }
    } else {
        // a staging pixel as the caller's pixel P: bytes 0..2 the colours in the caller's order, byte 3 the alpha of an RGBA
        // context, 255 (C == 4 on RGB: selector 0x0d) or 0 (C == 3: selector 0x0c)
        const uint32_t sel = (bgr ? 0x00000102u : 0x00020100u) | (C == 3 ? 0x0c000000u : PX == 4 ? 0x03000000u : 0x0d000000u);
        const uint32_t row_el = r.w * C;
        for (uint32_t it = wv; it < rows; it += 4) {
            const uint32_t y = y0 + it;
            const uint8_t *s = stage + r.stage + (uint64_t)y * stage_bpr;
            uint8_t *d = r.buf + (uint64_t)y * row_el * ES;
            auto P = [&](uint32_t p) {
                const uint32_t x = PX == 4 ? stage_ld32(s + 4 * p) : ld32u(s + 3 * p);
                return __builtin_amdgcn_perm(0u, x, sel);
            };
            auto one = [&](uint32_t j) {  // element j of the row
                const uint32_t p = j / C, c = j - p * C;
                return fma_f32(ubf<0>(P(p) >> (8 * c)), pick4(k.scale, c), pick4(k.bias, c));
            };
            uint32_t head = ((16u - (uint32_t)((uintptr_t)d & 15)) & 15u) / ES;
            if (head > row_el) head = row_el;
            const uint32_t nq = (row_el - head) / E, tail0 = head + E * nq;
            uint8_t *d16 = d + (uint64_t)head * ES;  // 16-byte aligned
            if (lane < head) store1<T>(d, lane, one(lane));
            if (tail0 + lane < row_el) store1<T>(d, tail0 + lane, one(tail0 + lane));
            for (uint32_t q = lane; q < nq; q += 64) {
                const uint32_t j = head + E * q, p = j / C, rr = j - p * C;  // the store starts at byte rr of pixel p
                float sa[4] = {}, ba[4] = {};
#pragma unroll
                for (uint32_t i = 0; i < (uint32_t)C; i++) {
                    const uint32_t c = rr + i < (uint32_t)C ? rr + i : rr + i - C;
                    sa[i] = pick4(k.scale, c); ba[i] = pick4(k.bias, c);
                }
                // S0 S1 (S2): the caller's byte stream from pixel p on; B0 (B1): the store's E bytes
                uint32_t S0, S1, S2 = 0, B0, B1 = 0;
                if constexpr (C == 4) {
                    S0 = P(p); S1 = P(p + 1);
                    if constexpr (E == 8) S2 = P(p + 2);
                } else {
                    const uint32_t t0 = P(p), t1 = P(p + 1);
                    S0 = t0 | (t1 << 24); S1 = t1 >> 8;
                    if constexpr (E == 8) {
                        const uint32_t t2 = P(p + 2), t3 = P(p + 3);
                        S1 |= t2 << 16; S2 = (t2 >> 16) | (t3 << 8);
                    }
                }
                B0 = __builtin_amdgcn_alignbyte(S1, S0, rr);
                if constexpr (E == 8) B1 = __builtin_amdgcn_alignbyte(S2, S1, rr);
                float v[8] = {};
                v[0] = ubf<0>(B0); v[1] = ubf<1>(B0); v[2] = ubf<2>(B0); v[3] = ubf<3>(B0);
                if constexpr (E == 8) { v[4] = ubf<0>(B1); v[5] = ubf<1>(B1); v[6] = ubf<2>(B1); v[7] = ubf<3>(B1); }
                out_st128(d16 + 16ull * q, float_chunk<T, C>(v, sa, ba));
            }
        }
    }
}

}  // namespace xpng
