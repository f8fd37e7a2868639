// What the host-run kernel programs of tests/ (*_kernels_host.cpp, pixel_transform_host.cpp) share: the launch shim that runs every
// thread of every block one after another, the error count, the byte shims of v_perm and v_alignbyte and - for the programs that
// ask for them with KERNEL_HOST_FLOAT_OPS - the checked reads of the staging raster, the checked stores into the caller's buffers
// and the round-to-nearest-even narrowing of the float copy-out kernels.  Which read is allowed is each program's own rule
// (chk_read), and so is its statement of the expected values.
// The product's own records and element types are never declared here or in a program: the test cuts their text out of the
// product headers and names the file in TYPES_TEXT, so a change of a record reaches the programs with the kernels'.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
struct D3 { uint32_t x, y, z; };
static D3 blockIdx, threadIdx, gridDim, blockDim;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
static int errors = 0;
static void bad(const char *what, long a, long b) { if (errors++ < 20) printf("%s %ld %ld\n", what, a, b); }
static uint64_t rup(uint64_t a, uint64_t b) { return (a + b - 1) / b * b; }
template <class F> static void launch(uint32_t gx, uint32_t gy, F f) {
    gridDim = {gx, gy, 1}; blockDim = {256, 1, 1};
    for (uint32_t y = 0; y < gy; y++) for (uint32_t x = 0; x < gx; x++) for (uint32_t t = 0; t < 256; t++) { blockIdx = {x, y, 0}; threadIdx = {t, 0, 0}; f(); }
}

static uint32_t bperm(uint32_t a, uint32_t b, uint32_t sel) {
    uint64_t in = ((uint64_t)a << 32) | b; uint32_t o = 0;
    for (int i = 0; i < 4; i++) { uint32_t s = (sel >> (8 * i)) & 0xff, v;
        if (s < 8) v = (in >> (8 * s)) & 0xff; else if (s == 0x0c) v = 0; else if (s >= 0x0d) v = 0xff; else { puts("sign selector"); abort(); }
        o |= v << (8 * i); }
    return o;
}
#define __builtin_amdgcn_perm bperm
static uint32_t balign(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3))); }
#define __builtin_amdgcn_alignbyte balign
static float fma_f32(float v, float s, float b) { return fmaf(v, s, b); }

#ifdef TYPES_TEXT
#include TYPES_TEXT  // the records and element types of the product that the program itself names, cut out of the product headers
#endif

#ifdef KERNEL_HOST_FLOAT_OPS
// ---- the staging reads: every one goes through the program's read rule
static void chk_read(const uint8_t *p, uint32_t n, uint32_t align);
static Dw4 stage_ld128(const uint8_t *p) { chk_read(p, 16, 4); Dw4 v; memcpy(&v, p, 16); return v; }
static Dw3 stage_ld96(const uint8_t *p) { chk_read(p, 12, 4); Dw3 v; memcpy(&v, p, 12); return v; }
static uint32_t stage_ld32(const uint8_t *p) { chk_read(p, 4, 4); uint32_t v; memcpy(&v, p, 4); return v; }
static uint32_t stage_ld8(const uint8_t *p) { chk_read(p, 1, 1); return *p; }
static uint32_t ld32u(const uint8_t *p) {
    uintptr_t a = (uintptr_t)p; const uint8_t *q = (const uint8_t *)(a & ~(uintptr_t)3); uint32_t sh = (a & 3) * 8;
    uint32_t lo = stage_ld32(q); if (!sh) return lo; return (lo >> sh) | (stage_ld32(q + 4) << (32 - sh));
}
// ---- the caller's buffers: a store must lie inside one of them and be aligned to its width
static std::vector<std::pair<uint8_t *, uint8_t *>> g_out;
static void chk_store(uint8_t *p, uint32_t n) {
    if ((uintptr_t)p % n) bad("misaligned store", (long)((uintptr_t)p & 15), n);
    for (auto &r : g_out) if (p >= r.first && p + n <= r.second) return;
    bad("store outside every buffer", 0, n); abort();
}
static void out_st128(uint8_t *p, uint4 v) { chk_store(p, 16); memcpy(p, &v, 16); }
static void out_st32(uint8_t *p, uint32_t v) { chk_store(p, 4); memcpy(p, &v, 4); }
static void out_st16(uint8_t *p, uint32_t v) { chk_store(p, 2); uint16_t h = (uint16_t)v; memcpy(p, &h, 2); }
// ---- round-to-nearest-even conversions, written out on the bits: the tests' own arithmetic, independent of the product's
static uint16_t to_bf16(float f) {
    uint32_t x; memcpy(&x, &f, 4);
    if ((x & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((x >> 16) | 0x40);
    return (uint16_t)((x + 0x7fffu + ((x >> 16) & 1)) >> 16);
}
static uint16_t to_f16(float f) {  // by value: scale into the f16 grid with exact double arithmetic, round with nearbyint (ties to even)
    uint32_t x; memcpy(&x, &f, 4);
    const uint16_t sign = (x >> 16) & 0x8000u;
    const double a = fabs((double)f);
    if (std::isnan(f)) return sign | 0x7e00;
    if (a >= 65520.0) return sign | 0x7c00;
    if (a < 6.103515625e-05) return sign | (uint16_t)nearbyint(a * 16777216.0);  // subnormal: units of 2^-24 (1024 = the smallest normal)
    int e; frexp(a, &e);  // a = m * 2^e, m in [0.5, 1)
    const double q = nearbyint(ldexp(a, 11 - e));  // 1024 .. 2048
    return sign | (uint16_t)(((e - 1 + 15) << 10) + ((int)q - 1024));  // (q == 2048 carries into the exponent)
}
static uint32_t cvt_pk_f16_rne(float lo, float hi) { return to_f16(lo) | ((uint32_t)to_f16(hi) << 16); }
static uint32_t cvt_pk_bf16_rne(float lo, float hi) { return to_bf16(lo) | ((uint32_t)to_bf16(hi) << 16); }
#endif
