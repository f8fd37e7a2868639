// Host run of k_images_stage_from (xpng_amd/csrc/stage_from.hpp): every thread of every block, one after another, for all 16
// instances (C 3 | 4, planar | interleaved, uint8 | f16 | bf16 | f32) and both colour orders, with shims for the device operations
// the kernel uses.  The shims of the reads check the read rule (aligned to their width - the wide ones to a dword - and inside the
// aligned dwords the image's buffer occupies), the shims of the stores check that every store is dword-aligned (the tail: single
// bytes) and inside the image's slot of the staged raster; sources and rasters live in sentinel-framed heap blocks, so
// AddressSanitizer sees anything else.  The widening and the quantisation shims are this file's own; the expected value of every
// byte is the rule of include/xpng_hip.h computed with fmaf().
// Built and run by tests/test_quant_kernels_host.py: g++ -fsanitize=address -static-libasan -DKERNEL_TEXT=\"...\".
#include "kernel_host.hpp"  // the launch shim, v_alignbyte, fma_f32; TYPES_TEXT: FloatConsts, the element types and pick4 (mixed_float.hpp)
struct ImgRec { uint8_t *in; uint8_t *norm; uint64_t npx; uint32_t pxsz_in, spare; };

// ---- the images of the launch: the shims look the running image up by blockIdx.y
struct Img { const uint8_t *src; uint64_t src_bytes; uint8_t *dst; uint64_t dst_bytes; };
static std::vector<Img> g_img;
static void chk_read(const uint8_t *p, uint32_t n, uint32_t align) {
    const Img &m = g_img[blockIdx.y];
    if ((uintptr_t)p % align) bad("misaligned read", (long)(p - m.src), align);
    const uintptr_t lo = (uintptr_t)m.src & ~(uintptr_t)3, hi = ((uintptr_t)m.src + m.src_bytes + 3) & ~(uintptr_t)3;  // the aligned dwords the buffer occupies
    if ((uintptr_t)p < lo || (uintptr_t)p + n > hi) { printf("read outside the buffer's dwords: image %u, %ld + %u of %lu\n", blockIdx.y, (long)(p - m.src), n, (unsigned long)m.src_bytes); fflush(stdout); abort(); }
}
static uint4 src_ld128(const uint8_t *p) { chk_read(p, 16, 4); uint4 v; memcpy(&v, p, 16); return v; }
static uint2 src_ld64(const uint8_t *p) { chk_read(p, 8, 4); uint2 v; memcpy(&v, p, 8); return v; }
static uint32_t src_ld32(const uint8_t *p) { chk_read(p, 4, 4); uint32_t v; memcpy(&v, p, 4); return v; }
static uint32_t src_ld16(const uint8_t *p) { chk_read(p, 2, 2); uint16_t v; memcpy(&v, p, 2); return v; }
static uint32_t src_ld8(const uint8_t *p) { chk_read(p, 1, 1); return *p; }
static void chk_store(uint8_t *p, uint32_t n, uint32_t align) {
    const Img &m = g_img[blockIdx.y];
    if ((uintptr_t)p % align) bad("misaligned store", (long)(p - m.dst), align);
    if (p < m.dst || p + n > m.dst + m.dst_bytes) { printf("store outside the slot: image %u, %ld + %u of %lu\n", blockIdx.y, (long)(p - m.dst), n, (unsigned long)m.dst_bytes); fflush(stdout); abort(); }
}
static void stg_st128(uint8_t *p, uint4 v) { chk_store(p, 16, 4); memcpy(p, &v, 16); }
static void stg_st96(uint8_t *p, uint32_t a, uint32_t b, uint32_t c) { chk_store(p, 12, 4); const uint32_t v[3] = {a, b, c}; memcpy(p, v, 12); }
static void stg_st8(uint8_t *p, uint32_t v) { chk_store(p, 1, 1); *p = (uint8_t)v; }
// ---- arithmetic, written out on the bits
static float cvt_f32_f16(uint32_t h) {  // by value: sign * m * 2^e in double, exact, then to float (exact too)
    const int e = (h >> 10) & 31, m = h & 1023;
    double v;
    if (e == 31) v = m ? NAN : INFINITY;
    else if (e == 0) v = ldexp((double)m, -24);
    else v = ldexp((double)(m + 1024), e - 25);
    return (float)((h & 0x8000u) ? -v : v);
}
static float cvt_f32_bf16(uint32_t b) { const uint32_t x = b << 16; float f; memcpy(&f, &x, 4); return f; }
static uint32_t quant_u8(float y) {
    if (std::isnan(y) || y <= 0.0f) return 0;
    if (y >= 255.0f) return 255;
    const float fl = floorf(y), d = y - fl;  // (exact: y < 255)
    uint32_t v = (uint32_t)fl;
    if (d > 0.5f || (d == 0.5f && (v & 1))) v++;
    return v;
}

#include KERNEL_TEXT  // the kernel and its helpers, cut out of xpng_amd/csrc/stage_from.hpp by the test

static const FloatConsts K = {{0.5f, 2.0f, 1.0f, 1.25f}, {0.5f, -3.0f, 0.25f, -1.0f}};
static const FloatConsts ONE = {{1.0f, 1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
static uint32_t rnd() { static uint64_t s = 88172645463325252ull; s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }

// element e of a buffer of kind (0 u8, 1 f16, 2 bf16, 3 f32): values around 0 .. 255 in quarter steps (exact ties), any bit pattern
// (NaN, infinities, subnormals), and the special values
template <class T> static void fill_elem(uint8_t *p) {
    constexpr int KIND = sizeof(T) == 1 ? 0 : FloatElem<T>::KIND;
    const uint32_t r = rnd();
    if (KIND == 0) { *p = (uint8_t)r; return; }
    static const float sp[] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 1e30f, -1e30f, 0.5f, 1.5f, 2.5f, 254.5f, 255.0f, 254.75f, 1e-40f, 6e-8f, -6e-8f};
    float f = ((int)(r % 1280) - 100) * 0.25f;
    if (r % 16 == 0) f = sp[(r >> 8) % 16];
    uint32_t fb; memcpy(&fb, &f, 4);
    if (KIND == 3) { if (r % 16 == 1) fb = rnd() ^ (rnd() << 16); memcpy(p, &fb, 4); return; }
    uint16_t h;
    if (r % 16 == 1) h = (uint16_t)rnd();                         // any pattern
    else if (r % 16 == 2) h = KIND == 1 ? (uint16_t)(rnd() % 1024) | (uint16_t)((r >> 5) & 0x8000u) : (uint16_t)(fb >> 16);  // f16 subnormals
    else if (KIND == 2) h = (uint16_t)(fb >> 16);
    else {  // f16 of a quarter step below 320: exact (11 bits suffice); of the specials: by the three classes
        const float a = fabsf(f);
        if (std::isnan(f)) h = 0x7e00; else if (a > 65504.0f) h = 0x7c00; else if (a < 6.2e-5f) h = (uint16_t)lrint(ldexp((double)a, 24));
        else { int e; frexp(a, &e); h = (uint16_t)(((e - 1 + 15) << 10) + ((int)lrint(ldexp((double)a, 11 - e)) - 1024)); }
        if (std::signbit(f)) h |= 0x8000u;
    }
    memcpy(p, &h, 2);
}
template <class T> static float elem_value(const uint8_t *p) {
    if (sizeof(T) == 4) { float f; memcpy(&f, p, 4); return f; }
    uint16_t h; memcpy(&h, p, 2);
    return FloatElem<T>::KIND == 1 ? cvt_f32_f16(h) : cvt_f32_bf16(h);
}
// the rule, for the expected bytes (its own clamp and rounding: nearbyintf in the default mode rounds half to even)
static uint8_t rule(float x, float s, float b) {
    const float y = fmaf(x, s, b);
    if (!(y > 0.0f)) return 0;
    if (y >= 255.0f) return 255;
    return (uint8_t)nearbyintf(y);
}

struct Spec { uint64_t npx; int C; uint32_t off; };  // off: the buffer starts `off` elements behind a 16-byte boundary
template <bool PLANAR, class T> static void run(const std::vector<Spec> &specs, uint32_t bgr, uint32_t gx, const FloatConsts &k) {
    constexpr uint64_t ES = sizeof(T);
    const uint32_t n = specs.size();
    // sources: one heap block, each buffer framed by 64 sentinel bytes; rasters: one heap block, 16-byte aligned slots with 32
    // sentinel bytes between them
    std::vector<uint64_t> so(n), sb(n), dof(n), db(n);
    uint64_t st = 64, dt = 32;
    for (uint32_t i = 0; i < n; i++) {
        sb[i] = specs[i].npx * specs[i].C * ES; so[i] = rup(st, 16) + specs[i].off * ES; st = so[i] + sb[i] + 64;
        db[i] = specs[i].npx * specs[i].C; dof[i] = rup(dt, 16); dt = dof[i] + db[i] + 32;
    }
    uint8_t *src = (uint8_t *)aligned_alloc(64, rup(st, 64)), *dst = (uint8_t *)aligned_alloc(64, rup(dt, 64));
    memset(src, 0xEE, st); memset(dst, 0xA5, dt);
    std::vector<ImgRec> rec(n); std::vector<const uint8_t *> srcs(n);
    g_img.clear();
    for (uint32_t i = 0; i < n; i++) {
        for (uint64_t e = 0; e < specs[i].npx * specs[i].C; e++) fill_elem<T>(src + so[i] + e * ES);
        rec[i] = ImgRec{dst + dof[i], nullptr, specs[i].npx, (uint32_t)specs[i].C, 0};
        srcs[i] = src + so[i];
        g_img.push_back(Img{src + so[i], sb[i], dst + dof[i], db[i]});
    }
    std::vector<uint8_t> src0(src, src + st);
    launch(gx, n, [&] { k_images_stage_from<3, PLANAR, T>(rec.data(), srcs.data(), bgr, k); });
    launch(gx, n, [&] { k_images_stage_from<4, PLANAR, T>(rec.data(), srcs.data(), bgr, k); });
    if (memcmp(src, src0.data(), st)) bad("a source byte was written", 0, 0);
    std::vector<uint8_t> exp(dt, 0xA5);
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t npx = specs[i].npx; const int C = specs[i].C;
        for (uint64_t p = 0; p < npx; p++) for (int c = 0; c < C; c++) {
            const int cc = bgr && c < 3 ? 2 - c : c;
            const uint8_t *e = src + so[i] + (PLANAR ? (uint64_t)cc * npx + p : p * C + cc) * ES;
            exp[dof[i] + p * C + c] = ES == 1 ? *e : rule(elem_value<T>(e), k.scale[cc], k.bias[cc]);
        }
    }
    for (uint64_t j = 0; j < dt; j++) if (dst[j] != exp[j]) {
        uint32_t i = 0; while (i + 1 < n && j >= dof[i + 1] - 16) i++;
        printf("byte %lu (image %u: npx %lu C %d off %u, at %ld) planar %d es %lu bgr %u: %u, expected %u\n", (unsigned long)j, i, (unsigned long)specs[i].npx, specs[i].C, specs[i].off,
               (long)(j - dof[i]), (int)PLANAR, (unsigned long)ES, bgr, dst[j], exp[j]);
        errors++; break;
    }
    free(src); free(dst);
}
template <class T> static void run_layouts(const std::vector<Spec> &specs, uint32_t gx) {
    for (uint32_t bgr = 0; bgr <= 2; bgr += 2) {  // (the kernel takes the layout word's bit: any non-zero value)
        run<false, T>(specs, bgr, gx, K); run<true, T>(specs, bgr, gx, K);
    }
    run<false, T>(specs, 0, gx, ONE); run<true, T>(specs, 2, gx, ONE);
}
static void run_all(const std::vector<Spec> &specs, uint32_t gx) {
    run_layouts<uint8_t>(specs, gx); run_layouts<f16_t>(specs, gx); run_layouts<bf16_t>(specs, gx); run_layouts<float>(specs, gx);
}
int main() {
    // the shims against known values
    struct { uint16_t h; float f; } t16[] = {{0x3c00, 1.0f}, {0x0001, 5.9604645e-8f}, {0x03ff, 6.0975552e-05f}, {0x0400, 6.103515625e-05f}, {0x7bff, 65504.0f}, {0xc000, -2.0f}, {0x5bf8, 255.0f}};
    for (auto &t : t16) if (cvt_f32_f16(t.h) != t.f) bad("cvt_f32_f16", t.h, 0);
    if (!std::isinf(cvt_f32_f16(0x7c00)) || !std::isnan(cvt_f32_f16(0x7e01)) || !std::signbit(cvt_f32_f16(0x8000))) bad("cvt_f32_f16 specials", 0, 0);
    struct { float y; uint32_t v; } tq[] = {{0.5f, 0}, {1.5f, 2}, {2.5f, 2}, {254.5f, 254}, {254.50002f, 255}, {0.50000006f, 1}, {-0.0f, 0}, {NAN, 0}, {INFINITY, 255}, {-INFINITY, 0}, {255.0f, 255}, {1e-40f, 0}, {3.49f, 3}};
    for (auto &t : tq) if (quant_u8(t.y) != t.v || rule(t.y, 1.0f, 0.0f) != t.v) bad("quant_u8", (long)t.y, t.v);
    // one image per launch: npx 1 .. 9 at every element offset 0 .. 7 inside the arena, as RGB and as RGBA
    for (uint64_t npx = 1; npx <= 9; npx++) for (uint32_t off = 0; off < 8; off++) for (int C = 3; C <= 4; C++) run_all({Spec{npx, C, off}}, 2);
    // more than one grid pass: 2 blocks of 256 lanes take 512 groups = 2048 pixels a pass
    for (uint32_t off : {0u, 1u, 3u}) for (int C = 3; C <= 4; C++) run_all({Spec{5003, C, off}}, 2);
    // several images per launch, RGB and RGBA mixed, every offset, sizes on both sides of a pass
    std::vector<Spec> mix;
    const uint64_t sizes[] = {1, 4, 7, 64, 255, 1023, 1024, 1025, 2051, 4100, 2, 9, 33, 3000};
    for (uint32_t i = 0; i < 14; i++) mix.push_back(Spec{sizes[i], (i % 3 == 1) ? 4 : 3, i % 8});
    run_all(mix, 1); run_all(mix, 3);
    printf("errors: %d\n", errors);
    return errors != 0;
}
