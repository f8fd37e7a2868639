// Host run of k_mixed_copy_as_float (xpng_amd/csrc/mixed_float.hpp): every thread of every block, one after another, over both pixel
// sizes, all 12 layouts and the three element types, with shims for the device operations the kernel uses.  The shims of the
// staging reads check the read rule (no read ends more than 7 bytes behind the pixels of the row it starts in, none starts before
// the raster), the shims of the stores check that every store lies inside the caller's buffer and is aligned to its width, and
// both buffers are heap blocks, so AddressSanitizer sees anything else.  The narrowing shims are this file's own round-to-nearest-
// even conversions; the expected value of every element is fmaf() and those conversions.
// Built and run by tests/test_float_kernels_host.py: g++ -fsanitize=address -static-libasan -DKERNEL_TEXT=\"...\".
#define KERNEL_HOST_FLOAT_OPS
#include "kernel_host.hpp"  // the launch shim, v_perm / v_alignbyte, the checked loads and stores, the narrowing; TYPES_TEXT: MixedLayout, MC_ROWS, Dw4, Dw3

// ---- the staging raster and the read rule
static const uint8_t *g_stage; static uint64_t g_bpr, g_need;
struct Slot { uint64_t off, end, rows, row_px_bytes; };
static std::vector<Slot> g_slots;
static void chk_read(const uint8_t *p, uint32_t n, uint32_t align) {
    if ((uintptr_t)p % align) bad("misaligned staging read", (long)(p - g_stage), align);
    if (p < g_stage || p + n > g_stage + g_need) { printf("staging read outside the raster: %ld + %u\n", (long)(p - g_stage), n); abort(); }
    const uint64_t o = p - g_stage;
    // the row the read starts in; a read that starts behind the last row of a slot (at most 7 bytes behind its pixels) belongs to that row
    for (auto &s : g_slots) if (o >= s.off && o < s.end) {
        const uint64_t row = std::min((o - s.off) / g_bpr, s.rows - 1), end = s.off + row * g_bpr + s.row_px_bytes;
        if (o + n > end + 7) bad("staging read more than 7 bytes behind its row", (long)o, (long)(o + n - end));
        return;
    }
    bad("staging read outside every slot", (long)o, n);
}

#include KERNEL_TEXT  // FloatConsts, the element types and the kernel, cut out of xpng_amd/csrc/mixed_float.hpp by the test

// the stored byte behind caller's element (y, x, c) of a layout, from an interleaved raster of px bytes
static uint8_t want(const uint8_t *ras, uint32_t w, int px, bool bgr, uint32_t y, uint32_t x, int c) {
    if (c == 3) return px == 4 ? ras[((uint64_t)y * w + x) * px + 3] : 0xFF;
    return ras[((uint64_t)y * w + x) * px + (bgr ? 2 - c : c)];
}
template <class T> static uint32_t elem_bits(float y) {
    if (sizeof(T) == 4) { uint32_t b; memcpy(&b, &y, 4); return b; }
    return FloatElem<T>::KIND == 1 ? to_f16(y) : to_bf16(y);
}
static const FloatConsts K = {{1.0f / 255.0f, 0.01712475383f, 2049.0f / 2048.0f, 259.0f / 256.0f}, {-2.1179039f, 0.5f, 0.0f, -3.25f}};

template <int PX, class T> static void run(const std::vector<std::pair<uint32_t, uint32_t>> &dims) {
    const uint32_t n = dims.size(), ES = sizeof(T); uint64_t maxw = 0, maxh = 0;
    for (auto &d : dims) { maxw = std::max<uint64_t>(maxw, d.first); maxh = std::max<uint64_t>(maxh, d.second); }
    const uint64_t bpr = rup(maxw * PX, 16);
    std::vector<uint64_t> slot(n + 1, 0);
    g_slots.clear();
    for (uint32_t i = 0; i < n; i++) { slot[i + 1] = slot[i] + rup(dims[i].second * bpr, 256); g_slots.push_back({slot[i], slot[i + 1], dims[i].second, (uint64_t)dims[i].first * PX}); }
    // (the library keeps 256 spare bytes behind the last slot; here the block ends 7 bytes behind the last row's pixels, so the
    // sanitizer, too, sees a read past the rule at the very end)
    const uint64_t need = slot[n - 1] + (dims[n - 1].second - 1) * bpr + (uint64_t)dims[n - 1].first * PX + 7;
    uint8_t *stage = (uint8_t *)malloc(need);
    g_stage = stage; g_bpr = bpr; g_need = need;
    std::vector<std::vector<uint8_t>> ras(n);
    for (uint32_t i = 0; i < n; i++) { ras[i].resize((uint64_t)dims[i].first * dims[i].second * PX); for (auto &b : ras[i]) b = rand(); }
    memset(stage, 0xEE, need);
    for (uint32_t i = 0; i < n; i++) for (uint32_t y = 0; y < dims[i].second; y++) memcpy(stage + slot[i] + y * bpr, ras[i].data() + (uint64_t)y * dims[i].first * PX, dims[i].first * PX);
    for (int C = 3; C <= 4; C++) for (int planar = 0; planar < 2; planar++) for (int bgr = 0; bgr < 2; bgr++) {
        std::vector<uint8_t *> out(n); std::vector<uint64_t> outsz(n); std::vector<MixedLayout> ml(n);
        g_out.clear();
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t sz = (uint64_t)C * dims[i].first * dims[i].second * ES, lead = 64 + ES * (i % 8);
            outsz[i] = lead + sz + 64; out[i] = (uint8_t *)aligned_alloc(64, rup(outsz[i], 64));  // (16-byte aligned base, so `lead` sets the start modulo 16)
            memset(out[i], 0xA5, outsz[i]);
            ml[i] = MixedLayout{slot[i], out[i] + lead, dims[i].first, dims[i].second};
            g_out.push_back({out[i] + lead, out[i] + lead + sz});
        }
        const uint32_t gx = (maxh + MC_ROWS - 1) / MC_ROWS;
        auto go = [&](auto k) { launch(gx, n, [&] { k(ml.data(), stage, bpr, (uint32_t)(bgr ? 2 : 0), K); }); };
        if (C == 3 && planar) go(k_mixed_copy_as_float<PX, 3, true, T>); else if (C == 3) go(k_mixed_copy_as_float<PX, 3, false, T>);
        else if (planar) go(k_mixed_copy_as_float<PX, 4, true, T>); else go(k_mixed_copy_as_float<PX, 4, false, T>);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t w = dims[i].first, h = dims[i].second; const uint64_t sz = (uint64_t)C * w * h * ES; const uint8_t *o = ml[i].buf;
            for (uint64_t k = 0; k < outsz[i]; k++) { const uint8_t *p = out[i] + k; if ((p < o || p >= o + sz) && *p != 0xA5) { printf("sentinel px%d C%d pl%d bgr%d es%u img%u (%ux%u) at %ld\n", PX, C, planar, bgr, ES, i, w, h, (long)(p - o)); errors++; break; } }
            int stop = 0;
            for (uint32_t y = 0; y < h && !stop; y++) for (uint32_t x = 0; x < w && !stop; x++) for (int c = 0; c < C; c++) {
                const uint64_t e = planar ? (uint64_t)c * w * h + (uint64_t)y * w + x : ((uint64_t)y * w + x) * C + c;
                uint32_t got = 0; memcpy(&got, o + e * ES, ES);
                const uint32_t exp = elem_bits<T>(fmaf((float)want(ras[i].data(), w, PX, bgr, y, x, c), K.scale[c], K.bias[c]));
                if (got != exp) { printf("value px%d C%d pl%d bgr%d kind%d img%u (%ux%u) y%u x%u c%d: %x, expected %x\n", PX, C, planar, bgr, FloatElem<T>::KIND, i, w, h, y, x, c, got, exp); errors++; stop = 1; break; }
            }
            free(out[i]);
        }
    }
    free(stage);
}
template <int PX> static void run_all(const std::vector<std::pair<uint32_t, uint32_t>> &dims) { run<PX, f16_t>(dims); run<PX, bf16_t>(dims); run<PX, float>(dims); }
int main() {
    // the conversions above against known values: ties to even both ways, the subnormal range, overflow
    struct { float f; uint16_t h; } t16[] = {{1.0f, 0x3c00}, {2049.0f / 2048.0f, 0x3c00}, {2051.0f / 2048.0f, 0x3c02}, {65504.0f, 0x7bff}, {65519.9f, 0x7bff}, {65520.0f, 0x7c00},
        {5.9604645e-8f, 0x0001}, {2.9802322e-8f, 0x0000}, {8.9406967e-8f, 0x0002}, {6.103515625e-05f, 0x0400}, {6.0975552e-05f, 0x03ff}, {-2.0f, 0xc000}, {0.0f, 0x0000}};
    for (auto &t : t16) if (to_f16(t.f) != t.h) bad("to_f16", to_f16(t.f), t.h);
    struct { float f; uint16_t h; } tb[] = {{1.0f, 0x3f80}, {257.0f / 256.0f, 0x3f80}, {259.0f / 256.0f, 0x3f82}, {-3.25f, 0xc050}, {3.4e38f, 0x7f80}};
    for (auto &t : tb) if (to_bf16(t.f) != t.h) bad("to_bf16", to_bf16(t.f), t.h);
    std::vector<std::pair<uint32_t, uint32_t>> dims;
    for (uint32_t w = 1; w <= 17; w++) for (uint32_t h = 1; h <= 3; h++) dims.push_back({w, h});
    for (auto d : {std::pair<uint32_t, uint32_t>{64, 64}, {445, 44}, {889, 13}, {100, 110}, {701, 30}, {255, 9}, {256, 8}, {257, 17}, {1031, 3}, {2111, 2}}) dims.push_back(d);
    run_all<3>(dims); run_all<4>(dims);
    std::reverse(dims.begin(), dims.end()); run_all<3>(dims); run_all<4>(dims);
    // every size once as the LAST (and only) image: the raster then ends 7 bytes behind its last pixel
    for (auto d : dims) if (d.first <= 17 || d.second <= 3) { run_all<3>({d}); run_all<4>({d}); }
    printf("errors: %d\n", errors);
    return errors != 0;
}
