// Host run of k_mixed_resample_as_float (xpng_amd/csrc/mixed_resample.hpp): every thread of every block, one after another, over
// both pixel sizes, all 12 layouts and the three element types (24 instances), with shims for the device operations the kernel uses
// (those of tests/float_kernels_host.cpp: the kernel reuses the named operations of mixed_float.hpp and resize_tap of
// mixed_resize.hpp, whose texts are compiled in front of it).
// The shims of the staging reads check the read rule (no read ends more than 7 bytes behind the pixels of the row it starts in,
// none starts before the raster) and, stricter, that every read of a launch lies inside the pixels of its image's RECTANGLE; the
// shims of the stores check that every store lies inside the caller's buffer and is aligned to its width; both buffers are heap
// blocks, so AddressSanitizer sees anything else.  The expected value of every element is this file's own plain statement of the
// rule: fmaf(), single fp32 sums and divisions, and its own round-to-nearest-even conversions.
// Built and run by tests/test_resample_kernels_host.py: g++ -ffp-contract=off -fsanitize=address -static-libasan -DFLOAT_TEXT=.. -DRESIZE_TEXT=.. -DKERNEL_TEXT=..
#define KERNEL_HOST_FLOAT_OPS
#include "kernel_host.hpp"  // the launch shim, v_perm / v_alignbyte, the checked loads and stores, the narrowing; TYPES_TEXT: MixedLayout, MC_ROWS, Dw4, Dw3

// ---- the staging raster, the read rule and the rectangles
static const uint8_t *g_stage; static uint64_t g_bpr, g_need; static int g_px;
struct Slot { uint64_t off, end, rows, row_px_bytes; uint32_t rx, ry, rw, rh; };
static std::vector<Slot> g_slots;
static void chk_read(const uint8_t *p, uint32_t n, uint32_t align) {
    if ((uintptr_t)p % align) bad("misaligned staging read", (long)(p - g_stage), align);
    if (p < g_stage || p + n > g_stage + g_need) { printf("staging read outside the raster: %ld + %u\n", (long)(p - g_stage), n); abort(); }
    const uint64_t o = p - g_stage;
    for (auto &s : g_slots) if (o >= s.off && o < s.end) {
        const uint64_t row = std::min((o - s.off) / g_bpr, s.rows - 1), start = s.off + row * g_bpr, end = start + s.row_px_bytes;
        if (o + n > end + 7) bad("staging read more than 7 bytes behind its row", (long)o, (long)(o + n - end));
        // the rectangle: its rows, and in them its pixels
        if (row < s.ry || row >= s.ry + s.rh || o < start + (uint64_t)s.rx * g_px || o + n > start + (uint64_t)(s.rx + s.rw) * g_px)
            bad("staging read outside the image's rectangle", (long)row, (long)(o - start));
        return;
    }
    bad("staging read outside every slot", (long)o, n);
}

#include FLOAT_TEXT   // FloatConsts, the element types, pick4, narrow2, store1, float_chunk (and the float kernel): mixed_float.hpp
#include RESIZE_TEXT  // ResizeRec, resize_tap (and the resize kernel): mixed_resize.hpp
#include KERNEL_TEXT  // ResampleRec, the window, the weight and the kernel, cut out of xpng_amd/csrc/mixed_resample.hpp by the test

template <class T> static uint32_t elem_bits(float y) {
    if (sizeof(T) == 4) { uint32_t b; memcpy(&b, &y, 4); return b; }
    return FloatElem<T>::KIND == 1 ? to_f16(y) : to_bf16(y);
}
static const FloatConsts K = {{1.0f / 255.0f, 0.01712475383f, 2049.0f / 2048.0f, 259.0f / 256.0f}, {-2.1179039f, 0.5f, 0.0f, -3.25f}};

// ---- the rule, stated plainly: one axis over a sequence q, then one element from a tight interleaved raster
template <class Q> static float axis_op(uint32_t u, uint32_t n, uint32_t n_out, Q q) {
    const float k = (float)n / (float)n_out;
    const float centre = (float)u + 0.5f;
    const float f = fmaf(centre, k, -0.5f);
    if (!(k > 1.0f)) {  // the two taps of the resized call
        const float s = f > 0.0f ? f : 0.0f;
        const uint32_t i0 = std::min((uint32_t)s, n - 1), i1 = std::min(i0 + 1, n - 1);
        const float l = s - (float)i0, q0 = q(i0), q1 = q(i1);
        const float d = q1 - q0;
        return fmaf(l, d, q0);
    }
    const float ik = 1.0f / k, lo = f - k, hi = f + k;
    const uint32_t j0 = lo > 0.0f ? (uint32_t)lo : 0, j1 = std::min((uint32_t)hi, n - 1);
    float W = 0.0f, A = 0.0f;
    for (uint32_t j = j0; j <= j1; j++) {
        const float d = fabsf((float)j - f);
        const float w = std::max(fmaf(-d, ik, 1.0f), 0.0f);
        W = W + w;
        A = fmaf(w, q(j), A);
    }
    if (!(W > 0.0f)) bad("a window without weight", (long)u, (long)n);
    return A / W;
}
struct Rect { uint32_t x, y, w, h, flip; };
static float rule(const uint8_t *ras, uint32_t w, int px, bool bgr, const Rect &rc, uint32_t OW, uint32_t OH, uint32_t oy, uint32_t ox, int c) {
    float v = 255.0f;
    if (!(c == 3 && px == 3)) {
        const int sc = c == 3 ? 3 : bgr ? 2 - c : c;
        auto H = [&](uint32_t yy) {
            return axis_op(rc.flip ? OW - 1 - ox : ox, rc.w, OW, [&](uint32_t xx) { return (float)ras[((uint64_t)(rc.y + yy) * w + rc.x + xx) * px + sc]; });
        };
        v = axis_op(oy, rc.h, OH, H);
    }
    return fmaf(v, K.scale[c], K.bias[c]);
}
// the rectangle of an image for a kind: whole, 1 x 1 at the last pixel, the last column, the last row, of the output's size,
// strictly inside the image (a tap outside the rectangle would read other pixels: the read rule above sees it)
static Rect rect_of(uint32_t w, uint32_t h, uint32_t kind, uint32_t OW, uint32_t OH, uint32_t flip) {
    switch (kind % 6) {
    case 5: if (w >= 3 && h >= 3) return {1, 1, w - 2, h - 2, flip};  // (else the whole image)
        break;
    case 1: return {w - 1, h - 1, 1, 1, flip};
    case 2: return {w - 1, 0, 1, h, flip};
    case 3: return {0, h - 1, w, 1, flip};
    case 4: if (w >= OW && h >= OH) return {w - OW, h - OH, OW, OH, flip};  // (else the whole image)
        break;
    }
    return {0, 0, w, h, flip};
}

template <int PX, class T> static void run(const std::vector<std::pair<uint32_t, uint32_t>> &dims, uint32_t OW, uint32_t OH, uint32_t shift) {
    const uint32_t n = dims.size(), ES = sizeof(T); uint64_t maxw = 0;
    for (auto &d : dims) maxw = std::max<uint64_t>(maxw, d.first);
    const uint64_t bpr = rup(maxw * PX, 16);
    std::vector<uint64_t> slot(n + 1, 0);
    std::vector<Rect> rc(n); std::vector<ResampleRec> rz(n);
    g_slots.clear(); g_px = PX;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t w = dims[i].first, h = dims[i].second;
        rc[i] = rect_of(w, h, i + shift, OW, OH, (i + (shift >> 1)) & 1);
        const float kx = (float)rc[i].w / (float)OW, ky = (float)rc[i].h / (float)OH;
        rz[i] = ResampleRec{rc[i].x, rc[i].y, rc[i].w, rc[i].h, kx, ky, 1.0f / kx, 1.0f / ky, rc[i].flip, {0, 0, 0}};
        slot[i + 1] = slot[i] + rup(h * bpr, 256);
        g_slots.push_back({slot[i], slot[i + 1], h, (uint64_t)w * PX, rc[i].x, rc[i].y, rc[i].w, rc[i].h});
    }
    // (the block ends with the last row's last pixel: this kernel needs no spare byte behind the raster)
    const uint64_t need = slot[n - 1] + (dims[n - 1].second - 1) * bpr + (uint64_t)dims[n - 1].first * PX;
    uint8_t *stage = (uint8_t *)malloc(need);
    g_stage = stage; g_bpr = bpr; g_need = need;
    std::vector<std::vector<uint8_t>> ras(n);
    for (uint32_t i = 0; i < n; i++) { ras[i].resize((uint64_t)dims[i].first * dims[i].second * PX); for (auto &b : ras[i]) b = rand(); }
    memset(stage, 0xEE, need);
    for (uint32_t i = 0; i < n; i++) for (uint32_t y = 0; y < dims[i].second; y++) memcpy(stage + slot[i] + y * bpr, ras[i].data() + (uint64_t)y * dims[i].first * PX, dims[i].first * PX);
    for (int C = 3; C <= 4; C++) for (int planar = 0; planar < 2; planar++) for (int bgr = 0; bgr < 2; bgr++) {
        std::vector<uint8_t *> out(n); std::vector<MixedLayout> ml(n);
        const uint64_t sz = (uint64_t)C * OW * OH * ES;
        g_out.clear();
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t lead = 64 + ES * (i % 8);
            out[i] = (uint8_t *)aligned_alloc(64, rup(lead + sz + 64, 64));  // (16-byte aligned base, so `lead` sets the start modulo 16)
            memset(out[i], 0xA5, lead + sz + 64);
            ml[i] = MixedLayout{slot[i], out[i] + lead, dims[i].first, dims[i].second};
            g_out.push_back({out[i] + lead, out[i] + lead + sz});
        }
        const uint32_t gx = (OH + MC_ROWS - 1) / MC_ROWS;
        auto go = [&](auto k) { launch(gx, n, [&] { k(ml.data(), rz.data(), stage, bpr, (uint32_t)(bgr ? 2 : 0), OW, OH, K); }); };
        if (C == 3 && planar) go(k_mixed_resample_as_float<PX, 3, true, T>); else if (C == 3) go(k_mixed_resample_as_float<PX, 3, false, T>);
        else if (planar) go(k_mixed_resample_as_float<PX, 4, true, T>); else go(k_mixed_resample_as_float<PX, 4, false, T>);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t w = dims[i].first; const uint8_t *o = ml[i].buf; const uint64_t lead = 64 + ES * (i % 8);
            for (uint64_t k = 0; k < lead + sz + 64; k++) { const uint8_t *p = out[i] + k; if ((p < o || p >= o + sz) && *p != 0xA5) { printf("sentinel px%d C%d pl%d bgr%d es%u img%u out %ux%u at %ld\n", PX, C, planar, bgr, ES, i, OW, OH, (long)(p - o)); errors++; break; } }
            int stop = 0;
            for (uint32_t y = 0; y < OH && !stop; y++) for (uint32_t x = 0; x < OW && !stop; x++) for (int c = 0; c < C; c++) {
                const uint64_t e = planar ? ((uint64_t)c * OH + y) * OW + x : ((uint64_t)y * OW + x) * C + c;
                uint32_t got = 0; memcpy(&got, o + e * ES, ES);
                const uint32_t exp = elem_bits<T>(rule(ras[i].data(), w, PX, bgr, rc[i], OW, OH, y, x, c));
                if (got != exp) { printf("value px%d C%d pl%d bgr%d kind%d img%u (%ux%u) rect %u,%u,%u,%u flip%u out %ux%u y%u x%u c%d: %x, expected %x\n", PX, C, planar, bgr, FloatElem<T>::KIND, i, w, dims[i].second, rc[i].x, rc[i].y, rc[i].w, rc[i].h, rc[i].flip, OW, OH, y, x, c, got, exp); errors++; stop = 1; break; }
            }
            free(out[i]);
        }
    }
    free(stage);
}
template <int PX> static void run_all(const std::vector<std::pair<uint32_t, uint32_t>> &dims, uint32_t OW, uint32_t OH, uint32_t shift) {
    run<PX, f16_t>(dims, OW, OH, shift); run<PX, bf16_t>(dims, OW, OH, shift); run<PX, float>(dims, OW, OH, shift);
}
int main() {
    std::vector<std::pair<uint32_t, uint32_t>> dims;
    // (the larger images first: the read rule looks an address up in the slots in order, and these have most of the reads)
    for (auto d : {std::pair<uint32_t, uint32_t>{64, 64}, {445, 14}, {889, 5}, {100, 40}, {2111, 2}, {300, 5}}) dims.push_back(d);
    for (uint32_t w = 1; w <= 17; w++) for (uint32_t h = 1; h <= 3; h++) dims.push_back({w, h});
    // output widths 1 .. 17 (every start of a row and of a plane row modulo 16 bytes, rows shorter than one 16-byte store), heights
    // of one block and of two, every rectangle kind and both flips on every image: ratios on both sides of 1 on each axis, alone and
    // mixed
    const uint32_t ohs[3] = {1, 3, 9};
    for (uint32_t OW = 1; OW <= 17; OW++) for (uint32_t shift = 0; shift < 6; shift++) { run_all<3>(dims, OW, ohs[(OW + shift) % 3], shift); run_all<4>(dims, OW, ohs[(OW + shift) % 3], shift); }
    // an output row wider than one pass of a wave (64 stores of 4 or 8 elements), planar and interleaved; an upscale and a downscale
    for (uint32_t shift = 0; shift < 2; shift++) { run_all<3>({{300, 5}, {1031, 3}, {7, 2}}, 601, 2, 5 * shift); run_all<4>({{300, 5}, {1031, 3}, {7, 2}}, 601, 2, 5 * shift); }
    run_all<3>({{64, 64}, {37, 29}, {200, 9}, {9, 200}}, 37, 29, 5); run_all<4>({{64, 64}, {37, 29}, {200, 9}, {9, 200}}, 37, 29, 5);
    printf("errors: %d\n", errors);
    return errors != 0;
}
