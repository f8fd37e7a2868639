// Host run of k_mixed_views_colour (xpng_amd/csrc/mixed_views_colour.hpp): every thread of every block, one after another, over both
// pixel sizes, all 12 layouts and the three element types (24 instances) and both filters, with the shims for the device operations
// of tests/kernel_host.hpp (the kernel reuses the named operations of mixed_float.hpp, resize_tap of mixed_resize.hpp, the window
// and the weight of mixed_resample.hpp, ViewRec of mixed_views.hpp and the end of a pixel and the row writer of
// mixed_views_pixel.hpp, whose texts are compiled in front of it).
// A launch holds several images and MORE views than images, as tests/views_kernels_host.cpp's: views of different sizes (the grid
// is the tallest view's, so blocks of short views must return), several views of one image, an image without a view, ratios on both
// sides of 1 on each axis, both flips, rectangles at the image's edges - and a different matrix per view: the identity, a
// non-symmetric permutation, the gray matrix, one that drives values below 0 and above 255, a dense one.  Views whose plane size is
// a multiple of 16 bytes (the planar kernel's 16-byte stores into every plane) stand beside views whose is not (a pixel per lane).
// The shim of the staging reads looks up the view of the running block and checks that every read lies inside the pixels of THAT
// view's rectangle; the shims of the stores check that every store lies inside THAT view's buffer and is aligned to its width; the
// buffers are heap blocks, so AddressSanitizer sees anything else.  The expected value of every element is this file's own plain
// statement of the rule: fmaf(), single fp32 sums and divisions, its own round-to-nearest-even conversions.
// Built and run by tests/test_views_colour_kernels_host.py.
#define KERNEL_HOST_FLOAT_OPS
#include "kernel_host.hpp"  // the launch shim, the checked loads and stores, the narrowing; TYPES_TEXT: MixedLayout, MC_ROWS, Dw4, Dw3

// ---- the staging raster and the rectangle of every view
static const uint8_t *g_stage; static uint64_t g_bpr, g_need; static int g_px;
struct ViewBox { uint64_t off, rows; uint32_t rx, ry, rw, rh; };  // the slot of the view's image and its rectangle
static std::vector<ViewBox> g_views;
static void chk_read(const uint8_t *p, uint32_t n, uint32_t align) {
    if ((uintptr_t)p % align) bad("misaligned staging read", (long)(p - g_stage), align);
    if (p < g_stage || p + n > g_stage + g_need) { printf("staging read outside the raster: %ld + %u\n", (long)(p - g_stage), n); abort(); }
    if (n != 1) bad("a staging read of more than one byte", (long)(p - g_stage), n);
    const ViewBox &b = g_views[blockIdx.y];  // the view of the running block
    const uint64_t o = p - g_stage;
    if (o < b.off) { bad("staging read in front of the view's image", (long)o, (long)blockIdx.y); return; }
    const uint64_t row = (o - b.off) / g_bpr, col = (o - b.off) % g_bpr;
    if (row < b.ry || row >= (uint64_t)b.ry + b.rh || col < (uint64_t)b.rx * g_px || col + n > (uint64_t)(b.rx + b.rw) * g_px)
        bad("staging read outside the view's rectangle", (long)row, (long)col);
}

#include FLOAT_TEXT     // FloatConsts, the element types, pick4, narrow2, store1, float_chunk: mixed_float.hpp
#include RESIZE_TEXT    // resize_tap: mixed_resize.hpp
#include RESAMPLE_TEXT  // resample_win, resample_weight, resample_div: mixed_resample.hpp
#include VIEWS_TEXT     // ViewRec: mixed_views.hpp
#include PIXEL_TEXT     // colour_row, pixel_finish, pixel_store, row_narrow, row_wide: mixed_views_pixel.hpp
#include KERNEL_TEXT    // ViewColour and the kernel, cut out of xpng_amd/csrc/mixed_views_colour.hpp by the test

template <class T> static uint32_t elem_bits(float y) {
    if (sizeof(T) == 4) { uint32_t b; memcpy(&b, &y, 4); return b; }
    return FloatElem<T>::KIND == 1 ? to_f16(y) : to_bf16(y);
}
static const FloatConsts K = {{1.0f / 255.0f, 0.01712475383f, 2049.0f / 2048.0f, 259.0f / 256.0f}, {-2.1179039f, 0.5f, 0.0f, -3.25f}};
static const float MATS[5][12] = {
    {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0},                                                                  // the identity
    {0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0},                                                                  // R <- B, G <- R, B <- G
    {0.299f, 0.587f, 0.114f, 0, 0.299f, 0.587f, 0.114f, 0, 0.299f, 0.587f, 0.114f, 0},                      // gray
    {3, -2, 0.5f, -300, -2, 3, 0, 300, 1, 1, -2, 40},                                                       // below 0 and above 255
    {0.70710678f, -0.31830989f, 0.57721566f, 12.345678f, 0.14142135f, 1.6180339f, -0.69314718f, -7.3890561f,
     -0.43429448f, 0.26179939f, 1.2020569f, 31.415926f},                                                    // dense
};

// ---- the rule, stated plainly: one axis over a sequence q, a pixel's resampled byte, then one element
template <class Q> static float axis_op(uint32_t filter, uint32_t u, uint32_t n, uint32_t n_out, Q q) {
    const float k = (float)n / (float)n_out;
    const float centre = (float)u + 0.5f;
    const float f = fmaf(centre, k, -0.5f);
    if (!filter || !(k > 1.0f)) {  // the two taps
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
struct View { uint32_t img, x, y, w, h, flip, ow, oh; };
static float resampled(uint32_t filter, const uint8_t *ras, uint32_t w, int px, const View &v, uint32_t oy, uint32_t ox, int sc) {
    auto H = [&](uint32_t yy) {
        return axis_op(filter, v.flip ? v.ow - 1 - ox : ox, v.w, v.ow, [&](uint32_t xx) { return (float)ras[((uint64_t)(v.y + yy) * w + v.x + xx) * px + sc]; });
    };
    return axis_op(filter, oy, v.h, v.oh, H);
}
static float rule(uint32_t filter, const uint8_t *ras, uint32_t w, int px, bool bgr, const View &v, const float *m, uint32_t oy, uint32_t ox, int c) {
    float val;
    if (c == 3) val = px == 3 ? 255.0f : resampled(filter, ras, w, px, v, oy, ox, 3);
    else {
        const float *row = m + 4 * (bgr ? 2 - c : c);  // position c holds colour 2 - c of a BGR buffer
        const float r = resampled(filter, ras, w, px, v, oy, ox, 0), g = resampled(filter, ras, w, px, v, oy, ox, 1), b = resampled(filter, ras, w, px, v, oy, ox, 2);
        const float t2 = fmaf(row[2], b, row[3]);
        const float t1 = fmaf(row[1], g, t2);
        const float t = fmaf(row[0], r, t1);
        val = t < 0.0f ? 0.0f : t > 255.0f ? 255.0f : t;
    }
    return fmaf(val, K.scale[c], K.bias[c]);
}

typedef std::vector<std::pair<uint32_t, uint32_t>> Dims;
template <int PX, class T> static void run(const Dims &dims, const std::vector<View> &views, uint32_t filter) {
    const uint32_t n = dims.size(), nv = views.size(), ES = sizeof(T); uint64_t maxw = 0; uint32_t max_oh = 0;
    for (auto &d : dims) maxw = std::max<uint64_t>(maxw, d.first);
    const uint64_t bpr = rup(maxw * PX, 16);
    std::vector<uint64_t> slot(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) slot[i + 1] = slot[i] + rup(dims[i].second * bpr, 256);
    // (the block ends with the last row's last pixel: this kernel needs no spare byte behind the raster)
    const uint64_t need = slot[n - 1] + (dims[n - 1].second - 1) * bpr + (uint64_t)dims[n - 1].first * PX;
    uint8_t *stage = (uint8_t *)malloc(need);
    g_stage = stage; g_bpr = bpr; g_need = need; g_px = PX;
    std::vector<std::vector<uint8_t>> ras(n);
    for (uint32_t i = 0; i < n; i++) { ras[i].resize((uint64_t)dims[i].first * dims[i].second * PX); for (auto &b : ras[i]) b = rand(); }
    memset(stage, 0xEE, need);
    for (uint32_t i = 0; i < n; i++) for (uint32_t y = 0; y < dims[i].second; y++) memcpy(stage + slot[i] + y * bpr, ras[i].data() + (uint64_t)y * dims[i].first * PX, dims[i].first * PX);
    g_views.clear();
    for (auto &v : views) { g_views.push_back({slot[v.img], dims[v.img].second, v.x, v.y, v.w, v.h}); max_oh = std::max(max_oh, v.oh); }
    // the matrices on the heap, exactly nv of them: a read of another view's index past the table is AddressSanitizer's to see
    ViewColour *vm = (ViewColour *)malloc(nv * sizeof(ViewColour));
    for (uint32_t v = 0; v < nv; v++) memcpy(vm[v].m, MATS[(v + filter) % 5], sizeof(ViewColour));
    for (int C = 3; C <= 4; C++) for (int planar = 0; planar < 2; planar++) for (int bgr = 0; bgr < 2; bgr++) {
        std::vector<uint8_t *> out(nv); std::vector<ViewRec> vr(nv); std::vector<uint64_t> sz(nv);
        std::vector<std::pair<uint8_t *, uint8_t *>> box;  // every view's buffer; g_out holds the running block's alone
        for (uint32_t v = 0; v < nv; v++) {
            const View &w = views[v];
            const uint64_t lead = 64 + ES * (v % 8);
            sz[v] = (uint64_t)C * w.ow * w.oh * ES;
            out[v] = (uint8_t *)aligned_alloc(64, rup(lead + sz[v] + 64, 64));  // (16-byte aligned base, so `lead` sets the start modulo 16)
            memset(out[v], 0xA5, lead + sz[v] + 64);
            const float kx = (float)w.w / (float)w.ow, ky = (float)w.h / (float)w.oh;
            vr[v] = ViewRec{slot[w.img], out[v] + lead, w.x, w.y, w.w, w.h, w.ow, w.oh, kx, ky, 1.0f / kx, 1.0f / ky, w.flip, 0};
            box.push_back({out[v] + lead, out[v] + lead + sz[v]});
        }
        const uint32_t gx = (max_oh + MC_ROWS - 1) / MC_ROWS;
        // a store must lie inside the buffer of the view whose block makes it: a stray store into a later view's buffer would be
        // overwritten before the values are compared
        auto go = [&](auto k) { launch(gx, nv, [&] { g_out.assign(1, box[blockIdx.y]); k(vr.data(), vm, stage, bpr, (uint32_t)(bgr ? 2 : 0), filter, K); }); };
        if (C == 3 && planar) go(k_mixed_views_colour<PX, 3, true, T>); else if (C == 3) go(k_mixed_views_colour<PX, 3, false, T>);
        else if (planar) go(k_mixed_views_colour<PX, 4, true, T>); else go(k_mixed_views_colour<PX, 4, false, T>);
        for (uint32_t v = 0; v < nv; v++) {
            const View &w = views[v]; const uint8_t *o = vr[v].buf; const uint64_t lead = 64 + ES * (v % 8);
            for (uint64_t k = 0; k < lead + sz[v] + 64; k++) { const uint8_t *p = out[v] + k; if ((p < o || p >= o + sz[v]) && *p != 0xA5) { printf("sentinel px%d C%d pl%d bgr%d es%u view%u out %ux%u at %ld\n", PX, C, planar, bgr, ES, v, w.ow, w.oh, (long)(p - o)); errors++; break; } }
            int stop = 0;
            for (uint32_t y = 0; y < w.oh && !stop; y++) for (uint32_t x = 0; x < w.ow && !stop; x++) for (int c = 0; c < C; c++) {
                const uint64_t e = planar ? ((uint64_t)c * w.oh + y) * w.ow + x : ((uint64_t)y * w.ow + x) * C + c;
                uint32_t got = 0; memcpy(&got, o + e * ES, ES);
                const uint32_t exp = elem_bits<T>(rule(filter, ras[w.img].data(), dims[w.img].first, PX, bgr, w, vm[v].m, y, x, c));
                if (got != exp) { printf("value px%d C%d pl%d bgr%d kind%d filter%u view%u img%u rect %u,%u,%u,%u flip%u out %ux%u y%u x%u c%d: %x, expected %x\n", PX, C, planar, bgr, FloatElem<T>::KIND, filter, v, w.img, w.x, w.y, w.w, w.h, w.flip, w.ow, w.oh, y, x, c, got, exp); errors++; stop = 1; break; }
            }
            free(out[v]);
        }
    }
    free(vm);
    free(stage);
}
template <int PX> static void run_all(const Dims &dims, const std::vector<View> &views) {
    for (uint32_t filter = 0; filter < 2; filter++) { run<PX, f16_t>(dims, views, filter); run<PX, bf16_t>(dims, views, filter); run<PX, float>(dims, views, filter); }
}
int main() {
    // image 5 has no view; images 0, 1 and 3 have several
    const Dims dims = {{64, 64}, {445, 14}, {100, 40}, {7, 3}, {1, 1}, {300, 5}};
    // output widths shifted by 0 .. 7: every start of a row and of a plane row modulo 16 bytes, rows shorter than one 16-byte store,
    // plane sizes on both sides of the planar kernel's test
    for (uint32_t sh = 0; sh < 8; sh++) {
        const std::vector<View> views = {
            {0, 0, 0, 64, 64, 0, 19 + sh, 13},         // the whole image, both axes shrink (the tallest view: two blocks)
            {0, 10, 10, 30, 30, 1, 33 + sh, 11},       // inside it: x grows, y shrinks, flipped
            {0, 20, 5, 44, 59, 0, 3 + sh, 5},          // overlaps both, reaches the right and the lower edge
            {1, 444, 0, 1, 14, 1, 1 + sh, 3},          // the last column
            {1, 0, 0, 445, 14, 1, 16 + sh, 8},         // a wide window on x; with sh == 0 the planes are multiples of 16 bytes
            {1, 0, 13, 445, 1, 0, 9 + sh, 2},          // the last row; y grows from one row
            {2, 84 - sh, 31, 16 + sh, 9, 0, 16 + sh, 9},  // a rectangle of the output's size at the last pixel: the identity
            {3, 0, 0, 7, 3, sh & 1, 13 + sh, 2},       // x grows, y shrinks
            {3, 6, 2, 1, 1, 1, 1, 1},                  // one pixel to one element
            {4, 0, 0, 1, 1, 0, 4 + sh, 8},             // one pixel to many
        };
        run_all<3>(dims, views); run_all<4>(dims, views);
    }
    // an output row wider than one pass of a wave (64 stores of 4 or 8 elements), an upscale and a downscale, beside a view of one row
    const std::vector<View> wide = {{5, 0, 0, 300, 5, 0, 600, 2}, {1, 3, 1, 440, 12, 1, 530, 1}, {5, 100, 0, 200, 5, 1, 96, 9}, {3, 0, 0, 7, 3, 0, 5, 3}};
    run_all<3>(dims, wide); run_all<4>(dims, wide);
    printf("errors: %d\n", errors);
    return errors != 0;
}
