// Host run of k_mixed_views_affine (xpng_amd/csrc/mixed_views_affine.hpp): every thread of every block, one after another, over both
// pixel sizes, all 12 layouts and the three element types (24 instances) and both filters, with the shims for the device operations
// of tests/kernel_host.hpp (the kernel reuses the named operations of mixed_float.hpp, the end of a pixel and the row writer of
// mixed_views_pixel.hpp and ViewColour of mixed_views_colour.hpp, whose texts are compiled in front of it).  Both lane mappings are run: the patch of four rows per wave
// that the product launches and the one row per wave of the timing study.
// A launch holds several images and MORE views than images: views of different heights (the grid is the tallest view's, so blocks of
// short views must return), rotations by generic angles, a shear with a scale, an exact quarter turn, a mirror, an integer
// translation, a view that hangs partly outside its image, a view whose footprint is empty, an image without a view - with a colour
// matrix per view or none, and a fill of zeros or not.  Views whose plane size is a multiple of 16 bytes stand beside views whose is
// not.  The footprint of every view is this program's own computation in long double from the fp32 entries.
// The shim of the staging reads looks up the view of the running block and checks that every read lies inside THAT view's
// footprint; the shims of the stores check that every store lies inside THAT view's buffer and is aligned to its width; the buffers
// are heap blocks, so AddressSanitizer sees anything else.  The expected value of every element is this file's own plain statement
// of the rule: fmaf(), single fp32 subtractions, floorf and rintf, its own round-to-nearest-even conversions.
// Built and run by tests/test_views_affine_kernels_host.py.
#define KERNEL_HOST_FLOAT_OPS
#include "kernel_host.hpp"  // the launch shim, the checked loads and stores, the narrowing; TYPES_TEXT: MixedLayout, MC_ROWS, Dw4, Dw3

// ---- the staging raster and the footprint of every view
static const uint8_t *g_stage; static uint64_t g_bpr, g_need; static int g_px;
struct ViewBox { uint64_t off; int64_t x0, y0, x1, y1; };  // the slot of the view's image and its footprint [x0, x1) x [y0, y1)
static std::vector<ViewBox> g_views;
static uint64_t g_reads;
static void chk_read(const uint8_t *p, uint32_t n, uint32_t align) {
    if ((uintptr_t)p % align) bad("misaligned staging read", (long)(p - g_stage), align);
    if (p < g_stage || p + n > g_stage + g_need) { printf("staging read outside the raster: %ld + %u\n", (long)(p - g_stage), n); abort(); }
    if (n != 1) bad("a staging read of more than one byte", (long)(p - g_stage), n);
    const ViewBox &b = g_views[blockIdx.y];  // the view of the running block
    const uint64_t o = p - g_stage;
    if (o < b.off) { bad("staging read in front of the view's image", (long)o, (long)blockIdx.y); return; }
    const int64_t row = (int64_t)((o - b.off) / g_bpr), col = (int64_t)((o - b.off) % g_bpr);
    if (row < b.y0 || row >= b.y1 || col < b.x0 * g_px || col + n > b.x1 * g_px) bad("staging read outside the view's footprint", (long)row, (long)col);
    g_reads++;
}

#include FLOAT_TEXT     // FloatConsts, the element types, pick4, narrow2, store1, float_chunk: mixed_float.hpp
#include PIXEL_TEXT     // colour_row, pixel_finish, pixel_store, row_narrow, row_wide: mixed_views_pixel.hpp
#include COLOUR_TEXT    // ViewColour: mixed_views_colour.hpp
#include KERNEL_TEXT    // AffineRec, AffineFill and the kernel, cut out of xpng_amd/csrc/mixed_views_affine.hpp by the test

template <class T> static uint32_t elem_bits(float y) {
    if (sizeof(T) == 4) { uint32_t b; memcpy(&b, &y, 4); return b; }
    return FloatElem<T>::KIND == 1 ? to_f16(y) : to_bf16(y);
}
static const FloatConsts K = {{1.0f / 255.0f, 0.01712475383f, 2049.0f / 2048.0f, 259.0f / 256.0f}, {-2.1179039f, 0.5f, 0.0f, -3.25f}};
static const float MATS[4][12] = {
    {0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0},                                                                  // R <- B, G <- R, B <- G
    {0.299f, 0.587f, 0.114f, 0, 0.299f, 0.587f, 0.114f, 0, 0.299f, 0.587f, 0.114f, 0},                      // gray
    {3, -2, 0.5f, -300, -2, 3, 0, 300, 1, 1, -2, 40},                                                       // below 0 and above 255
    {0.70710678f, -0.31830989f, 0.57721566f, 12.345678f, 0.14142135f, 1.6180339f, -0.69314718f, -7.3890561f,
     -0.43429448f, 0.26179939f, 1.2020569f, 31.415926f},                                                    // dense
};
static const float FILLS[2][4] = {{0, 0, 0, 0}, {10.0f, 200.5f, 30.0f, 77.0f}};

struct View { uint32_t img; float m[6]; uint32_t ow, oh; };
// the inverse matrix of a rotation by `deg` and a scale about the centre of the w x h rectangle at (x, y), shown at ow x oh
static View turned(uint32_t img, double x, double y, double w, double h, uint32_t ow, uint32_t oh, double deg, double scale, double shear) {
    const double a = deg * 3.14159265358979323846 / 180.0, c = cos(a) / scale, s = sin(a) / scale, kx = w / ow, ky = h / oh;
    // source = centre + R (P - output centre), then the shear of x by y, then the crop's ratios
    const double r[4] = {c + shear * s, -s + shear * c, s, c};
    View v{img, {}, ow, oh};
    v.m[0] = (float)(kx * r[0]); v.m[1] = (float)(kx * r[1]); v.m[2] = (float)(x + kx * (ow / 2.0 - r[0] * ow / 2.0 - r[1] * oh / 2.0));
    v.m[3] = (float)(ky * r[2]); v.m[4] = (float)(ky * r[3]); v.m[5] = (float)(y + ky * (oh / 2.0 - r[2] * ow / 2.0 - r[3] * oh / 2.0));
    return v;
}
// the footprint, plainly: the four corners in long double, floor - 1 and floor + 2, clipped; empty: all zero
static ViewBox footprint(const View &v, uint64_t off, uint32_t W, uint32_t H) {
    long double lo[2], hi[2];
    for (int a = 0; a < 2; a++) for (int q = 0; q < 4; q++) {
        const long double X = (q & 1 ? v.ow - 1 : 0) + 0.5L, Y = (q & 2 ? v.oh - 1 : 0) + 0.5L;
        const long double s = (long double)v.m[3 * a] * X + (long double)v.m[3 * a + 1] * Y + (long double)v.m[3 * a + 2] - 0.5L;
        if (!q || s < lo[a]) lo[a] = s;
        if (!q || s > hi[a]) hi[a] = s;
    }
    const int64_t x0 = std::max<int64_t>((int64_t)floorl(lo[0]) - 1, 0), x1 = std::min<int64_t>((int64_t)floorl(hi[0]) + 2, (int64_t)W - 1) + 1;
    const int64_t y0 = std::max<int64_t>((int64_t)floorl(lo[1]) - 1, 0), y1 = std::min<int64_t>((int64_t)floorl(hi[1]) + 2, (int64_t)H - 1) + 1;
    if (x0 >= x1 || y0 >= y1) return ViewBox{off, 0, 0, 0, 0};
    return ViewBox{off, x0, y0, x1, y1};
}

// ---- the rule, stated plainly
static float tap(const uint8_t *ras, uint32_t w, int px, const ViewBox &f, const float *fill, int64_t j, int64_t i, int sc) {
    if (j < f.x0 || j >= f.x1 || i < f.y0 || i >= f.y1) return fill[sc];
    return (float)ras[((uint64_t)i * w + (uint64_t)j) * px + sc];
}
static float sampled(uint32_t filter, const uint8_t *ras, uint32_t w, int px, const View &v, const ViewBox &f, const float *fill, uint32_t oy, uint32_t ox, int sc) {
    const float X = (float)ox + 0.5f, Y = (float)oy + 0.5f;
    const float ax = fmaf(v.m[1], Y, v.m[2]), ay = fmaf(v.m[4], Y, v.m[5]);
    const float bx = fmaf(v.m[0], X, ax), by = fmaf(v.m[3], X, ay);
    const float sx = bx - 0.5f, sy = by - 0.5f;
    if (filter == 3) return tap(ras, w, px, f, fill, (int64_t)rintf(sx), (int64_t)rintf(sy), sc);
    const float x0 = floorf(sx), y0 = floorf(sy);
    const float lx = sx - x0, ly = sy - y0;
    const int64_t j = (int64_t)x0, i = (int64_t)y0;
    const float q00 = tap(ras, w, px, f, fill, j, i, sc), q10 = tap(ras, w, px, f, fill, j + 1, i, sc);
    const float q01 = tap(ras, w, px, f, fill, j, i + 1, sc), q11 = tap(ras, w, px, f, fill, j + 1, i + 1, sc);
    const float d0 = q10 - q00, d1 = q11 - q01;
    const float t = fmaf(lx, d0, q00), u = fmaf(lx, d1, q01);
    const float d = u - t;
    return fmaf(ly, d, t);
}
static float rule(uint32_t filter, const uint8_t *ras, uint32_t w, int px, bool bgr, const View &v, const ViewBox &f, const float *fill, const float *m,
                  uint32_t oy, uint32_t ox, int c) {
    float val;
    if (c == 3) val = px == 3 ? 255.0f : sampled(filter, ras, w, px, v, f, fill, oy, ox, 3);
    else {
        const int k = bgr ? 2 - c : c;  // position c holds colour 2 - c of a BGR buffer
        if (!m) val = sampled(filter, ras, w, px, v, f, fill, oy, ox, k);
        else {
            const float *row = m + 4 * k;
            const float r = sampled(filter, ras, w, px, v, f, fill, oy, ox, 0), g = sampled(filter, ras, w, px, v, f, fill, oy, ox, 1), b = sampled(filter, ras, w, px, v, f, fill, oy, ox, 2);
            const float t2 = fmaf(row[2], b, row[3]);
            const float t1 = fmaf(row[1], g, t2);
            const float t = fmaf(row[0], r, t1);
            val = t < 0.0f ? 0.0f : t > 255.0f ? 255.0f : t;
        }
    }
    return fmaf(val, K.scale[c], K.bias[c]);
}

typedef std::vector<std::pair<uint32_t, uint32_t>> Dims;
template <int PX, class T, int PR> static void run(const Dims &dims, const std::vector<View> &views, uint32_t filter, bool colour, const float *fill) {
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
    for (auto &v : views) { g_views.push_back(footprint(v, slot[v.img], dims[v.img].first, dims[v.img].second)); max_oh = std::max(max_oh, v.oh); }
    // the matrices on the heap, exactly nv of them: a read of another view's index past the table is AddressSanitizer's to see
    ViewColour *vm = colour ? (ViewColour *)malloc(nv * sizeof(ViewColour)) : nullptr;
    for (uint32_t v = 0; colour && v < nv; v++) memcpy(vm[v].m, MATS[(v + filter) % 4], sizeof(ViewColour));
    AffineFill af; memcpy(af.v, fill, 16);
    for (int C = 3; C <= 4; C++) for (int planar = 0; planar < 2; planar++) for (int bgr = 0; bgr < 2; bgr++) {
        std::vector<uint8_t *> out(nv); std::vector<uint64_t> sz(nv);
        AffineRec *vr = (AffineRec *)malloc(nv * sizeof(AffineRec));
        std::vector<std::pair<uint8_t *, uint8_t *>> box;  // every view's buffer; g_out holds the running block's alone
        for (uint32_t v = 0; v < nv; v++) {
            const View &w = views[v]; const ViewBox &f = g_views[v];
            const uint64_t lead = 64 + ES * (v % 8);
            sz[v] = (uint64_t)C * w.ow * w.oh * ES;
            out[v] = (uint8_t *)aligned_alloc(64, rup(lead + sz[v] + 64, 64));  // (16-byte aligned base, so `lead` sets the start modulo 16)
            memset(out[v], 0xA5, lead + sz[v] + 64);
            vr[v] = AffineRec{slot[w.img], out[v] + lead, {w.m[0], w.m[1], w.m[2], w.m[3], w.m[4], w.m[5]}, w.ow, w.oh, (int32_t)f.x0, (int32_t)f.y0, (int32_t)f.x1, (int32_t)f.y1};
            box.push_back({out[v] + lead, out[v] + lead + sz[v]});
        }
        const uint32_t gx = (max_oh + AF_ROWS - 1) / AF_ROWS;
        // a store must lie inside the buffer of the view whose block makes it
        auto go = [&](auto k) { launch(gx, nv, [&] { g_out.assign(1, box[blockIdx.y]); k(vr, vm, stage, bpr, (uint32_t)(bgr ? 2 : 0), filter, af, K); }); };
        if (C == 3 && planar) go(k_mixed_views_affine<PX, 3, true, T, PR>); else if (C == 3) go(k_mixed_views_affine<PX, 3, false, T, PR>);
        else if (planar) go(k_mixed_views_affine<PX, 4, true, T, PR>); else go(k_mixed_views_affine<PX, 4, false, T, PR>);
        for (uint32_t v = 0; v < nv; v++) {
            const View &w = views[v]; const uint8_t *o = vr[v].buf; const uint64_t lead = 64 + ES * (v % 8);
            for (uint64_t k = 0; k < lead + sz[v] + 64; k++) { const uint8_t *p = out[v] + k; if ((p < o || p >= o + sz[v]) && *p != 0xA5) { printf("sentinel px%d C%d pl%d bgr%d es%u view%u out %ux%u at %ld\n", PX, C, planar, bgr, ES, v, w.ow, w.oh, (long)(p - o)); errors++; break; } }
            int stop = 0;
            for (uint32_t y = 0; y < w.oh && !stop; y++) for (uint32_t x = 0; x < w.ow && !stop; x++) for (int c = 0; c < C; c++) {
                const uint64_t e = planar ? ((uint64_t)c * w.oh + y) * w.ow + x : ((uint64_t)y * w.ow + x) * C + c;
                uint32_t got = 0; memcpy(&got, o + e * ES, ES);
                const uint32_t exp = elem_bits<T>(rule(filter, ras[w.img].data(), dims[w.img].first, PX, bgr, w, g_views[v], fill, colour ? vm[v].m : nullptr, y, x, c));
                if (got != exp) { printf("value px%d C%d pl%d bgr%d kind%d filter%u pr%d view%u img%u out %ux%u y%u x%u c%d: %x, expected %x\n", PX, C, planar, bgr, FloatElem<T>::KIND, filter, PR, v, w.img, w.ow, w.oh, y, x, c, got, exp); errors++; stop = 1; break; }
            }
            free(out[v]);
        }
        free(vr);
    }
    free(vm);
    free(stage);
}
template <int PX, int PR> static void run_all(const Dims &dims, const std::vector<View> &views, int round) {
    for (uint32_t filter = 0; filter < 4; filter += 3) {
        const bool colour = (round + filter) & 1;
        const float *fill = FILLS[(round + (filter ? 1 : 0)) & 1];
        run<PX, f16_t, PR>(dims, views, filter, colour, fill); run<PX, bf16_t, PR>(dims, views, filter, !colour, fill); run<PX, float, PR>(dims, views, filter, colour, FILLS[1]);
    }
}
int main() {
    // image 5 has no view; images 0 and 1 have several
    const Dims dims = {{64, 64}, {445, 14}, {100, 40}, {7, 3}, {1, 1}, {300, 5}};
    // output widths shifted by 0 .. 7: every start of a row and of a plane row modulo 16 bytes, rows shorter than one 16-byte store,
    // plane sizes on both sides of the planar kernel's test
    for (uint32_t sh = 0; sh < 8; sh++) {
        const std::vector<View> views = {
            turned(0, 8, 8, 48, 48, 19 + sh, 35, 30.0, 1.0, 0.0),        // a rotated view inside its image, the tallest: three blocks
            turned(0, 10, 10, 30, 30, 33 + sh, 11, -45.0, 0.8, 0.18),     // a shear with a scale: hangs over the image's corners
            turned(0, 40, 30, 44, 59, 3 + sh, 5, 77.7, 1.3, -0.36),       // partly outside the image on the right and below
            {1, {1, 0, 440, 0, 1, 3}, 9 + sh, 8},                          // an integer translation that runs past the last column
            {1, {-1, 0, 445, 0, 1, 0}, 16 + sh, 8},                        // a mirror; with sh == 0 the planes are multiples of 16 bytes
            {1, {0, 1, 100, -1, 0, 14}, 14, 9 + sh},                       // an exact quarter turn
            {2, {1, 0, 1000, 0, 1, -500}, 16 + sh, 9},                     // an empty footprint: all fill, no read
            turned(2, 0, 0, 100, 40, 16, 16 + sh, 12.5, 0.5, 0.0),        // zoomed out: the image inside a frame of fill
            turned(3, 0, 0, 7, 3, 13 + sh, 2, 170.0, 1.0, 0.0),           // a tiny image upside down
            {4, {0.25f, 0, 0, 0, 0.25f, 0}, 4 + sh, 8},                    // one pixel to many
        };
        for (auto &v : views) for (int e = 0; e < 6; e++) if (!(fabs((double)v.m[e]) * (e % 3 == 0 ? v.ow : e % 3 == 1 ? v.oh : 1) <= 262144.0)) bad("a view outside the entry bounds", e, 0);
        g_reads = 0;
        run_all<3, 4>(dims, views, (int)sh); run_all<4, 4>(dims, views, (int)sh);
        if (sh < 2) { run_all<3, 1>(dims, views, (int)sh); run_all<4, 1>(dims, views, (int)sh); }
        if (!g_reads) bad("no staging read at all", sh, 0);
    }
    // an output row wider than one pass of a row's lanes (16 or 64 stores of 4 or 8 elements), beside a view of one row
    const std::vector<View> wide = {turned(5, 0, 0, 300, 5, 600, 2, 1.0, 1.0, 0.0), turned(1, 3, 1, 440, 12, 530, 1, -2.0, 1.0, 0.0),
                                    turned(5, 100, 0, 200, 5, 96, 19, 90.0, 1.0, 0.0), turned(3, 0, 0, 7, 3, 5, 3, 45.0, 1.0, 0.0)};
    run_all<3, 4>(dims, wide, 0); run_all<4, 4>(dims, wide, 1); run_all<3, 1>(dims, wide, 1); run_all<4, 1>(dims, wide, 0);
    printf("errors: %d\n", errors);
    return errors != 0;
}
