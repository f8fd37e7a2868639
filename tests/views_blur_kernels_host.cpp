// Host run of k_mixed_views_blur (xpng_amd/csrc/mixed_views_blur.hpp): every thread of every block, over both channel counts, both
// layouts, both colour orders and the three element types (all 12 instances, each with and without the BGR exchange), with the shims
// for the device operations of tests/kernel_host.hpp (the kernel reuses fma_f32, pick4 and store1 of mixed_float.hpp and pixel_store of mixed_views_pixel.hpp, whose text is
// compiled in front of it).
// The kernel has barriers, so a block's 256 threads cannot simply run one after another: every thread is a fiber (ucontext) with a
// stack of its own, the barrier hands control back to the block's scheduler, and the scheduler resumes the threads round after
// round.  It also checks what a barrier requires: in every round either all of a block's live threads reach a barrier or none does.
// The kernel's LDS arrays are statics of the instance; a block that read what it never wrote would read the block before it.
// One launch holds views of every radius in {0, 1, 11, 31} with widths out of {R + 1, 63, 64, 65, 130} and heights out of
// {R + 1, 15, 16, 17, 40} - every edge of the 64 x 16 tile from both sides, more than one tile on both axes, views of one tile, and
// the grid is the largest view's, so blocks of small views must return - with the solarise off, at 0, 128, 255 and at 100.5, and with
// planes that hold values below 0 and above 255 so that the clamp is taken.  Each view's planes are a slice of one scratch block
// rounded up to 256 bytes, as the call lays them out.
// The shim of the scratch reads checks that every read lies inside the slice of the view whose block makes it; the shims of the
// stores check that every store lies inside THAT view's buffer and is aligned to its width; the buffers are heap blocks, so
// AddressSanitizer sees anything else.  The expected value of every element is this file's own plain statement of the rule
// (DESIGN.md 23): its own weights in double, fmaf(), single fp32 sums, its own round-to-nearest-even conversions.
// Built and run by tests/test_views_blur_kernels_host.py.
#define KERNEL_HOST_FLOAT_OPS
#include <ucontext.h>

#include <functional>

#include "kernel_host.hpp"  // the error count, the checked stores, the narrowing; TYPES_TEXT: MixedLayout, MC_ROWS, Dw4, Dw3

static void chk_read(const uint8_t *, uint32_t, uint32_t) { bad("a staging read: this kernel has none", 0, 0); abort(); }

// ---- the scratch and the slice of every view
static const float *g_scratch;
struct Slice { uint64_t off, n; };  // in floats
static std::vector<Slice> g_slices;
static float scratch_ld(const float *p) {
    const Slice &s = g_slices[blockIdx.y];  // the view of the running block
    if (p < g_scratch + s.off || p >= g_scratch + s.off + s.n) { printf("scratch read outside the view's slice: view %u at %ld\n", blockIdx.y, (long)(p - g_scratch)); abort(); }
    return *p;
}

// ---- a block's threads as fibers
constexpr size_t FIBER_STACK = 256 << 10;
static ucontext_t g_sched, g_fib[256];
static char *g_stack[256];
static bool g_done[256], g_at_barrier[256];
static uint32_t g_cur;
static std::function<void()> g_body;
static void fiber_main() {
    g_body();
    g_done[g_cur] = true;
    swapcontext(&g_fib[g_cur], &g_sched);
}
static void blur_sync() {
    g_at_barrier[g_cur] = true;
    swapcontext(&g_fib[g_cur], &g_sched);
}
template <class F> static void launch_fibers(uint32_t gx, uint32_t gy, F f) {
    gridDim = {gx, gy, 1}; blockDim = {256, 1, 1};
    g_body = f;
    for (uint32_t y = 0; y < gy; y++) for (uint32_t x = 0; x < gx; x++) {
        blockIdx = {x, y, 0};
        for (uint32_t t = 0; t < 256; t++) {
            if (!g_stack[t]) g_stack[t] = (char *)malloc(FIBER_STACK);
            getcontext(&g_fib[t]);
            g_fib[t].uc_stack.ss_sp = g_stack[t]; g_fib[t].uc_stack.ss_size = FIBER_STACK; g_fib[t].uc_link = nullptr;
            makecontext(&g_fib[t], fiber_main, 0);
            g_done[t] = false;
        }
        for (;;) {
            uint32_t waiting = 0, finished = 0, ran = 0;
            for (uint32_t t = 0; t < 256; t++) {
                if (g_done[t]) continue;
                g_cur = t; threadIdx = {t, 0, 0}; g_at_barrier[t] = false; ran++;
                swapcontext(&g_sched, &g_fib[t]);
                if (g_at_barrier[t]) waiting++; else finished++;
            }
            if (!ran) break;
            if (waiting && finished) { bad("a barrier that not every live thread of the block reached", x, y); abort(); }
        }
    }
}

#define __shared__ static
#include FLOAT_TEXT   // FloatConsts, the element types, pick4, narrow2, store1: mixed_float.hpp
#include PIXEL_TEXT   // pixel_store (and the row writers, which this kernel does not use): mixed_views_pixel.hpp
#include KERNEL_TEXT  // BlurRec, blur_refl and the kernel, cut out of xpng_amd/csrc/mixed_views_blur.hpp by the test

template <class T> static uint32_t elem_bits(float y) {
    if (sizeof(T) == 4) { uint32_t b; memcpy(&b, &y, 4); return b; }
    return FloatElem<T>::KIND == 1 ? to_f16(y) : to_bf16(y);
}
static const FloatConsts K = {{1.0f / 255.0f, 0.01712475383f, 2049.0f / 2048.0f, 259.0f / 256.0f}, {-2.1179039f, 0.5f, 0.0f, -3.25f}};

// ---- the rule, stated plainly
struct View { uint32_t ow, oh, R; float sigma, thr; };
static void weights(float sigma, uint32_t R, float *w) {
    double g[32], t = 0.0;
    const double s = (double)sigma;
    for (uint32_t d = 0; d <= R; d++) g[d] = R ? exp(-(double)(d * d) / (2.0 * s * s)) : 1.0;
    for (uint32_t d = 1; d <= R; d++) t += g[d];
    const double S = g[0] + 2.0 * t;
    for (uint32_t d = 0; d <= R; d++) w[d] = (float)(g[d] / S);
}
static long refl(long i, long n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }
// the blurred and clamped plane of q (oh x ow)
static std::vector<float> blurred(const float *q, const View &v, const float *w) {
    std::vector<float> h((size_t)v.oh * v.ow), o((size_t)v.oh * v.ow);
    for (long y = 0; y < v.oh; y++) for (long x = 0; x < v.ow; x++) {
        float A = 0.0f;
        for (long d = v.R; d >= 1; d--) { const float s = q[y * v.ow + refl(x - d, v.ow)] + q[y * v.ow + refl(x + d, v.ow)]; A = fmaf(w[d], s, A); }
        h[y * v.ow + x] = fmaf(w[0], q[y * v.ow + x], A);
    }
    for (long y = 0; y < v.oh; y++) for (long x = 0; x < v.ow; x++) {
        float A = 0.0f;
        for (long d = v.R; d >= 1; d--) { const float s = h[refl(y - d, v.oh) * v.ow + x] + h[refl(y + d, v.oh) * v.ow + x]; A = fmaf(w[d], s, A); }
        A = fmaf(w[0], h[y * v.ow + x], A);
        o[y * v.ow + x] = A < 0.0f ? 0.0f : A > 255.0f ? 255.0f : A;
    }
    return o;
}

static long g_clamped = 0;
template <int C, class T> static void run(const std::vector<View> &views) {
    const uint32_t nv = views.size(), ES = sizeof(T);
    // the scratch: every view's C planes in a slice rounded up to 256 bytes; the block ends with the last view's last float
    std::vector<Slice> sl(nv);
    uint64_t total = 0, need = 0;
    for (uint32_t v = 0; v < nv; v++) {
        sl[v] = {total, (uint64_t)C * views[v].oh * views[v].ow};
        need = total + sl[v].n;
        total += rup(sl[v].n * 4, 256) / 4;
    }
    float *scratch = (float *)malloc(need * 4);
    for (uint64_t i = 0; i < need; i++) scratch[i] = (float)(rand() % 70000) / 256.0f - 6.0f;  // -6 .. 267.4: past both ends of the clamp
    g_scratch = scratch; g_slices = sl;
    // what the rule gives before solarise and the constants: per view, C planes
    std::vector<std::vector<float>> b(nv);
    uint32_t max_tiles = 0;
    for (uint32_t v = 0; v < nv; v++) {
        const View &w = views[v]; const uint64_t plane = (uint64_t)w.oh * w.ow;
        b[v].assign(scratch + sl[v].off, scratch + sl[v].off + sl[v].n);
        if (w.R) {
            float wt[32]; weights(w.sigma, w.R, wt);
            for (int q = 0; q < 3; q++) {
                const std::vector<float> o = blurred(scratch + sl[v].off + q * plane, w, wt);
                for (float f : o) g_clamped += f == 0.0f || f == 255.0f;
                std::copy(o.begin(), o.end(), b[v].begin() + q * plane);
            }
        }
        max_tiles = std::max(max_tiles, ((w.ow + 63) / 64) * ((w.oh + 15) / 16));
    }
    for (int planar = 0; planar < 2; planar++) for (int bgr = 0; bgr < 2; bgr++) {
        std::vector<uint8_t *> out(nv); std::vector<uint64_t> sz(nv);
        std::vector<std::pair<uint8_t *, uint8_t *>> box;  // every view's buffer; g_out holds the running block's alone
        BlurRec *br = (BlurRec *)malloc(nv * sizeof(BlurRec));  // exactly nv records on the heap
        for (uint32_t v = 0; v < nv; v++) {
            const View &w = views[v];
            const uint64_t lead = 64 + ES * (v % 8);
            sz[v] = (uint64_t)C * w.ow * w.oh * ES;
            out[v] = (uint8_t *)aligned_alloc(64, rup(lead + sz[v] + 64, 64));
            memset(out[v], 0xA5, lead + sz[v] + 64);
            br[v] = BlurRec{sl[v].off, out[v] + lead, w.ow, w.oh, w.R, w.thr, {}};
            weights(w.sigma, w.R, br[v].w);
            box.push_back({out[v] + lead, out[v] + lead + sz[v]});
        }
        auto go = [&](auto k) { launch_fibers(max_tiles, nv, [&] { g_out.assign(1, box[blockIdx.y]); k(br, scratch, (uint32_t)(bgr ? 2 : 0), K); }); };
        if (planar) go(k_mixed_views_blur<C, true, T>); else go(k_mixed_views_blur<C, false, T>);
        for (uint32_t v = 0; v < nv; v++) {
            const View &w = views[v]; const uint8_t *o = br[v].buf; const uint64_t lead = 64 + ES * (v % 8), plane = (uint64_t)w.oh * w.ow;
            for (uint64_t k = 0; k < lead + sz[v] + 64; k++) { const uint8_t *p = out[v] + k; if ((p < o || p >= o + sz[v]) && *p != 0xA5) { printf("sentinel C%d pl%d bgr%d es%u view%u out %ux%u at %ld\n", C, planar, bgr, ES, v, w.ow, w.oh, (long)(p - o)); errors++; break; } }
            int stop = 0;
            for (uint32_t y = 0; y < w.oh && !stop; y++) for (uint32_t x = 0; x < w.ow && !stop; x++) for (int c = 0; c < C; c++) {
                const uint64_t e = planar ? ((uint64_t)c * w.oh + y) * w.ow + x : ((uint64_t)y * w.ow + x) * C + c;
                uint32_t got = 0; memcpy(&got, o + e * ES, ES);
                float val = b[v][(uint64_t)(c == 3 ? 3 : bgr ? 2 - c : c) * plane + (uint64_t)y * w.ow + x];
                if (c < 3 && w.thr < 256.0f && val >= w.thr) val = 255.0f - val;
                const uint32_t exp = elem_bits<T>(fmaf(val, K.scale[c], K.bias[c]));
                if (got != exp) { printf("value C%d pl%d bgr%d kind%d view%u out %ux%u R%u thr %g y%u x%u c%d: %x, expected %x\n", C, planar, bgr, FloatElem<T>::KIND, v, w.ow, w.oh, w.R, (double)w.thr, y, x, c, got, exp); errors++; stop = 1; break; }
            }
            free(out[v]);
        }
        free(br);
    }
    free(scratch);
}
int main() {
    std::vector<View> views;
    const uint32_t radii[4] = {0, 1, 11, 31};
    const float sigmas[4] = {0.0f, 0.5f, 3.7f, 9.5f}, thrs[5] = {256.0f, 0.0f, 128.0f, 255.0f, 100.5f};
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t R = radii[r], ows[5] = {R + 1, 63, 64, 65, 130}, ohs[5] = {R + 1, 15, 16, 17, 40};
        // every width and every height of the list at least once per radius, where the radius lies below it
        for (uint32_t i = 0; i < 5; i++) for (uint32_t j : {i, (i + 1 + r) % 5}) {
            if (R >= ows[i] || R >= ohs[j]) continue;
            views.push_back({ows[i], ohs[j], R, sigmas[r], R ? thrs[views.size() % 5] : thrs[1 + views.size() % 4]});  // (radius 0: solarise alone)
        }
    }
    for (const View &v : views) if (v.R == 0 && v.thr == 256.0f) { printf("a view that needs no second pass\n"); return 1; }
    run<3, f16_t>(views); run<3, bf16_t>(views); run<3, float>(views);
    run<4, f16_t>(views); run<4, bf16_t>(views); run<4, float>(views);
    if (!g_clamped) { printf("the clamp was never taken\n"); errors++; }
    printf("views: %zu\nerrors: %d\n", views.size(), errors);
    return errors != 0;
}
