// Host run of k_mixed_views_tone_stats and k_mixed_views_tone_apply (xpng_amd/csrc/mixed_views_tone.hpp): every thread of every
// block of both kernels, launched step index after step index as the call launches them, over views of 3 and of 4 planes.
// The kernels have barriers and a wave exchange, so a block's 256 threads are fibers (ucontext) with stacks of their own: the
// barrier and the exchange hand control back to the block's scheduler, which resumes the threads round after round and checks that
// in every round either all of a block's live threads stop there or none does.  The exchange is a table of the 256 lanes' values
// in two alternating copies: a lane writes its value, stops, and reads its partner's after the round.  The host run is sequential,
// so the LDS and global atomics are plain operations.  The kernels' LDS arrays are statics; a block that read what it never wrote
// would read the block before it.
// One launch holds views of 1 x 1, 1 x 300, 300 x 1, 15 x 16, 16 x 16, every pair out of 63, 64, 65 by 15, 16, 17, 130 x 40, and
// 300 x 200 (several chunks), with one to four steps, up to three of them statistics steps, so blocks of views with fewer chunks,
// with another kind of step or with no step at that index must return.  Planes hold values below 0 and above 255 and -0.0f (the
// entry clamp), whole numbers (so that equalise moves them), flat regions, constant planes, extremes that lie only in the last
// short chunk, and planes whose range is so small that autocontrast's scale is infinite.  Each view's planes are a slice of one scratch block rounded up to 256 bytes, as the call lays them out.
// The shims check that every read and write of the scratch lies inside the three colour planes of the view whose block makes it
// and that a 16-byte access is aligned, and that every statistics access lies inside the slot of that view and step; the scratch
// and the slots are heap blocks, so AddressSanitizer sees anything else.  The expected value of every float is this file's own plain
// statement of the rule (include/xpng_hip.h), and the alpha plane must come back untouched.
// Built and run by tests/test_views_tone_kernels_host.py.
#include <ucontext.h>

#include <functional>

#include "kernel_host.hpp"

struct float4 { float x, y, z, w; };

// ---- the scratch, the slots and what the running block may touch
static float *g_scratch;
static uint32_t *g_stats;
struct Slice { uint64_t off, n; };  // the three colour planes, in floats
static std::vector<Slice> g_slices;
static std::vector<std::vector<uint32_t>> g_slots;  // per view and step index: the slot, or ~0u
static uint32_t g_si;
constexpr uint32_t SLOT_WORDS = 3 * 258;
static void chk_scratch(const float *p, uint32_t n) {
    const Slice &s = g_slices[blockIdx.y];
    if (p < g_scratch + s.off || p + n > g_scratch + s.off + s.n) { printf("scratch access outside the view's colour planes: view %u at %ld (%u floats)\n", blockIdx.y, (long)(p - g_scratch), n); abort(); }
    if (n == 4 && ((uintptr_t)p & 15)) { printf("misaligned 16-byte access: view %u at %ld\n", blockIdx.y, (long)(p - g_scratch)); abort(); }
}
static void chk_stat(const uint32_t *p) {
    const uint32_t slot = g_slots[blockIdx.y][g_si];
    if (slot == ~0u || p < g_stats + (uint64_t)slot * SLOT_WORDS || p >= g_stats + (uint64_t)(slot + 1) * SLOT_WORDS) { printf("statistics access outside the view's slot: view %u step %u at %ld\n", blockIdx.y, g_si, (long)(p - g_stats)); abort(); }
}
static float tone_ld(const float *p) { chk_scratch(p, 1); return *p; }
static void tone_st(float *p, float v) { chk_scratch(p, 1); *p = v; }
static float4 tone_ld4(const float *p) { chk_scratch(p, 4); float4 v; memcpy(&v, p, 16); return v; }
static void tone_st4(float *p, float4 v) { chk_scratch(p, 4); memcpy(p, &v, 16); }
static void tone_lds_add(uint32_t *p) { (*p)++; }
static uint32_t tone_stat_ld(const uint32_t *p) { chk_stat(p); return *p; }
static void tone_stat_add(uint32_t *p, uint32_t v) { chk_stat(p); *p += v; }
static void tone_stat_max(uint32_t *p, uint32_t v) { chk_stat(p); *p = std::max(*p, v); }
static float tone_div(float a, float b) { return a / b; }  // IEEE: correctly rounded

// ---- a block's threads as fibers
constexpr size_t FIBER_STACK = 256 << 10;
static ucontext_t g_sched, g_fib[256];
static char *g_stack[256];
static bool g_done[256], g_stopped[256];
static uint32_t g_cur, g_xv[2][256], g_xn[256];
static std::function<void()> g_body;
static void fiber_main() {
    g_body();
    g_done[g_cur] = true;
    swapcontext(&g_fib[g_cur], &g_sched);
}
static void tone_sync() {
    g_stopped[g_cur] = true;
    swapcontext(&g_fib[g_cur], &g_sched);
}
static uint32_t tone_xor(uint32_t v, uint32_t m) {
    const uint32_t me = g_cur, copy = g_xn[me]++ & 1;
    g_xv[copy][me] = v;
    tone_sync();
    return g_xv[copy][(me & ~63u) | ((me ^ m) & 63u)];
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
            g_done[t] = false; g_xn[t] = 0;
        }
        for (;;) {
            uint32_t waiting = 0, finished = 0, ran = 0;
            for (uint32_t t = 0; t < 256; t++) {
                if (g_done[t]) continue;
                g_cur = t; threadIdx = {t, 0, 0}; g_stopped[t] = false; ran++;
                swapcontext(&g_sched, &g_fib[t]);
                if (g_stopped[t]) waiting++; else finished++;
            }
            if (!ran) break;
            if (waiting && finished) { bad("a barrier or an exchange that not every live thread of the block reached", x, y); abort(); }
        }
    }
}

#define __shared__ static
#include KERNEL_TEXT  // the ops, the chunk, ToneRec, tone_entry and both kernels, cut out of xpng_amd/csrc/mixed_views_tone.hpp by the test

// ---- the rule, stated plainly
struct Step { uint32_t op; float arg; };  // posterise: bits
struct View { uint32_t ow, oh; int kind; std::vector<Step> steps; };
static void plain_steps(float *p, uint64_t N, const std::vector<Step> &steps) {
    for (uint64_t i = 0; i < N; i++) p[i] = p[i] > 0.0f ? (p[i] > 255.0f ? 255.0f : p[i]) : 0.0f;
    for (const Step &s : steps) {
        if (s.op == 1) {
            float lo = p[0], hi = p[0];
            for (uint64_t i = 0; i < N; i++) { lo = std::min(lo, p[i]); hi = std::max(hi, p[i]); }
            if (hi == lo) continue;
            const float sc = 255.0f / (hi - lo);
            if (std::isinf(sc)) continue;
            for (uint64_t i = 0; i < N; i++) { const float d = p[i] - lo; const float t = d * sc; p[i] = t > 255.0f ? 255.0f : t; }
        } else if (s.op == 2) {
            std::vector<uint64_t> h(256, 0);
            for (uint64_t i = 0; i < N; i++) h[(uint32_t)nearbyintf(p[i])]++;
            int last = 255;
            while (!h[last]) last--;
            const uint64_t step = (N - h[last]) / 255;
            if (!step) continue;
            std::vector<float> lut(256);
            uint64_t before = 0;
            for (int n = 0; n < 256; n++) { lut[n] = (float)std::min<uint64_t>(255, (step / 2 + before) / step); before += h[n]; }
            for (uint64_t i = 0; i < N; i++) p[i] = lut[(uint32_t)nearbyintf(p[i])];
        } else if (s.op == 3) {
            const float m = (float)(1u << (8u - (uint32_t)s.arg));
            for (uint64_t i = 0; i < N; i++) p[i] = p[i] - fmodf(p[i], m);
        } else if (s.op == 4) {
            for (uint64_t i = 0; i < N; i++) p[i] = p[i] >= s.arg ? 255.0f - p[i] : p[i];
        } else {
            for (uint64_t i = 0; i < N; i++) p[i] = 255.0f - p[i];
        }
    }
}

static long g_clamped = 0, g_step0 = 0, g_returned = 0;
static void fill_plane(float *p, uint64_t N, int kind, int q) {
    for (uint64_t i = 0; i < N; i++) {
        if (kind == 5) { p[i] = (i & 1) ? 2e-38f : 0.0f; continue; }  // hi - lo so small that 255 / (hi - lo) is infinite
        switch ((kind + q) % 5) {
        case 0: p[i] = (float)(rand() % 70000) / 256.0f - 6.0f; break;   // -6 .. 267.4: past both ends of the clamp
        case 1: p[i] = (float)(rand() % 256); break;                      // whole numbers
        case 2: p[i] = i % 97 == 0 ? -0.0f : 40.0f + (float)(rand() % 3); break;  // a flat region: three bins, and -0.0f
        case 3: p[i] = 77.25f; break;                                     // constant
        default: p[i] = 50.0f + (float)(rand() % 100) * 0.5f;             // the extremes only at the very end (below)
        }
    }
    if ((kind + q) % 5 == 4 && N > 2) { p[N - 2] = 1.5f; p[N - 1] = 254.0f; }
}
static void run(int C, const std::vector<View> &views) {
    const uint32_t nv = views.size();
    std::vector<Slice> sl(nv);
    std::vector<uint64_t> off(nv);
    uint64_t total = 0, need = 0;
    for (uint32_t v = 0; v < nv; v++) {
        const uint64_t N = (uint64_t)views[v].oh * views[v].ow;
        off[v] = total;
        sl[v] = {total, 3 * N};
        need = total + C * N;
        total += rup(C * N * 4, 256) / 4;
    }
    float *scratch = (float *)aligned_alloc(256, rup(need * 4, 256));  // (ends within the last view's rounding: ASan sees a step past it)
    std::vector<float> want(need);
    ToneRec *tr = (ToneRec *)malloc(nv * sizeof(ToneRec));  // exactly nv records on the heap
    std::vector<std::vector<uint32_t>> slots(nv, std::vector<uint32_t>(4, ~0u));
    uint32_t nslots = 0, max_chunks = 0;
    for (uint32_t v = 0; v < nv; v++) {
        const View &w = views[v];
        const uint64_t N = (uint64_t)w.oh * w.ow;
        for (int q = 0; q < C; q++) fill_plane(scratch + off[v] + q * N, N, w.kind, q);
        std::copy(scratch + off[v], scratch + off[v] + C * N, want.begin() + off[v]);
        for (int q = 0; q < 3; q++) {
            for (uint64_t i = 0; i < N; i++) { const float f = want[off[v] + q * N + i]; g_clamped += f < 0.0f || f > 255.0f; }
            plain_steps(want.data() + off[v] + q * N, N, w.steps);
        }
        tr[v] = ToneRec{off[v], (uint32_t)N, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (size_t si = 0; si < w.steps.size(); si++) {
            tr[v].op[si] = (uint8_t)w.steps[si].op;
            tr[v].arg[si] = w.steps[si].op == 3 ? (float)(1u << (8u - (uint32_t)w.steps[si].arg)) : w.steps[si].arg;
            if (w.steps[si].op == 1 || w.steps[si].op == 2) { slots[v][si] = nslots; tr[v].slot[si] = nslots++; }
        }
        max_chunks = std::max(max_chunks, (uint32_t)((3 * N + TONE_CHUNK - 1) / TONE_CHUNK));
    }
    uint32_t *stats = (uint32_t *)calloc((size_t)nslots * SLOT_WORDS, 4);  // zeroed, as the call zeroes them on the stream
    g_scratch = scratch; g_stats = stats; g_slices = sl; g_slots = slots;
    for (uint32_t si = 0; si < 4; si++) {
        bool any = false, stat = false;
        for (uint32_t v = 0; v < nv; v++) { any |= tr[v].op[si] != 0; stat |= tr[v].op[si] == 1 || tr[v].op[si] == 2; g_returned += tr[v].op[si] == 0; }
        if (!any) break;
        g_si = si;
        if (stat) launch_fibers(max_chunks, nv, [&] { k_mixed_views_tone_stats(tr, scratch, stats, si); });
        launch_fibers(max_chunks, nv, [&] { k_mixed_views_tone_apply(tr, scratch, stats, si); });
    }
    for (uint32_t v = 0; v < nv; v++) {
        const View &w = views[v];
        const uint64_t N = (uint64_t)w.oh * w.ow;
        for (uint64_t i = 0; i < (uint64_t)C * N; i++) {
            uint32_t a, b;
            memcpy(&a, scratch + off[v] + i, 4); memcpy(&b, &want[off[v] + i], 4);
            if (a != b) { printf("value C%d view%u %ux%u kind%d steps%zu plane%lu at %lu: %x, expected %x\n", C, v, w.ow, w.oh, w.kind, w.steps.size(), (unsigned long)(i / N), (unsigned long)(i % N), a, b); errors++; break; }
        }
        // an equalise alone over at most 255 pixels has step 0 and must leave fractional values as the entry clamp left them
        if (w.steps.size() == 1 && w.steps[0].op == 2 && N <= 255) g_step0++;
    }
    free(stats); free(tr); free(scratch);
}
int main() {
    const Step AC{1, 0.0f}, EQ{2, 0.0f}, INV{5, 0.0f};
    const std::vector<std::vector<Step>> lists = {
        {AC}, {EQ}, {{3, 3.0f}}, {{4, 100.5f}}, {INV}, {EQ, AC}, {AC, EQ}, {EQ, {4, 128.0f}, AC, {3, 2.0f}}, {INV, EQ, {4, 0.0f}, EQ}, {{3, 0.0f}, AC},
        {{3, 8.0f}}, {AC, AC, EQ, INV}, {{4, 255.0f}, EQ}, {{3, 1.0f}, {3, 4.0f}}, {EQ, EQ}};
    std::vector<std::pair<uint32_t, uint32_t>> sizes = {{1, 1}, {1, 300}, {300, 1}, {15, 16}, {16, 16}, {130, 40}, {300, 200}};
    for (uint32_t w : {63u, 64u, 65u}) for (uint32_t h : {15u, 16u, 17u}) sizes.push_back({w, h});
    std::vector<View> views;
    for (size_t i = 0; i < sizes.size(); i++)
        for (size_t j = 0; j < 2; j++) views.push_back({sizes[i].first, sizes[i].second, (int)(i + 2 * j), lists[(2 * i + j) % lists.size()]});
    views.push_back({15, 16, 0, {EQ}});   // 240 pixels: step 0
    views.push_back({300, 200, 4, {AC, EQ}});  // the extremes in the last short chunk of a view of 22 chunks
    views.push_back({70, 50, 4, {EQ, AC, INV}});
    views.push_back({65, 17, 5, {AC, EQ, AC}});  // an infinite scale: autocontrast leaves the planes, no NaN reaches equalise
    run(3, views);
    run(4, views);
    if (!g_clamped) { printf("the entry clamp was never taken\n"); errors++; }
    if (!g_step0) { printf("no equalise with step 0\n"); errors++; }
    if (!g_returned) { printf("no block had to return for a missing step\n"); errors++; }
    printf("views: %zu\nerrors: %d\n", views.size(), errors);
    return errors != 0;
}
