// Host run of k_mixed_copy / k_mixed_pack and k_mixed_copy_as / k_mixed_pack_from (xpng_amd/csrc/mixed.hpp): every thread of every
// block, one after another, the tight pair and all layouts, with shims for v_perm, v_alignbyte and ld32u.  ld32u checks the read
// rule (every aligned dword it loads holds a byte of an allowed range); the staging raster is a heap block of its exact size, so
// AddressSanitizer sees any other access outside it.
// Built and run by tests/test_layout_kernels_host.py: g++ -fsanitize=address -static-libasan -DKERNEL_TEXT=\"...\".
#include "kernel_host.hpp"  // the launch shim, v_perm and v_alignbyte
// allowed read ranges for ld32u: every aligned dword it loads must hold a byte of one of them
static std::vector<std::pair<uintptr_t, uintptr_t>> g_ok;
static void chk(uintptr_t q) { for (auto &r : g_ok) if (q + 4 > r.first && q < r.second) return; printf("ld32u outside: %lx\n", (unsigned long)q); abort(); }
static uint32_t ld32u(const uint8_t *p) {
    uintptr_t a = (uintptr_t)p; const uint32_t *q = (const uint32_t *)(a & ~(uintptr_t)3); uint32_t sh = (a & 3) * 8;
    chk((uintptr_t)q); uint32_t lo = q[0]; if (!sh) return lo; chk((uintptr_t)(q + 1)); return (lo >> sh) | (q[1] << (32 - sh));
}
#include KERNEL_TEXT  // the four kernels, their record and MC_ROWS, cut out of xpng_amd/csrc/mixed.hpp by the test
// caller's byte (img, y, x, c) of layout from an interleaved raster of px bytes
static uint8_t want(const uint8_t *ras, uint32_t w, int px, int C, bool bgr, uint32_t y, uint32_t x, int c) {
    if (c == 3) return px == 4 ? ras[((uint64_t)y * w + x) * px + 3] : 0xFF;
    return ras[((uint64_t)y * w + x) * px + (bgr ? 2 - c : c)];
}
template <int PX> static void run(const std::vector<std::pair<uint32_t, uint32_t>> &dims) {
    const uint32_t n = dims.size(); uint64_t maxw = 0, maxh = 0;
    for (auto &d : dims) { maxw = std::max<uint64_t>(maxw, d.first); maxh = std::max<uint64_t>(maxh, d.second); }
    const uint64_t bpr = rup(maxw * PX, 16);
    std::vector<uint64_t> slot(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) slot[i + 1] = slot[i] + rup(dims[i].second * bpr, 256);
    const uint64_t need = slot[n] + 256;
    uint8_t *stage = (uint8_t *)aligned_alloc(256, rup(need, 256));  // (ASan: exact size)
    std::vector<std::vector<uint8_t>> ras(n);
    for (uint32_t i = 0; i < n; i++) { ras[i].resize((uint64_t)dims[i].first * dims[i].second * PX); for (auto &b : ras[i]) b = rand(); }
    const uint32_t gx = (maxh + MC_ROWS - 1) / MC_ROWS;
    auto fill_stage = [&] {
        memset(stage, 0xEE, need);
        for (uint32_t i = 0; i < n; i++) for (uint32_t y = 0; y < dims[i].second; y++) memcpy(stage + slot[i] + y * bpr, ras[i].data() + (uint64_t)y * dims[i].first * PX, dims[i].first * PX);
        g_ok = {{(uintptr_t)stage, (uintptr_t)stage + need}};
    };
    // the staging raster after a pack: every row the raster's, and pitch padding, slot tails and spare bytes still the fill value
    auto check_stage = [&](const char *what, int planar, int bgr) {
        for (uint32_t i = 0; i < n; i++) { uint32_t w = dims[i].first, h = dims[i].second;
            for (uint32_t y = 0; y < h; y++) { const uint8_t *row = stage + slot[i] + y * bpr;
                if (memcmp(row, ras[i].data() + (uint64_t)y * w * PX, w * PX)) { printf("%s value px%d pl%d bgr%d img%u (%ux%u) y%u\n", what, PX, planar, bgr, i, w, h, y); errors++; break; }
                int e = 0; for (uint64_t k = w * PX; k < bpr; k++) if (row[k] != 0xEE) e = 1;
                if (e) { printf("%s pad written px%d pl%d bgr%d img%u y%u\n", what, PX, planar, bgr, i, y); errors++; break; } }
            for (uint64_t k = slot[i] + dims[i].second * bpr; k < slot[i + 1]; k++) if (stage[k] != 0xEE) { printf("%s slot tail written img%u\n", what, i); errors++; break; } }
        for (uint64_t k = slot[n]; k < need; k++) if (stage[k] != 0xEE) { printf("%s spare written\n", what); errors++; break; }
    };
    {   // ---- the tight pair: k_mixed_copy out of the stage into tight rasters at every alignment, k_mixed_pack back from them
        fill_stage();
        std::vector<std::vector<uint8_t>> out(n); std::vector<MixedLayout> ml(n);
        for (uint32_t i = 0; i < n; i++) { out[i].assign(64 + 4 + ras[i].size() + 256, 0xA5);
            ml[i] = MixedLayout{slot[i], out[i].data() + 64 + (i % 4), dims[i].first, dims[i].second}; }
        launch(gx, n, [&] { k_mixed_copy(ml.data(), stage, bpr, (uint32_t)PX); });
        for (uint32_t i = 0; i < n; i++) { const uint8_t *o = ml[i].buf; const uint64_t sz = ras[i].size();
            for (uint64_t k = 0; k < out[i].size(); k++) { const uint8_t *p = out[i].data() + k; if ((p < o || p >= o + sz) && *p != 0xA5) { printf("COPY sentinel px%d img%u (%ux%u) at %ld\n", PX, i, dims[i].first, dims[i].second, (long)(p - o)); errors++; break; } }
            for (uint64_t k = 0; k < sz; k++) if (o[k] != ras[i][k]) { printf("COPY value px%d img%u (%ux%u) byte %lu\n", PX, i, dims[i].first, dims[i].second, (unsigned long)k); errors++; break; } }
        memset(stage, 0xEE, need);
        g_ok.clear();
        for (uint32_t i = 0; i < n; i++) g_ok.push_back({(uintptr_t)ml[i].buf, (uintptr_t)ml[i].buf + ras[i].size()});
        launch(gx, n, [&] { k_mixed_pack(ml.data(), stage, bpr, (uint32_t)PX); });
        check_stage("PACK", 0, 0);
    }
    for (int C = 3; C <= 4; C++) for (int planar = 0; planar < 2; planar++) for (int bgr = 0; bgr < 2; bgr++) {
        // ---- decode direction
        fill_stage();
        std::vector<std::vector<uint8_t>> out(n); std::vector<MixedLayout> ml(n);
        for (uint32_t i = 0; i < n; i++) { uint64_t sz = (uint64_t)C * dims[i].first * dims[i].second; out[i].assign(64 + 4 + sz + 256, 0xA5);
            ml[i] = MixedLayout{slot[i], out[i].data() + 64 + (i % 4), dims[i].first, dims[i].second}; }
        auto go = [&](auto k) { launch(gx, n, [&] { k(ml.data(), stage, bpr, (uint32_t)(bgr ? 2 : 0)); }); };
        if (C == 3 && planar) go(k_mixed_copy_as<PX, 3, true>); else if (C == 3) go(k_mixed_copy_as<PX, 3, false>);
        else if (planar) go(k_mixed_copy_as<PX, 4, true>); else go(k_mixed_copy_as<PX, 4, false>);
        for (uint32_t i = 0; i < n; i++) { uint32_t w = dims[i].first, h = dims[i].second; uint64_t sz = (uint64_t)C * w * h; const uint8_t *o = out[i].data() + 64 + (i % 4);
            for (uint64_t k = 0; k < out[i].size(); k++) { const uint8_t *p = out[i].data() + k; if ((p < o || p >= o + sz) && *p != 0xA5) { printf("DEC sentinel px%d C%d pl%d bgr%d img%u (%ux%u) at %ld\n", PX, C, planar, bgr, i, w, h, (long)(p - o)); errors++; break; } }
            int bad = 0;
            for (uint32_t y = 0; y < h && !bad; y++) for (uint32_t x = 0; x < w && !bad; x++) for (int c = 0; c < C; c++) {
                uint8_t g = planar ? o[(uint64_t)c * w * h + (uint64_t)y * w + x] : o[((uint64_t)y * w + x) * C + c];
                if (g != want(ras[i].data(), w, PX, C, bgr, y, x, c)) { printf("DEC value px%d C%d pl%d bgr%d img%u (%ux%u) y%u x%u c%d\n", PX, C, planar, bgr, i, w, h, y, x, c); errors++; bad = 1; break; } } }
        if (C != PX) continue;
        // ---- encode direction: from out[] (now verified layout buffers) back into the stage
        memset(stage, 0xEE, need);
        g_ok.clear();
        for (uint32_t i = 0; i < n; i++) { uintptr_t a = (uintptr_t)ml[i].buf, b = a + (uint64_t)C * dims[i].first * dims[i].second; g_ok.push_back({a, b}); }
        auto ge = [&](auto k) { launch(gx, n, [&] { k(ml.data(), stage, bpr, (uint32_t)(bgr ? 2 : 0)); }); };
        if (planar) ge(k_mixed_pack_from<PX, true>); else ge(k_mixed_pack_from<PX, false>);
        check_stage("ENC", planar, bgr);
    }
    free(stage);
}
int main() {
    std::vector<std::pair<uint32_t, uint32_t>> dims;
    for (uint32_t w = 1; w <= 9; w++) for (uint32_t h = 1; h <= 9; h += 2) dims.push_back({w, h});
    for (auto d : {std::pair<uint32_t, uint32_t>{17, 4}, {64, 64}, {445, 44}, {889, 13}, {100, 110}, {701, 30}, {255, 9}, {256, 8}, {257, 17}, {1031, 3}}) dims.push_back(d);
    run<3>(dims); run<4>(dims);
    std::reverse(dims.begin(), dims.end()); run<3>(dims); run<4>(dims);
    printf("errors: %d\n", errors);
    return errors != 0;
}
