// Host run of m1_pixel_interior (xpng_amd/csrc/m1_encode.hpp): the byte-parallel per-pixel arithmetic of the LDS-staged transforms -
// the gradient predictor in two 16-bit lanes, lerp for the average, per-byte subtract, the green subtraction and the zig-zag -
// against a plain scalar restatement of libxpng.c:497-513, with shims for the two device operations it uses.
// Every (L, U, UL) out of 16 values per channel (the ends and the middle of the byte range, where the damped gradient
// ((3L + 3U - 2UL) + 2) >> 2 leaves 0..255: 383 at (255, 255, 0), -127 at (0, 0, 255)), a different triple in each channel so that a
// carry between the lanes shows, 64 current pixels each, the four predictors, column 0 and interior, alpha 0 / 1 / 255.
// Built and run by tests/test_pixel_transform_host.py: g++ -fsanitize=undefined,address -DKERNEL_TEXT=\"...\".
#include "kernel_host.hpp"  // __device__ and __forceinline__
constexpr uint32_t NL_NONE = 0xFFu;
static inline int bit_width(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }
static inline uint32_t times3(uint32_t x) { return x + (x << 1); }
static inline uint32_t lerp_shim(uint32_t a, uint32_t b, uint32_t c) {  // v_lerp_u8: per byte (a + b + (c & 1)) >> 1
    uint32_t o = 0;
    for (int i = 0; i < 4; i++) o |= (((((a >> (8 * i)) & 255u) + ((b >> (8 * i)) & 255u) + ((c >> (8 * i)) & 1u)) >> 1) & 255u) << (8 * i);
    return o;
}
#define __builtin_amdgcn_lerp lerp_shim
#include KERNEL_TEXT

static int zz(int d) { int v = (int8_t)d; return ((int)((unsigned)v << 1) ^ (v >> 31)) & 0xFF; }
// libxpng.c:497-513 for an interior pixel (col0: column 0 of a row below the first)
static uint32_t reference(int useGrad, int useG, uint32_t cur, uint32_t L, uint32_t U, uint32_t UL, uint32_t &nl, bool col0) {
    const int pa = col0 ? (int)(U >> 24) : (int)(L >> 24);
    const uint32_t za = (uint32_t)zz((int)(cur >> 24) - pa);
    if ((cur >> 24) == 0) { nl = NL_NONE; return za << 24; }
    int d[3];
    for (int c = 0; c < 3; c++) {
        const int v = (cur >> (8 * c)) & 255, l = (L >> (8 * c)) & 255, u = (U >> (8 * c)) & 255, ul = (UL >> (8 * c)) & 255;
        const int pred = col0 ? u : useGrad ? ((3 * l + 3 * u - 2 * ul) + 2) >> 2 : (l + u + 1) >> 1;
        d[c] = v - pred;
    }
    if (useG && !col0) { d[0] -= d[1]; d[2] -= d[1]; }
    const uint32_t zr = (uint32_t)zz(d[0]), zg = (uint32_t)zz(d[1]), zb = (uint32_t)zz(d[2]);
    nl = (uint32_t)bit_width(zr | zg | zb);
    return zr | (zg << 8) | (zb << 16) | (za << 24);
}

int main() {
    static const uint32_t V[16] = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 190, 191, 192, 253, 254, 255};
    static const uint32_t A[3] = {0, 1, 255};
    long errors = 0, runs = 0;
    uint32_t h = 12345u;
    for (uint32_t k = 0; k < 4096; k++) {
        const uint32_t t[3] = {k, (k * 7 + 3) & 4095u, (k * 13 + 5) & 4095u};
        uint32_t L = 0, U = 0, UL = 0;
        for (int c = 0; c < 3; c++) { L |= V[t[c] >> 8] << (8 * c); U |= V[(t[c] >> 4) & 15] << (8 * c); UL |= V[t[c] & 15] << (8 * c); }
        for (int rep = 0; rep < 64; rep++) {
            h = h * 1664525u + 1013904223u;
            // current pixel: half of them near a prediction (small residuals), half anywhere
            uint32_t cur = (rep & 1) ? (h >> 8) & 0xFFFFFFu : ((((L & 0xFEFEFEu) >> 1) + ((U & 0xFEFEFEu) >> 1) + ((h >> 8) & 0x030303u)) & 0xFFFFFFu);
            for (int ai = 0; ai < 3; ai++) {
                const uint32_t c4 = cur | (A[ai] << 24), L4 = L | (A[(ai + rep) % 3] << 24), U4 = U | (A[(ai + k) % 3] << 24), UL4 = UL | (h & 0xFF000000u);
                for (int pr = 0; pr < 4; pr++)
                    for (int col0 = 0; col0 < 2; col0++) {
                        uint32_t nl, enl;
                        const uint32_t z = m1_pixel_interior((pr >> 1) & 1, pr & 1, c4, L4, U4, UL4, nl, col0 != 0);
                        const uint32_t e = reference((pr >> 1) & 1, pr & 1, c4, L4, U4, UL4, enl, col0 != 0);
                        runs++;
                        if ((z != e || nl != enl) && errors++ < 20)
                            printf("pr %d col0 %d cur %08x L %08x U %08x UL %08x: got %08x nl %u, want %08x nl %u\n", pr, col0, c4, L4, U4, UL4, z, nl, e, enl);
                    }
            }
        }
    }
    printf("runs: %ld\nerrors: %ld\n", runs, errors);
    return errors != 0;
}
