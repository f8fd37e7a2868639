// Host run of the decode's pixel rule (xpng_amd/csrc/recon.hpp): recon_px_band - the byte-parallel form of the band reconstruction,
// with the gradient predictor in two 16-bit lanes, lerp for the average and the per-byte add - and the scalar recon_px<3> and
// recon_px<4> of the other two forms, against a plain scalar restatement of libxpng.c:798-813 and against each other, with shims
// for the two device operations the byte-parallel form uses.
// Every (L, U, UL) out of 16 values per channel (the ends and the middle of the byte range, where the damped gradient
// ((3L + 3U - 2UL) + 2) >> 2 leaves 0..255: 383 at (255, 255, 0), -127 at (0, 0, 255)), a different triple in each channel so that a
// carry between the lanes shows, 16 residual words each, the four predictor modes, row 0 / column 0 / the tile's first pixel /
// interior, and a marker byte (RGBA: the pixel's alpha) of 0, 1 and 255.
// Built and run by tests/test_recon_pixel_host.py: g++ -fsanitize=undefined,address -DKERNEL_TEXT=\"...\".
#include "kernel_host.hpp"  // __device__ and __forceinline__
static inline uint32_t times3(uint32_t x) { return x + (x << 1); }
static inline uint32_t lerp_shim(uint32_t a, uint32_t b, uint32_t c) {  // v_lerp_u8: per byte (a + b + (c & 1)) >> 1
    uint32_t o = 0;
    for (int i = 0; i < 4; i++) o |= (((((a >> (8 * i)) & 255u) + ((b >> (8 * i)) & 255u) + ((c >> (8 * i)) & 1u)) >> 1) & 255u) << (8 * i);
    return o;
}
#define __builtin_amdgcn_lerp lerp_shim
#include KERNEL_TEXT  // pred_avg and pred_grad (common.hpp), then swar_add8, recon_px_band and recon_px (recon.hpp)

// libxpng.c:798-813 for one pixel: the marker byte decides (802), each channel adds its prediction mod 256 (811, 814); row 0
// predicts from the left and column 0 from above (819, 820), the interior by the tile's predictor (p2a, p3a; gray tiles of level 2
// also p1x, p1y: 890-895); the tile's first pixel is stored as it is (850)
static uint32_t reference(uint32_t rw, uint32_t L, uint32_t U, uint32_t UL, bool col0, bool row0, int predmode, uint32_t first) {
    if (col0 && row0) return first;
    if ((rw >> 24) == 0) return 0;
    uint32_t px = rw & 0xFF000000u;
    for (int c = 0; c < 3; c++) {
        const int l = (L >> (8 * c)) & 255, u = (U >> (8 * c)) & 255, ul = (UL >> (8 * c)) & 255;
        int pred;
        if (row0) pred = l;
        else if (col0) pred = u;
        else if (predmode == 0) pred = (l + u + 1) / 2;
        else if (predmode == 1) pred = (int)floor((3 * l + 3 * u - 2 * ul + 2) / 4.0);  // (an arithmetic shift: rounds towards minus infinity)
        else pred = predmode == 2 ? l : u;
        px |= (uint32_t)(((int)((rw >> (8 * c)) & 255u) + pred + 256) % 256) << (8 * c);
    }
    return px;
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
        for (int rep = 0; rep < 16; rep++) {
            h = h * 1664525u + 1013904223u;
            // residual bytes: half of them small (what a predicted pixel leaves, either sign), half anywhere
            const uint32_t res = (rep & 1) ? (h >> 8) & 0xFFFFFFu : ((((h >> 8) & 0x070707u) + ((h >> 4) & 0x010101u) * 0xF8u) & 0xFFFFFFu);
            const uint32_t first = h ^ 0x5A5A5A5Au;
            // (the neighbours' top bytes - their alpha - take no part in a colour channel: any value)
            const uint32_t L4 = L | (A[rep % 3] << 24), U4 = U | (A[(rep + k) % 3] << 24), UL4 = UL | (h & 0xFF000000u);
            for (int ai = 0; ai < 3; ai++) {
                const uint32_t rw = res | (A[ai] << 24);
                for (int predmode = 0; predmode < 4; predmode++)
                    for (int edge = 0; edge < 4; edge++) {
                        const bool col0 = edge & 1, row0 = edge & 2;
                        const int32_t x = col0 ? 0 : 1 + (int32_t)(h & 1023u);
                        const uint32_t y = row0 ? 0u : 1u + ((h >> 10) & 1023u);
                        const uint32_t e = reference(rw, L4, U4, UL4, col0, row0, predmode, first);
                        const uint32_t b = recon_px_band(rw, L4, U4, UL4, predmode, predmode == 1, x, y, first);
                        const uint32_t s4 = recon_px<4>(rw, L4, U4, UL4, x, y, predmode, first);
                        const uint32_t s3 = recon_px<3>(rw, L4, U4, UL4, x, y, predmode, first & 0xFFFFFFu);  // (RGB: what is stored is the low three bytes)
                        runs++;
                        if ((b != e || s4 != e || s3 != (e & 0xFFFFFFu)) && errors++ < 20)
                            printf("predmode %d col0 %d row0 %d rw %08x L %08x U %08x UL %08x: band %08x px<4> %08x px<3> %06x, want %08x\n",
                                   predmode, col0, row0, rw, L4, U4, UL4, b, s4, s3, e);
                    }
            }
        }
    }
    printf("runs: %ld\nerrors: %ld\n", runs, errors);
    return errors != 0;
}
