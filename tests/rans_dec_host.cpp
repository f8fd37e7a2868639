// Host run of the rANS decoders' symbol look-up and state update (xpng_amd/csrc/rans_dec.hpp): rans_dec_owner - the search that fills
// every coarse table -, wd_reg9 - the register search of the wide chains' small layout - and wd_advance - their 64x32 state update -,
// each against a plain restatement of decompress_block (libxpng.c:283-296): cum2sym[] filled symbol by symbol, the owner of a slot
// read out of it, state = F (state >> pb) + slot - cum in 64 bits.  Shims stand in for v_alignbit_b32 and the 24-bit multiply.
// Built and run by tests/test_rans_dec_host.py: g++ -fsanitize=undefined,address -DKERNEL_TEXT=\"...\".
#include "kernel_host.hpp"  // __device__ and __forceinline__
static inline uint32_t alignbit_shim(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sh & 31)); }
static inline uint32_t umul24_shim(uint32_t a, uint32_t b) { return (a & 0xFFFFFFu) * (b & 0xFFFFFFu); }
#define __builtin_amdgcn_alignbit alignbit_shim
#define __umul24 umul24_shim
#include KERNEL_TEXT  // pick32, rans_dec_owner, wd_reg9, wd_advance

static long cases = 0;
static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 17; rnd_state ^= rnd_state << 5; return rnd_state; }

// every slot of one table: F[0 .. N) adds up to 2^pb
static void check_table(const std::vector<uint32_t> &F, uint32_t pb, bool reg9) {
    const uint32_t N = (uint32_t)F.size(), total = 1u << pb;
    std::vector<uint32_t> cum(N + 1, 0);
    for (uint32_t i = 0; i < N; i++) cum[i + 1] = cum[i] + F[i];
    if (cum[N] != total) { bad("table does not add up", cum[N], total); return; }
    std::vector<uint8_t> cum2sym(total);
    for (uint32_t i = 0; i < N; i++) memset(cum2sym.data() + cum[i], (int)i, F[i]);  // libxpng.c:283
    uint32_t fc[256];                                                                // as rans_dec_cum leaves it: 0 behind N
    for (uint32_t i = 0; i < 256; i++) fc[i] = i < N ? F[i] | (cum[i] << 16) : 0;
    uint32_t c[10];                                                                  // as wd_cm_load leaves it: 2^pb from N on
    for (uint32_t i = 1; i <= 9; i++) c[i] = i < N ? cum[i] : total;
    for (uint32_t slot = 0; slot < total; slot++) {
        const uint32_t want = cum2sym[slot], wF = F[want], woff = slot - cum[want];
        const uint32_t o = rans_dec_owner(fc, N, slot);
        cases++;
        if (o != want || (fc[o] & 0xFFFFu) != wF || slot - (fc[o] >> 16) != woff) bad("rans_dec_owner", slot, o);
        if (reg9) {
            uint32_t gF = ~0u, goff = ~0u;
            const uint32_t g = wd_reg9(slot, c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], gF, goff);
            cases++;
            if (g != want || gF != wF || goff != woff) bad("wd_reg9", slot, g);
        }
    }
}

// `used` symbols out of N share 2^pb: one count each, the rest of the slots by a random split
static std::vector<uint32_t> random_table(uint32_t N, uint32_t pb, const std::vector<bool> &used) {
    std::vector<uint32_t> F(N, 0), idx;
    for (uint32_t i = 0; i < N; i++) if (used[i]) { F[i] = 1; idx.push_back(i); }
    uint32_t left = (1u << pb) - (uint32_t)idx.size();
    while (left) { const uint32_t give = 1 + rnd() % left; F[idx[rnd() % idx.size()]] += give; left -= give; }
    return F;
}

int main() {
    static const uint32_t PB[4] = {10, 11, 12, 14};
    for (uint32_t pb : PB) {
        const uint32_t total = 1u << pb;
        for (uint32_t N = 2; N <= 9; N++) {
            std::vector<uint32_t> F(N, total / N);                                   // flat
            F[N - 1] += total - total / N * N;
            check_table(F, pb, true);
            F.assign(N, 1); F[0] = total - N + 1;                                    // one dominant symbol, first and last
            check_table(F, pb, true);
            F.assign(N, 1); F[N - 1] = total - N + 1;
            check_table(F, pb, true);
            for (uint32_t z = 0; z < N; z++) {                                       // one zero-frequency symbol: front, middle, end
                F.assign(N, total / (N - 1)); F[z] = 0; F[z ? 0 : 1] += total - total / (N - 1) * (N - 1);
                check_table(F, pb, true);
            }
            for (int rep = 0; rep < 8; rep++) {                                      // random splits, every second with random zeros
                std::vector<bool> used(N, true);
                if (rep & 1) for (uint32_t i = 0; i < N; i++) used[i] = rnd() & 1;
                used[rnd() % N] = true;
                check_table(random_table(N, pb, used), pb, true);
            }
        }
        {   // symbol 8 alone behind zeros, with and without zeros at the front
            std::vector<uint32_t> F(9, 0);
            F[0] = total - 3; F[8] = 3; check_table(F, pb, true);
            F[0] = 0; F[1] = total - 1; F[8] = 1; check_table(F, pb, true);
            F.assign(9, 0); F[3] = total / 2; F[8] = total / 2; check_table(F, pb, true);
        }
    }
    for (int rep = 0; rep < 6; rep++) {  // N = 256 at pb 15: runs of zero-frequency symbols between the used ones
        std::vector<bool> used(256, false);
        for (uint32_t i = rep == 0 ? 0 : rnd() % 16; i < 256;) {
            const uint32_t run = 1 + rnd() % 5;
            for (uint32_t k = 0; k < run && i < 256; k++) used[i++] = true;
            i += rnd() % (rep < 3 ? 24 : 3);
        }
        if (rep == 1) used[255] = true;
        used[128] = true;
        check_table(random_table(256, 15, used), 15, false);
    }
    // wd_advance: F (s >> pb) + off in 64 bits, need = (the result < 2^31)
    for (uint32_t pb = 10; pb <= 15; pb++) {
        const uint32_t Fs[4] = {1, 2, (1u << pb) - 1, 1u << pb};  // (2^pb: the identity entry an idle lane steps on)
        for (int si = 0; si < 4 + 4096; si++) {
            uint64_t s = si == 0 ? 1ull << 31 : si == 1 ? (1ull << 32) - 1 : si == 2 ? 1ull << 32 : (1ull << 63) - 1;
            if (si >= 4) {  // random points of [2^31, 2^63), every magnitude
                s = ((uint64_t)rnd() << 32) | rnd();
                s >>= 1 + rnd() % 32;
                if (s < (1ull << 31)) s |= 1ull << 31;
            }
            for (uint32_t F : Fs) for (int oi = 0; oi < 2; oi++) {
                const uint32_t off = oi ? F - 1 : 0;
                const uint64_t want = (uint64_t)F * (s >> pb) + off;
                uint32_t nlo = 0, nhi = 0;
                const bool need = wd_advance((uint32_t)s, (uint32_t)(s >> 32), pb, F, off, nlo, nhi);
                cases++;
                if ((((uint64_t)nhi << 32) | nlo) != want || need != (want < (1ull << 31))) bad("wd_advance", (long)pb, (long)F);
            }
        }
    }
    printf("cases: %ld\nerrors: %d\n", cases, errors);
    return errors != 0;
}
