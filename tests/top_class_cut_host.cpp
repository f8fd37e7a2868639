// Host run of the cut rule of the batched level-1 form (xpng_amd/csrc/top_class_cut.hpp): the header itself, named by CUT_TEXT, and
// the table of cases the test writes from the tile tables (CASES_TEXT: {"name", B, expected k, {pixel counts, size-sorted}}).
// Built and run by tests/test_top_class_cut_host.py.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <functional>
#include <vector>

#include CUT_TEXT

struct Case { const char *name; uint32_t B, want; std::vector<uint32_t> n; };
static const Case CASES[] = {
#include CASES_TEXT
};

static long errors = 0;
static void bad(const char *what, long a, long b, long c) { if (errors++ < 20) printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c); }

int main() {
    long rows = 0;
    for (const Case &c : CASES) {
        const uint32_t k = xpng::top_class_cut(c.n.data(), (uint32_t)c.n.size(), c.B);
        printf("%-28s T = %4zu  B = %3u  k = %u (expected %u)\n", c.name, c.n.size(), c.B, k, c.want);
        if (k != c.want) bad(c.name, k, c.want, c.B);
        rows++;
    }
    // random size-sorted inputs out of a few distinct sizes (so that classes of equal tiles of every length appear)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&](uint32_t m) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)((s >> 33) % m); };
    long cases = 0, cut = 0;
    for (int it = 0; it < 200000; it++) {
        const uint32_t T = 1 + rnd(48), B = 1 + rnd(it & 1 ? 200 : 8), kinds = 1 + rnd(4);
        uint32_t sizes[4];
        for (uint32_t q = 0; q < kinds; q++) sizes[q] = 1 + rnd(it & 2 ? 300000 : 12);
        std::vector<uint32_t> n(T);
        for (uint32_t i = 0; i < T; i++) n[i] = sizes[rnd(kinds)];
        std::sort(n.begin(), n.end(), std::greater<uint32_t>());
        const uint32_t k = xpng::top_class_cut(n.data(), T, B);
        cases++;
        if ((uint64_t)k * B > xpng::TOP_CUT_CAP) bad("k * B <= 128", k, B, T);
        if (k >= T && k) bad("k < T", k, B, T);
        if (n[0] == n[T - 1] && k) bad("all tiles equal: k = 0", k, B, T);
        if (k) {
            cut++;
            if (n[k - 1] != n[0]) bad("only tiles as large as the largest", k, n[k - 1], n[0]);
            const uint64_t narrow = (2ull * n[0] + 2) / 3, t = std::max<uint64_t>(narrow, n[k]);
            if (10 * t > 9ull * n[0]) bad("a cut gains at least a tenth", k, (long)t, n[0]);
            if (n[k] == n[0]) bad("a cut takes the whole top class", k, n[k], n[0]);
        }
    }
    if (xpng::top_class_cut(nullptr, 0, 1) != 0) bad("no tiles", 0, 0, 0);
    const uint32_t one[1] = {1000};
    if (xpng::top_class_cut(one, 1, 1) != 0) bad("one tile", 0, 0, 0);
    printf("table rows: %ld\ncases: %ld (%ld with a cut)\nerrors: %ld\n", rows, cases, cut, errors);
    return errors ? 1 : 0;
}
