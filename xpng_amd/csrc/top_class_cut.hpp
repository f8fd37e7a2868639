// The cut rule of the batched (wide) level-1 form: how many of a launch's biggest tiles get a wavefront of their own for the alpha
// chain (the narrow alpha role of k_rans2_chain_all, rans2_wide.hpp) instead of a lane pair of a wide wavefront.
//
// A serial launch lasts as long as its longest chain, and a chain's length is its tile's pixel count.  A wavefront that carries ONE
// stream steps about 1.5 times faster than one that carries 32 (scalar cursors, no cross-lane bookkeeping: DESIGN.md 4), so the
// biggest tiles' chains on wavefronts of their own end when wide chains of two thirds their length end, and the launch is then
// bounded by the biggest tile that stayed wide.  Only the TOP CLASS is a candidate - the tiles as large as the largest - and never
// every tile of the launch: a launch of equal tiles has nothing to cut.
//
// Pure host arithmetic, no HIP: tests/test_top_class_cut_host.py compiles this file with g++.
#pragma once
#include <stdint.h>

namespace xpng {

constexpr uint32_t TOP_CUT_CAP = 128;                  // narrow wavefronts per role and launch
constexpr uint32_t TOP_CUT_NUM = 2, TOP_CUT_DEN = 3;   // chain step, narrow : wide (conservative against both measured pairs)

// n[0..T): the pixel counts of the launch's tiles in its size-sorted order (non-increasing); B: images per launch.
// Returns k: the alpha streams of the k leading tiles - work items [0, k * B) - go to the narrow role.
//   t(k) = max(ceil(2 n[0] / 3), n[k])  (n[T] = 0): the modelled length of the launch, in wide steps
//   k runs over 1 .. min(E, T - 1, CAP / B), E = the number of tiles as large as n[0]; the smallest k with the smallest t(k) wins,
//   and k = 0 when that gains less than a tenth (10 t(k) > 9 n[0]).
inline uint32_t top_class_cut(const uint32_t *n, uint32_t T, uint32_t B) {
    if (!n || T < 2 || B == 0 || n[0] == 0) return 0;
    uint32_t E = 1;
    while (E < T && n[E] == n[0]) E++;
    uint32_t kmax = TOP_CUT_CAP / B;
    if (kmax > E) kmax = E;
    if (kmax > T - 1) kmax = T - 1;
    const uint64_t narrow = ((uint64_t)TOP_CUT_NUM * n[0] + TOP_CUT_DEN - 1) / TOP_CUT_DEN;
    uint64_t best = n[0];
    uint32_t k = 0;
    for (uint32_t q = 1; q <= kmax; q++) {
        const uint64_t t = narrow > n[q] ? narrow : n[q];
        if (t < best) { best = t; k = q; }
    }
    return 10 * best > 9 * (uint64_t)n[0] ? 0 : k;
}

}  // namespace xpng
