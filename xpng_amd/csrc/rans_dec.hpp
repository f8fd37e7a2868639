// rans_dec.hpp -- what the four rANS DECODERS share: the decode counterpart of rans2.hpp's rans_histogram / rans_alphabet / rans_tables.
//
// v2 blocks (level 1, decompress_block_v2, libxpng.c:429-493) and v1 blocks (level 2, decompress_block, 262-301) each have a narrow
// form (one wavefront per stream: k_rans2_decode in m1_decode.hpp, k_rans1_decode in m2_decode.hpp) and a wide form (a prep kernel
// and chain kernels: rans2_wide_dec.hpp, rans1_wide_dec.hpp).  All four build the same tables from a block's frequencies, and the two
// chain kernels share every piece of their step that does not depend on the direction they decode in.  Here:
//   types      DecTile, WDec, the table layouts, the address-space typedefs, the unaligned loads, the bit readers
//   look-up    rans_dec_owner (slot -> symbol over fc[]), wd_reg9 (the same over nine counts in registers), wd_advance (the state update)
//   nibbles    ctxn_* (the packed context queues between the wide v2 decoders and the lane-per-tile walk: the layout and its arithmetic)
//   set-up     rans_dec_cum, rans2_dec_freqs, rans2_dec_plain / rans1_dec_plain (the blocks that need no chain)
//   wide prep  wd_store_tables
//   wide chain WdChainLds, wd_load_tables, wd_cm_load, wd_land, wave_max
#pragma once
#include "common.hpp"

namespace xpng {

struct DecTile {  // per-tile parse result of level 1 (device)
    const uint8_t *blob;  // the tile blob (inside its image's blob buffer)
    uint32_t type;      // tile type byte (0 = raw rows)
    uint32_t kbytes;    // bytes of k words
    uint32_t blk_off[10];  // block offsets relative to the blob start
    uint32_t blk_n[10];    // symbols per block
    uint32_t ctx_start[10];  // 16-byte aligned start of context stream c inside the tile's symbol area (ctx_start[9] = total coded)
};
constexpr uint32_t TILE_BAD = 0xEE;  // type value of a tile whose headers failed validation: every kernel skips it

struct WDec {          // per (tile, stream) descriptor written by the prep kernels of the wide forms
    uint32_t kind;     // 0 = nothing left to do; rANS chain to run: 1 = small table layout, 2 = big
    uint32_t pb, N, n;
    uint32_t nw;       // renormalisation words of the block
    uint32_t words_off;  // byte offset of words[0] inside the tile blob
    uint64_t out_off;  // symbol destination, relative to the plane the chain kernel writes
    uint32_t hot0, hot1;  // the two most probable symbols
    uint32_t rsh;         // v2 alpha layout: the coarse bytes are indexed by (cold rank >> rsh), see k_rans2_dec_prep
};

// Decode tables of one stream: fc[FCN + 1] dwords (F | cum << 16; entries >= N hold F = 0xFFFF, cum = 0, which stops any
// scan), then the coarse slot -> symbol bytes: entry g = the symbol owning slot g << shift, the start of a short forward
// scan.  A wave runs for its slowest lane, so the scan must be short for EVERY slot: buckets are 16 slots wide.
// Two layouts, chosen per stream by the prep kernel:
//   small (kind 1): nl-context streams as the reference writes them (pb <= 12, at most 16 symbols): 17 + 2^8 bytes/4..,
//                   32-word ring -> 16 KB of LDS per wave, so every chain of a large batch is resident at once
//   big   (kind 2): alpha streams (pb 15, up to 256 symbols); a context stream that does not fit `small` (never written
//                   by the reference encoder) is left to the one-wave-per-stream kernel
template <bool BIG> struct WdLayout {
    static constexpr uint32_t CBITS = BIG ? 10 : 8, FCN = BIG ? 256 : 16, RING = BIG ? 64 : 32, KIND = BIG ? 2 : 1;
    static constexpr uint32_t REGN = 9;  // small layout: at most 9 symbols (nl = 0..8), searched in registers
    static constexpr uint32_t CO_OFF = 4 * (FCN + 1), TAB = CO_OFF + (1u << CBITS);
};
// Alpha streams of mode 1 (pb 15, up to 256 symbols) use a denser form of the big layout: 16-bit cumulative counts
// cum[0 .. N] (cum[N] = 2^pb; entries behind it 0x8000, which stops any scan), F = cum[sym + 1] - cum[sym], and 2^9 coarse
// bytes (64-slot buckets): 1 KB instead of 2 KB of LDS per resident stream, the largest LDS holder of a pipelined batch.
struct WdLayoutA {
    static constexpr uint32_t CBITS = 9, FCN = 256, RING = 64, REGN = 9, KIND = 2;
    static constexpr uint32_t CO_OFF = 2 * (FCN + 2), TAB = CO_OFF + (1u << CBITS);
};
constexpr uint32_t WD_TAB_MAX = WdLayout<true>::TAB;  // HBM stride of one stream's tables

// A pointer read out of a device structure is "generic" to the compiler: it would emit flat_load, which also counts on
// lgkmcnt and so couples every LDS wait to outstanding global loads.  These go through address space 1 explicitly.
typedef const __attribute__((address_space(1))) uint32_t *gptr32;
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef const __attribute__((address_space(1))) u32x4_a4 *gptr128;
typedef __attribute__((address_space(3))) uint8_t lds8;
typedef __attribute__((address_space(3))) uint32_t lds32;
typedef __attribute__((address_space(3))) uint16_t lds16;
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4_t lds128;
typedef u32x4_t u32x4_al4 __attribute__((aligned(4)));
typedef __attribute__((address_space(3))) u32x4_al4 lds128_al4;
// Symbol staging of the wide DECODE chains: every stream of a wave owns OB_STRIDE bytes of LDS - the 16 symbol bytes of a block and
// a dump byte for inactive steps.  36 bytes, not 32: a step stores one byte per lane at the same position of every stream, and
// with 32 bytes per stream eight streams share each bank (an 8-deep serialised store per step; 4 conflict cycles per LDS
// instruction in the counters), with 9 words per stream the 32 streams fall on 32 banks.  The block's 16 bytes leave by a
// 4-byte aligned 16-byte read.
constexpr uint32_t OB_STRIDE = 36;

// unaligned-safe little-endian u32 load from global memory (tile blobs are only byte-aligned after a raw RGB tile)
__device__ __forceinline__ uint32_t ld32u(const uint8_t *p) {
    const uintptr_t a = (uintptr_t)p;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3) * 8;
    const uint32_t lo = q[0];
    if (sh == 0) return lo;
    return (lo >> sh) | (q[1] << (32 - sh));
}
__device__ __forceinline__ uint64_t ld64u(const uint8_t *p) { return (uint64_t)ld32u(p) | ((uint64_t)ld32u(p + 4) << 32); }
__device__ __forceinline__ uint32_t gld32u(uintptr_t a) {  // the same through address space 1
    const gptr32 q = (gptr32)(a & ~(uintptr_t)3);
    const uint32_t sh = (uint32_t)(a & 3) * 8;
    const uint32_t lo = q[0];
    if (sh == 0) return lo;
    return (lo >> sh) | (q[1] << (32 - sh));
}

// MSB-first bit reader over u32 words (BITSTREAM_FILL / BITSTREAM_READ, libxpng.c:9,12); words past `end` read as 0
struct BitR {
    uint64_t acc;
    uint32_t have;
    const uint8_t *p, *end;
    __device__ __forceinline__ uint32_t get(uint32_t c) {
        if (have < 32) {
            acc <<= 32; have += 32;
            if (p < end) { acc += ld32u(p); p += 4; }
        }
        have -= c;
        return (uint32_t)((acc >> have) & ((1ull << c) - 1));
    }
};
// random-access MSB-first bit read from the words at `w` (bits past `endbit` read as 0, like BITSTREAM_FILL past DP)
__device__ __forceinline__ uint32_t bits_at(const uint8_t *w, uint64_t pos, uint32_t c, uint64_t endbit) {
    const uint64_t wi = pos >> 5;
    const uint32_t a = wi * 32 < endbit ? ld32u(w + wi * 4) : 0u, b = (wi + 1) * 32 < endbit ? ld32u(w + wi * 4 + 4) : 0u;
    const uint64_t two = ((uint64_t)a << 32) | b;
    return (uint32_t)((two >> (64 - (pos & 31) - c)) & ((1ull << c) - 1));
}

// ---- look-up and state update (tests/test_rans_dec_host.py runs the text from here to the end mark on the host) ----------------
__device__ __forceinline__ uint32_t pick32(bool c, uint32_t a, uint32_t b) { return c ? a : b; }

// The symbol that owns slot s in fc[i] = F | cum << 16, i < N: the largest index with cum <= s, then back over zero-frequency
// symbols (they share their successor's cum; behind the last used symbol only a corrupt table, whose counts do not add up to 2^pb,
// gets there).  N <= 256: 8 probes.  Every coarse table of the four decoders is filled by it.
__device__ __forceinline__ uint32_t rans_dec_owner(const uint32_t *fc, uint32_t N, uint32_t s) {
    uint32_t lo = 0, hi = N - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if ((fc[mid] >> 16) <= s) lo = mid; else hi = mid - 1;
    }
    while (lo > 0 && (fc[lo] & 0xFFFF) == 0) lo--;
    return lo;
}

// Small layout of the wide chains (at most 9 symbols): the cumulative counts c1..c9 live in registers (c_i = 2^pb for i >= N) and a
// step finds its symbol by a binary search over c1..c8 (three compares, a fourth for symbol 8), then [cum, next) by the same
// decisions: ~30 VALU instructions, the same for every lane, no LDS - instead of two dependent LDS reads and a data-dependent scan
// that the whole wave waits for.
// (every select goes through pick32 and the counts come BY VALUE: a ?: between two array elements inside a chain's step becomes a
//  select of ADDRESSES, which sends the array to scratch memory and puts a scratch load on every step)
__device__ __forceinline__ uint32_t wd_reg9(uint32_t slot, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4, uint32_t c5, uint32_t c6,
                                            uint32_t c7, uint32_t c8, uint32_t c9, uint32_t &F, uint32_t &off) {
    const bool b2 = slot >= c4;
    const bool b1 = slot >= pick32(b2, c6, c2);
    const uint32_t t3 = pick32(b2, pick32(b1, c7, c5), pick32(b1, c3, c1));
    const bool b0 = slot >= t3;
    const bool b3 = b2 && b1 && b0 && slot >= c8;
    const uint32_t sym = (b2 ? 4u : 0u) + (b1 ? 2u : 0u) + (b0 ? 1u : 0u) + (b3 ? 1u : 0u);
    // cum = c[sym], next = c[sym + 1] (c0 = 0)
    const uint32_t lo01 = pick32(b0, c1, 0u), lo23 = pick32(b0, c3, c2), lo45 = pick32(b0, c5, c4), lo67 = pick32(b0, c7, c6);
    const uint32_t hi01 = pick32(b0, c2, c1), hi23 = pick32(b0, c4, c3), hi45 = pick32(b0, c6, c5), hi67 = pick32(b0, c8, c7);
    const uint32_t lo03 = pick32(b1, lo23, lo01), lo47 = pick32(b1, lo67, lo45), hi03 = pick32(b1, hi23, hi01), hi47 = pick32(b1, hi67, hi45);
    uint32_t cum = pick32(b2, lo47, lo03), nxt = pick32(b2, hi47, hi03);
    cum = pick32(b3, c8, cum); nxt = pick32(b3, c9, nxt);
    F = nxt - cum; off = slot - cum;
    return sym;
}

// The state update of a chain step, s = F (s >> pb) + off on the state shi:slo: one 64x32 multiply-add built from v_mad_u64_u32 +
// v_mad_u32_u24 (the high half of s >> pb is < 2^21, F <= 2^15).  Returns whether the new state nhi:nlo must refill (s < 2^31).
__device__ __forceinline__ bool wd_advance(uint32_t slo, uint32_t shi, uint32_t pb, uint32_t F, uint32_t off, uint32_t &nlo, uint32_t &nhi) {
    const uint32_t qlo = __builtin_amdgcn_alignbit(shi, slo, pb), qhi = shi >> pb;  // s >> pb
    const uint64_t r0 = (uint64_t)qlo * F + off;
    nlo = (uint32_t)r0; nhi = __umul24(qhi, F) + (uint32_t)(r0 >> 32);
    return (nhi | (nlo >> 31)) == 0;
}
// (end of the host-run pieces)

// ---- context symbols at four bits (tests/test_ctx_nibbles_host.py runs the text from here to the end mark on the host) -----------
// The wide level-1 decode hands the nine context queues of a PACKED work item (every work item of the lane-per-tile walk
// k_dec_walk_wide; the first one is a launch argument of the producers) from the rANS kernels to the walk two symbols to a byte:
//     symbol i of queue c = nibble (i & 1), low nibble first, of byte ctx_start[c] + (i >> 1)
// so a dword holds 8 symbols and an aligned 16-byte chunk CTXN_CHUNK = 32 - as many as one queue can lose between two services of
// the walk.  The symbols are nl = 0..8; anything above (only a stream the reference cannot write) is stored as 9, which the walk
// turns into "park".  Queue starts stay where k_dec_parse puts them: a packed queue uses the first half of its room.
constexpr uint32_t CTXN_CHUNK = 32;
__host__ __device__ __forceinline__ uint32_t ctxn_clamp(uint32_t sym) { return sym < 9u ? sym : 9u; }
// producers without a pair of lanes: the byte of symbols 2 k (s0) and 2 k + 1 (s1; 0 behind an odd queue's end)
__host__ __device__ __forceinline__ uint32_t ctxn_byte(uint32_t s0, uint32_t s1) { return ctxn_clamp(s0) | (ctxn_clamp(s1) << 4); }
// chain: a lane gathers its symbol (< 16) of pair step u = 0..7 of a block into the dword u >> 2 at BYTE u & 3 (low nibble) ...
__host__ __device__ __forceinline__ uint32_t ctxn_gather(uint32_t acc, uint32_t sym, uint32_t u) { return acc | (sym << (8 * (u & 3u))); }
// ... and at the block boundary the even lane (state 0: symbols 2 u) takes the odd lane's dword (state 1: symbols 2 u + 1) on top
__host__ __device__ __forceinline__ uint32_t ctxn_merge(uint32_t even, uint32_t odd) { return even | (odd << 4); }
// walk: the head dword holds the next symbol lowest; position p lies in dword p >> 3 and chunk p >> 5 of its queue
__host__ __device__ __forceinline__ uint32_t ctxn_sym(uint32_t lo) { return lo & 15u; }
__host__ __device__ __forceinline__ uint32_t ctxn_pop(uint32_t lo) { return lo >> 4; }
__host__ __device__ __forceinline__ bool ctxn_cross(uint32_t npos) { return (npos & 7u) == 0; }
__host__ __device__ __forceinline__ uint32_t ctxn_dword(uint32_t pos) { return pos >> 3; }
__host__ __device__ __forceinline__ uint32_t ctxn_chunk(uint32_t pos) { return pos >> 5; }
// (end of the nibble pieces)

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off); v = o > v ? o : v; }
    return v;
}

// ---- set-up, one wavefront per stream ----------------------------------------------------------------------------------------
// Frequencies freq(i), i < N <= 256 -> fc[i] = F | cum << 16 for ALL 256 entries (0 behind N), by 4-per-lane partial sums and a wave
// scan.  Returns (x, y) = the keys (F << 8 | sym) of the two most probable symbols; an alphabet with one used symbol (which cannot
// happen in a type-3/4 block) gives y = x: the second hot entry then repeats the first and can never win over it.
template <class Freq>
__device__ __forceinline__ uint2 rans_dec_cum(Freq freq, uint32_t N, uint32_t *fc) {
    const uint32_t b = (threadIdx.x & 63) * 4;
    const uint32_t f0 = b + 0 < N ? freq(b + 0) : 0, f1 = b + 1 < N ? freq(b + 1) : 0, f2 = b + 2 < N ? freq(b + 2) : 0, f3 = b + 3 < N ? freq(b + 3) : 0;
    const uint32_t tot = f0 + f1 + f2 + f3;
    const uint32_t incl = wave_scan_incl(tot);
    const uint32_t c0 = incl - tot, c1 = c0 + f0, c2 = c1 + f1, c3 = c2 + f2;
    fc[b + 0] = b + 0 < N ? f0 | (c0 << 16) : 0;
    fc[b + 1] = b + 1 < N ? f1 | (c1 << 16) : 0;
    fc[b + 2] = b + 2 < N ? f2 | (c2 << 16) : 0;
    fc[b + 3] = b + 3 < N ? f3 | (c3 << 16) : 0;
    const uint32_t k0 = (f0 << 8) | (b + 0), k1 = (f1 << 8) | (b + 1), k2 = (f2 << 8) | (b + 2), k3 = (f3 << 8) | (b + 3);
    uint32_t m = k0 > k1 ? k0 : k1; m = k2 > m ? k2 : m; m = k3 > m ? k3 : m;
    const uint32_t hot0 = wave_max(m);
    auto ex = [&](uint32_t k) { return k == hot0 ? 0u : k; };
    uint32_t m2 = ex(k0) > ex(k1) ? ex(k0) : ex(k1); m2 = ex(k2) > m2 ? ex(k2) : m2; m2 = ex(k3) > m2 ? ex(k3) : m2;
    const uint32_t hot1 = wave_max(m2);
    return make_uint2(hot0, (hot1 >> 8) == 0 ? hot0 : hot1);
}

// v2: the block's frequency table -> Fs[0 .. N): <= 256 short fields, dense (type 3) or sparse (type 4); lane 0's serial bit reader
__device__ __forceinline__ void rans2_dec_freqs(uint32_t type, uint32_t pb, uint32_t N, const uint8_t *table, const uint8_t *end, uint32_t *Fs) {
    if ((threadIdx.x & 63) != 0) return;
    BitR tr{0, 0, table, end};
    for (uint32_t i = 0; i < N; i++) {
        uint32_t F;
        if (type == 3) F = tr.get(pb);
        else F = tr.get(1) ? tr.get(pb) : 0;
        Fs[i] = F;
    }
}

// The blocks that need no chain: one distinct symbol (type 1) and raw symbols (type 2).  Each returns whether it finished the block.
// packed: a context queue of a packed work item, two symbols to a byte (ctxn_byte above)
__device__ __forceinline__ bool rans2_dec_plain(uint32_t type, const uint8_t *in, const uint8_t *end, uint32_t n, uint32_t v2, uint8_t *out,
                                                bool packed = false) {
    const uint32_t lane = threadIdx.x & 63;
    auto raw = [&](uint32_t i) -> uint32_t {  // v2 bits per symbol behind the two header words, MSB first
        const uint64_t b0 = (uint64_t)i * v2;
        const uint8_t *wp = in + 8 + (b0 >> 5) * 4;
        const uint32_t rel = (uint32_t)(b0 & 31);
        const uint64_t two = ((uint64_t)ld32u(wp) << 32) | (wp + 4 < end ? ld32u(wp + 4) : 0u);
        return (uint32_t)((two >> (64 - rel - v2)) & ((1u << v2) - 1));
    };
    if (packed) {
        if (type == 1) {
            for (uint32_t i = 2 * lane; i < n; i += 128) out[i >> 1] = (uint8_t)ctxn_byte(v2, i + 1 < n ? v2 : 0u);
        } else if (type == 2) {
            for (uint32_t i = 2 * lane; i < n; i += 128) out[i >> 1] = (uint8_t)ctxn_byte(raw(i), i + 1 < n ? raw(i + 1) : 0u);
        }
    } else if (type == 1) {
        for (uint32_t i = lane; i < n; i += 64) out[i] = (uint8_t)v2;
    } else if (type == 2) {
        for (uint32_t i = lane; i < n; i += 64) out[i] = (uint8_t)raw(i);
    }
    return type == 1 || type == 2;
}
// v1: `pbits` is the single symbol (type 1) or the bit offset of the raw symbols, rb bits each, in the tile's shared bit stream
// b = bw[0 .. endbit) (type 2, libxpng.c:273)
__device__ __forceinline__ bool rans1_dec_plain(uint32_t type, uint32_t pbits, uint32_t rb, const uint8_t *bw, uint64_t endbit, uint32_t n, uint8_t *out) {
    const uint32_t lane = threadIdx.x & 63;
    if (type == 1) {
        for (uint32_t i = lane; i < n; i += 64) out[i] = (uint8_t)pbits;
    } else if (type == 2) {
        for (uint32_t i = lane; i < n; i += 64) out[i] = (uint8_t)bits_at(bw, (uint64_t)pbits + (uint64_t)i * rb, rb, endbit);
    }
    return type == 1 || type == 2;
}

// ---- wide prep: a stream's tables in HBM ---------------------------------------------------------------------------------------
// gt <- the small layout's fc[] dwords or (LA, the big layout of the caller) the 16-bit cum[] (entries behind cum[N] = 2^pb hold
// 0x8000: greater than any slot, and slot - entry keeps its 16-bit sign bit set), then the coarse bytes: entry g names the owner of
// slot index_to_slot(g << sh).
template <class LA, class Slot>
__device__ __forceinline__ void wd_store_tables(uint8_t *gt, bool small, const uint32_t *fc, uint32_t N, uint32_t pb, uint32_t sh, Slot index_to_slot) {
    typedef WdLayout<false> LS;
    const uint32_t lane = threadIdx.x & 63;
    if (small) {
        uint32_t *gfc = reinterpret_cast<uint32_t *>(gt);
        for (uint32_t i = lane; i <= LS::FCN; i += 64) gfc[i] = i < N ? fc[i] : 0xFFFFu;
    } else {
        uint16_t *gcu = reinterpret_cast<uint16_t *>(gt);
        for (uint32_t i = lane; i <= LA::FCN + 1; i += 64) gcu[i] = (uint16_t)(i < N ? fc[i] >> 16 : (i == N ? 1u << pb : 0x8000u));
    }
    const uint32_t co_off = small ? LS::CO_OFF : LA::CO_OFF, entries = small ? 1u << (pb - sh) : 1u << LA::CBITS;
    for (uint32_t g0 = lane * 4; g0 < entries; g0 += 256) {
        uint32_t pk = 0;
        for (uint32_t q = 0; q < 4; q++) pk |= rans_dec_owner(fc, N, index_to_slot((g0 + q) << sh)) << (8 * q);
        *reinterpret_cast<uint32_t *>(gt + co_off + g0) = pk;
    }
}

// ---- wide chain: the pieces of k_rans2_dec_chain and k_rans1_dec_chain that do not depend on the direction --------------------
// dynamic LDS of one launch (common.hpp: why dynamic): a table of LTAB bytes and a ring of L::RING words (and a mirror word) per
// stream, OB_STRIDE symbol bytes per stream and for SPARE more (the lanes without a stream, where STREAMS < 32)
template <class L, uint32_t LT, uint32_t STREAMS, uint32_t SPARE> struct WdChainLds {
    static constexpr uint32_t LTAB = LT, TSTRIDE = LTAB + 4;  // +1 bank per table, the lanes mostly look up the same symbol
    static constexpr uint32_t RSTRIDE = 4 * L::RING + 4;
    static constexpr uint32_t OFF_RING = (STREAMS * TSTRIDE + 15u) & ~15u, OFF_OBUF = (OFF_RING + STREAMS * RSTRIDE + 31u) & ~31u;
    static constexpr size_t BYTES = OFF_OBUF + (STREAMS + SPARE) * OB_STRIDE + 12;
};

// decode tables of the wave's streams (tiles j0 .., stream c of `per_tile`) -> LDS, LTAB bytes each
template <class L, uint32_t LTAB, uint32_t STREAMS>
__device__ __forceinline__ void wd_load_tables(uint8_t *ltab, uint32_t j0, uint32_t total, const WDec *wdec, const uint8_t *dtab,
                                               uint32_t per_tile, uint32_t c) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t ts = 0; ts < STREAMS; ts++) {
        const uint32_t jj = j0 + ts;
        uint32_t *dst = reinterpret_cast<uint32_t *>(ltab + ts * (LTAB + 4));
        if (jj >= total || sgpr(wdec[(uint64_t)jj * per_tile + c].kind) != L::KIND) {
            // no chain in this slot: its lanes idle through the loop, but their table lookups must still terminate
            // (big layout: cum[0] = 0, every other entry 0x8000: symbol 0 owns every slot)
            for (uint32_t i = lane; i < LTAB / 4; i += 64) dst[i] = i < L::CO_OFF / 4 ? (L::KIND == 2 ? (i ? 0x80008000u : 0x80000000u) : 0xFFFFu) : 0u;  // every coarse byte names symbol 0, whose entry stops the scan
            continue;
        }
        const uint32_t *src = reinterpret_cast<const uint32_t *>(dtab + ((uint64_t)jj * per_tile + c) * WD_TAB_MAX);
#pragma unroll 4
        for (uint32_t i = lane; i < LTAB / 4; i += 64) dst[i] = src[i];
    }
}

// (k_rans1_dec_chain keeps the text of wd_cm_load and wd_reg9 in its body: see there)
// the counts c1..c9 of wd_reg9 out of the stream's fc[] in LDS (REG: the small layout; a lane without a chain, or of the big layout, gets 2^pb throughout)
template <bool REG>
__device__ __forceinline__ void wd_cm_load(uint32_t (&cm)[10], bool live, const WDec *wd, uint32_t a_fc, uint32_t pb) {
#pragma unroll
    for (int i = 1; i <= 9; i++) {
        cm[i] = 1u << pb;
        if (REG && live && (uint32_t)i < wd->N) cm[i] = *(const lds32 *)(uintptr_t)(a_fc + 4 * i) >> 16;
    }
}

// The words a lane requested at the last block boundary (PER + 1 dwords from the aligned address below word fa0) land in the
// stream's ring (word slot i at a_ring + 4 i), as far as they lie below fhi (fhi = 0: nothing was requested).
template <uint32_t RING>
__device__ __forceinline__ void wd_land(uint32_t a_ring, uint4 q0, uint4 q1, uint32_t qx, uint32_t fa0, uint32_t fhi, uint32_t fsh) {
    constexpr uint32_t PER = RING / 8;
    const uint32_t dw[9] = {q0.x, q0.y, q0.z, q0.w, PER > 4 ? q1.x : qx, q1.y, q1.z, q1.w, qx};
#pragma unroll
    for (int i = 0; i < (int)PER; i++) {
        const uint32_t a = fa0 + (uint32_t)i;
        if (a < fhi) *(lds32 *)(uintptr_t)(a_ring + 4 * (a & (RING - 1))) = __builtin_amdgcn_alignbyte(dw[i + 1], dw[i], fsh);
    }
}

}  // namespace xpng
