// m1_decode.hpp -- mode-1 tile DECODE kernels for gfx950.
//
// Reference path restated: dec_1_th (libxpng.c:834-863) = decompress_block_v2 (429-493) + m1d_* (796-830).
// The reference decodes a tile in one serial loop; its three serial couplings are separated here:
//
//   k_dec_parse       tile header, k extent, the 9(+1) v2 block offsets / symbol counts     (1 thread / tile)
//   k_rans2_decode    one wavefront per (tile, stream); 2 lanes carry the interleaved states (429-493)
//   k_dec_alpha       alpha plane = column-0 prefix sum, then per-row prefix sums mod 256   (798-800: alpha uses
//                     the left neighbour everywhere except column 0)
//   k_dec_walk        the context chain nl = *cx[nl]++ (803): strictly serial per tile; lanes 0..8 of one wave
//                     own the nine queues in registers and the chain advances by v_readlane
//   k_dec_resid       bit cursor = scan of 3*nl; residual extraction from k; zig-zag / green add-back (804-813)
//   k_dec_recon       causal prediction from reconstructed L/U/UL: anti-diagonal wavefront, one row per thread (recon.hpp,
//                     shared with mode 2)
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "rans_dec.hpp"  // DecTile, WDec, ld32u, the decode set-up
#include "recon.hpp"
#include "rans2_wide_dec.hpp"

namespace xpng {

// The decode workspace of one context.  It BORROWS the context's side stream and its stream scratch (`arena`: the five symbol /
// residual planes, 8 B per pixel, are carved out of it - no decode kernel reads the encode's intermediates and no encode kernel runs
// while a decode of the same context does); dec_prepare (xpng_hip.hip) lends both before every launch.  Its per-tile tables grow on
// demand inside the context's workspace table (WsTable, common.hpp), which frees them; it OWNS its events only.
struct DecodeWs {
    uint64_t cap_tiles = 0, cap_plane = 0;
    WDec *d_wdec = nullptr;              // wide rANS decode: per (tile, stream) descriptors and decode tables
    uint8_t *d_dtab = nullptr;
    WDec *d_wdec2 = nullptr;             // the same for mode 2 (21 slots per tile), allocated on first use
    uint8_t *d_dtab2 = nullptr;
    uint64_t cap2 = 0;
    std::vector<uint64_t> last_off;      // tile offsets already resident in d_off (skip the upload when unchanged)
    uint32_t last_t0 = 0;
    hipStream_t side = nullptr;          // the context's one side stream (narrow level-1 RGBA decode: the alpha branch beside the nl-context branch; level 2: rans1_wide_dec.hpp); the wide level-1 form has none
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DecTile *d_info = nullptr;
    uint64_t *d_off = nullptr;
    uint8_t *d_ctxsym = nullptr, *d_asym = nullptr, *d_alpha = nullptr, *d_nlseq = nullptr;  // (inside the arena)
    uint32_t *d_resid = nullptr;         // (inside the arena, 16 words in: k_dec_recon_band reads up to 3 words before a tile's first)
    uint8_t *arena = nullptr;
    uint64_t arena_bytes = 0;
};
inline void decode_ws_free(DecodeWs &w) {
    for (hipEvent_t e : {w.ev_fork, w.ev_join}) if (e) (void)hipEventDestroy(e);
    w = DecodeWs();
}
// an event of the workspace, created when a launch sequence first needs it
inline bool decode_ws_event(hipEvent_t &e) { return e || hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; }

// The reference decoder trusts the file ("no bounds checks on file contents"); on a GPU a wild
// offset is a fault that can take the device down, so every length / offset / count is checked here, once, and a bad
// tile is skipped (its pixels stay untouched) with bit 0 of *status set.
__global__ void k_dec_parse(const uint8_t *const *__restrict__ blobs, const uint64_t *__restrict__ off,
                            const uint64_t *__restrict__ blob_len, uint32_t cnt, uint32_t total, uint32_t spt, int pxsz,
                            const TileDesc *__restrict__ tiles, TileSel sel, DecTile *__restrict__ info,
                            uint32_t *__restrict__ status) {
    bw_prio();
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const uint32_t vt = vtile(sel, j), il = imglin(sel, vt);  // off[] is image-major (host order)
    const TileDesc t = tiles[vt];
    DecTile d{};
    d.blob = blobs[t.img] + off[il];
    const uint64_t avail = blob_len[t.img] > off[il] ? blob_len[t.img] - off[il] : 0;
    const uint8_t *f = d.blob;
    bool ok = avail >= 4;
    uint32_t L = 0;
    if (ok) {
        const uint32_t h0 = ld32u(f);
        d.type = h0 >> 24;
        L = h0 & 0xFFFFFF;
        ok = L <= avail;
    }
    if (ok && d.type == 0) ok = L == t.n * (uint32_t)pxsz + 4;
    else if (ok) {
        ok = L >= 12 && (d.type >> 4) == 1;
        const uint32_t ksz = ok ? ld32u(f + 4) : 0;  // includes itself (libxpng.c:556)
        ok = ok && ksz >= 8 && (ksz & 3) == 0 && 4 + (uint64_t)ksz <= L;
        d.kbytes = ksz - 4;
        uint64_t o = 4 + (uint64_t)ksz;
        uint32_t acc = 0, coded = 0;  // acc: 16-byte aligned start of the next context stream inside the tile's symbol area
        for (uint32_t c = 0; c < spt && ok; c++) {
            ok = o + 4 <= L;
            if (!ok) break;
            const uint32_t b0 = ld32u(f + o), ty = b0 >> 24, sz = ty == 0 ? 4 : (b0 & 0xFFFFFF);
            ok = ty <= 4 && sz >= (ty == 0 ? 4u : 8u) && (sz & 3) == 0 && o + sz <= L;
            if (!ok) break;
            const uint32_t w1 = ty ? ld32u(f + o + 4) : 0, n = w1 & 0xFFFFFF, v2 = w1 >> 24;
            if (ty == 2) ok = v2 >= 1 && v2 <= 8 && 8 + 4 * (((uint64_t)n * v2 + 31) >> 5) <= sz;
            if (ty >= 3) {
                ok = sz >= 28 + 4 && v2 <= 254;
                if (ok) {
                    const uint32_t h2 = ld32u(f + o + 8), toff = h2 & 0xFFFFFF, pb = h2 >> 24;
                    ok = pb >= 10 && pb <= 15 && toff >= 5 && 8 + 4 * (uint64_t)toff < sz;
                }
            }
            d.blk_off[c] = (uint32_t)o;
            d.blk_n[c] = ty == 0 ? 0 : n;
            if (c < 9) { d.ctx_start[c] = acc; acc = (acc + d.blk_n[c] + 15u) & ~15u; coded += d.blk_n[c]; ok = ok && coded <= t.n - 1; }
            else ok = ok && d.blk_n[c] <= t.n - 1;
            o += sz;
        }
        d.ctx_start[9] = coded;
    }
    if (!ok) { d.type = TILE_BAD; atomicOr(status, 1u); }
    info[j] = d;
}

// --------------------------------------------------------------------------------------------------
// one v2 block -> symbols (decompress_block_v2, libxpng.c:429-493).  Single-wave workgroup per (tile, stream).
//
// The recurrence runs backwards over the symbols with two interleaved states; even lanes carry state0, odd lanes
// state1 (lanes 2..63 replicate lanes 0/1, so nothing in the loop needs a lane mask except the stores).  The
// dependent chain per step is kept short:
//   * hot-symbol cache: the two most probable symbols' (cum, F) live in registers; a step whose slot falls into one of
//     them needs no table lookup at all (alpha and nl streams are heavily skewed).  Otherwise slot -> symbol comes
//     from an LDS byte table and (F, cum) from a 256-entry LDS table;
//   * renormalisation words: the cursor is a SCALAR (it moves by popcount of a 2-bit ballot; state1 pops first as in
//     libxpng.c:486-487); words are staged coalesced into an LDS ring and the two candidates words[rw-1], words[rw-2]
//     are read speculatively at the top of the step, off the dependent chain;
//   * decoded symbols go to an LDS ring and are flushed 512 at a time.
// MAXPB bounds the slot table (2^MAXPB bytes of LDS): 12 for the nl-context streams, 15 for alpha.  A block whose
// header asks for more than MAXPB is left to the general (MAXPB = 15) launch (`only_over` selects those).
// One rANS v2 block, one wavefront (the body of k_rans2_decode and of k_rans2_decode_rest below).
// COARSE = false: no slot table at all - a slot is resolved by a binary search over the cumulative counts.  Slow, but 4.6 KB of
// LDS instead of 37: the form k_rans2_decode_rest uses (streams the reference never writes; its launch sits on the critical path of
// every batched decode and used to wait milliseconds for 128 x 37 KB of LDS to find nothing to do).
template <int MAXPB, bool COARSE = true>
__device__ __forceinline__ void rans2_decode_stream(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles, TileSel sel,
                                                    const uint32_t j, const uint32_t c, int only_over, uint8_t *__restrict__ ctxsym,
                                                    uint8_t *__restrict__ asym, uint64_t *__restrict__ dbg, const bool packed = false) {
    // per group of 8 slots: (F | cum << 16, symbol) of the symbol owning slot (g << 3): ONE LDS read resolves a slot whose group
    // lies inside one symbol's range (wide symbols: the probable ones), else a short forward scan over fc[] follows
    __shared__ uint2 coarse[COARSE ? 1 << (MAXPB - 3) : 1];
    __shared__ uint32_t fc[256];
    __shared__ uint32_t Fs[260];
    __shared__ uint32_t wring[512];
    __shared__ __align__(8) uint8_t oring[512];
    const uint32_t lane = threadIdx.x & 63, par = lane & 1;
    const DecTile d = info[j];
    if (d.type == 0 || d.type == TILE_BAD) return;
    const uint32_t vt = vtile(sel, j);
    const TileDesc t = tiles[vt];
    const uint8_t *in = d.blob + d.blk_off[c];
    uint8_t *out = c < 9 ? ctxsym + t.pbase + d.ctx_start[c] : asym + t.pbase;
    const uint32_t h0 = sgpr(ld32u(in)), type = h0 >> 24;  // header words are wave-uniform: keep them (and every loop
    if (type == 0) return;                                  // cursor derived from them) in SGPRs
    const uint32_t csz = h0 & 0xFFFFFF;
    const uint8_t *end = in + csz;
    const uint32_t h1 = sgpr(ld32u(in + 4)), n = h1 & 0xFFFFFF, v2 = h1 >> 24;
    if (type <= 2 && only_over) return;
    if (rans2_dec_plain(type, in, end, n, v2, out, packed)) return;
    const uint32_t N = v2 + 2;
    const uint32_t h2 = sgpr(ld32u(in + 8));
    const int pb = (int)(h2 >> 24);
    if ((pb > MAXPB) || (only_over == 1 && pb <= 12)) return;  // handled by the other launch
    uint64_t *stamp = dbg ? dbg + ((uint64_t)vt * 10 + c) * 8 : nullptr;
#define XPNG_DSTAMP(k) do { if (stamp && lane == 0) stamp[k] = __builtin_readcyclecounter(); } while (0)
    XPNG_DSTAMP(0);
    const uint8_t *words = in + 12;
    const uint8_t *table = in + 8 + 4ull * (h2 & 0xFFFFFF);
    rans2_dec_freqs(type, (uint32_t)pb, N, table, end, Fs);
    __syncthreads();
    const uint2 hot = rans_dec_cum([&](uint32_t i) { return Fs[i]; }, N, fc);  // (F << 8 | sym) of the two most probable symbols
    __syncthreads();
    if (COARSE) {   // coarse slot -> symbol: the owner of every 8th slot
        const uint32_t groups = 1u << (pb - 3);
        for (uint32_t g = lane; g < groups; g += 64) {
            const uint32_t lo = rans_dec_owner(fc, N, g << 3);
            coarse[g] = make_uint2(fc[lo], lo);
        }
    }
    __syncthreads();
    XPNG_DSTAMP(1);
    const uint32_t sym0 = hot.x & 255u, sym1 = hot.y & 255u;
    const uint32_t e0 = fc[sym0], e1 = fc[sym1];
    const uint32_t F0 = e0 & 0xFFFF, C0 = e0 >> 16, F1 = e1 & 0xFFFF, C1 = e1 >> 16;
    const uint32_t mask = (1u << pb) - 1;
    const uint8_t *sp = table - 16;  // state0 at table-16, state1 at table-8
    const uint32_t nw = (uint32_t)((sp - words) >> 2);  // renormalisation words below the states
    uint32_t rw = nw;                                    // scalar cursor: next word to pop is words[rw-1]
    uint32_t ring_lo = nw > 512 ? nw - 512 : 0;          // ring holds word indices [ring_lo, ring_lo + 512)
    for (uint32_t i = ring_lo + lane; i < nw; i += 64) wring[i & 511u] = ld32u(words + 4ull * i);
    uint64_t s = ld64u(sp + 8 * par);
    __syncthreads();
    // The step pieces below are MACROS, not lambdas: with by-reference closures used from three loops (prologue, straight-line
    // blocks, epilogue) the compiler kept the closures - and with them the state, the cursors and the word candidates - in
    // scratch memory behind pointers (ScratchSize 464, a scratch access every few instructions of the chain).
    // uniform: bring the next lower 256 words into the ring before the cursor reaches them
#define XPNG_DEC_REFILL()                                                                                         \
    do {                                                                                                          \
        if (ring_lo > 0 && rw < ring_lo + 128) {                                                                  \
            const uint32_t new_lo_ = ring_lo > 256 ? ring_lo - 256 : 0;                                           \
            __syncthreads();                                                                                      \
            for (uint32_t i_ = new_lo_ + lane; i_ < ring_lo; i_ += 64) wring[i_ & 511u] = ld32u(words + 4ull * i_); \
            ring_lo = new_lo_;                                                                                    \
            __syncthreads();                                                                                      \
        }                                                                                                         \
    } while (0)
    // uniform: symbols [base, min(base+512, n)) leave the LDS ring (packed: two to a byte, rans_dec.hpp; base is even)
#define XPNG_DEC_FLUSH(base)                                                                                      \
    do {                                                                                                          \
        __syncthreads();                                                                                          \
        const uint32_t hi_ = (base) + 512 < n ? (base) + 512 : n;                                                 \
        if (packed) {                                                                                             \
            for (uint32_t i_ = (base) + 2 * lane; i_ < hi_; i_ += 128)                                            \
                out[i_ >> 1] = (uint8_t)ctxn_byte(oring[i_ & 511u], i_ + 1 < hi_ ? oring[(i_ + 1) & 511u] : 0u);  \
        } else {                                                                                                  \
            for (uint32_t i_ = (base) + lane; i_ < hi_; i_ += 64) out[i_] = oring[i_ & 511u];                     \
        }                                                                                                         \
        __syncthreads();                                                                                          \
    } while (0)
    // one symbol out of this lane's state -> sym; need = the state must refill
#define XPNG_DEC_ONE(sym, need)                                                                                   \
    do {                                                                                                          \
        const uint32_t slot_ = (uint32_t)s & mask;                                                                \
        const uint32_t d0_ = slot_ - C0, d1_ = slot_ - C1;                                                        \
        const bool hit0_ = d0_ < F0, hit1_ = d1_ < F1;                                                            \
        uint32_t F_, off_;                                                                                        \
        if (__ballot(!(hit0_ || hit1_)) == 0) {                                                                   \
            F_ = hit0_ ? F0 : F1; off_ = hit0_ ? d0_ : d1_; sym = hit0_ ? sym0 : sym1;                            \
        } else {                                                                                                  \
            uint32_t e_;                                                                                          \
            if (COARSE) { const uint2 cg_ = coarse[slot_ >> 3]; sym = cg_.y; e_ = cg_.x; }                        \
            else { sym = rans_dec_owner(fc, N, slot_); e_ = fc[sym]; }                                            \
            while (slot_ - (e_ >> 16) >= (e_ & 0xFFFF) && sym + 1 < N) e_ = fc[++sym];  /* to the symbol whose [cum, cum+F) holds the slot */ \
            F_ = e_ & 0xFFFF; off_ = slot_ - (e_ >> 16);                                                          \
        }                                                                                                         \
        s = (uint64_t)F_ * (s >> pb) + off_;                                                                      \
        need = s < RANS_L;                                                                                        \
    } while (0)
    // uniform, rare: state1 refills first (libxpng.c:486-487); the candidates words[rw-1], words[rw-2] live in registers and are
    // re-read from the LDS ring only in the steps that consumed one
#define XPNG_DEC_RENORM(need, m)                                                          \
    do {                                                                                  \
        const uint32_t n1_ = (m) >> 1, n0_ = (m) & 1u;                                    \
        const uint32_t wsel_ = par ? w1 : (n1_ ? w2 : w1);                                \
        if (need) s = (s << 32) | wsel_;                                                  \
        rw = rw > n0_ + n1_ ? rw - (n0_ + n1_) : 0;                                       \
        XPNG_DEC_REFILL();                                                                \
        w1 = wring[(rw > 0 ? rw - 1 : 0) & 511u];                                         \
        w2 = wring[(rw > 1 ? rw - 2 : 0) & 511u];                                         \
    } while (0)
#define XPNG_DEC_PAIR()                                                                   \
    do {                                                                                  \
        i -= 2;                                                                           \
        uint32_t sym_ = 0;                                                                \
        bool need_;                                                                       \
        XPNG_DEC_ONE(sym_, need_);                                                        \
        const uint32_t m_ = sgpr((uint32_t)__ballot(need_) & 3u);                         \
        if (lane < 2) oring[(i + par) & 511u] = (uint8_t)sym_;                            \
        if (m_) XPNG_DEC_RENORM(need_, m_);                                               \
        if ((i & 511u) == 0) XPNG_DEC_FLUSH(i);                                           \
    } while (0)
    rw = sgpr(rw); ring_lo = sgpr(ring_lo);
    uint32_t i = sgpr(n);  // scalar
    if (n & 1) {  // odd tail comes from state0 only (libxpng.c:471-476)
        i--;
        uint32_t sym = 0;
        const uint64_t keep = s;
        bool need;
        XPNG_DEC_ONE(sym, need);
        if (par) s = keep;
        const uint32_t need0 = sgpr((uint32_t)__ballot(need && !par) & 1u);
        if (need0) {
            if (rw > 0) rw--;
            if (!par) s = (s << 32) | wring[rw & 511u];
        }
        if (lane == 0) oring[i & 511u] = (uint8_t)sym;
        if ((i & 511u) == 0) XPNG_DEC_FLUSH(i);
    }
    uint32_t w1 = wring[(rw > 0 ? rw - 1 : 0) & 511u], w2 = wring[(rw > 1 ? rw - 2 : 0) & 511u];
    while (i >= 2 && (i & 7u)) XPNG_DEC_PAIR();  // down to a multiple of 8 symbols
    // Main loop: straight-line blocks of 4 pair steps.  A lane packs its four symbols into one register; at the block end the
    // pair's 8 bytes are interleaved (DPP swap + two v_perm) and leave as ONE 8-byte LDS store, and the ring flush is checked
    // once: the per-step store / address arithmetic / loop bookkeeping (and the wait for that store at the top of every step)
    // are gone from the dependent chain.
    while (i >= 8) {
        uint32_t acc = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            // (tried in round 3: the step first computed as if both states sat in a hot symbol and needed no refill, ONE ballot of
            //  "cold symbol OR refill" guarding the general path - 16.4 -> 16.7 ms on the 4096^2 image: on this alpha stream the pair
            //  is in the general path more than half of the steps, and those then pay the speculative work on top)
            uint32_t sym = 0;
            bool need;
            XPNG_DEC_ONE(sym, need);
            const uint32_t m = sgpr((uint32_t)__ballot(need) & 3u);
            if (m) XPNG_DEC_RENORM(need, m);
            acc = (acc << 8) | sym;
        }
        i -= 8;
        const uint32_t oth = swap_pair(acc);
        const uint32_t lo = __builtin_amdgcn_perm(oth, acc, 0x05010400u), hi = __builtin_amdgcn_perm(oth, acc, 0x07030602u);
        if (lane == 0) *reinterpret_cast<uint2 *>(oring + (i & 511u)) = make_uint2(lo, hi);
        if ((i & 511u) == 0) XPNG_DEC_FLUSH(i);
    }
    while (i >= 2) XPNG_DEC_PAIR();
#undef XPNG_DEC_PAIR
#undef XPNG_DEC_RENORM
#undef XPNG_DEC_ONE
#undef XPNG_DEC_FLUSH
#undef XPNG_DEC_REFILL
    XPNG_DSTAMP(2);
}

template <int MAXPB>
__global__ __launch_bounds__(64) void k_rans2_decode(const DecTile *__restrict__ info,
                                                     const TileDesc *__restrict__ tiles, TileSel sel, uint32_t c_first,
                                                     uint32_t c_count, int only_over, uint8_t *__restrict__ ctxsym,
                                                     uint8_t *__restrict__ asym, uint64_t *__restrict__ dbg) {
    rans2_decode_stream<MAXPB>(info, tiles, sel, blockIdx.x / c_count, c_first + blockIdx.x % c_count, only_over, ctxsym, asym, dbg);
}

// Wide mode: the streams k_rans2_dec_prep left to the narrow form (kind 2 among the context streams: never written by the
// reference).  A small fixed grid looks through the stream list 64 entries at a time - one workgroup per stream, as above, is
// 46 656 workgroups asking for 38 KB of LDS each to find nothing, on the critical path between the context chains and the walk.
template <int MAXPB>
__global__ __launch_bounds__(64) void k_rans2_decode_rest(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles, TileSel sel,
                                                          uint32_t total, uint32_t c_first, uint32_t c_count, uint8_t *__restrict__ ctxsym,
                                                          uint8_t *__restrict__ asym, uint64_t *__restrict__ dbg, const WDec *__restrict__ wdec,
                                                          uint32_t pk0) {
    const uint32_t lane = threadIdx.x & 63, n = total * c_count;
    for (uint32_t base = blockIdx.x * 64; base < n; base += gridDim.x * 64) {
        const uint32_t idx = base + lane;
        const bool mine = idx < n && wdec[(uint64_t)(idx / c_count) * 10 + c_first + idx % c_count].kind == 2;
        uint64_t m = __ballot(mine);
        while (m) {
            const uint32_t id2 = sgpr(base + (uint32_t)__builtin_ctzll(m));
            m &= m - 1;
            const uint32_t cs = c_first + id2 % c_count;
            rans2_decode_stream<MAXPB, false>(info, tiles, sel, id2 / c_count, cs, 2, ctxsym, asym, dbg, cs < 9 && id2 / c_count >= pk0);
            __syncthreads();
        }
    }
}

// --------------------------------------------------------------------------------------------------
// alpha plane (RGBA).  a(x,y) = a(left) + d, except column 0: a(0,y) = a(0,y-1) + d (libxpng.c:798-800 with
// pr = p1x_ for rows 0 / interior and p1y_ for column 0).  grid = tiles, block = 1024.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_dec_alpha(const DecTile *__restrict__ info,
                                                    const TileDesc *__restrict__ tiles, TileSel sel,
                                                    const uint8_t *__restrict__ asym, uint8_t *__restrict__ alpha) {
    const uint32_t j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const DecTile d = info[j];
    if (d.type == 0 || d.type == TILE_BAD) return;
    const TileDesc t = tiles[vtile(sel, j)];
    const uint8_t *sy = asym + t.pbase;  // sy[i-1] = symbol of pixel i
    uint8_t *al = alpha + t.pbase;
    __shared__ uint32_t s_wave[THREADS / 64];
    __shared__ uint32_t s_carry;
    // first pixel's alpha: 4th byte of the first k word (MSB-first R,G,B,A)
    const uint32_t a0 = ld32u(d.blob + 8) & 0xFF;
    // ---- column 0: inclusive scan down the rows
    if (tid == 0) s_carry = a0;
    __syncthreads();
    if (tid == 0) al[0] = (uint8_t)a0;
    for (uint32_t y0 = 1; y0 < t.h; y0 += THREADS) {
        const uint32_t y = y0 + tid;
        const uint32_t dv = y < t.h ? (uint32_t)zz_dec(sy[(uint64_t)y * t.w - 1]) & 255u : 0u;
        uint32_t incl = dv;
        incl = wave_scan_incl(incl);
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        uint32_t base = s_carry;
        for (uint32_t w2 = 0; w2 < wv; w2++) base += s_wave[w2];
        if (y < t.h) al[(uint64_t)y * t.w] = (uint8_t)(base + incl);
        __syncthreads();
        if (tid == THREADS - 1) s_carry = (base + incl) & 255u;
        __syncthreads();
    }
    __syncthreads();
    // ---- rows: each wave scans whole rows left to right, 256 pixels per step (a lane owns one aligned dword of the plane);
    // the symbol dwords and the row's column-0 value are read one step ahead, interior dwords are stored whole
    if (t.w == 1) return;
    constexpr uint32_t NWV = THREADS / 64;
    const uint32_t *sy4 = reinterpret_cast<const uint32_t *>(sy);
    uint32_t *al4 = reinterpret_cast<uint32_t *>(al);
    const uint32_t spr = ((t.w + 6) / 4 + 63) / 64;  // steps per row (rows start at any byte alignment)
    uint32_t y = wv, st = 0, carry = 0;
    uint32_t n_cur = 0, n_prev = 0, n_c0 = 0;
    if (y < t.h) {
        const uint32_t rs = y * t.w, g = (rs >> 2) + lane;
        if (4 * g < rs + t.w) { n_cur = sy4[g]; n_prev = g ? sy4[g - 1] : 0u; }
        n_c0 = al[rs];
    }
    while (y < t.h) {
        const uint32_t cur = n_cur, prev = n_prev, c0 = n_c0;
        const uint32_t rs = y * t.w, re = rs + t.w, g = (rs >> 2) + lane + 64 * st, idx0 = 4 * g;
        uint32_t ny = y, nst = st + 1;
        if (nst == spr) { nst = 0; ny = y + NWV; }
        if (ny < t.h) {
            const uint32_t nrs = ny * t.w, ng = (nrs >> 2) + lane + 64 * nst;
            if (4 * ng < nrs + t.w) { n_cur = sy4[ng]; n_prev = ng ? sy4[ng - 1] : 0u; }
            if (nst == 0) n_c0 = al[nrs];
        }
        if (st == 0) carry = c0;
        // deltas of pixels idx0 .. idx0+3 (symbol of pixel i sits at sy[i-1]); pixels outside (rs, re) contribute nothing
        const uint32_t u = __builtin_amdgcn_alignbyte(cur, prev, 3);
        uint32_t d4 = ((u >> 1) & 0x7F7F7F7Fu) ^ ((u & 0x01010101u) * 255u);
        const int32_t lo = (int32_t)rs - (int32_t)idx0 + 1, hi = (int32_t)re - (int32_t)idx0;  // bytes [lo, hi) of the dword are in the row
        uint32_t mask = lo <= 0 ? 0xFFFFFFFFu : (lo >= 4 ? 0u : 0xFFFFFFFFu << (8 * lo));
        mask &= hi >= 4 ? 0xFFFFFFFFu : (hi <= 0 ? 0u : ~(0xFFFFFFFFu << (8 * hi)));
        d4 &= mask;
        const uint32_t p0 = d4 & 255u, p1 = p0 + ((d4 >> 8) & 255u), p2 = p1 + ((d4 >> 16) & 255u), p3 = p2 + (d4 >> 24);
        const uint32_t incl = wave_scan_incl(p3);
        const uint32_t base = carry + incl - p3;
        const uint32_t b0 = (base + p0) & 255u, b1 = (base + p1) & 255u, b2 = (base + p2) & 255u, b3 = (base + p3) & 255u;
        if (mask == 0xFFFFFFFFu) al4[g] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        else if (mask) {
            if (mask & 0x000000FFu) al[idx0] = (uint8_t)b0;
            if (mask & 0x0000FF00u) al[idx0 + 1] = (uint8_t)b1;
            if (mask & 0x00FF0000u) al[idx0 + 2] = (uint8_t)b2;
            if (mask & 0xFF000000u) al[idx0 + 3] = (uint8_t)b3;
        }
        carry = (carry + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63)) & 255u;
        y = ny; st = nst;
    }
}

// --------------------------------------------------------------------------------------------------
// context chain (libxpng.c:803: nl = *cx[nl]++, starting from 0).  Strictly serial per tile: one wave per tile, and the step is
// made as short as the hardware allows.  `base` = 256-byte aligned start of the tile's symbol area, qs = this lane's queue start
// inside it (lanes 0..8), total = number of symbols to produce; output: the nl sequence in coded-pixel order.  Single-wave workgroup.
constexpr uint32_t WALK_RING = 512, WALK_UNIT = WALK_RING / 2;  // LDS ring of one context queue, and the unit it is refilled in
// The chain runs on the SCALAR unit.  (Its predecessor kept the queue heads in VGPR lanes: a step of ~16 VALU instructions of which
// five are dependent - readlane -> s_and -> v_cmp -> v_cndmask -> 64-bit shift -> readlane - 45-60 ns.  It has no caller left and is
// gone; git history has it.)  Here the nine queue heads are 64-bit SGPR pairs s[40+2c : 41+2c] = (four symbols | marker bit 32) and the
// step is nine scalar instructions, ~21 ns:
//     m0 = 2 cur;  t = SGPR[40 + m0] (s_movrels_b64);  cur = t & 0xff;  t >>= 8;  t == 1 ? refill;  SGPR[40 + m0] = t;  out lane k = cur
// The refill (once per four pops of a queue) takes the queue's next dword from lane c's register pair (w0, w1 <- its LDS ring)
// by v_readlane; the LDS read that tops w1 up has eight pops of that queue to land.  The head registers live in VGPR lanes
// between blocks of 64 steps (the compiler may use any SGPR between two asm statements), symbols > 8 (corrupt streams only)
// are masked to 4 bits and index spare pairs s[58:71], so no register outside s[40:77] is ever touched.
// Requires 4-byte aligned queue starts (k_dec_parse aligns them to 16).
#define XPNG_WS(k)                                                                                                                  \
    "s_lshl_b32 m0, %[cur], 1\n s_nop 0\n s_movrels_b64 s[74:75], s[40:41]\n s_and_b32 %[cur], s74, 0xff\n s_lshr_b64 s[74:75], s[74:75], 8\n" \
    "s_cmp_eq_u64 s[74:75], 1\n s_cbranch_scc1 .Lwr%=_" #k "\n.Lwa%=_" #k ":\n s_movreld_b64 s[40:41], s[74:75]\n v_writelane_b32 %[vout], %[cur], " #k "\n"
#define XPNG_WR(k)                                                                                                                  \
    ".Lwr%=_" #k ":\n s_lshr_b32 s72, m0, 1\n s_nop 3\n v_readlane_b32 s74, %[w0], s72\n s_and_b32 s74, s74, 0x0f0f0f0f\n s_mov_b32 s75, 1\n"   \
    "v_cmp_eq_u32 vcc, s72, %[lanev]\n s_and_saveexec_b64 s[76:77], vcc\n s_waitcnt lgkmcnt(0)\n v_mov_b32 %[w0], %[w1]\n"               \
    "v_and_b32 %[vt], 0x1ff, %[rd]\n v_add_u32 %[vt], %[vt], %[rbase]\n ds_read_b32 %[w1], %[vt]\n v_add_u32 %[rd], 4, %[rd]\n"           \
    "s_mov_b64 exec, s[76:77]\n s_branch .Lwa%=_" #k "\n"
__device__ inline void ctx_walk_salu(const uint8_t *__restrict__ base, uint32_t qs_in, uint32_t total, uint8_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    __shared__ __align__(16) uint8_t qring[9][WALK_RING];
    const uint32_t qs = lane < 9 ? qs_in : 0;
    const uint32_t qsa = qs & ~15u;
    for (uint32_t c = 0; c < 9; c++) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)qsa, (int)c);
        if (lane < WALK_RING / 16) reinterpret_cast<uint4 *>(qring[c])[lane] = (reinterpret_cast<const uint4 *>(base + a) + lane)[0];  // both units
    }
    __syncthreads();
    uint32_t filled = 2;                      // units staged for this lane's queue
    const uint32_t ql = lane < 9 ? lane : 0;  // lanes >= 9 alias queue 0's ring; nothing they hold is ever a real symbol
    const uint32_t p0 = qs & 12u;
    const uint32_t *r0 = reinterpret_cast<const uint32_t *>(&qring[ql][p0]);
    uint32_t qlo = lane < 9 ? (r0[0] & 0x0F0F0F0Fu) : 0u, qhi = 1u;
    uint32_t w0 = r0[1], w1 = r0[2], rd = p0 + 12, vt, vout;
    const uint32_t rbase = (uint32_t)(uintptr_t)&qring[ql][0];  // LDS byte address of this lane's ring (low 32 bits of the flat address)
    uint32_t cur = 0;
    for (uint32_t k = 0; k < total; k += 64) {
        {   // stage one more unit for every queue whose reads can reach the end of what is staged within this block
            uint64_t m = __ballot(lane < 9 && rd + 96 >= filled * WALK_UNIT);
            if (m) {
                __syncthreads();
                while (m) {
                    const int c = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)qsa, c);
                    const uint32_t u = (uint32_t)__builtin_amdgcn_readlane((int)filled, c);
                    if (lane < WALK_UNIT / 16) reinterpret_cast<uint4 *>(qring[c])[(u & 1u) * (WALK_UNIT / 16) + lane] = (reinterpret_cast<const uint4 *>(base + a) + lane)[u * (WALK_UNIT / 16)];
                    if ((int)lane == c) filled++;
                }
                __syncthreads();
            }
        }
        asm volatile(
            "s_mov_b32 s73, m0\n"
        "v_readlane_b32 s40, %[qlo], 0\n v_readlane_b32 s41, %[qhi], 0\n"
        "v_readlane_b32 s42, %[qlo], 1\n v_readlane_b32 s43, %[qhi], 1\n"
        "v_readlane_b32 s44, %[qlo], 2\n v_readlane_b32 s45, %[qhi], 2\n"
        "v_readlane_b32 s46, %[qlo], 3\n v_readlane_b32 s47, %[qhi], 3\n"
        "v_readlane_b32 s48, %[qlo], 4\n v_readlane_b32 s49, %[qhi], 4\n"
        "v_readlane_b32 s50, %[qlo], 5\n v_readlane_b32 s51, %[qhi], 5\n"
        "v_readlane_b32 s52, %[qlo], 6\n v_readlane_b32 s53, %[qhi], 6\n"
        "v_readlane_b32 s54, %[qlo], 7\n v_readlane_b32 s55, %[qhi], 7\n"
        "v_readlane_b32 s56, %[qlo], 8\n v_readlane_b32 s57, %[qhi], 8\n"
        "v_readlane_b32 s58, %[qlo], 9\n v_readlane_b32 s59, %[qhi], 9\n"
        "v_readlane_b32 s60, %[qlo], 10\n v_readlane_b32 s61, %[qhi], 10\n"
        "v_readlane_b32 s62, %[qlo], 11\n v_readlane_b32 s63, %[qhi], 11\n"
        "v_readlane_b32 s64, %[qlo], 12\n v_readlane_b32 s65, %[qhi], 12\n"
        "v_readlane_b32 s66, %[qlo], 13\n v_readlane_b32 s67, %[qhi], 13\n"
        "v_readlane_b32 s68, %[qlo], 14\n v_readlane_b32 s69, %[qhi], 14\n"
        "v_readlane_b32 s70, %[qlo], 15\n v_readlane_b32 s71, %[qhi], 15\n"
        "s_nop 3\n"
        XPNG_WS(0)
        XPNG_WS(1)
        XPNG_WS(2)
        XPNG_WS(3)
        XPNG_WS(4)
        XPNG_WS(5)
        XPNG_WS(6)
        XPNG_WS(7)
        XPNG_WS(8)
        XPNG_WS(9)
        XPNG_WS(10)
        XPNG_WS(11)
        XPNG_WS(12)
        XPNG_WS(13)
        XPNG_WS(14)
        XPNG_WS(15)
        XPNG_WS(16)
        XPNG_WS(17)
        XPNG_WS(18)
        XPNG_WS(19)
        XPNG_WS(20)
        XPNG_WS(21)
        XPNG_WS(22)
        XPNG_WS(23)
        XPNG_WS(24)
        XPNG_WS(25)
        XPNG_WS(26)
        XPNG_WS(27)
        XPNG_WS(28)
        XPNG_WS(29)
        XPNG_WS(30)
        XPNG_WS(31)
        XPNG_WS(32)
        XPNG_WS(33)
        XPNG_WS(34)
        XPNG_WS(35)
        XPNG_WS(36)
        XPNG_WS(37)
        XPNG_WS(38)
        XPNG_WS(39)
        XPNG_WS(40)
        XPNG_WS(41)
        XPNG_WS(42)
        XPNG_WS(43)
        XPNG_WS(44)
        XPNG_WS(45)
        XPNG_WS(46)
        XPNG_WS(47)
        XPNG_WS(48)
        XPNG_WS(49)
        XPNG_WS(50)
        XPNG_WS(51)
        XPNG_WS(52)
        XPNG_WS(53)
        XPNG_WS(54)
        XPNG_WS(55)
        XPNG_WS(56)
        XPNG_WS(57)
        XPNG_WS(58)
        XPNG_WS(59)
        XPNG_WS(60)
        XPNG_WS(61)
        XPNG_WS(62)
        XPNG_WS(63)
            "s_branch .Lwend%=\n"
        XPNG_WR(0)
        XPNG_WR(1)
        XPNG_WR(2)
        XPNG_WR(3)
        XPNG_WR(4)
        XPNG_WR(5)
        XPNG_WR(6)
        XPNG_WR(7)
        XPNG_WR(8)
        XPNG_WR(9)
        XPNG_WR(10)
        XPNG_WR(11)
        XPNG_WR(12)
        XPNG_WR(13)
        XPNG_WR(14)
        XPNG_WR(15)
        XPNG_WR(16)
        XPNG_WR(17)
        XPNG_WR(18)
        XPNG_WR(19)
        XPNG_WR(20)
        XPNG_WR(21)
        XPNG_WR(22)
        XPNG_WR(23)
        XPNG_WR(24)
        XPNG_WR(25)
        XPNG_WR(26)
        XPNG_WR(27)
        XPNG_WR(28)
        XPNG_WR(29)
        XPNG_WR(30)
        XPNG_WR(31)
        XPNG_WR(32)
        XPNG_WR(33)
        XPNG_WR(34)
        XPNG_WR(35)
        XPNG_WR(36)
        XPNG_WR(37)
        XPNG_WR(38)
        XPNG_WR(39)
        XPNG_WR(40)
        XPNG_WR(41)
        XPNG_WR(42)
        XPNG_WR(43)
        XPNG_WR(44)
        XPNG_WR(45)
        XPNG_WR(46)
        XPNG_WR(47)
        XPNG_WR(48)
        XPNG_WR(49)
        XPNG_WR(50)
        XPNG_WR(51)
        XPNG_WR(52)
        XPNG_WR(53)
        XPNG_WR(54)
        XPNG_WR(55)
        XPNG_WR(56)
        XPNG_WR(57)
        XPNG_WR(58)
        XPNG_WR(59)
        XPNG_WR(60)
        XPNG_WR(61)
        XPNG_WR(62)
        XPNG_WR(63)
            ".Lwend%=:\n"
        "v_writelane_b32 %[qlo], s40, 0\n v_writelane_b32 %[qhi], s41, 0\n"
        "v_writelane_b32 %[qlo], s42, 1\n v_writelane_b32 %[qhi], s43, 1\n"
        "v_writelane_b32 %[qlo], s44, 2\n v_writelane_b32 %[qhi], s45, 2\n"
        "v_writelane_b32 %[qlo], s46, 3\n v_writelane_b32 %[qhi], s47, 3\n"
        "v_writelane_b32 %[qlo], s48, 4\n v_writelane_b32 %[qhi], s49, 4\n"
        "v_writelane_b32 %[qlo], s50, 5\n v_writelane_b32 %[qhi], s51, 5\n"
        "v_writelane_b32 %[qlo], s52, 6\n v_writelane_b32 %[qhi], s53, 6\n"
        "v_writelane_b32 %[qlo], s54, 7\n v_writelane_b32 %[qhi], s55, 7\n"
        "v_writelane_b32 %[qlo], s56, 8\n v_writelane_b32 %[qhi], s57, 8\n"
            "s_mov_b32 m0, s73\n"
            : [qlo] "+v"(qlo), [qhi] "+v"(qhi), [w0] "+v"(w0), [w1] "+v"(w1), [rd] "+v"(rd), [vt] "=&v"(vt), [vout] "=&v"(vout), [cur] "+s"(cur)
            : [rbase] "v"(rbase), [lanev] "v"(lane)
            : "s40", "s41", "s42", "s43", "s44", "s45", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55", "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "vcc", "scc", "memory");
        if (k + lane < total) out[k + lane] = (uint8_t)vout;
    }
}
#undef XPNG_WS
#undef XPNG_WR

__global__ __launch_bounds__(64) void k_dec_walk(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles,
                                                 TileSel sel, const uint8_t *__restrict__ ctxsym,
                                                 uint8_t *__restrict__ nlseq) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x & 63;
    const DecTile d = info[j];
    if (d.type == 0 || d.type == TILE_BAD) return;
    const TileDesc t = tiles[vtile(sel, j)];
    const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.ctx_start[9]);
    XPNG_PROBE_BEGIN()
    ctx_walk_salu(ctxsym + t.pbase, lane < 9 ? d.ctx_start[lane] : 0, total, nlseq + t.pbase);  // (k_dec_parse aligns the queue starts to 16 bytes)
    XPNG_PROBE_END(6)
}

// --------------------------------------------------------------------------------------------------
// The same walk for large batches: one LANE per tile, 64 tiles per wave (k_dec_walk keeps a whole wave, and 9 KB of
// LDS, busy per tile; with thousands of tiles in flight that footprint, not the chain latency, is what hurts).
// Its queues are PACKED, two symbols to a byte (rans_dec.hpp has the layout and the ctxn_* arithmetic; the producers pack every work
// item from this kernel's j0 on): a dword holds 8 symbols, a 16-byte chunk 32.
//   head[c][lane]  = { symbols left in the current dword of queue c (next symbol in the lowest nibble), position, the following dword }
//   ringw[c][w][lane] = 64-byte window of queue c (128 symbols) as 16 dwords, lane-minor so that 64 lanes never share a bank
// The dependent chain of a step is ONE LDS round trip: ds_read_b128 head[cur] -> symbol -> cur.  The bookkeeping of the
// previous step (advance the position, pull the next window dword, write the head back) is issued behind that read and
// completes while it is in flight; when the same queue is popped twice in a row the read is stale and the registers of
// the previous step are forwarded instead.  Queue 9 is a parking queue that returns 9 forever: a lane whose tile is
// finished walks it.  Global memory is touched only at 16-step block boundaries: ONE aligned 16-byte chunk is requested for a
// queue at one service (every 32 steps) and lands in its window at the next (the chunk starts are 16-byte aligned, k_dec_parse) -
// 9 loads per lane and 32 steps.  (With a symbol to a byte a chunk held 16 symbols, a queue could lose two chunks between two
// services and each service had to request two: 18 loads, of which roughly eight in nine were requested again later.)
// LPW = tiles per wavefront (lanes 0 .. LPW - 1 carry one each, the others idle through the loop): the LDS of a wavefront is 800 LPW
// bytes - 51 KB at 64.  [r4] A workgroup that asks for 51 KB is placed only when a compute unit has that much free at once, and the
// chip-filling kernels of the other pipeline slots re-occupy every smaller hole at once: profiles/r03_wave_probe_p4.txt has the
// wide walk's wavefronts starting up to 6 (p90) / 10 ms (max) after the first one - on the decode's critical path, a kernel of ~20 ms
// of work spans ~30.  With 32 tiles per wavefront a workgroup asks for 25.6 KB (and waits for 288 scattered lines per service
// instead of 576); the price is twice the wavefronts, i.e. twice the walk's vector instructions.
constexpr uint32_t WALK_WIDE_COLS(uint32_t lpw) { return lpw + (lpw < 64 ? 1u : 0u); }  // LDS columns: one per tile + one that the idle lanes share
constexpr uint32_t WALK_WIDE_WCH = 4;  // 16-byte chunks (32 symbols each) in a queue's window: 4, or 2 (which does NOT hold the walk's invariant: see k_dec_walk_wide)
constexpr size_t WALK_WIDE_LDS_BYTES(uint32_t lpw) { return 10 * (size_t)WALK_WIDE_COLS(lpw) * 16 + 10 * 4 * WALK_WIDE_WCH * (size_t)WALK_WIDE_COLS(lpw) * 4; }  // heads + windows (k_dec_walk_wide)
// (A device function of the role-local workgroup index `bid`: k_dec_walk_wide launches it alone, k_dec_serial beside the alpha chains.)
template <uint32_t LPW>
__device__ __attribute__((always_inline)) inline void dec_walk_wide_body(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles,
                                                      TileSel sel, uint32_t total_tiles, const uint8_t *__restrict__ ctxsym,
                                                      uint8_t *__restrict__ nlseq, uint32_t j0, const uint32_t bid) {
    // window: WCH chunks of 16 B per queue; a queue is serviced every SVC-th block.  (8 chunks / every 4th block is ~8 % faster
    // alone, but 90 KB of LDS per wave instead of 50 costs the kernels beside it more than that.)
    constexpr uint32_t WCH = WALK_WIDE_WCH, SVC = 2, INIT = 2, WDW = WCH * 4, lpw = LPW, COLS = WALK_WIDE_COLS(LPW);
    static_assert(16 * SVC == CTXN_CHUNK && INIT <= WCH, "one chunk is what a queue can lose between two of its services");
    static_assert(WALK_WIDE_LDS_BYTES(LPW) == 10 * COLS * 16 + 10 * WDW * COLS * 4 && LPW >= 8 && LPW <= 64, "LDS layout");
    extern __shared__ __align__(16) uint8_t walk_wide_lds[];  // dynamic (common.hpp: why)
    u32x4_t *const head = reinterpret_cast<u32x4_t *>(walk_wide_lds);                         // [10 * COLS]
    uint32_t *const ringw = reinterpret_cast<uint32_t *>(walk_wide_lds + 10 * COLS * 16);    // [10 * WDW * COLS]
    __builtin_amdgcn_s_setprio(XPNG_CHAIN_PRIO);  // a serial chain: its latency is the critical path, the throughput kernels beside it are not
    XPNG_PROBE_BEGIN()
    const uint32_t lane_ = threadIdx.x & 63, j = j0 + bid * lpw + lane_;  // work items [j0, total_tiles)
    bool live = lane_ < lpw && j < total_tiles;
    const uint32_t lane = lane_ < lpw ? lane_ : lpw;  // LDS column of this lane (the idle lanes of a narrower form share the last one: they only ever walk the parking queue, whose heads are self-consistent whoever wrote them)
    const DecTile *d = info + (live ? j : 0);
    live = live && d->type != 0 && d->type != TILE_BAD;
    const TileDesc *t = tiles + vtile(sel, live ? j : 0);
    const uint32_t total = live ? d->ctx_start[9] : 0;
    const uintptr_t base = (uintptr_t)(ctxsym + t->pbase);
    uint8_t *out = nlseq + t->pbase;
    // where a lane without (more) symbols stores: behind the nl sequence of the tile its `out` points at (the planes carry >= 192
    // bytes of slack behind a tile; a lane without a tile points at its placeholder tile, whose sequence another lane may be writing)
    const DecTile *dh = info + (live ? j : 0);  // the tile `out` points at
    const uint32_t seq_here = (dh->type != 0 && dh->type != TILE_BAD) ? dh->ctx_start[9] : 0u;
    const uint32_t dump = (seq_here + 15u) & ~15u;
    uint32_t qoff[9], have[9];
    u32x4_t fl[9];  // in flight per queue: chunk `have`
    typedef const __attribute__((address_space(1))) u32x4_t *gp128;
    const u32x4_t zero4 = {0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 9; c++) {
        qoff[c] = live ? d->ctx_start[c] : 0;
        const gp128 src = (gp128)(base + qoff[c]);
#pragma unroll
        for (int q = 0; q < (int)INIT; q++) {
            u32x4_t v = zero4;
            if (live) v = src[q];
            ringw[(c * WDW + q * 4 + 0) * COLS + lane] = v.x; ringw[(c * WDW + q * 4 + 1) * COLS + lane] = v.y;
            ringw[(c * WDW + q * 4 + 2) * COLS + lane] = v.z; ringw[(c * WDW + q * 4 + 3) * COLS + lane] = v.w;
            if (q == 0) { const u32x4_t h = {v.x, 0u, v.y, 0u}; head[c * COLS + lane] = h; }
        }
        have[c] = INIT;
        fl[c] = zero4;
        if (live) fl[c] = src[INIT];
    }
#pragma unroll
    for (int w = 0; w < (int)WDW; w++) ringw[(9 * WDW + w) * COLS + lane] = 0x99999999u;
    { const u32x4_t h = {0x99999999u, 0u, 0x99999999u, 0u}; head[9 * COLS + lane] = h; }
    uint32_t T = total;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t v = __shfl_xor(T, o); T = v > T ? v : T; }
    T = sgpr(T);
    uint32_t cur = total > 0 ? 0u : 9u;
    // registers of the previous step: its queue and the head it popped from (lo, pos, nxt); queue 9 at start (harmless)
    uint32_t pcur = 9, plo = 0x99999999u, ppos = 0, pnxt = 0x99999999u;
    auto block = [&](uint32_t kb) __attribute__((always_inline)) {
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 16; u++) {
            // bookkeeping of the previous step: its window read goes out first, then this step's head read; both are in
            // flight together
            const uint32_t npos = ppos + 1;
            const bool cross = ctxn_cross(npos);
            const uint32_t rr = ringw[(pcur * WDW + ((ctxn_dword(npos) + 1) & (WDW - 1))) * COLS + lane];
            const u32x4_t r = head[cur * COLS + lane];               // (stale if cur == pcur: forwarded below)
            const uint32_t nlo = cross ? pnxt : ctxn_pop(plo), nnxt = cross ? rr : pnxt;
            { const u32x4_t h = {nlo, npos, nnxt, 0u}; head[pcur * COLS + lane] = h; }
            const bool same = cur == pcur;
            plo = same ? nlo : r.x; ppos = same ? npos : r.y; pnxt = same ? nnxt : (r.z | r.w);  // (r.w == 0; keeps the 4th register of the read alive so nothing else is loaded into it early)
            pcur = cur;
            const uint32_t sym = ctxn_sym(plo);
            o[u >> 2] |= sym << (8 * (u & 3));
            cur = kb + (uint32_t)u + 1 >= total ? 9u : (sym < 9u ? sym : 9u);  // (symbols > 8 only in corrupt streams)
        }
        // (an UNCONDITIONAL store: a lane past the end of its sequence writes its 16 bytes into the slack behind it.  Loads and stores
        //  retire in order on gfx9; with a store that may or may not have been issued the wait in front of a landing has to assume it was
        //  not, and then retires one load too many - one that is only a block old.)
        *reinterpret_cast<uint4 *>(out + (kb < total ? kb : dump)) = make_uint4(o[0], o[1], o[2], o[3]);
    };
    // Service of the queues of one phase, every SVC-th block boundary (so a request has 16 * SVC steps, not 16, to come back:
    // 64 lanes x 9 queues are 576 different cache lines per round).  ONE chunk is in flight per queue: it lands when the slot it
    // goes to has been read out, and the next missing chunk is requested again either way.  Between two services a queue loses at
    // most 16 * SVC = 32 symbols, one chunk, so a landing per service keeps up with it.  What the window must hold behind a service
    // at position p is the 32 symbols that may go and the dword behind them that the head looks ahead to: dwords up to
    // (p >> 3) + 5, i.e. chunk (p >> 5) + 2 when p sits in its chunk's last dword.  With WCH = 4 the service keeps
    // have >= (p >> 5) + 3 (it starts at INIT = 2 chunks at p = 0, where chunk 1 is enough, and every service that sees the
    // position in a new chunk has room to land one).  With WCH = 2 the window cannot hold chunk (p >> 5) + 2 at all: a queue
    // popped on every step (a flat raster's queue 0) reads a dword that has not landed.  tests/ctx_nibbles_host.cpp runs this
    // rule for both sizes; only the four-chunk form passes, so that is the one built.
    // (The head of queue pcur in LDS is one pop behind the registers; a chunk index can only be underestimated by that.)
    auto service = [&](int phase) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < 9; c++) {
            if ((c & (int)(SVC - 1)) != phase) continue;
            const uint32_t cq = ctxn_chunk(head[c * COLS + lane].y);  // chunk the queue is reading from
            if (have[c] - cq < WCH) {
                const uint32_t w0 = (c * WDW + (have[c] & (WCH - 1)) * 4) * COLS + lane;
                ringw[w0] = fl[c].x; ringw[w0 + COLS] = fl[c].y; ringw[w0 + 2 * COLS] = fl[c].z; ringw[w0 + 3 * COLS] = fl[c].w;
                have[c]++;
            }
            {   // (unconditional: a branch around this load makes the compiler copy the loaded registers into the loop-carried
                //  ones, and a copy is a use - it waits for the load it has just issued; lanes without a tile read their
                //  placeholder tile's bytes, which nobody looks at)
                const gp128 src = (gp128)(base + qoff[c]) + have[c];
                fl[c] = src[0];
            }
        }
    };
    // Two blocks per loop iteration, each followed by the service of ITS phase as a compile-time constant: every in-flight
    // register set is then written at one fixed place of the loop body, so no register copies (= early waits) are needed
    // and the wait in front of a landing counts only what was issued before it.
    static_assert(SVC == 2, "the loop body below is written for two service phases");
#pragma unroll 1
    for (uint32_t kb = 0; kb < T; kb += 32) {
        block(kb);
        service(0);
        block(kb + 16);
        service(1);
    }
    XPNG_PROBE_END(5)
}
template <uint32_t LPW>
__global__ __launch_bounds__(64) void k_dec_walk_wide(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles,
                                                      TileSel sel, uint32_t total_tiles, const uint8_t *__restrict__ ctxsym,
                                                      uint8_t *__restrict__ nlseq, uint32_t j0) {
    dec_walk_wide_body<LPW>(info, tiles, sel, total_tiles, ctxsym, nlseq, j0, blockIdx.x);
}

// The two serial stages of a batched decode that need nothing of each other, in ONE launch: workgroups [0, agroups) are the alpha
// chains (the longest: dispatched first; none for RGB), the rest the lane-per-tile walk over all work items.  Through round 4 they
// ran beside each other on two streams, each holding a hardware queue for its whole duration; as two ranges of one grid they run
// beside each other on the chip just the same and hold ONE queue for the longer of the two.  The role branch is
// uniform over the (single-wavefront) workgroup.  Dynamic LDS: the larger of the roles present (dec_serial_lds_bytes).
inline size_t dec_serial_lds_bytes(uint32_t agroups, uint32_t wgroups) {
    const size_t a = agroups ? DecChainLds<true, 32>::BYTES : 0, w = wgroups ? WALK_WIDE_LDS_BYTES(64) : 0;
    return a > w ? a : w;
}
__global__ __launch_bounds__(64) void k_dec_serial(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles, TileSel sel,
                                                   uint32_t total, const WDec *__restrict__ wdec, const uint8_t *__restrict__ dtab,
                                                   uint8_t *__restrict__ ctxsym, uint8_t *__restrict__ asym,
                                                   uint8_t *__restrict__ nlseq, uint32_t agroups) {
    if (blockIdx.x < agroups) rans2_dec_chain_body<true, 32, true>(info, total, 9, 1, wdec, dtab, ctxsym, asym, total, blockIdx.x);
    else dec_walk_wide_body<64>(info, tiles, sel, total, ctxsym, nlseq, 0, blockIdx.x - agroups);
}

// --------------------------------------------------------------------------------------------------
// residual extraction.  Walks the tile's pixels in raster order, 1024 per step: coded flag (alpha != 0),
// coded index = running count, bit cursor = running sum of 3*nl; pulls 3*nl bits out of k, undoes zig-zag
// and the green subtraction, and stores one packed word per pixel: r | g<<8 | b<<16 | coded<<24.
//
// FOLD [r4] (RGBA, every tile at least 4 pixels wide): the alpha plane is never materialised.  Through round 3 k_dec_alpha turned the
// alpha symbols into a plane (1 B/px read, 1 B/px written, 2.6 B/px by the counters) that this kernel read back; now it takes the
// symbols themselves.  alpha(x, y) = alpha(0, y) + sum of the row's deltas up to x, alpha(0, y) = a0 + sum of column 0's deltas up to
// y (libxpng.c:798-800: left neighbour everywhere except column 0), all mod 256.  A prologue scans column 0 (h strided symbols) into
// the tile's first h bytes of the `alpha` buffer (scratch now); in the raster-order walk every row start is a "head" whose alpha is
// that absolute value, every other pixel adds its delta to a running sum P that is NEVER reset:
//     alpha(pixel) = P(pixel) + H,   H = (alpha - P) at the latest head at or before the pixel
// so one plain prefix sum (P) and one "latest head" propagation (a running maximum of (lane + 1) << 8 | H over the wave) do it; across
// waves and iterations two bytes are carried (P and H).  One more barrier per iteration than the plane-reading form.
template <int PXSZ, int THREADS, bool FOLD = false>
__global__ __launch_bounds__(THREADS) void k_dec_resid(const DecTile *__restrict__ info,
                                                    const TileDesc *__restrict__ tiles, TileSel sel,
                                                    uint8_t *__restrict__ alpha, const uint8_t *__restrict__ asym, const uint8_t *__restrict__ nlseq,
                                                    uint32_t *__restrict__ resid, uint32_t j0) {
    bw_prio();
    static_assert(!FOLD || PXSZ == 4, "only RGBA tiles carry alpha");
    // One workgroup walks a tile in raster order, THREADS * 4 pixels per iteration; a lane owns 4 consecutive pixels: one
    // dword of the alpha plane (read one iteration ahead), up to 4 consecutive nl symbols, up to 96 bits of k, one 16-byte
    // store of residual words.  Two wave scans (coded pixels, bit lengths) and two barriers per iteration.
    const uint32_t j = j0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const DecTile d = info[j];
    if (d.type == 0 || d.type == TILE_BAD) return;
    const TileDesc t = tiles[vtile(sel, j)];
    const uint8_t *kbase = d.blob + 8;
    const uint32_t kmis = (uint32_t)(reinterpret_cast<uintptr_t>(kbase) & 3);  // tile blobs are only byte-aligned after a raw RGB tile
    const uint32_t *kal = reinterpret_cast<const uint32_t *>(kbase - kmis);
    const uint32_t kwords = (d.kbytes + kmis + 3) >> 2;  // aligned dwords that hold k bytes
    const uint32_t *al = reinterpret_cast<const uint32_t *>(alpha + t.pbase);
    const uint32_t *nls = reinterpret_cast<const uint32_t *>(nlseq + t.pbase);
    uint32_t *rs = resid + t.pbase;
    const bool useG = d.type & 1;
    constexpr uint32_t NW = THREADS / 64, PX = THREADS * 4;
    __shared__ uint32_t s_wc[2][NW], s_wb[2][NW];
    __shared__ uint32_t s_wa[2][NW];  // FOLD: per wave: sum of its deltas | H of its last head << 8 | "has a head" << 16
    __shared__ uint32_t s_colw[NW], s_colc;
    uint32_t run_cnt = 0, run_bits = 8 * PXSZ, par = 0;
    // (x, y) of the lane's first pixel, advanced by PX pixels per iteration (the green add-back and the row starts of FOLD need it)
    uint32_t py = (4 * tid) / t.w, px = 4 * tid - py * t.w;
    const uint32_t dy = PX / t.w, dx = PX - dy * t.w;

    // ---- FOLD: column 0 into c0[0 .. h), then the symbol dwords and the head value of the first iteration
    const uint8_t *sy = FOLD ? asym + t.pbase : nullptr;               // sy[i - 1] = symbol of pixel i
    const uint32_t *sy4 = reinterpret_cast<const uint32_t *>(sy);
    uint8_t *c0 = alpha + t.pbase;
    uint32_t carryP = 0, carryH = 0, nx_cur = 0, nx_prev = 0, nx_A = 0;
    // head of a lane whose first pixel is (x, y) with tile index i: position hk inside the lane's four pixels and its row
    auto head_of = [&](uint32_t x, uint32_t y, uint32_t i, uint32_t &hk, uint32_t &hy) __attribute__((always_inline)) -> bool {
        hk = x == 0 ? 0u : t.w - x; hy = x == 0 ? y : y + 1;
        return (x == 0 || x + 4 > t.w) && i + hk < t.n;
    };
    if (FOLD) {
        const uint32_t a0 = ld32u(d.blob + 8) & 0xFF;  // first pixel's alpha: 4th byte of the first k word (MSB-first R,G,B,A)
        if (tid == 0) { s_colc = a0; c0[0] = (uint8_t)a0; }
        __syncthreads();
        for (uint32_t y0 = 1; y0 < t.h; y0 += THREADS) {
            const uint32_t y = y0 + tid;
            const uint32_t dv = y < t.h ? (uint32_t)zz_dec(sy[(uint64_t)y * t.w - 1]) & 255u : 0u;
            const uint32_t incl = wave_scan_incl(dv);
            if (lane == 63) s_colw[wv] = incl;
            __syncthreads();
            uint32_t base = s_colc;
            for (uint32_t w2 = 0; w2 < wv; w2++) base += s_colw[w2];
            if (y < t.h) c0[y] = (uint8_t)(base + incl);
            __syncthreads();
            if (tid == THREADS - 1) s_colc = (base + incl) & 255u;
            __syncthreads();
        }
        __threadfence_block();  // c0[] is read back below by other waves of this workgroup
        __syncthreads();
        if (4 * tid < t.n) {
            nx_cur = sy4[tid]; nx_prev = tid ? sy4[tid - 1] : 0u;
            uint32_t hk, hy;
            if (head_of(px, py, 4 * tid, hk, hy)) nx_A = c0[hy];
        }
    }

    uint32_t nx_a = 0;
    if (PXSZ == 4 && !FOLD && 4 * tid < t.n) nx_a = al[tid];
    for (uint32_t i0 = 0; i0 < t.n; i0 += PX, par ^= 1) {
        const uint32_t i = i0 + 4 * tid;
        uint32_t a4 = PXSZ == 4 ? nx_a : 0x01010101u;
        if (PXSZ == 4 && !FOLD) { const uint32_t in = i + PX; nx_a = 0; if (in < t.n) nx_a = al[in >> 2]; }
        if (FOLD) {
            const uint32_t cur = nx_cur, prev = nx_prev, A = nx_A;
            uint32_t hk, hy;
            const bool has_head = head_of(px, py, i, hk, hy);
            {   // the next iteration's symbol dwords and head value
                const uint32_t in = i + PX;
                uint32_t npx = px + dx, npy = py + dy;
                if (npx >= t.w) { npx -= t.w; npy++; }
                nx_cur = 0; nx_prev = 0; nx_A = 0;
                if (in < t.n) {
                    nx_cur = sy4[in >> 2]; nx_prev = sy4[(in >> 2) - 1];
                    uint32_t nhk, nhy;
                    if (head_of(npx, npy, in, nhk, nhy)) nx_A = c0[nhy];
                }
            }
            // deltas of pixels i .. i+3 (symbol of pixel i sits at sy[i-1]); a head and the pixels past the tile add nothing to P
            const uint32_t u = __builtin_amdgcn_alignbyte(cur, prev, 3);
            uint32_t d4 = ((u >> 1) & 0x7F7F7F7Fu) ^ ((u & 0x01010101u) * 255u);
            if (i >= t.n) d4 = 0;
            else if (t.n - i < 4) d4 &= 0xFFFFFFFFu >> (8 * (4 - (t.n - i)));
            if (has_head) d4 &= ~(0xFFu << (8 * hk));
            const uint32_t p0 = d4 & 255u, p1 = p0 + ((d4 >> 8) & 255u), p2 = p1 + ((d4 >> 16) & 255u), p3 = p2 + (d4 >> 24);
            const uint32_t incl = wave_scan_incl(p3);
            const uint32_t pb_ = incl - p3;  // wave-local P in front of this lane's first pixel
            const uint32_t pbefore = hk == 0 ? 0u : (hk == 1 ? p0 : (hk == 2 ? p1 : p2));  // the lane's deltas in front of its head
            const uint32_t Hown = (A - (pb_ + pbefore)) & 255u;
            const uint32_t M = wave_scan_max(has_head ? ((lane + 1u) << 8) | Hown : 0u);
            const uint32_t Mex = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)M, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);  // latest head in the lanes below
            if (lane == 63) s_wa[par][wv] = (incl & 255u) | ((M & 255u) << 8) | (M ? 1u << 16 : 0u);
            __syncthreads();
            uint32_t B = carryP, H = carryH, Cin = 0;
            for (uint32_t w2 = 0; w2 < NW; w2++) {
                const uint32_t e = s_wa[par][w2];
                if (w2 == wv) Cin = B + H;            // no head in this wave before the pixel: P and H both come from outside
                if (e >> 16) H = ((e >> 8) & 255u) - B;  // (a wave publishes H relative to its own P: B, the P in front of it, cancels inside the wave)
                B += e & 255u;
            }
            carryP = B & 255u; carryH = H & 255u;
            const uint32_t before = Mex ? Mex & 255u : Cin;  // H for the pixels in front of this lane's own head (or all four)
            const uint32_t pk[4] = {p0, p1, p2, p3};
            a4 = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t off = (has_head && (uint32_t)k >= hk) ? Hown : before;
                a4 |= ((pb_ + pk[k] + off) & 255u) << (8 * k);
            }
        }
        if (i >= t.n) a4 = 0;
        else if (t.n - i < 4) a4 &= 0xFFFFFFFFu >> (8 * (4 - (t.n - i)));  // pixels past the tile
        if (i == 0) a4 &= 0xFFFFFF00u;                                      // the first pixel is not coded
        bool coded[4];
        uint32_t cnt = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { coded[k] = ((a4 >> (8 * k)) & 255u) != 0; cnt += coded[k]; }
        const uint32_t cincl = wave_scan_incl(cnt);
        if (lane == 63) s_wc[par][wv] = cincl;
        __syncthreads();
        uint32_t cbase = run_cnt, ctot = 0;
        for (uint32_t w2 = 0; w2 < NW; w2++) { const uint32_t v = s_wc[par][w2]; if (w2 < wv) cbase += v; ctot += v; }
        // the lane's nl symbols: cnt consecutive bytes of the nl sequence
        uint32_t u = 0;
        if (cnt) {
            const uint32_t s0 = cbase + cincl - cnt;
            const uint32_t lo = nls[s0 >> 2], hi = nls[(s0 >> 2) + 1];
            u = __builtin_amdgcn_alignbyte(hi, lo, s0 & 3);
        }
        uint32_t nl[4], len[4], lane_len = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            nl[k] = coded[k] ? min(u & 255u, 8u) : 0u;
            u = coded[k] ? u >> 8 : u;
            len[k] = 3 * nl[k];
            lane_len += len[k];
        }
        const uint32_t bincl = wave_scan_incl(lane_len);
        if (lane == 63) s_wb[par][wv] = bincl;
        __syncthreads();
        uint32_t bbase = run_bits, btot = 0;
        for (uint32_t w2 = 0; w2 < NW; w2++) { const uint32_t v = s_wb[par][w2]; if (w2 < wv) bbase += v; btot += v; }
        if (i < t.n) {
            // bits [eb - lane_len, eb) of k, right-aligned in s2:s1:s0 (<= 96 bits): the four k words that end at bit eb
            uint32_t s0 = 0, s1 = 0, s2 = 0;
            if (lane_len) {
                const uint32_t eb = bbase + bincl;
                const int32_t we = (int32_t)((eb - 1) >> 5);
                uint32_t A[5];
#pragma unroll
                for (int k = 0; k < 5; k++) {  // aligned dwords we-3 .. we+1 of the (possibly misaligned) word array
                    const int32_t q = we - 3 + k;
                    A[k] = (q >= 0 && (uint32_t)q < kwords) ? kal[q] : 0u;
                }
                uint32_t Bw[4];
#pragma unroll
                for (int k = 0; k < 4; k++) Bw[k] = __builtin_amdgcn_alignbyte(A[k + 1], A[k], kmis);
                const uint32_t r = (0u - eb) & 31u;  // bits of the last word behind the lane's string
                s0 = __builtin_amdgcn_alignbit(Bw[2], Bw[3], r);
                s1 = __builtin_amdgcn_alignbit(Bw[1], Bw[2], r);
                s2 = __builtin_amdgcn_alignbit(Bw[0], Bw[1], r);
            }
            uint32_t word[4];
#pragma unroll
            for (int k = 3; k >= 0; k--) {  // last pixel first: its bits are the lowest
                const uint32_t v = __builtin_amdgcn_ubfe(s0, 0, len[k]);
                s0 = __builtin_amdgcn_alignbit(s1, s0, len[k]);
                s1 = __builtin_amdgcn_alignbit(s2, s1, len[k]);
                s2 >>= len[k];
                const uint32_t mk = (1u << nl[k]) - 1;
                int dr = zz_dec((int)(v >> (2 * nl[k]))), dg = zz_dec((int)((v >> nl[k]) & mk)), db = zz_dec((int)(v & mk));
                if (useG) {  // green add-back everywhere but row 0 / column 0 (libxpng.c:813)
                    uint32_t x = px + k, y = py;
                    if (x >= t.w) { x -= t.w; y++; }
                    if (x > 0 && y > 0) { dr += dg; db += dg; }
                }
                // top byte: "coded" marker = the pixel's alpha for RGBA (non-zero exactly when coded), 1 for RGB
                const uint32_t w = ((uint32_t)dr & 255u) | (((uint32_t)dg & 255u) << 8) | (((uint32_t)db & 255u) << 16) | (((a4 >> (8 * k)) & 255u) << 24);
                word[k] = coded[k] ? w : 0u;
            }
            *reinterpret_cast<u32x4_t *>(rs + i) = u32x4_t{word[0], word[1], word[2], word[3]};
        }
        run_cnt += ctot; run_bits += btot;
        px += dx; py += dy;
        if (px >= t.w) { px -= t.w; py++; }
    }
}

// --------------------------------------------------------------------------------------------------
// The serial size walk of the reference decoder (libxpng.c:982: t[i].f = r.p + x; x += low24(first u32)) for a caller whose
// blobs already live in HBM: one lane per image, cnt dependent loads.  The reference trusts the sizes; here a size that is
// zero or leaves the buffer parks every later tile at the end of the buffer, where k_dec_parse rejects it (avail < 4).
__global__ void k_dec_offsets(const uint8_t *const *__restrict__ blobs, const uint64_t *__restrict__ blob_len, uint32_t cnt,
                              uint32_t nimg, uint64_t *__restrict__ off) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nimg) return;
    const uint8_t *p = blobs[b];
    const uint64_t L = blob_len[b];
    uint64_t o = 0;
    for (uint32_t i = 0; i < cnt; i++) {
        off[(uint64_t)b * cnt + i] = o;
        const uint32_t sz = o + 4 <= L ? ld32u(p + o) & 0xFFFFFFu : 0u;
        o = sz ? (o + sz <= L ? o + sz : L) : L;
    }
}

// The same walk for a mixed-size batch (mixed.hpp), whose images have different tile counts: image b owns entries
// [first[b], first[b + 1]) of the M-entry concatenated table, and off[] is indexed by table entry.  The same truncation rule: a size
// that is zero or leaves the buffer parks every later tile of THAT image at the end of its buffer, where the parse rejects it.
__global__ void k_dec_offsets_mixed(const uint8_t *const *__restrict__ blobs, const uint64_t *__restrict__ blob_len,
                                    const uint32_t *__restrict__ first, uint32_t nimg, uint64_t *__restrict__ off) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nimg) return;
    const uint8_t *p = blobs[b];
    const uint64_t L = blob_len[b];
    const uint32_t i1 = first[b + 1];
    uint64_t o = 0;
    for (uint32_t i = first[b]; i < i1; i++) {
        off[i] = o;
        const uint32_t sz = o + 4 <= L ? ld32u(p + o) & 0xFFFFFFu : 0u;
        o = sz ? (o + sz <= L ? o + sz : L) : L;
    }
}

// One decode job: what a launch sequence decodes, from where, to where.  Filled by dec_launch (xpng_hip.hip), read by
// decode_m1_launch and decode_m2_launch.
struct DecodeJob {
    // geometry: B images of n_tiles tiles, `plane` bytes per symbol plane of the batch, rasters W pixels wide; the widest, tallest
    // and narrowest tile of the selection
    uint32_t B; uint64_t n_tiles, plane, W; uint32_t max_w, max_h, min_w; int pxsz;
    // selection: tiles [t0, t1) of every image, enumerated by `order` or image-major (order == nullptr); or, for a region decode,
    // the list_n work items of `list` (TileSel::list; t0, t1 = 0, n_tiles; no order)
    uint32_t t0, t1; const uint32_t *order; const uint32_t *list; uint32_t list_n;
    // device tables: tile table, B blob pointers and lengths, B raster pointers, status word; tile_off is a HOST array of blob
    // offsets (image-major: B * (t1 - t0), or B * n_tiles for a list) or nullptr (walk the sizes on the device)
    const TileDesc *tiles; const uint8_t *const *blobs; const uint64_t *blob_len; uint8_t *const *rasters; uint32_t *status;
    const uint64_t *tile_off;
    hipStream_t s;
    uint64_t *stamps;  // phase stamps of the narrow chains (probe builds, XPNG_STAMPS) or nullptr
    // a mixed-size batch (mixed.hpp): B = 1 and n_tiles = M, the concatenated table; `list` holds all M entries.
    // img_first: device array of img_n + 1 table indices, image i owns [img_first[i], img_first[i + 1]) - the size walk follows it;
    // tile_off then holds M offsets.  bpr: row pitch of the rasters in bytes when it is not W * pxsz (0: it is)
    const uint32_t *img_first; uint32_t img_n; uint64_t bpr;
    uint64_t pitch() const { return bpr ? bpr : W * (uint64_t)pxsz; }
    uint32_t cnt() const { return list ? list_n : t1 - t0; }        // work items per image (list: in all)
    uint32_t total() const { return list ? list_n : B * (t1 - t0); }
    TileSel sel() const { return TileSel{t0, cnt(), (uint32_t)n_tiles, B, list ? nullptr : order, list}; }
};

// (re)allocate the per-tile tables, place the five planes in the arena and bring the tile offsets to the device
inline int decode_ws_prepare(DecodeWs &ws, WsTable &tab, const DecodeJob &j, std::string &err) {
    auto bad = [&](const char *m) { err = m; return 1; };
    const uint64_t vn = (uint64_t)j.B * j.n_tiles, plane = j.plane;
    const uint32_t total = j.list ? (uint32_t)vn : j.total();  // offsets to bring
    if (ws.cap_tiles < vn || ws.cap_plane < plane) {
        for (void **q : {(void **)&ws.d_info, (void **)&ws.d_off, (void **)&ws.d_wdec, (void **)&ws.d_dtab}) tab.drop(q);
        ws.cap_tiles = ws.cap_plane = 0;
        ws.last_off.clear();
        // (the context symbol area carries one largest tile of slack: a corrupt payload can make the walk pop one queue for all
        //  of a tile's steps, i.e. read up to a tile's pixel count past that queue's start)
        const uint64_t sz[5] = {rup(plane + 8192 + 450000, 256), rup(plane + 64, 256), rup(plane + 64, 256), rup(plane + 64, 256), rup(4 * plane + 1024, 256)};
        // (an allocation of their own as a fallback for the planes existed behind a probe switch; the context's arena always has the room, so it could never run)
        if (!ws.arena || ws.arena_bytes < sz[0] + sz[1] + sz[2] + sz[3] + sz[4] + 256) return bad("internal error: the decode arena is too small for the symbol planes of this batch");
        uint8_t *pl[5], *q = reinterpret_cast<uint8_t *>(rup(reinterpret_cast<uintptr_t>(ws.arena), 256));
        for (int i = 0; i < 5; i++) { pl[i] = q; q += sz[i]; }
        ws.d_ctxsym = pl[0]; ws.d_asym = pl[1]; ws.d_alpha = pl[2]; ws.d_nlseq = pl[3];
        ws.d_resid = reinterpret_cast<uint32_t *>(pl[4]) + 16;
        if (tab.get((void **)&ws.d_info, vn * sizeof(DecTile)) != hipSuccess || tab.get((void **)&ws.d_off, vn * 8) != hipSuccess ||
            tab.get((void **)&ws.d_wdec, vn * 10 * sizeof(WDec)) != hipSuccess ||
            tab.get((void **)&ws.d_dtab, vn * 10 * WD_TAB_MAX) != hipSuccess)
            return bad("hipMalloc failed (decode workspace)");
        ws.cap_tiles = vn; ws.cap_plane = plane;
    }
    if (!j.tile_off) {
        if (!j.blobs || !j.blob_len) return bad("device-side size walk needs the blob tables");
        if (j.img_first) k_dec_offsets_mixed<<<(j.img_n + 63) / 64, 64, 0, j.s>>>(j.blobs, j.blob_len, j.img_first, j.img_n, ws.d_off);
        else k_dec_offsets<<<(j.B + 63) / 64, 64, 0, j.s>>>(j.blobs, j.blob_len, total / j.B, j.B, ws.d_off);
        ws.last_off.clear();
        return 0;
    }
    if (ws.last_off.size() != total || ws.last_t0 != j.t0 || memcmp(ws.last_off.data(), j.tile_off, (size_t)total * 8) != 0) {
        // pageable host memory: the copy is staged synchronously, so only pay for it when the offsets changed
        if (hipMemcpyAsync(ws.d_off, j.tile_off, (uint64_t)total * 8, hipMemcpyHostToDevice, j.s) != hipSuccess) return bad("tile offset upload failed");
        if (hipStreamSynchronize(j.s) != hipSuccess) return bad("tile offset upload failed");
        ws.last_off.assign(j.tile_off, j.tile_off + total);
        ws.last_t0 = j.t0;
    }
    return 0;
}

constexpr uint32_t WD_CTX_STREAMS = 32, WD_ALPHA_STREAMS = 32;  // streams per chain wavefront (16 alpha streams per wave - half the LDS per workgroup, twice the waves - measures the same)
static_assert(WD_ALPHA_STREAMS == 32, "k_dec_serial's alpha role is written for 32 streams per wavefront");

// What decode_m1_launch decides before its first kernel.
struct DecodePlan {
    // Many tiles in flight: instruction issue is the bound, so the rANS chains run 32 streams to a wave (rans2_wide_dec.hpp);
    // few tiles: latency is the bound and a wave per stream (scalar cursors, hot-symbol registers) is quicker.
    bool wide;
    // RGBA: the residual kernel rebuilds alpha from its symbols itself (k_dec_resid FOLD) when every tile is at least 4 pixels wide -
    // every tile of a file the reference can write (RGBA narrower than 4 px is stored at level 7); otherwise k_dec_alpha makes the plane
    bool fold;
    uint32_t pk0;  // work items from pk0 on go to the lane-per-tile walk: their context queues are packed (rans_dec.hpp); 0 = all of them (the wide form), `total` = none
    ReconPlan recon;  // the form of the reconstruction (recon.hpp)
    // probe builds: bytes of unused dynamic LDS per workgroup (occupancy throttles); all 0 in the release library
    size_t pad_chain, pad_alpha, pad_walk, pad_resid;
};
inline DecodePlan decode_m1_plan(const DecodeJob &j) {
    DecodePlan p{};
    const uint32_t total = j.total(), spt = j.pxsz == 4 ? 10 : 9;
    p.wide = wide_form((uint64_t)total * spt);
    p.fold = j.pxsz == 4 && j.min_w >= 4 && !probe_env("XPNG_NO_ALPHA_FOLD");
    p.recon = recon_geometry(j.max_w, j.max_h, p.wide);
    p.pk0 = p.wide && !probe_env("XPNG_NARROW_WALK") ? 0 : total;
    p.pad_chain = probe_pad("XPNG_PAD_CHAIN"); p.pad_alpha = probe_pad("XPNG_PAD_AL"); p.pad_walk = probe_pad("XPNG_PAD_WALK");
    p.pad_resid = probe_pad("XPNG_PAD_RS");
    return p;
}

// The tail of a decode: residual extraction, then reconstruction, of all `n` work items on stream st (knock-out names of probe
// builds: resid_big, recon_big).
template <int PXSZ>
inline void dec_tail(const DecodeWs &ws, const DecodeJob &j, const DecodePlan &p, const TileSel &sel, uint32_t n, hipStream_t st) {
    if (dbg_skip("resid_big")) {}
    else if constexpr (PXSZ == 4) {
        if (p.wide && p.fold) k_dec_resid<4, 256, true><<<n, 256, p.pad_resid, st>>>(ws.d_info, j.tiles, sel, ws.d_alpha, ws.d_asym, ws.d_nlseq, ws.d_resid, 0);
        else if (p.wide) k_dec_resid<4, 256><<<n, 256, p.pad_resid, st>>>(ws.d_info, j.tiles, sel, ws.d_alpha, ws.d_asym, ws.d_nlseq, ws.d_resid, 0);
        else if (p.fold) k_dec_resid<4, 1024, true><<<n, 1024, 0, st>>>(ws.d_info, j.tiles, sel, ws.d_alpha, ws.d_asym, ws.d_nlseq, ws.d_resid, 0);
        else k_dec_resid<4, 1024><<<n, 1024, 0, st>>>(ws.d_info, j.tiles, sel, ws.d_alpha, ws.d_asym, ws.d_nlseq, ws.d_resid, 0);
    } else {  // (RGB has no alpha to fold)
        if (p.wide) k_dec_resid<3, 256><<<n, 256, p.pad_resid, st>>>(ws.d_info, j.tiles, sel, ws.d_alpha, ws.d_asym, ws.d_nlseq, ws.d_resid, 0);
        else k_dec_resid<3, 1024><<<n, 1024, 0, st>>>(ws.d_info, j.tiles, sel, ws.d_alpha, ws.d_asym, ws.d_nlseq, ws.d_resid, 0);
    }
    if (!dbg_skip("recon_big")) recon_launch<PXSZ>(p.recon, ws.d_info, j.tiles, sel, ws.d_resid, j.rasters, j.pitch(), 0, n, st);
}

// Launch the whole level-1 decode of a job.
inline int decode_m1_launch(DecodeWs &ws, WsTable &tab, const DecodeJob &j, std::string &err) {
    auto bad = [&](const char *m) { err = m; return 1; };
    const DecodePlan p = decode_m1_plan(j);
    const TileSel sel = j.sel();
    const uint32_t cnt = j.cnt(), total = j.total(), spt = j.pxsz == 4 ? 10 : 9;
    const hipStream_t s = j.s;
    const bool rgba = j.pxsz == 4;
    const auto tail = rgba ? &dec_tail<4> : &dec_tail<3>;
    dbg_count_sequence();
    if (decode_ws_prepare(ws, tab, j, err)) return 1;
    // (a null workspace pointer handed to a kernel is a GPU fault, i.e. abort(): refuse to launch instead)
    if (!ws.d_info || !ws.d_off || !ws.d_wdec || !ws.d_dtab || !ws.d_ctxsym || !ws.d_asym || !ws.d_alpha || !ws.d_nlseq || !ws.d_resid || !j.tiles || !j.blobs || !j.rasters)
        return bad("internal error: a decode workspace buffer was never allocated");

    k_dec_parse<<<(total + 63) / 64, 64, 0, s>>>(j.blobs, ws.d_off, j.blob_len, cnt, total, spt, j.pxsz, j.tiles, sel, ws.d_info, j.status);

    if (p.wide) {
        // ---- the wide form: every kernel on the caller's stream, no fork, no event.  The serial stages that need nothing of each other
        // - the alpha chains and the context walk - are two ranges of ONE grid (k_dec_serial) behind the context chains: a hardware queue
        // is held for the longer of the two, not two queues for their sum, and no barrier packet stands in a queue that other contexts'
        // streams share (the runtime gives a process 4 queues unless it asked for more before HIP started: DESIGN.md 6.2).  (Through round
        // 4: the alpha chains on a side stream beside the context chains, and two tile size classes walked, extracted and reconstructed
        // side by side on the two streams.)
        const uint32_t groups = (total + WD_CTX_STREAMS - 1) / WD_CTX_STREAMS;
        if (!dbg_skip("dec_prep")) k_rans2_dec_prep<<<total * spt, 64, 0, s>>>(ws.d_info, j.tiles, sel, spt, ws.d_ctxsym, ws.d_asym, ws.d_wdec, ws.d_dtab, p.pk0);
        if (!dbg_skip("dec_chain_c")) k_rans2_dec_chain<false, WD_CTX_STREAMS, false><<<groups * 9, 64, DecChainLds<false, WD_CTX_STREAMS>::BYTES + p.pad_chain, s>>>(ws.d_info, total, 0, 9, ws.d_wdec, ws.d_dtab, ws.d_ctxsym, ws.d_asym, p.pk0);
        // context streams the small layout cannot hold (PROB_BITS > 12 or more than 16 symbols: never written by the reference)
        if (!dbg_skip("dec_odd")) k_rans2_decode_rest<15><<<128, 64, 0, s>>>(ws.d_info, j.tiles, sel, total, 0, 9, ws.d_ctxsym, ws.d_asym, j.stamps, ws.d_wdec, p.pk0);
        // (k_rans2_decode_rest resolves slots by binary search: 4.6 KB of LDS, so its 128 workgroups are placed at once - with the
        //  37 KB slot table of k_rans2_decode<15> they waited up to 5 ms, between the chains and the walk, to find nothing to do)
        // (probe builds: XPNG_NARROW_ALPHA / XPNG_NARROW_WALK run that stage in its one-wavefront-per-stream / per-tile form, a launch of
        //  its own; a knocked-out role gets no workgroups, and a launch without workgroups is not made)
        uint32_t agroups = rgba && !dbg_skip("dec_chain_a") ? (total + WD_ALPHA_STREAMS - 1) / WD_ALPHA_STREAMS : 0;
        uint32_t wgroups = dbg_skip("walk_small") ? 0 : (total + 63) / 64;  // (the lane-per-tile walk keeps its name; walk_big, resid_small and recon_small name nothing any more)
        if (rgba && probe_env("XPNG_NARROW_ALPHA")) { agroups = 0; k_rans2_decode<15><<<total, 64, 0, s>>>(ws.d_info, j.tiles, sel, 9, 1, 0, ws.d_ctxsym, ws.d_asym, j.stamps); }
        if (probe_env("XPNG_NARROW_WALK")) { wgroups = 0; k_dec_walk<<<total, 64, 0, s>>>(ws.d_info, j.tiles, sel, ws.d_ctxsym, ws.d_nlseq); }
        if (agroups + wgroups)
            k_dec_serial<<<agroups + wgroups, 64, dec_serial_lds_bytes(agroups, wgroups) + p.pad_chain + p.pad_walk, s>>>(ws.d_info, j.tiles, sel, total, ws.d_wdec, ws.d_dtab, ws.d_ctxsym, ws.d_asym, ws.d_nlseq, agroups);
        if (rgba && !p.fold && !dbg_skip("dec_alpha")) k_dec_alpha<256><<<total, 256, p.pad_alpha, s>>>(ws.d_info, j.tiles, sel, ws.d_asym, ws.d_alpha);
        tail(ws, j, p, sel, total, s);
    } else {
        // ---- the narrow form: a wavefront per stream.  The alpha branch runs on the side stream: its rANS block is the longest serial
        // chain of a tile, and it is independent of the nl-context branch (nine short rANS blocks, then the serial context walk) until
        // k_dec_resid
        const hipStream_t side = ws.side;
        if (rgba) {
            if (!side) return bad("internal error: the decode has no side stream");
            if (!decode_ws_event(ws.ev_fork) || !decode_ws_event(ws.ev_join)) return bad("event creation failed");
            if (hipEventRecord(ws.ev_fork, s) != hipSuccess || hipStreamWaitEvent(side, ws.ev_fork, 0) != hipSuccess) return bad("fork failed");
            k_rans2_decode<15><<<total, 64, 0, side>>>(ws.d_info, j.tiles, sel, 9, 1, 0, ws.d_ctxsym, ws.d_asym, j.stamps);
            if (!p.fold && !dbg_skip("dec_alpha")) k_dec_alpha<1024><<<total, 1024, 0, side>>>(ws.d_info, j.tiles, sel, ws.d_asym, ws.d_alpha);
            if (hipEventRecord(ws.ev_join, side) != hipSuccess) return bad("join record failed");
        }
        k_rans2_decode<12><<<total * 9, 64, 0, s>>>(ws.d_info, j.tiles, sel, 0, 9, 0, ws.d_ctxsym, ws.d_asym, j.stamps);
        k_rans2_decode<15><<<total * 9, 64, 0, s>>>(ws.d_info, j.tiles, sel, 0, 9, 1, ws.d_ctxsym, ws.d_asym, j.stamps);  // blocks with PROB_BITS > 12 only
        k_dec_walk<<<total, 64, 0, s>>>(ws.d_info, j.tiles, sel, ws.d_ctxsym, ws.d_nlseq);
        if (rgba && s != side && hipStreamWaitEvent(s, ws.ev_join, 0) != hipSuccess) return bad("join failed");
        tail(ws, j, p, sel, total, s);
    }
    if (hipGetLastError() != hipSuccess) return bad("decode kernel launch failed");
    return 0;
}

}  // namespace xpng
