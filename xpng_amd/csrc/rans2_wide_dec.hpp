// "Wide" rANS v2 block decode (decompress_block_v2, libxpng.c:429-493) for large batches of tiles.
//
// k_rans2_decode (m1_decode.hpp) gives a whole wavefront to one stream: 2 useful lanes.  With thousands of tiles in
// flight the machine is bound by instruction issue, so here the lanes are filled instead:
//
//   k_rans2_dec_prep   one wave per (tile, stream): block types 0/1/2 are finished on the spot; for rANS blocks the
//                      frequency table is parsed and the decode tables ((F | cum << 16)[256], coarse slot -> symbol
//                      [256]) are left in HBM together with a small descriptor
//   k_rans2_dec_chain  one wave = the SAME stream class (context c, or alpha) of 32 tiles: lanes 2k / 2k+1 carry the
//                      two interleaved states of tile k.  Chains of one class have similar lengths, so the wave's
//                      trip count (its longest chain) wastes little.
//
// The chain loop touches global memory only at block boundaries (every 8 steps): renormalisation words are staged
// through a 64-word LDS ring per stream, refilled by loads that are issued at one boundary and landed at the next
// (so no s_waitcnt for global memory sits inside the 8 steps), and decoded symbols leave as one aligned 16-byte
// store per stream and block - or, for the context streams of a work item that the lane-per-tile walk will read (from the launch
// argument pk0 on), two symbols to a byte (rans_dec.hpp: ctxn_*) as one aligned 8-byte store: a lane gathers its eight symbols of a
// block in two registers, one shift-or per step instead of an LDS byte store, and the pair merges them at the boundary with one
// cross-lane move per dword.  k_rans2_dec_prep packs the blocks it finishes itself (types 1 and 2) the same way.
#pragma once
#include "common.hpp"
#include "rans_dec.hpp"

#include <type_traits>
namespace xpng {

__global__ __launch_bounds__(64) void k_rans2_dec_prep(const DecTile *__restrict__ info, const TileDesc *__restrict__ tiles,
                                                       TileSel sel, uint32_t spt, uint8_t *__restrict__ ctxsym,
                                                       uint8_t *__restrict__ asym, WDec *__restrict__ wdec,
                                                       uint8_t *__restrict__ dtab, uint32_t pk0) {
    bw_prio();
    __shared__ uint32_t fc[256];
    __shared__ uint32_t Fs[260];
    const uint32_t j = blockIdx.x / spt, c = blockIdx.x % spt, lane = threadIdx.x & 63;
    WDec *wd = wdec + (uint64_t)j * 10 + c;
    const DecTile d = info[j];
    if (lane == 0) wd->kind = 0;
    if (d.type == 0 || d.type == TILE_BAD) return;
    const TileDesc t = tiles[vtile(sel, j)];
    const uint8_t *in = d.blob + d.blk_off[c];
    const uint64_t out_off = c < 9 ? t.pbase + d.ctx_start[c] : t.pbase;
    uint8_t *out = (c < 9 ? ctxsym : asym) + out_off;
    const uint32_t h0 = sgpr(ld32u(in)), type = h0 >> 24;
    if (type == 0) return;
    const uint32_t csz = h0 & 0xFFFFFF;
    const uint8_t *end = in + csz;
    const uint32_t h1 = sgpr(ld32u(in + 4)), n = h1 & 0xFFFFFF, v2 = h1 >> 24;
    if (rans2_dec_plain(type, in, end, n, v2, out, c < 9 && j >= pk0)) return;  // (work items from pk0 on: packed context queues, rans_dec.hpp)
    const uint32_t N = v2 + 2;
    const uint32_t h2 = sgpr(ld32u(in + 8));
    const uint32_t pb = h2 >> 24;  // 10..15, checked by k_dec_parse
    const uint8_t *words = in + 12;
    const uint8_t *table = in + 8 + 4ull * (h2 & 0xFFFFFF);
    rans2_dec_freqs(type, pb, N, table, end, Fs);
    __syncthreads();
    const uint2 hot = rans_dec_cum([&](uint32_t i) { return Fs[i]; }, N, fc);  // (F << 8 | sym) of the two most probable symbols
    __syncthreads();
    uint8_t *gt = dtab + ((uint64_t)j * 10 + c) * WD_TAB_MAX;
    const bool small = c < 9 && pb <= 12 && N <= WdLayout<false>::REGN;
    // Alpha layout: the coarse bytes are indexed by the slot's COLD RANK (its position among the slots that belong to neither of
    // the two hot symbols, which the chain resolves in registers).  A skewed alphabet squeezes its two hundred rare symbols into
    // a few hundred slots: in slot space a 64-slot bucket of that region holds dozens of symbol boundaries, in rank space the
    // whole region usually fits the 512 entries one slot apiece (rsh = 0) and the lookup is exact.
    uint32_t rsh = 0, Ca = 0, Fa = 0, Cb = 0, Fb = 0;
    if (!small) {
        const uint32_t e0 = fc[hot.x & 255u], e1 = fc[hot.y & 255u];
        Ca = e0 >> 16; Fa = e0 & 0xFFFFu;
        if ((hot.y & 255u) != (hot.x & 255u)) { Cb = e1 >> 16; Fb = e1 & 0xFFFFu; }
        if (Fb && Cb < Ca) { const uint32_t tc = Ca, tf = Fa; Ca = Cb; Fa = Fb; Cb = tc; Fb = tf; }  // a = the lower one
        const uint32_t cold = (1u << pb) - Fa - Fb;
        while ((cold >> rsh) > (1u << WdLayoutA::CBITS)) rsh++;
    }
    // coarse (slot or cold rank) -> symbol; rank -> slot: step over the hot ranges
    wd_store_tables<WdLayoutA>(gt, small, fc, N, pb, small ? pb - WdLayout<false>::CBITS : rsh, [&](uint32_t s) {
        if (small) return s;
        if (s >= Ca) s += Fa;
        if (Fb && s >= Cb) s += Fb;
        return s < (1u << pb) ? s : (1u << pb) - 1;
    });
    const uint8_t *sp = table - 16;  // state0 at table-16, state1 at table-8
    if (lane == 0) {
        WDec w;
        w.kind = small ? 1u : 2u; w.pb = pb; w.N = N; w.n = n;
        w.nw = (uint32_t)((sp - words) >> 2);
        w.words_off = d.blk_off[c] + 12;
        w.out_off = out_off;
        w.hot0 = hot.x & 255u; w.hot1 = hot.y & 255u;
        w.rsh = rsh;
        *wd = w;
    }
}

// dynamic LDS of one launch: the small layout is searched in registers, so only its fc[] dwords come in (the coarse bytes stay in
// HBM): LDS per wave is what limits how many chains of a pipelined batch are resident at once
template <bool BIG, int STREAMS>
using DecChainLds = WdChainLds<typename std::conditional<BIG, WdLayoutA, WdLayout<false>>::type, BIG ? WdLayoutA::TAB : WdLayout<false>::CO_OFF, STREAMS, 1>;
static_assert(DecChainLds<false, 32>::BYTES == 7728 && DecChainLds<true, 32>::BYTES == 42544, "LDS per wave of the v2 chains");

// Per decode step and lane (fast path, every lane active): slot -> coarse byte -> (F | cum << 16) are two dependent LDS reads; the
// state update is one 64x32 multiply-add built from v_mad_u64_u32 + v_mad_u32_u24 (the high half of s >> pb is < 2^21,
// F < 2^16); the pair's word cursor is an LDS address that wraps inside a 256-byte aligned ring by a bit-field insert,
// and both candidate words come back with one ds_read2 (a mirror dword in front of the ring covers the wrap).
// STREAMS per wave (2 lanes each; further lanes idle).  HOT: the (F, cum) of the two most probable symbols live in registers
// and a step in which EVERY lane of the wave lands in one of them skips both table reads (which is most steps when the
// streams are skewed and the wave carries few of them: alpha runs 8 streams per wave for that reason, trading lanes for
// latency on the longest chain of the decode).
// (A device function of the role-local workgroup index `bid`: k_rans2_dec_chain launches one class; the alpha class of a batched
//  decode is a range of k_dec_serial's grid, m1_decode.hpp.)
template <bool BIG, int STREAMS, bool HOT>
__device__ __attribute__((always_inline)) inline void rans2_dec_chain_body(const DecTile *__restrict__ info, uint32_t total, uint32_t c_first,
                                                        uint32_t c_count, const WDec *__restrict__ wdec,
                                                        const uint8_t *__restrict__ dtab, uint8_t *__restrict__ ctxsym,
                                                        uint8_t *__restrict__ asym, uint32_t pk0, const uint32_t bid) {
    __builtin_amdgcn_s_setprio(XPNG_CHAIN_PRIO);  // a serial chain: its latency is the critical path, the throughput kernels beside it are not
    XPNG_PROBE_BEGIN()
    typedef typename std::conditional<BIG, WdLayoutA, WdLayout<false>>::type L;
    typedef DecChainLds<BIG, STREAMS> LD;
    constexpr uint32_t CBITS = L::CBITS, WD_RING = L::RING, KIND = L::KIND, WD_STREAMS = STREAMS;
    constexpr uint32_t LTAB = LD::LTAB, TSTRIDE = LD::TSTRIDE;
    constexpr uint32_t PER = WD_RING / 8;      // words one lane requests per boundary (the pair: a quarter of the ring)
    constexpr uint32_t RSTRIDE = LD::RSTRIDE;  // per stream: [mirror of the last ring word][WD_RING words]
    extern __shared__ __align__(32) uint8_t dec_chain_lds[];
    uint8_t *const ltab = dec_chain_lds;                 // [WD_STREAMS * TSTRIDE]
    uint8_t *const ring = dec_chain_lds + LD::OFF_RING;  // [WD_STREAMS * RSTRIDE]
    uint8_t *const obuf = dec_chain_lds + LD::OFF_OBUF;  // [(WD_STREAMS + 1) * OB_STRIDE] per stream: 16 symbol bytes of the block + a dump byte nobody reads; the last slot belongs to the lanes without a stream (STREAMS < 32)
    const uint32_t lane = threadIdx.x & 63, kraw = lane >> 1, k = kraw < WD_STREAMS ? kraw : 0, par = lane & 1;  // (idle lanes alias stream 0's LDS harmlessly)
    const uint32_t c = c_first + bid % c_count, grp = bid / c_count;
    const uint32_t j = grp * WD_STREAMS + kraw;
    bool live = kraw < WD_STREAMS && j < total;
    // context streams of packed work items (from pk0 on, a multiple of STREAMS: the whole wavefront or none of it) leave two symbols
    // to a byte (rans_dec.hpp: the layout): 8 bytes per block and stream, gathered in registers instead of the LDS staging bytes
    const bool packed = !BIG && sgpr(grp * WD_STREAMS) >= pk0;
    wd_load_tables<L, LTAB, WD_STREAMS>(ltab, grp * WD_STREAMS, total, wdec, dtab, 10, c);
    __syncthreads();
    const WDec *wd = wdec + (uint64_t)(live ? j : 0) * 10 + c;
    live = live && wd->kind == KIND;
    const uintptr_t words = live ? (uintptr_t)info[j].blob + wd->words_off : 0;
    const uintptr_t words_safe = live ? words : (uintptr_t)dtab;  // (idle lanes still issue the block loads: any readable address)
    uint8_t *out = (c < 9 ? ctxsym : asym) + (live ? wd->out_off : 0);
    const uint32_t n = live ? wd->n : 0, pb = live ? wd->pb : 12, nw = live ? wd->nw : 0;
    const uint32_t npairs = n >> 1, mask = (1u << pb) - 1;
    const uint32_t ident = 1u << pb;  // table entry (F = 2^pb, cum = 0): the step maps s to s, which is how an idle lane waits
    // LDS byte addresses
    const uint32_t a_fc = (uint32_t)(uintptr_t)(lds8 *)ltab + k * TSTRIDE, a_co = a_fc + L::CO_OFF;
    const uint32_t a_ring = (uint32_t)(uintptr_t)(lds8 *)ring + k * RSTRIDE + 4;  // word slot i at a_ring + 4 i, the mirror at a_ring - 4
    const uint32_t a_ob = (uint32_t)(uintptr_t)(lds8 *)obuf + (kraw < WD_STREAMS ? kraw : WD_STREAMS) * OB_STRIDE;
    auto ring_w = [&](uint32_t idx) __attribute__((always_inline)) -> lds32 * { return (lds32 *)(uintptr_t)(a_ring + 4 * (idx & (WD_RING - 1))); };
    // ---- initial ring contents: the top 64 words; the states sit right above the words
    uint32_t rw = nw;                               // next word to pop is words[rw - 1]
    uint32_t lo = nw > WD_RING ? nw - WD_RING : 0;  // lowest word index resident in the ring
#pragma unroll 4
    for (uint32_t q = 0; q < WD_RING / 2; q++) {
        const uint32_t a = lo + 2 * q + par;
        if (a < nw) *ring_w(a) = gld32u(words + 4ull * a);
    }
    *(lds32 *)(uintptr_t)(a_ring - 4) = *ring_w(WD_RING - 1);
    uint32_t slo = 0x80000000u, shi = 0;  // state = shi:slo
    if (live) { const uintptr_t sp = words + 4ull * nw + 8 * par; slo = gld32u(sp); shi = gld32u(sp + 4); }
    uint32_t lof = lo;                              // lowest word index resident or in flight
    uint32_t fa0 = 0, fhi = 0, fsh = 0;             // in-flight chunk: first word index, landing bound, byte misalignment
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    uint32_t qx = 0;
    uint32_t wi = (rw - 1) & (WD_RING - 1);         // ring slot of w1 = words[rw - 1]; w2 = words[rw - 2] sits 4 bytes below (mirror for slot 0)
    uint32_t w1, w2;
    auto fetch_w = [&]() __attribute__((always_inline)) {
        const lds32 *p = (const lds32 *)(uintptr_t)(a_ring - 4 + 4 * wi);
        w2 = p[0]; w1 = p[1];
    };
    fetch_w();
    uint32_t hs0 = 0, hs1 = 0, hC0 = 0, hF0 = 0x10000u, hC1 = 0, hF1 = 0;  // idle lanes: "always hit" (their step is the identity anyway)
    if (HOT && live) {
        hs0 = wd->hot0; hs1 = wd->hot1;
        if (BIG) {
            hC0 = *(const lds16 *)(uintptr_t)(a_fc + 2 * hs0); hF0 = *(const lds16 *)(uintptr_t)(a_fc + 2 * hs0 + 2) - hC0;
            hC1 = *(const lds16 *)(uintptr_t)(a_fc + 2 * hs1); hF1 = *(const lds16 *)(uintptr_t)(a_fc + 2 * hs1 + 2) - hC1;
        } else {
            const uint32_t e0 = *(const lds32 *)(uintptr_t)(a_fc + 4 * hs0), e1 = *(const lds32 *)(uintptr_t)(a_fc + 4 * hs1);
            hF0 = e0 & 0xFFFFu; hC0 = e0 >> 16; hF1 = e1 & 0xFFFFu; hC1 = e1 >> 16;
        }
    }
    // alpha layout: cold rank of a slot = slot minus the hot ranges below it; the coarse bytes are indexed by rank >> rsh
    const uint32_t rE0 = hC0 + hF0, rE1 = hC1 + hF1, rF1 = hs1 != hs0 ? hF1 : 0u;
    const uint32_t rsh = (BIG && live) ? wd->rsh : 0u;
    const bool exact = BIG && __ballot(rsh != 0) == 0;  // every stream of the wave resolves a cold slot with one table byte
    uint32_t cm[10];  // small layout (nl-context streams, at most 9 symbols): the cumulative counts c1..c9 of wd_reg9
    wd_cm_load<!BIG>(cm, live, wd, a_fc, pb);
    // one symbol out of this lane's state, the pair's renormalisation (state1 refills first, libxpng.c:486-487)
    uint32_t acc0 = 0, acc1 = 0;  // packed: this lane's symbols of pair steps 0..3 and 4..7 of the block, one to a byte
    auto step = [&](auto pk, bool act, uint32_t obpos, uint32_t u) __attribute__((always_inline)) -> uint32_t {
        const uint32_t slot = slo & mask;
        uint32_t sym, F, off;
        const uint32_t d0 = slot - hC0, d1 = slot - hC1;
        const bool h0 = d0 < hF0, h1 = d1 < hF1;
        if (HOT && __ballot(!(h0 || h1)) == 0) {
            sym = h0 ? hs0 : hs1; F = h0 ? hF0 : hF1; off = h0 ? d0 : d1;
        } else if (!BIG) {
            sym = wd_reg9(slot, cm[1], cm[2], cm[3], cm[4], cm[5], cm[6], cm[7], cm[8], cm[9], F, off);
        } else {
            // slot -> symbol without a data-dependent scan (a wave waits for its slowest lane, and a 64-slot bucket of a skewed
            // alphabet holds half a dozen narrow symbols: the serial scan cost 5-6 dependent LDS reads per cold step): the coarse
            // byte names the symbol owning the bucket's first slot, the next eight cumulative counts come in ONE 16-byte read
            // and are compared at once (packed 16-bit differences: cum is non-decreasing, so the count of "slot >= cum" is the
            // position of the first set sign bit); buckets with more than seven boundaries (rare) go round again
            typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));
            typedef uint32_t u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));
            typedef __attribute__((address_space(3))) u32x4_a2 lds128u;
            typedef uint32_t u32_a2 __attribute__((aligned(2)));
            typedef __attribute__((address_space(3))) u32_a2 lds32u;
            const uint32_t rank = slot - (slot >= rE0 ? hF0 : 0u) - (slot >= rE1 ? rF1 : 0u);
            const uint32_t ridx = rank >> rsh;
            sym = *(const lds8 *)(uintptr_t)(a_co + (ridx < (1u << CBITS) ? ridx : (1u << CBITS) - 1));
            const uint32_t slot2 = slot | (slot << 16);
            auto count8 = [&](uint32_t from) __attribute__((always_inline)) -> uint32_t {  // how many of cum[from + 1 .. from + 8] are <= slot
                const u32x4_a2 v = *(const lds128u *)(uintptr_t)(a_fc + 2 * from + 2);
                uint32_t m[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t vq = v[q];  // (by value: __builtin_bit_cast of the vector ELEMENT expression reads element 0)
                    const u16x2 d = __builtin_bit_cast(u16x2, slot2) - __builtin_bit_cast(u16x2, vq);
                    m[q] = __builtin_bit_cast(uint32_t, d) & 0x80008000u;  // the two sign bits
                }
                // sign bits (bit 15 / 31 of m[q]) -> bit 2q (low half: value 2q) and bit 16 + 2q (high half: value 2q + 1)
                uint32_t all = (m[0] >> 15) | (m[1] >> 13) | (m[2] >> 11) | (m[3] >> 9);
                all = (all | (all >> 15)) & 0xFFu;
                return (uint32_t)__builtin_ctz(all | 0x100u);
            };
            const bool hotlane = h0 || h1;     // (resolved in registers below: its table result is not used)
            uint32_t t = exact ? 0u : count8(sym);
            t = hotlane ? 0u : t;
            sym += t;
            if (!exact && __ballot(t == 8)) {  // (uniform) a bucket with more than seven boundaries: second round
                t = t == 8 ? count8(sym) : 0u;
                sym += t;
                if (__ballot(t == 8)) {        // still not there (dense alphabets, corrupt tables): plain scan, bounded by the sentinels
                    uint32_t c1 = *(const lds16 *)(uintptr_t)(a_fc + 2 * sym + 2);
                    while (slot >= c1 && sym < 255u) { sym++; c1 = *(const lds16 *)(uintptr_t)(a_fc + 2 * sym + 2); }
                }
            }
            sym = sym < 255u ? sym : 255u;
            const uint32_t cc = *(const lds32u *)(uintptr_t)(a_fc + 2 * sym);
            const uint32_t c0 = cc & 0xFFFFu, c1 = cc >> 16;
            F = c1 - c0; off = slot - c0;
            if (HOT) {  // lanes that landed in a hot symbol while another lane of the wave did not
                sym = h0 ? hs0 : (h1 ? hs1 : sym); F = h0 ? hF0 : (h1 ? hF1 : F); off = h0 ? d0 : (h1 ? d1 : off);
            }
        }
        if (!act) { F = ident; off = slot; }
        uint32_t nlo, nhi;
        const bool need = wd_advance(slo, shi, pb, F, off, nlo, nhi);
        const uint32_t needi = need ? 1u : 0u, other = swap_pair(needi);
        const uint32_t take = pick32(!par && other, w2, w1);
        shi = need ? nlo : nhi;
        slo = need ? take : nlo;
        const uint32_t cons = needi + other;
        wi = (wi - cons) & (WD_RING - 1);
        fetch_w();
        if constexpr (decltype(pk)::value) {  // (u is a constant of the unrolled block: one shift-or; an inactive step leaves its place alone)
            if (u < 4) acc0 = ctxn_gather(acc0, act ? sym : 0u, u); else acc1 = ctxn_gather(acc1, act ? sym : 0u, u);
        } else {
            *(lds8 *)(uintptr_t)(a_ob + (act ? obpos : 16u)) = (uint8_t)sym;
        }
        return sym;
    };
    if (n & 1) {  // odd tail comes from state0 only (libxpng.c:471-476)
        const uint32_t sym = step(std::false_type{}, par == 0, (n - 1) & 15u, 0);
        if (par == 0 && !packed) out[n - 1] = (uint8_t)sym;
        if (par == 0 && packed) {
            // a byte of its own (the nibble above it lies behind the stream's end), and its place in the stream's top block, whose
            // 8-byte store covers that byte - unless the pairs fill their blocks exactly: then the tail's block is never stored
            out[(n - 1) >> 1] = (uint8_t)sym;
            const uint32_t ut = npairs & 7u;
            if (ut) { if (ut < 4) acc0 = ctxn_gather(0u, sym, ut); else acc1 = ctxn_gather(0u, sym, ut); }
        }
    }
    // the wave's trip count, and the pairs every lane is inside its stream for (a lane without a chain steps on the identity entry
    // whatever the variant: it counts as 0xFFFFFFFF pairs, and the minimum is the complement's maximum)
    const uint32_t T = sgpr((wave_max(npairs) + 7) & ~7u), Tmin = sgpr(~wave_max(live ? ~npairs : 0u));
    // (nothing may be pending on vmcnt when the loop is entered: the compiler merges the counter state of the loop entry with
    //  that of the back edge conservatively, and a load still in flight from before the loop turns into a wait at the top of
    //  EVERY iteration - right behind the block loads the previous iteration has just issued)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    // the loop, once per output form (pk: packed); a wavefront runs one of them
    auto run = [&](auto pk) __attribute__((always_inline)) {
        for (uint32_t jb = T; jb > 0;) {
            jb -= 8;
            const uint32_t wi0 = wi;
            if (jb + 8 <= Tmin) {  // every lane of the wave is inside its stream
#pragma unroll
                for (int u = 7; u >= 0; u--) step(pk, true, 2 * (uint32_t)u + par, (uint32_t)u);
            } else {
#pragma unroll
                for (int u = 7; u >= 0; u--) step(pk, jb + (uint32_t)u < npairs, 2 * (uint32_t)u + par, (uint32_t)u);
            }
            rw -= (wi0 - wi) & (WD_RING - 1);  // words the pair consumed in this block (at most two per step)
            // ---- block boundary: in-flight words land, symbols out, next words requested
            // (landing first: its wait then covers only what the previous boundary issued, 8 steps ago, not this block's store)
            XPNG_PROBE_WAIT()
            XPNG_PROBE_ISSUE_BEGIN()
            wd_land<WD_RING>(a_ring, q0, q1, qx, fa0, fhi, fsh);  // (unconditional, like the request below: fhi == 0 when nothing was requested)
            *(lds32 *)(uintptr_t)(a_ring - 4) = *ring_w(WD_RING - 1);
            if constexpr (decltype(pk)::value) {
                // the pair's 16 symbols: one cross-lane move per dword, the odd lane's (state 1) symbols into the high nibbles.  A block
                // that is not stored (the stream has not begun: every step inactive) keeps its registers - they may hold the odd tail
                const bool st = jb < npairs;
                const uint32_t m0 = ctxn_merge(acc0, swap_pair(acc0)), m1 = ctxn_merge(acc1, swap_pair(acc1));
                if (st && par == 0) *reinterpret_cast<uint2 *>(out + jb) = make_uint2(m0, m1);
                acc0 = st ? 0u : acc0; acc1 = st ? 0u : acc1;
            } else {
                if (jb < npairs && par == 0) *reinterpret_cast<u32x4_t *>(out + 2ull * jb) = *(const lds128_al4 *)(uintptr_t)a_ob;
            }
            lo = lof;
            {
                int32_t want = (int32_t)lo - (int32_t)(2 * PER);
                const int32_t room = (int32_t)rw - (int32_t)WD_RING;
                want = want > room ? want : room;
                want = want > 0 ? want : 0;
                {   // The loads are issued on every boundary, from a clamped address when there is nothing to fetch (fhi = 0 then keeps
                    // the landing from writing): a branch around them makes the compiler load into temporaries and copy those into
                    // the loop-carried registers at once - a wait for loads it has just issued, once per block.
                    const bool any = (uint32_t)want < lo;
                    const uint32_t a0r = (uint32_t)want + PER * par;
                    const bool req = any && a0r < lo;
                    const uint32_t a0 = req ? a0r : 0u;
                    const uintptr_t A = words_safe + 4ull * a0;
                    const gptr32 p = (gptr32)(A & ~(uintptr_t)3);
                    const u32x4_a4 v0 = *(gptr128)p;
                    q0 = make_uint4(v0.x, v0.y, v0.z, v0.w);
                    if (PER > 4) { const u32x4_a4 v1 = *(gptr128)(p + 4); q1 = make_uint4(v1.x, v1.y, v1.z, v1.w); }
                    qx = p[PER];
                    fa0 = a0; fhi = req ? lo : 0u; fsh = (uint32_t)(A & 3);
                    lof = any ? (uint32_t)want : lof;
                }
            }
            XPNG_PROBE_ISSUE_END()
        }
    };
    if constexpr (BIG) run(std::false_type{});
    else if (packed) run(std::true_type{});
    else run(std::false_type{});
    XPNG_PROBE_END(BIG ? 4 : 3)
}
template <bool BIG, int STREAMS, bool HOT>
__global__ __launch_bounds__(64) void k_rans2_dec_chain(const DecTile *__restrict__ info, uint32_t total, uint32_t c_first,
                                                        uint32_t c_count, const WDec *__restrict__ wdec,
                                                        const uint8_t *__restrict__ dtab, uint8_t *__restrict__ ctxsym,
                                                        uint8_t *__restrict__ asym, uint32_t pk0) {
    rans2_dec_chain_body<BIG, STREAMS, HOT>(info, total, c_first, c_count, wdec, dtab, ctxsym, asym, pk0, blockIdx.x);
}

}  // namespace xpng
