// Host run of the four-bit context queues of the wide level-1 decode (xpng_amd/csrc/rans_dec.hpp: ctxn_*).
//   1. the pack (ctxn_byte), gather / merge (the chain's registers) and unpack (the walk's head) arithmetic against the layout's
//      restatement: symbol i of a queue = (byte[i >> 1] >> 4 (i & 1)) & 15, symbols above 8 stored as 9;
//   2. a model of k_dec_walk_wide's service rule on one lane, for a window of 4 and of 2 chunks: one chunk requested per queue and
//      service, landed at the next service if its slot has been read out, the head one dword ahead of the position.  Every window
//      dword carries the index of the queue dword it holds; a head that takes a dword which is not the one it asks for counts as a
//      violation, and the walked sequence is compared with the direct walk nl = *cx[nl]++.
// Built and run by tests/test_ctx_nibbles_host.py: g++ -fsanitize=undefined,address -DKERNEL_TEXT=\"...\" -DSHIPPED_WCH=n.
#include "kernel_host.hpp"  // __device__ and __forceinline__
#define __host__
#include KERNEL_TEXT  // CTXN_CHUNK, ctxn_clamp, ctxn_byte, ctxn_gather, ctxn_merge, ctxn_sym, ctxn_pop, ctxn_cross, ctxn_dword, ctxn_chunk

static long cases = 0;
static uint32_t rnd_state = 2463534242u;
static uint32_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 17; rnd_state ^= rnd_state << 5; return rnd_state; }

// the layout, restated
static uint32_t stored(uint32_t s) { return s < 9 ? s : 9; }
static uint32_t unpack(const std::vector<uint8_t> &b, uint32_t i) { return (b[i >> 1] >> (4 * (i & 1))) & 15u; }
static void check_queue(const char *what, const std::vector<uint8_t> &b, const std::vector<uint32_t> &s) {
    for (uint32_t i = 0; i < s.size(); i++) { cases++; if (unpack(b, i) != stored(s[i])) bad(what, i, (long)s.size()); }
}

// ---- 1a. the producers without a pair of lanes (rans2_dec_plain, the flush of rans2_decode_stream): a byte per two symbols
static void pack_plain(const std::vector<uint32_t> &s) {
    const uint32_t n = (uint32_t)s.size();
    std::vector<uint8_t> b((n + 15) / 16 * 16 + 16, 0xEE);
    for (uint32_t i = 0; i < n; i += 2) b[i >> 1] = (uint8_t)ctxn_byte(s[i], i + 1 < n ? s[i + 1] : 0u);
    check_queue("ctxn_byte", b, s);
    for (uint32_t k = (n + 1) / 2; k < b.size(); k++) if (b[k] != 0xEE) bad("ctxn_byte wrote behind the queue", k, n);
}

// ---- 1b. the chain (k_rans2_dec_chain<false, ...>): the pair of lanes of one stream inside a wavefront whose trip count is T
// pairs (a multiple of 8, >= the stream's own).  Blocks run from the top down; an inactive step gathers nothing; a block is stored
// (8 bytes, by the even lane) when it begins below the stream's pair count and the registers are cleared only then; the odd tail
// goes out as a byte of its own and into its place of the top block.
static void pack_chain(const std::vector<uint32_t> &s, uint32_t extra_blocks) {
    const uint32_t n = (uint32_t)s.size(), npairs = n >> 1, T = ((npairs + 7) & ~7u) + 8 * extra_blocks;
    std::vector<uint8_t> b((n + 15) / 16 * 16 + 16, 0xEE);
    uint32_t acc[2][2] = {{0, 0}, {0, 0}};  // [lane of the pair][dword]
    if (n & 1) {
        b[(n - 1) >> 1] = (uint8_t)s[n - 1];
        const uint32_t ut = npairs & 7u;
        if (ut) acc[0][ut >> 2] = ctxn_gather(0u, s[n - 1], ut);
    }
    for (uint32_t jb = T; jb > 0;) {
        jb -= 8;
        for (int u = 7; u >= 0; u--)
            for (uint32_t par = 0; par < 2; par++) {
                const bool act = jb + (uint32_t)u < npairs;
                const uint32_t sym = act ? s[2 * (jb + (uint32_t)u) + par] : rnd() % 9;  // (an idle step still resolves some symbol)
                acc[par][u >> 2] = ctxn_gather(acc[par][u >> 2], act ? sym : 0u, (uint32_t)u);
            }
        const bool st = jb < npairs;
        const uint32_t m0 = ctxn_merge(acc[0][0], acc[1][0]), m1 = ctxn_merge(acc[0][1], acc[1][1]);
        if (st) {
            if (jb + 8 > b.size()) { bad("chain store outside the queue's room", jb, n); return; }
            memcpy(b.data() + jb, &m0, 4); memcpy(b.data() + jb + 4, &m1, 4);
        }
        for (uint32_t par = 0; par < 2; par++) for (uint32_t w = 0; w < 2; w++) acc[par][w] = st ? 0u : acc[par][w];
    }
    check_queue("chain gather/merge", b, s);
    for (uint32_t k = (n + 15) / 16 * 8; k < b.size(); k++) if (b[k] != 0xEE) bad("chain wrote behind the queue's packed room", k, n);
}

// ---- 1c. the walk's head: dword by dword, next symbol in the lowest nibble
static void unpack_head(const std::vector<uint32_t> &s) {
    const uint32_t n = (uint32_t)s.size();
    std::vector<uint8_t> b((n + 15) / 16 * 16 + 16, 0);
    for (uint32_t i = 0; i < n; i++) b[i >> 1] |= (uint8_t)(stored(s[i]) << (4 * (i & 1)));
    auto dw = [&](uint32_t d) { uint32_t v; memcpy(&v, b.data() + 4 * d, 4); return v; };
    uint32_t lo = dw(0), pos = 0, nxt = dw(1);
    for (uint32_t i = 0; i < n; i++) {
        cases++;
        if (ctxn_sym(lo) != stored(s[i])) bad("head unpack", i, n);
        const uint32_t npos = pos + 1;
        if (ctxn_cross(npos)) { lo = nxt; nxt = dw(ctxn_dword(npos) + 1); } else lo = ctxn_pop(lo);
        pos = npos;
        if (ctxn_dword(pos) != pos / 8 || ctxn_chunk(pos) != pos / CTXN_CHUNK) bad("position arithmetic", pos, 0);
    }
}

// ---- 2. the service rule of k_dec_walk_wide on one lane
struct Dw { uint32_t v; long tag; };  // a dword and the index of the queue dword it is (-1: nothing has landed here)
template <uint32_t WCH> struct WalkModel {
    static constexpr uint32_t SVC = 2, INIT = 2, WDW = WCH * 4;
    std::vector<std::vector<uint32_t>> mem;  // the nine queues, packed, as dwords; zero dwords behind the end (the loads run past it)
    Dw ringw[10][WDW];
    struct Head { Dw lo; uint32_t pos; Dw nxt; } head[10];
    uint32_t have[9];
    long fl[9];  // chunk in flight
    long violations = 0;
    uint32_t qdw(uint32_t c, long d) const { return (size_t)d < mem[c].size() ? mem[c][(size_t)d] : 0u; }
    void land(uint32_t c, uint32_t slot, long chunk) { for (uint32_t w = 0; w < 4; w++) ringw[c][slot * 4 + w] = Dw{qdw(c, 4 * chunk + w), 4 * chunk + w}; }

    std::vector<uint32_t> run(const std::vector<std::vector<uint32_t>> &queues, uint32_t total) {
        mem.assign(9, {});
        for (uint32_t c = 0; c < 9; c++) {
            mem[c].assign(queues[c].size() / 8 + 1, 0u);
            for (uint32_t i = 0; i < queues[c].size(); i++) mem[c][i >> 3] |= stored(queues[c][i]) << (4 * (i & 7));
            for (uint32_t w = 0; w < WDW; w++) ringw[c][w] = Dw{0xDEADBEEFu, -1};
            for (uint32_t q = 0; q < INIT; q++) land(c, q, q);
            head[c] = Head{ringw[c][0], 0, ringw[c][1]};
            have[c] = INIT; fl[c] = INIT;
        }
        for (uint32_t w = 0; w < WDW; w++) ringw[9][w] = Dw{0x99999999u, -2};
        head[9] = Head{Dw{0x99999999u, -2}, 0, Dw{0x99999999u, -2}};
        std::vector<uint32_t> out;
        uint32_t cur = total > 0 ? 0u : 9u, pcur = 9;
        Dw plo{0x99999999u, -2}, pnxt{0x99999999u, -2};
        uint32_t ppos = 0;
        const uint32_t T = (total + 31) / 32 * 32;
        for (uint32_t kb = 0; kb < T; kb += 16) {
            for (uint32_t u = 0; u < 16; u++) {
                const uint32_t npos = ppos + 1;
                const bool cross = ctxn_cross(npos);
                const Dw rr = ringw[pcur][(ctxn_dword(npos) + 1) & (WDW - 1)];
                const Head r = head[cur];
                // the dword the head takes over must be the one behind its new current dword (the parking queue has no positions)
                if (cross && pcur != 9 && rr.tag != (long)ctxn_dword(npos) + 1) violations++;
                const Dw nlo = cross ? pnxt : Dw{ctxn_pop(plo.v), plo.tag}, nnxt = cross ? rr : pnxt;
                head[pcur] = Head{nlo, npos, nnxt};
                const bool same = cur == pcur;
                plo = same ? nlo : r.lo; ppos = same ? npos : r.pos; pnxt = same ? nnxt : r.nxt;
                pcur = cur;
                // the dword a symbol is popped from must be the one its position lies in
                if (cur != 9 && plo.tag != (long)ctxn_dword(ppos)) violations++;
                const uint32_t sym = ctxn_sym(plo.v);
                if (kb + u < total) out.push_back(sym);
                cur = kb + u + 1 >= total ? 9u : (sym < 9u ? sym : 9u);
            }
            const uint32_t phase = (kb / 16) & (SVC - 1);
            for (uint32_t c = 0; c < 9; c++) {
                if ((c & (SVC - 1)) != phase) continue;
                const uint32_t cq = ctxn_chunk(head[c].pos);
                if (have[c] - cq < WCH) { land(c, have[c] & (WCH - 1), fl[c]); have[c]++; }
                fl[c] = have[c];
            }
        }
        return out;
    }
};

// the queues that make the direct walk produce `seq` (seq[0] is popped from queue 0, seq[k + 1] from queue seq[k])
static std::vector<std::vector<uint32_t>> queues_of(const std::vector<uint32_t> &seq) {
    std::vector<std::vector<uint32_t>> q(9);
    uint32_t cur = 0;
    for (uint32_t s : seq) { q[cur].push_back(s); cur = s; }
    return q;
}
static std::vector<uint32_t> direct_walk(const std::vector<std::vector<uint32_t>> &q, uint32_t total) {
    std::vector<uint32_t> out; size_t at[9] = {0}; uint32_t nl = 0;
    for (uint32_t k = 0; k < total; k++) { nl = q[nl][at[nl]++]; out.push_back(nl); }
    return out;
}
template <uint32_t WCH> static long model_case(const std::vector<uint32_t> &seq, bool count_errors) {
    const auto q = queues_of(seq);
    const auto want = direct_walk(q, (uint32_t)seq.size());
    WalkModel<WCH> m;
    const auto got = m.run(q, (uint32_t)seq.size());
    cases += (long)seq.size();
    long v = m.violations + (got != want ? 1 : 0);
    if (want != seq) bad("the test's own queues", 0, 0);
    if (count_errors && v) bad("walk model", (long)WCH, v);
    return v;
}

int main() {
    // ---- 1
    static const uint32_t LEN[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 3, 5, 7, 9, 11, 13, 21, 27, 127, 130};
    for (uint32_t n : LEN)
        for (int rep = 0; rep < 8; rep++) {
            std::vector<uint32_t> s(n);
            for (auto &x : s) x = rep == 0 ? 8 : rnd() % 9;
            pack_chain(s, 0); pack_chain(s, 1); pack_chain(s, 3);
            unpack_head(s);
            pack_plain(s);
            for (auto &x : s) x = rnd() % 3 ? rnd() % 9 : 9 + rnd() % 247;  // symbols only a stream the reference cannot write holds
            pack_plain(s);
        }
    // ---- 2
    std::vector<std::vector<uint32_t>> seqs;
    for (uint32_t total : {0u, 1u, 15u, 16u, 17u, 31u, 32u, 33u, 40u, 100u, 257u, 1000u}) {
        seqs.push_back(std::vector<uint32_t>(total, 0));                                   // one queue on every step (the other eight empty from the start)
        std::vector<uint32_t> a(total);
        for (uint32_t k = 0; k < total; k++) a[k] = (k & 1) ? 0 : 1;                         // two queues alternating
        seqs.push_back(a);
        for (uint32_t k = 0; k < total; k++) a[k] = (k & 1) ? 8 : 7;
        seqs.push_back(a);
    }
    for (uint32_t run : {1u, 7u, 8u, 9u, 23u, 24u, 25u, 31u, 32u, 33u, 40u, 63u, 64u, 65u, 95u, 97u, 129u})  // a queue that ends mid-chunk, then another takes every pop
        for (uint32_t lead = 0; lead < 34; lead++) {
            std::vector<uint32_t> a;
            for (uint32_t k = 0; k < lead; k++) a.push_back(k & 1 ? 0 : 3);
            for (uint32_t r = 0; r < 6; r++) { const uint32_t s = (r * 5 + 2) % 9; for (uint32_t k = 0; k < run + r; k++) a.push_back(s); }
            seqs.push_back(a);
        }
    for (int rep = 0; rep < 300; rep++) {  // random runs: long bursts of one queue between short visits to the others
        std::vector<uint32_t> a;
        const uint32_t total = 1 + rnd() % 1500;
        while (a.size() < total) { const uint32_t s = rnd() % 9, len = rnd() % 4 ? 1 + rnd() % 4 : 1 + rnd() % 100; for (uint32_t k = 0; k < len && a.size() < total; k++) a.push_back(s); }
        seqs.push_back(a);
    }
    long v4 = 0, v2 = 0;
    for (const auto &s : seqs) { v4 += model_case<4>(s, SHIPPED_WCH == 4); v2 += model_case<2>(s, SHIPPED_WCH == 2); }
    printf("window of 4 chunks: %ld violations; window of 2 chunks: %ld violations; shipped: %d chunks\n", v4, v2, SHIPPED_WCH);
    if (SHIPPED_WCH != 4 && SHIPPED_WCH != 2) bad("unknown window size", SHIPPED_WCH, 0);
    printf("cases: %ld\nerrors: %d\n", cases, errors);
    return errors ? 1 : 0;
}
