// mixed_views_tone.hpp -- the TONE steps of a views call: autocontrast, equalise, posterise, solarise and invert per view, up to four
// in a row (xpnghip_decode_varsize_device_batch_views_tone / _views_affine_tone).  Autocontrast and equalise need a
// statistic over the whole finished plane before the first pixel can be rewritten, so a view with a step is a second-pass view: its
// fp32 planes in byte units lie in the context's scratch (mixed_views_blur.hpp), the kernels here rewrite them IN PLACE step index
// after step index, and k_mixed_views_blur with a record that is all off writes them into the caller's buffer.
//
// The rule, per colour plane (alpha, or the 255 an RGB context lacks, is untouched), N = oh * ow:
//     entry         b = q > 0.0f ? (q > 255.0f ? 255.0f : q) : 0.0f        (from here on b is a non-negative float, never -0.0f)
//     autocontrast  lo, hi the plane's extremes; hi == lo: unchanged; else s = 255.0f / (hi - lo), correctly rounded; s infinite
//                   (hi - lo below about 7.5e-37): unchanged;
//                   t = (b - lo) * s, two operations; b = t > 255.0f ? 255.0f : t
//     equalise      h[n] the count of n = (uint32_t)rintf(b); last the highest non-empty bin; step = (N - h[last]) / 255;
//                   step == 0: unchanged; else b = (float)min(255, (step / 2 + h[0] + .. + h[n - 1]) / step)
//     posterise k   m = 2^(8 - k); b = b - fmodf(b, m)     (here floorf(b * (1 / m)) * m: m is a power of two, both forms are exact)
//     solarise thr  b = b >= thr ? 255.0f - b : b
//     invert        b = 255.0f - b
// Minimum, maximum and integer counts do not depend on the order of reduction, so the device equals the host rule bit for bit.
// The entry clamp is idempotent and no step leaves 0 .. 255 or makes a -0.0f or a NaN (with a finite s, (b - lo) * s is at most
// 255 up to rounding), so both kernels apply it to every value they read.
#pragma once
#include <stdint.h>

#include "mixed_views_blur.hpp"

namespace xpng {

// the kernels' accesses to the scratch, to LDS counters and to the statistics slots, their wave exchange, barrier and division: the
// host program replaces each and checks every address against the slice and the slots of the view whose block makes it
__device__ __forceinline__ float tone_ld(const float *p) { return *p; }
__device__ __forceinline__ void tone_st(float *p, float v) { *p = v; }
__device__ __forceinline__ float4 tone_ld4(const float *p) { return *(const float4 *)p; }
__device__ __forceinline__ void tone_st4(float *p, float4 v) { *(float4 *)p = v; }
__device__ __forceinline__ void tone_lds_add(uint32_t *p) { atomicAdd(p, 1u); }
__device__ __forceinline__ uint32_t tone_stat_ld(const uint32_t *p) { return *p; }
__device__ __forceinline__ void tone_stat_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void tone_stat_max(uint32_t *p, uint32_t v) { atomicMax(p, v); }
__device__ __forceinline__ uint32_t tone_xor(uint32_t v, uint32_t m) { return (uint32_t)__shfl_xor((int)v, (int)m, 64); }
__device__ __forceinline__ void tone_sync() { __syncthreads(); }
// (__fdiv_rn is a plain a / b in this ROCm's headers: it is correctly rounded because the build keeps hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt and has no fast-math flag - the v_div_scale / v_div_fmas / v_div_fixup sequence; the GPU bit
// tests of autocontrast are what holds a change of the flags up)
__device__ __forceinline__ float tone_div(float a, float b) { return __fdiv_rn(a, b); }

// ---- views tone ------------------------------------------------------------------------------------------------------------
// (the text from here on is what tests/views_tone_kernels_host.cpp compiles)
constexpr uint32_t TONE_NONE = 0, TONE_AUTOCONTRAST = 1, TONE_EQUALISE = 2, TONE_POSTERISE = 3, TONE_SOLARISE = 4, TONE_INVERT = 5;
// The unit of work.  The three colour planes of a view lie back to back at the start of its slice, which is aligned to 256 bytes:
// they are walked as ONE array of 3 * N floats in chunks of TONE_CHUNK, so every 16-byte access is aligned whatever N is, and the
// plane of an element is (e >= N) + (e >= 2 * N).  A block takes one chunk: 256 lanes, TONE_IT aligned groups of four floats each,
// a wave's 64 lanes on 1024 neighbouring bytes; the last group of the array may be short and goes float by float.
constexpr uint32_t TONE_IT = 8, TONE_CHUNK = 256 * 4 * TONE_IT;
// The statistics slot of one (view, statistics step), zeroed on the stream by every call: per colour plane 256 counts, then the bit
// pattern of hi, then the COMPLEMENT of the bit pattern of lo - both grow, so zero is the start of both, and unsigned order is
// float order because the entry clamp leaves non-negative floats without -0.0f.
constexpr uint32_t TONE_PLANE_WORDS = 258, TONE_SLOT_WORDS = 3 * TONE_PLANE_WORDS;

// one tone view, 48 bytes: where its planes lie in the scratch, N, its steps and the slot of each step (statistics steps only)
struct ToneRec {
    uint64_t src;   // offset of the view's slice in the scratch, in floats
    uint32_t n;     // oh * ow
    uint8_t op[4];
    float arg[4];   // posterise: m = 2^(8 - bits); solarise: the threshold
    uint32_t slot[4];
};
static_assert(sizeof(ToneRec) == 48, "DESIGN.md 25 states the size of a tone view's record");

__device__ __forceinline__ float tone_entry(float q) { return q > 0.0f ? (q > 255.0f ? 255.0f : q) : 0.0f; }
__device__ __forceinline__ uint32_t tone_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ float tone_float(uint32_t v) { return __builtin_bit_cast(float, v); }

// The statistics of step index `si`.  Grid (the most chunks of any tone view, tone views), 256 threads; a block returns at once when
// its view has fewer chunks or its step `si` is neither autocontrast nor equalise (uniform for the block).  Autocontrast: a lane
// keeps the extremes of its elements per plane, the wave reduces them by exchange, and lane 0 of each wave merges them into the slot
// - no LDS.  Equalise: every wave counts into a sub-histogram of its own in LDS (a flat region then serialises on one bin of one
// wave, not of four), the four are summed, and each non-empty bin is merged into the slot with one global atomic.
__global__ __launch_bounds__(256) void k_mixed_views_tone_stats(const ToneRec *__restrict__ tr, const float *__restrict__ scratch, uint32_t *__restrict__ stats, uint32_t si) {
    __shared__ uint32_t s_h[4 * 3 * 256];
    const ToneRec &z = tr[blockIdx.y];
    const uint32_t op = z.op[si], N = z.n, total = 3u * N;
    const uint32_t e0 = blockIdx.x * TONE_CHUNK;
    if (e0 >= total || (op != TONE_AUTOCONTRAST && op != TONE_EQUALISE)) return;
    const float *src = scratch + z.src;
    uint32_t *slot = stats + (uint64_t)z.slot[si] * TONE_SLOT_WORDS;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const bool eq = op == TONE_EQUALISE;
    uint32_t hi[3] = {0u, 0u, 0u}, nlo[3] = {0u, 0u, 0u};  // bit patterns: the largest value, the complement of the smallest
    if (eq) {
        for (uint32_t i = threadIdx.x; i < 4 * 3 * 256; i += 256) s_h[i] = 0;
        tone_sync();
    }
    auto take = [&](uint32_t e, float q) {
        const float b = tone_entry(q);
        const uint32_t p = (e >= N) + (e >= 2u * N);
        if (eq) {
            tone_lds_add(&s_h[(wv * 3 + p) * 256 + (uint32_t)rintf(b)]);
        } else {
            const uint32_t u = tone_bits(b);
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                if (p != k) continue;
                hi[k] = u > hi[k] ? u : hi[k];
                nlo[k] = ~u > nlo[k] ? ~u : nlo[k];
            }
        }
    };
#pragma unroll 2
    for (uint32_t it = 0; it < TONE_IT; it++) {
        const uint32_t e = e0 + (it * 256 + threadIdx.x) * 4;
        if (e + 4 <= total) {
            const float4 q = tone_ld4(src + e);
            take(e, q.x); take(e + 1, q.y); take(e + 2, q.z); take(e + 3, q.w);
        } else {
            for (uint32_t j = e; j < total; j++) take(j, tone_ld(src + j));
        }
    }
    if (eq) {
        tone_sync();
        for (uint32_t i = threadIdx.x; i < 3 * 256; i += 256) {
            const uint32_t p = i >> 8, n = i & 255u;
            const uint32_t t = s_h[p * 256 + n] + s_h[(3 + p) * 256 + n] + s_h[(6 + p) * 256 + n] + s_h[(9 + p) * 256 + n];
            if (t) tone_stat_add(slot + p * TONE_PLANE_WORDS + n, t);
        }
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
#pragma unroll
        for (uint32_t m = 32; m >= 1; m >>= 1) {
            const uint32_t a = tone_xor(hi[k], m), c = tone_xor(nlo[k], m);
            hi[k] = a > hi[k] ? a : hi[k];
            nlo[k] = c > nlo[k] ? c : nlo[k];
        }
        // (a plane none of the wave's elements lies in has nlo == 0: nothing to merge.  A plane it has elements in has nlo >=
        // ~bits(255.0f) > 0)
        if (lane == 0 && nlo[k]) {
            tone_stat_max(slot + k * TONE_PLANE_WORDS + 256, hi[k]);
            tone_stat_max(slot + k * TONE_PLANE_WORDS + 257, nlo[k]);
        }
    }
}

// Step index `si` applied in place.  The grid and the early return are the statistics kernel's, for every kind of step.  Equalise
// rebuilds the three planes' 256-entry tables in LDS from the slot: an inclusive scan of the counts over the block (eight doubling
// rounds between two buffers), `last` and `step` from the scanned totals, then the table value of every bin; a plane whose step is 0
// gets no table and stays as it is.  Autocontrast reads the extremes and divides once per plane.  Reads and writes are the
// statistics kernel's accesses: aligned 16-byte groups inside the view's slice, the short last group float by float.
__global__ __launch_bounds__(256) void k_mixed_views_tone_apply(const ToneRec *__restrict__ tr, float *__restrict__ scratch, const uint32_t *__restrict__ stats, uint32_t si) {
    __shared__ uint32_t s_c[2][3 * 256];
    __shared__ float s_lut[3 * 256];
    __shared__ uint32_t s_last[3];
    const ToneRec &z = tr[blockIdx.y];
    const uint32_t op = z.op[si], N = z.n, total = 3u * N;
    const uint32_t e0 = blockIdx.x * TONE_CHUNK;
    if (e0 >= total || op == TONE_NONE) return;
    float *src = scratch + z.src;
    const float arg = z.arg[si], inv = op == TONE_POSTERISE ? tone_div(1.0f, arg) : 0.0f;
    float lo[3] = {0.0f, 0.0f, 0.0f}, sc[3] = {0.0f, 0.0f, 0.0f};
    bool on[3] = {false, false, false};  // autocontrast: hi != lo and a finite s; equalise: step != 0
    if (op == TONE_AUTOCONTRAST) {
        const uint32_t *slot = stats + (uint64_t)z.slot[si] * TONE_SLOT_WORDS;  // (a call without a statistics step has no slots)
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const float hi = tone_float(tone_stat_ld(slot + k * TONE_PLANE_WORDS + 256));
            lo[k] = tone_float(~tone_stat_ld(slot + k * TONE_PLANE_WORDS + 257));
            on[k] = hi != lo[k];
            if (on[k]) {
                sc[k] = tone_div(255.0f, hi - lo[k]);
                on[k] = sc[k] <= 3.4028235e38f;  // (an infinite s: the plane stays as it is)
            }
        }
    } else if (op == TONE_EQUALISE) {
        const uint32_t *slot = stats + (uint64_t)z.slot[si] * TONE_SLOT_WORDS;
        const uint32_t t = threadIdx.x;
        uint32_t h[3];
        if (t < 3) s_last[t] = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) { h[k] = tone_stat_ld(slot + k * TONE_PLANE_WORDS + t); s_c[0][k * 256 + t] = h[k]; }
        tone_sync();
        uint32_t cur = 0;
        for (uint32_t d = 1; d < 256; d <<= 1) {
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) s_c[cur ^ 1][k * 256 + t] = s_c[cur][k * 256 + t] + (t >= d ? s_c[cur][k * 256 + t - d] : 0u);
            cur ^= 1;
            tone_sync();
        }
        // the inclusive sums are in s_c[cur]; bin t is the last non-empty one when its count is not 0 and the sum behind it is N
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
            if (h[k] && s_c[cur][k * 256 + t] == N) s_last[k] = h[k];
        tone_sync();
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const uint32_t step = (N - s_last[k]) / 255u;
            on[k] = step != 0;
            if (on[k]) {
                const uint32_t v = (step / 2u + (s_c[cur][k * 256 + t] - h[k])) / step;
                s_lut[k * 256 + t] = (float)(v < 255u ? v : 255u);
            }
        }
        tone_sync();
    }
    auto put = [&](uint32_t e, float q) -> float {
        float b = tone_entry(q);
        const uint32_t p = (e >= N) + (e >= 2u * N);
        if (op == TONE_AUTOCONTRAST) {
            const float l = p == 0 ? lo[0] : p == 1 ? lo[1] : lo[2], s = p == 0 ? sc[0] : p == 1 ? sc[1] : sc[2];
            const bool o = p == 0 ? on[0] : p == 1 ? on[1] : on[2];
            if (o) {
                const float d = b - l;
                const float t = d * s;  // (nothing is added to the product: there is no fused form to contract into)
                b = t > 255.0f ? 255.0f : t;
            }
        } else if (op == TONE_EQUALISE) {
            const bool o = p == 0 ? on[0] : p == 1 ? on[1] : on[2];
            if (o) b = s_lut[p * 256 + (uint32_t)rintf(b)];
        } else if (op == TONE_POSTERISE) {
            b = floorf(b * inv) * arg;  // (arg is a power of two in 1 .. 256: every operation is exact)
        } else if (op == TONE_SOLARISE) {
            b = b >= arg ? 255.0f - b : b;
        } else {
            b = 255.0f - b;
        }
        return b;
    };
#pragma unroll 2
    for (uint32_t it = 0; it < TONE_IT; it++) {
        const uint32_t e = e0 + (it * 256 + threadIdx.x) * 4;
        if (e + 4 <= total) {
            float4 q = tone_ld4(src + e);
            q.x = put(e, q.x); q.y = put(e + 1, q.y); q.z = put(e + 2, q.z); q.w = put(e + 3, q.w);
            tone_st4(src + e, q);
        } else {
            for (uint32_t j = e; j < total; j++) tone_st(src + j, put(j, tone_ld(src + j)));
        }
    }
}

}  // namespace xpng
