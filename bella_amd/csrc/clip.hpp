// clip.hpp -- clipped ends: every traced alignment cut to its maximum-scoring segment under an identity threshold, on gfx950.
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h, and the test
// kit's numpy statement of it, which the kernel must EQUAL).  With t = identity in permille an '=' run weighs len (1000 - t), every
// other run -len t; P is the prefix sum of the weights (P_0 = 0); the clip is the (a, b), a < b, with the largest P_b - P_a, ties to
// the smallest b and then to the largest a; a maximum that is not positive empties the pair.
//
// Mapping: k_pile_vote's -- one wavefront per pair, 64 runs per chunk in registers, 256-thread blocks whose wavefronts are independent,
// no LDS.  Pass 1, per chunk: a 64-bit inclusive wave scan of the weights on top of the carried P; a prefix-minimum scan over the
// lanes' (P_a, a) (smaller P, then larger a) merged with the carried minimum -- for the end b = r + 1 the starts a <= r compete, so the
// scan includes the lane's own exclusive prefix; value_b = P_b - min; a butterfly reduction to the chunk's best (value, b, a) (larger
// value, then smaller b), merged into the carried best.  Three things are carried between chunks: P, the minimum and the best.
// Pass 2 reads the runs [0, b) once more and sums bases and counts in front of a and inside [a, b) per lane, then reduces them: the
// other choice, prefix counters carried through pass 1, costs six more 64-bit scans per chunk and twelve more live registers for
// sums that only the winning (a, b) needs; the second read is 4 bytes per run out of L2.
// Every sum is 64 bits wide: a caller's single run may be 2^28 - 1 columns long, times a weight of up to 999.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "trace.hpp"

namespace bella {

// one pair as the clip kernel reads it
struct ClipPair {
    uint64_t op_off;       // first run in the op array
    uint32_t nops;
    int32_t i0, j0;        // tbegV, tbegH
    uint32_t pad;
};

constexpr int kClipBlock = 256;        // four independent wavefronts

#if defined(__HIPCC__)
__device__ __forceinline__ long long clip_shfl(long long x, int src) {
    const int lo = __shfl((int)(uint32_t)(unsigned long long)x, src, 64), hi = __shfl((int)(uint32_t)((unsigned long long)x >> 32), src, 64);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ long long clip_shfl_up(long long x, int d) {
    const int lo = __shfl_up((int)(uint32_t)(unsigned long long)x, d, 64), hi = __shfl_up((int)(uint32_t)((unsigned long long)x >> 32), d, 64);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ long long clip_shfl_xor(long long x, int d) {
    const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)x, d, 64), hi = __shfl_xor((int)(uint32_t)((unsigned long long)x >> 32), d, 64);
    return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ unsigned long long clip_wave_sum(unsigned long long x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += (unsigned long long)clip_shfl_xor((long long)x, d);
    return x;
}

__global__ __launch_bounds__(kClipBlock) void k_clip(const ClipPair* pp, uint32_t npairs, const uint32_t* ops, uint32_t t, bella_clip* out) {
    const uint32_t q = (uint32_t)(((uint64_t)blockIdx.x * kClipBlock + threadIdx.x) >> 6);
    if (q >= npairs) return;                                          // (whole wavefronts leave)
    const int lane = (int)(threadIdx.x & 63);
    const ClipPair P = pp[q];
    const uint32_t* const po = ops + P.op_off;
    constexpr long long kNone = 0x7fffffffffffffffll;
    const long long w_eq = 1000ll - (long long)t, w_other = -(long long)t;
    long long carryP = 0;                                             // P at the chunk's first run
    long long minP = kNone;                                           // the smallest P_a of the chunks before, at its largest a
    uint32_t minA = 0;
    long long bestV = -kNone;                                         // the best (value, b, a) of the chunks before
    uint32_t bestB = 0, bestA = 0;
    // ---- pass 1: the segment
    for (uint32_t c0 = 0; c0 < P.nops; c0 += 64) {
        const uint32_t idx = c0 + lane;
        const bool live = idx < P.nops;
        const uint32_t w = live ? po[idx] : 0u;
        const uint32_t op = w & 15u, len = w >> 4;
        const long long wt = live ? (long long)len * (op == kOpEq ? w_eq : w_other) : 0ll;
        long long incl = wt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long y = clip_shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        incl += carryP;                                               // P_{idx + 1}
        long long cp = live ? incl - wt : kNone;                      // P_idx, a start for every end from idx + 1 on
        uint32_t ca = idx;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long yp = clip_shfl_up(cp, d);
            const uint32_t ya = __shfl_up(ca, d, 64);
            if (lane >= d && (yp < cp || (yp == cp && ya > ca))) { cp = yp; ca = ya; }
        }
        if (minP < cp) { cp = minP; ca = minA; }                      // (equal: the lane's own a is the larger one)
        long long v = live ? incl - cp : -kNone;
        uint32_t vb = idx + 1, va = ca;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long yv = clip_shfl_xor(v, d);
            const uint32_t yb = __shfl_xor(vb, d, 64), ya = __shfl_xor(va, d, 64);
            if (yv > v || (yv == v && yb < vb)) { v = yv; vb = yb; va = ya; }
        }
        if (v > bestV) { bestV = v; bestB = vb; bestA = va; }         // (equal: the carried end is the smaller one)
        carryP = clip_shfl(incl, 63);
        minP = clip_shfl(cp, 63);
        minA = __shfl(ca, 63, 64);
    }
    bella_clip r{};
    r.begV = r.endV = P.i0;
    r.begH = r.endH = P.j0;
    if (P.nops == 0 || bestV <= 0) {
        if (lane == 0) out[q] = r;
        return;
    }
    // ---- pass 2: bases in front of the segment, bases and counts inside it
    unsigned long long preV = 0, preH = 0, cnt[4] = {0, 0, 0, 0};
    for (uint32_t c0 = 0; c0 < bestB; c0 += 64) {
        const uint32_t idx = c0 + lane;
        if (idx >= bestB) continue;
        const uint32_t w = po[idx];
        const uint32_t op = w & 15u, len = w >> 4;
        if (idx < bestA) {
            if (op != kOpDel) preV += len;
            if (op != kOpIns) preH += len;
        } else {
#pragma unroll
            for (int o = 0; o < 4; ++o) cnt[o] += op == (uint32_t)o ? len : 0u;
        }
    }
    preV = clip_wave_sum(preV);
    preH = clip_wave_sum(preH);
#pragma unroll
    for (int o = 0; o < 4; ++o) cnt[o] = clip_wave_sum(cnt[o]);
    if (lane == 0) {
        r.first_run = bestA;
        r.nruns = bestB - bestA;
        r.begV = (int32_t)((long long)P.i0 + (long long)preV);
        r.begH = (int32_t)((long long)P.j0 + (long long)preH);
        r.endV = (int32_t)((long long)r.begV + (long long)(cnt[kOpEq] + cnt[kOpX] + cnt[kOpIns]));
        r.endH = (int32_t)((long long)r.begH + (long long)(cnt[kOpEq] + cnt[kOpX] + cnt[kOpDel]));
        r.n_eq = (uint32_t)cnt[kOpEq]; r.n_x = (uint32_t)cnt[kOpX]; r.n_ins = (uint32_t)cnt[kOpIns]; r.n_del = (uint32_t)cnt[kOpDel];
        r.score = (int32_t)((long long)cnt[kOpEq] - (long long)cnt[kOpX] - (long long)cnt[kOpIns] - (long long)cnt[kOpDel]);
        r.clip_score = bestV;
        out[q] = r;
    }
}
#endif

}  // namespace bella
