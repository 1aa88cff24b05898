// trace.hpp -- base-level alignments: banded DP with stored directions, backtrace and run-length ops on gfx950.
//
// Nothing in the reference does this (its PAF carries a score and end points only); the definition is this project's own and is
// written down in DESIGN.md section 9.  In short: an EXTENSION is a DP anchored at the seed (cell (0,0) = 0, match +1, mismatch -1,
// gap -1 linear, the X-drop's scoring) over the rectangle rows i = 0..n (bases of V) x columns j = 0..m (bases of the oriented H),
// free at the far end: it ends at the cell with the best score, ties to the smallest i + j, then the smallest i.  A pair is the left
// extension (both sequences reversed from the seed's start), the seed's k columns, and the right extension.
//
// Mapping.  One wavefront per extension, the band of B = 64 * C cells across the lanes, lane L owning the C adjacent diagonals
// p = L*C .. L*C + C-1 (p = j - i + B/2), scores in VGPRs.  The sweep is row by row: with a linear gap the dependence inside a row is
//     S[i][j] = max_{j' <= j} (cand[j'] + j') - j,        cand = max(diagonal + sub, up - 1)
// i.e. ONE prefix maximum over the band per row: C - 1 dependent maxima inside the lane and a 6-step scan over the wave.  The
// anti-diagonal sweep (the shape of the X-drop kernels) has no scan but needs both neighbours from the two previous anti-diagonals and
// 2 (n + m) steps instead of n: twice the steps, and in each step half the band's cells belong to the other parity.  With B >= 256 the
// row sweep's scan (12 cross-lane operations) is a small part of a row's ~30 * C VALU instructions, so the row sweep it is.
// In band coordinates the diagonal neighbour of (i, p) is (i-1, p) and the upper one (i-1, p+1): a row needs ONE value from the next
// lane.  The bases of H slide one position per row through a 2-bit-per-base register window; the base of V is wave-uniform.
// Directions: 2 bits per cell (0 diagonal, 1 up = consumes V, 2 left = consumes H), byte p/4 of the row, rows of B/4 bytes: a lane
// stores its C cells as one u8 / u16 / u32 -- a wave writes 64 / 128 / 256 contiguous bytes per row with ordinary vector stores.
// Bands above 1,024 cells (widened extensions, tests that force the band to cover the rectangle) run k_trace_dp_wide: the same row
// code on tiles of 256 cells, the previous row in a global scratch of 2 * B ints per extension.
// The backtrace is one thread per pair (a serial pointer chase): a counting walk (runs, op totals, whether the path touched the band
// edge) and, once the host has laid out the op array, a writing walk -- left part forwards, right part from the pair's end backwards.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "core.hpp"

namespace bella {

constexpr int kTrNeg = -(1 << 28);
constexpr uint32_t kTrMinBand = 256, kTrRegBand = 1024;      // register kernel: C = 4, 8, 16
constexpr uint32_t kTrMaxBand = 1u << 18;                    // covers any rectangle of reads < 65,536 (2 * 65,536 = 2^17)
enum { kOpEq = 0, kOpX = 1, kOpIns = 2, kOpDel = 3 };

// one extension; sequence element t of H is base gH + dH * t of the packed reads (complemented if comp), of V base gV + dV * t
struct TraceExt {
    int64_t gH, gV;
    uint64_t dir_off;      // bytes into the direction buffer: rows 1..rows, B/4 bytes each
    uint64_t scr_off;      // wide kernel: ints into the scratch (2 * B per extension)
    uint32_t n, m;         // rows (bases of V), columns (bases of H)
    uint32_t band;         // B: power of two >= 256
    int32_t dH, dV;
    uint32_t comp;         // 3: H is complemented
    uint32_t pad;
};
struct TraceExtRes { int32_t score; uint32_t bi, bj, pad; };
// what the counting walk reports per pair of the batch
struct TracePairRes {
    uint32_t nops, n_eq, n_x, n_ins, n_del;
    uint32_t touch;        // bit0: the left path touched the band edge, bit1: the right one
    int32_t seed_score;
    uint32_t pad;
};

BELLA_HD uint32_t trace_rows(uint32_t n, uint32_t m, uint32_t band) {        // rows that hold a cell of the rectangle inside the band
    const uint64_t r = (uint64_t)m + band / 2;
    return r < n ? (uint32_t)r : n;
}
BELLA_HD uint32_t trace_cover_band(uint32_t n, uint32_t m) {                  // smallest band that holds the whole rectangle
    uint32_t need = 2 * (n > m + 1 ? n : m + 1), b = kTrMinBand;
    while (b < need) b <<= 1;
    return b;
}

BELLA_HD int trace_base(const uint32_t* packed, int64_t g0, int d, uint32_t comp, int64_t t) {
    const int64_t g = g0 + (int64_t)d * t;
    return (int)(((packed[g >> 4] >> ((uint32_t)(g & 15) * 2)) & 3u) ^ comp);
}

#if defined(__HIPCC__)
struct TraceBest { int s; int sum; int i; };
__device__ __forceinline__ void trace_best_take(TraceBest& b, int s, int sum, int i) {
    const bool better = s > b.s || (s == b.s && (sum < b.sum || (sum == b.sum && i < b.i)));
    if (better) { b.s = s; b.sum = sum; b.i = i; }
}

// One row of one tile of 64 * C cells: prev[c] = S[i-1] at the lane's positions, upn = S[i-1] at the next lane's first position;
// hwin holds the lane's C bases of H for this row (2 bits each), vb the row's base of V; jb = column j of the lane's first cell;
// carry = prefix maximum of (cand + position) over the tiles before this one.  Leaves S[i] in prev, returns the 2C direction bits.
template <int C>
__device__ __forceinline__ uint32_t trace_row_tile(int (&prev)[C], int upn, uint32_t hwin, int vb, int jb, int m, int p0, int& carry, int i,
                                                   TraceBest& best) {
    const int lane = (int)(threadIdx.x & 63);
    int cd[C], cu[C], loc[C];
    int run = kTrNeg;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = jb + c;
        const bool valid = j >= 0 && j <= m;
        const int sub = ((int)((hwin >> (2 * c)) & 3u) == vb) ? 1 : -1;
        const int up = c + 1 < C ? prev[c + 1] : upn;
        cd[c] = (j >= 1 && valid) ? prev[c] + sub : kTrNeg;           // (i-1, j-1): inside the rectangle when 1 <= j <= m
        cu[c] = valid ? up - 1 : kTrNeg;                               // (i-1, j)
        int cand = cd[c] > cu[c] ? cd[c] : cu[c];
        if (cand < kTrNeg) cand = kTrNeg;
        const int e = cand + (p0 + c);
        run = e > run ? e : run;
        loc[c] = run;
    }
    // inclusive maximum scan of the lanes' totals, then the exclusive value of this lane
    int x = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d && y > x) x = y;
    }
    int ex = __shfl_up(x, 1, 64);
    if (lane == 0) ex = kTrNeg;
    if (carry > ex) ex = carry;
    const int total = __shfl(x, 63, 64);
    if (total > carry) carry = total;
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = jb + c;
        const bool valid = j >= 0 && j <= m;
        const int mx = loc[c] > ex ? loc[c] : ex;
        int s = mx - (p0 + c);
        if (!valid || s < kTrNeg) s = kTrNeg;
        const uint32_t d = s == cd[c] ? 0u : (s == cu[c] ? 1u : 2u);
        bits |= d << (2 * c);
        if (valid) trace_best_take(best, s, i + j, i);
        prev[c] = s;
    }
    return bits;
}

__device__ __forceinline__ void trace_best_reduce(TraceBest& b) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int s = __shfl_xor(b.s, d, 64), sum = __shfl_xor(b.sum, d, 64), i = __shfl_xor(b.i, d, 64);
        trace_best_take(b, s, sum, i);
    }
}

template <int C> struct TraceDirWord;
template <> struct TraceDirWord<4> { using type = uint8_t; };
template <> struct TraceDirWord<8> { using type = uint16_t; };
template <> struct TraceDirWord<16> { using type = uint32_t; };

constexpr int kTraceBlock = 256;      // four independent wavefronts

// band of 64 * C cells in registers; list[w] = the extension of wavefront w
template <int C>
__global__ __launch_bounds__(kTraceBlock) void k_trace_dp(const TraceExt* exts, const uint32_t* list, uint32_t nlist, const uint32_t* packed,
                                                          uint8_t* dirs, TraceExtRes* res) {
    using Word = typename TraceDirWord<C>::type;
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= nlist) return;                                           // (whole wavefronts leave)
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t slot = list[w];
    const TraceExt e = exts[slot];
    constexpr int B = 64 * C, half = B / 2;
    const int n = (int)e.n, m = (int)e.m;
    const int rows = (int)trace_rows(e.n, e.m, (uint32_t)B);
    const int p0 = lane * C;
    int prev[C];
    TraceBest best{kTrNeg, 0, 0};
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = p0 + c - half;
        prev[c] = (j >= 0 && j <= m) ? -j : kTrNeg;
        if (j >= 0 && j <= m) trace_best_take(best, -j, j, 0);
    }
    // the lane's bases of H for row 1: cell c is column j = 1 + p0 + c - half, its base h[j - 1]
    uint32_t hwin = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int t = p0 + c - half;
        if (t >= 0 && t < m) hwin |= (uint32_t)trace_base(packed, e.gH, e.dH, e.comp, t) << (2 * c);
    }
    Word* const drow = (Word*)(dirs + e.dir_off) + lane;
    uint32_t vw = 0;
    int64_t vwi = -1;
    for (int i = 1; i <= rows; ++i) {
        const int64_t gv = e.gV + (int64_t)e.dV * (i - 1);
        if ((gv >> 4) != vwi) { vwi = gv >> 4; vw = packed[vwi]; }
        const int vb = (int)((vw >> ((uint32_t)(gv & 15) * 2)) & 3u);
        int upn = __shfl_down(prev[0], 1, 64);
        if (lane == 63) upn = kTrNeg;
        int carry = kTrNeg;
        const uint32_t bits = trace_row_tile<C>(prev, upn, hwin, vb, i + p0 - half, m, p0, carry, i, best);
        drow[(size_t)(i - 1) * 64] = (Word)bits;
        // slide the window: the new top base is h[t], t = i + p0 + C - 1 - half (the column j - 1 of the last cell in row i + 1)
        const int t = i + p0 + C - 1 - half;
        uint32_t nb = 0;
        if (t >= 0 && t < m) nb = (uint32_t)trace_base(packed, e.gH, e.dH, e.comp, t);
        hwin = (C == 16 ? (hwin >> 2) : ((hwin >> 2) & ((1u << (2 * (C - 1))) - 1u))) | (nb << (2 * (C - 1)));
    }
    (void)n;
    trace_best_reduce(best);
    if (lane == 0) res[slot] = TraceExtRes{best.s, (uint32_t)best.i, (uint32_t)(best.sum - best.i), 0u};
}

// any band: tiles of 256 cells, the previous row in global scratch (two rows of B ints, swapped per row); one wavefront per block.
// INVARIANT the kernel leans on: the second scratch row starts uninitialised, and a row only computes (and stores direction bytes
// for) the tiles that hold a column 0 .. m.  What lies outside is never USED: trace_row_tile masks every neighbour by the column it
// stands for (cd needs 1 <= j <= m, cu needs 0 <= j <= m, and those cells were computed by the row before), and the walk only visits
// cells of the rectangle.  Do not read prev[] or a direction byte without that mask.
__global__ __launch_bounds__(64) void k_trace_dp_wide(const TraceExt* exts, const uint32_t* list, uint32_t nlist, const uint32_t* packed, uint8_t* dirs,
                                                      int* scratch, TraceExtRes* res) {
    const uint32_t w = blockIdx.x;
    if (w >= nlist) return;
    const int lane = (int)threadIdx.x;
    const uint32_t slot = list[w];
    const TraceExt e = exts[slot];
    const int B = (int)e.band, half = B / 2;
    const int m = (int)e.m;
    const int rows = (int)trace_rows(e.n, e.m, e.band);
    int* bufP = scratch + e.scr_off;
    int* bufC = bufP + B;
    TraceBest best{kTrNeg, 0, 0};
    for (int p = lane; p < B; p += 64) {
        const int j = p - half;
        const bool valid = j >= 0 && j <= m;
        bufP[p] = valid ? -j : kTrNeg;
        if (valid) trace_best_take(best, -j, j, 0);
    }
    __syncthreads();
    uint8_t* const dbase = dirs + e.dir_off;
    const size_t rowbytes = (size_t)B / 4;
    for (int i = 1; i <= rows; ++i) {
        const int vb = trace_base(packed, e.gV, e.dV, 0u, i - 1);
        const int plo = half - i > 0 ? half - i : 0;                                  // positions of the columns 0 .. m in this row
        const int phi = half - i + m < B - 1 ? half - i + m : B - 1;
        int carry = kTrNeg;
        for (int t = plo >> 8; t <= (phi >> 8); ++t) {
            const int p0 = t * 256 + lane * 4;
            int prev[4];
            const int4 q = *(const int4*)(bufP + p0);
            prev[0] = q.x; prev[1] = q.y; prev[2] = q.z; prev[3] = q.w;
            const int upn = p0 + 4 < B ? bufP[p0 + 4] : kTrNeg;
            const int jb = i + p0 - half;
            uint32_t hwin = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int tt = jb + c - 1;
                if (tt >= 0 && tt < m) hwin |= (uint32_t)trace_base(packed, e.gH, e.dH, e.comp, tt) << (2 * c);
            }
            const uint32_t bits = trace_row_tile<4>(prev, upn, hwin, vb, jb, m, p0, carry, i, best);
            *(int4*)(bufC + p0) = make_int4(prev[0], prev[1], prev[2], prev[3]);
            dbase[(size_t)(i - 1) * rowbytes + (size_t)(p0 >> 2)] = (uint8_t)bits;
        }
        __syncthreads();                                                              // the row is in memory before the next one reads it
        int* tmp = bufP; bufP = bufC; bufC = tmp;
    }
    trace_best_reduce(best);
    if (lane == 0) res[slot] = TraceExtRes{best.s, (uint32_t)best.i, (uint32_t)(best.sum - best.i), 0u};
}

// ---- backtrace ------------------------------------------------------------------------------------------------------------------
// Walks one extension from its best cell back to the seed and hands every op to `put` (far end first).  Returns whether the path
// touched the first or the last diagonal of the band.
template <class Put>
__device__ __forceinline__ bool trace_walk(const TraceExt& e, const TraceExtRes& r, const uint32_t* packed, const uint8_t* dirs, Put&& put) {
    int i = (int)r.bi, j = (int)r.bj;
    const int B = (int)e.band, half = B / 2;
    const uint8_t* const d0 = dirs + e.dir_off;
    const size_t rowbytes = (size_t)B / 4;
    bool touch = false;
    while (i > 0 || j > 0) {
        int p = j - i + half;
        if (p <= 0 || p >= B - 1) { touch = true; p = p < 0 ? 0 : (p > B - 1 ? B - 1 : p); }      // (a path never leaves the band; the clamp keeps a read in bounds whatever the bytes say)
        uint32_t d = 2;
        if (i > 0) {
            d = j == 0 ? 1u : (uint32_t)((d0[(size_t)(i - 1) * rowbytes + (size_t)(p >> 2)] >> (2 * (p & 3))) & 3u);
            if (d == 3) d = 2;
        }
        if (d == 0) {
            const int hb = trace_base(packed, e.gH, e.dH, e.comp, j - 1), vb = trace_base(packed, e.gV, e.dV, 0u, i - 1);
            put(hb == vb ? kOpEq : kOpX);
            --i; --j;
        } else if (d == 1) { put(kOpIns); --i; }
        else { put(kOpDel); --j; }
    }
    return touch;
}

struct TraceRuns {               // runs of a part, in the order the ops arrive
    int first = -1, last = -1;
    uint32_t nruns = 0;
    uint32_t cnt[4] = {0, 0, 0, 0};
    __device__ __forceinline__ void operator()(int op) {
        if (op != last) { ++nruns; if (first < 0) first = op; last = op; }
        ++cnt[op];
    }
};

// seed column t: base t of the k-mer on the oriented H against base t on V (the right extension's sequences continue the seed)
__device__ __forceinline__ int trace_seed_op(const TraceExt& right, const uint32_t* packed, int k, int t) {
    const int hb = trace_base(packed, right.gH, right.dH, right.comp, (int64_t)t - k), vb = trace_base(packed, right.gV, right.dV, 0u, (int64_t)t - k);
    return hb == vb ? kOpEq : kOpX;
}

// one thread per pair of the batch: exts[2q] = left, exts[2q + 1] = right
__global__ void k_trace_count(const TraceExt* exts, const TraceExtRes* res, uint32_t npairs, const uint32_t* packed, const uint8_t* dirs, int k,
                              TracePairRes* out) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npairs) return;
    const TraceExt L = exts[2 * q], R = exts[2 * q + 1];
    TraceRuns rl, rs, rr;
    const bool tl = trace_walk(L, res[2 * q], packed, dirs, rl);
    int ss = 0;
    for (int t = 0; t < k; ++t) { const int op = trace_seed_op(R, packed, k, t); rs(op); ss += op == kOpEq ? 1 : -1; }
    const bool tr = trace_walk(R, res[2 * q + 1], packed, dirs, rr);
    // runs of left ++ seed ++ reverse(right): the right part arrives far end first
    uint32_t nops = 0;
    int last = -1;
    if (rl.nruns) { nops += rl.nruns; last = rl.last; }
    if (rs.nruns) { nops += rs.nruns - (rs.first == last ? 1u : 0u); last = rs.last; }
    if (rr.nruns) { nops += rr.nruns - (rr.last == last ? 1u : 0u); }
    TracePairRes o;
    o.nops = nops;
    o.n_eq = rl.cnt[0] + rs.cnt[0] + rr.cnt[0]; o.n_x = rl.cnt[1] + rs.cnt[1] + rr.cnt[1];
    o.n_ins = rl.cnt[2] + rs.cnt[2] + rr.cnt[2]; o.n_del = rl.cnt[3] + rs.cnt[3] + rr.cnt[3];
    o.touch = (tl ? 1u : 0u) | (tr ? 2u : 0u);
    o.seed_score = ss;
    o.pad = 0;
    out[q] = o;
}

struct TraceEmit {               // merges adjacent equal ops; step = +1 writes forwards from idx, -1 backwards from idx - 1
    uint32_t* out;
    int64_t idx;
    int step;
    int op = -1;
    uint32_t len = 0;
    __device__ __forceinline__ void flush() {
        if (op < 0) return;
        if (step > 0) out[idx++] = (len << 4) | (uint32_t)op;
        else out[--idx] = (len << 4) | (uint32_t)op;
        op = -1; len = 0;
    }
    __device__ __forceinline__ void operator()(int o) {
        if (o == op) { ++len; return; }
        flush();
        op = o; len = 1;
    }
};

// one thread per finished pair: ops[op_off .. op_off + nops) in V order; op_off == ~0: the pair is traced again with a wider band
__global__ void k_trace_write(const TraceExt* exts, const TraceExtRes* res, uint32_t npairs, const uint32_t* packed, const uint8_t* dirs, int k,
                              const uint64_t* op_off, const TracePairRes* cnt, uint32_t* ops) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= npairs) return;
    const uint64_t off = op_off[q];
    if (off == ~0ull) return;
    const TraceExt L = exts[2 * q], R = exts[2 * q + 1];
    TraceEmit fw{ops, (int64_t)off, 1}, bw{ops, (int64_t)(off + cnt[q].nops), -1};
    trace_walk(L, res[2 * q], packed, dirs, fw);
    for (int t = 0; t < k; ++t) fw(trace_seed_op(R, packed, k, t));
    trace_walk(R, res[2 * q + 1], packed, dirs, bw);
    if (fw.op >= 0 && fw.op == bw.op) { fw.len += bw.len; bw.op = -1; }
    fw.flush();
    bw.flush();
}
#endif

}  // namespace bella
