// band.hpp -- the banded, direction-storing alignment sweep and its backtrace, written once for the families that use it on
// gfx950: trace.hpp, realign.hpp (sections 18 to 20), links.hpp (section 26) and pairalign.hpp (section 28).
// DESIGN.md section 27.
//
// The DP.  Rows i = 0 .. n are bases of V, columns j = 0 .. m bases of H; match +1, mismatch -1, gap -1 linear (the X-drop's
// scoring).  A band of B diagonals around the centre diagonal c is computed: position p of row i is column j = i + c + p - B/2.
//
// Mapping.  One wavefront per alignment, the band of B = 64 * C cells across the lanes, lane L owning the C adjacent positions
// p = L*C .. L*C + C-1, scores in VGPRs.  The sweep is row by row: with a linear gap the dependence inside a row is
//     S[i][j] = max_{j' <= j} (cand[j'] + j') - j,        cand = max(diagonal + sub, up - 1)
// i.e. ONE prefix maximum over the band per row: C - 1 dependent maxima inside the lane and a 6-step scan over the wave.  The
// anti-diagonal sweep (the shape of the X-drop kernels) has no scan but needs both neighbours from the two previous anti-diagonals and
// 2 (n + m) steps instead of n: twice the steps, and in each step half the band's cells belong to the other parity.  With B >= 256 the
// row sweep's scan (12 cross-lane operations) is a small part of a row's ~30 * C VALU instructions, so the row sweep it is.
// In band coordinates the diagonal neighbour of (i, p) is (i-1, p) and the upper one (i-1, p+1): a row needs ONE value from the next
// lane.  The bases of H slide one position per row through a 2-bit-per-base register window; the base of V is wave-uniform.
// Directions: 2 bits per cell (0 diagonal, 1 up = consumes V, 2 left = consumes H), byte p/4 of the row, rows of B/4 bytes: a lane
// stores its C cells as one u8 / u16 / u32 -- a wave writes 64 / 128 / 256 contiguous bytes per row with ordinary vector stores.
// Bands above 1,024 cells run band_sweep_wide: the same row code on tiles of 256 cells, the previous row in a global scratch of
// 2 * B ints per alignment, one wavefront per block.
//
// INVARIANT the wide sweep leans on: the second scratch row starts uninitialised, and a row only computes (and stores direction bytes
// for) the tiles that hold a column 0 .. m.  What lies outside is never USED: trace_row_tile masks every neighbour by the column it
// stands for (cd needs 1 <= j <= m, cu needs 0 <= j <= m, and those cells were computed by the row before), and the walk only visits
// cells of the rectangle.  Do not read prev[] or a direction byte without that mask.
//
// What a family brings.  A PROBLEM: a small struct of accessors over its job --
//     m()  rows(B)  centre()  row0(j)            columns, rows the band of B holds, centre diagonal, the score of cell (0, j)
//     h(t)                                       base t of H
//     vpack()  vidx(t)  vcomp()                  the pack that holds V, the index of V's base t in it, its complement mask
//     dir_off()  scr_off()  band()               bytes into the direction buffer, ints into the scratch, B
//     anchored                                   the path starts in (0, 0) (else anywhere in row 0)
//     touch_row0                                 anchored only: a cell of row 0 on the band's first or last diagonal counts as touched
//     End                                        its end rule
// and an END RULE, which owns what the sweep reports: a TraceBest `best` that trace_row_tile keeps (the best cell so far, ties to the
// smallest i + j, then the smallest i) and four hooks --
//     row0(s, j, m)                              at a cell (0, j) of the rectangle, its score s
//     before_row(i, rows)
//     after_row(prev, cm, i)                     prev[] = S[i] at the lane's cells; cell cm is column m, if 0 <= cm < C
//     reduce()                                   over the wave
// The backtrace is one thread per alignment (a serial pointer chase): band_walk hands every op to `put`, far end first.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "core.hpp"

namespace bella {

constexpr int kTrNeg = -(1 << 28);
enum { kOpEq = 0, kOpX = 1, kOpIns = 2, kOpDel = 3 };

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

constexpr int kTraceBlock = 256;      // the register kernels' block: four independent wavefronts

template <class Problem>
__device__ __forceinline__ int band_v(const Problem& P, int64_t t) {         // base t of V
    const int64_t g = P.vidx(t);
    return (int)(((P.vpack()[g >> 4] >> ((uint32_t)(g & 15) * 2)) & 3u) ^ P.vcomp());
}

// The register sweep: the calling wavefront runs problem P with a band of 64 * C cells.  Returns the end rule, reduced.
template <int C, class Problem>
__device__ __forceinline__ typename Problem::End band_sweep(const Problem& P, uint8_t* dirs) {
    using Word = typename TraceDirWord<C>::type;
    constexpr int B = 64 * C, half = B / 2;
    const int lane = (int)(threadIdx.x & 63);
    const int m = P.m(), rows = P.rows((uint32_t)B);
    const int p0 = lane * C;
    const int j0 = P.centre() + p0 - half;                            // column of the lane's first cell in row 0
    int prev[C];
    typename Problem::End end;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = j0 + c;
        const bool valid = j >= 0 && j <= m;
        prev[c] = valid ? P.row0(j) : kTrNeg;
        if (valid) end.row0(prev[c], j, m);
    }
    // the lane's bases of H for row 1: cell c is column j0 + c + 1, its base h[j0 + c]
    uint32_t hwin = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int t = j0 + c;
        if (t >= 0 && t < m) hwin |= (uint32_t)P.h(t) << (2 * c);
    }
    Word* const drow = (Word*)(dirs + P.dir_off()) + lane;
    const uint32_t* const vpack = P.vpack();
    uint32_t vw = 0;
    int64_t vwi = -1;
    for (int i = 1; i <= rows; ++i) {
        const int64_t gv = P.vidx(i - 1);
        if ((gv >> 4) != vwi) { vwi = gv >> 4; vw = vpack[vwi]; }
        const int vb = (int)(((vw >> ((uint32_t)(gv & 15) * 2)) & 3u) ^ P.vcomp());
        int upn = __shfl_down(prev[0], 1, 64);
        if (lane == 63) upn = kTrNeg;
        int carry = kTrNeg;
        const int jb = i + p0 - half + P.centre();                    // (i + p0 first: with the centre a constant 0 the compiler sees two non-negative terms and folds the column tests)
        end.before_row(i, rows);
        const uint32_t bits = trace_row_tile<C>(prev, upn, hwin, vb, jb, m, p0, carry, i, end.best);
        drow[(size_t)(i - 1) * 64] = (Word)bits;
        end.after_row(prev, m - jb, i);
        const int t = jb + C - 1;                                     // slide the window: the column j - 1 of the lane's last cell in row i + 1
        uint32_t nb = 0;
        if (t >= 0 && t < m) nb = (uint32_t)P.h(t);
        hwin = (C == 16 ? (hwin >> 2) : ((hwin >> 2) & ((1u << (2 * (C - 1))) - 1u))) | (nb << (2 * (C - 1)));
    }
    end.reduce();
    return end;
}

// The tiled sweep, any band: the calling block (one wavefront) runs problem P on tiles of 256 cells, the previous row in P's two
// scratch rows of B ints, swapped per row.  See the INVARIANT above.
template <class Problem>
__device__ __forceinline__ typename Problem::End band_sweep_wide(const Problem& P, uint8_t* dirs, int* scratch) {
    const int lane = (int)threadIdx.x;
    const int B = (int)P.band(), half = B / 2;
    const int m = P.m(), rows = P.rows(P.band());
    int* bufP = scratch + P.scr_off();
    int* bufC = bufP + B;
    typename Problem::End end;
    for (int p = lane; p < B; p += 64) {
        const int j = P.centre() + p - half;
        const bool valid = j >= 0 && j <= m;
        const int s = valid ? P.row0(j) : kTrNeg;
        bufP[p] = s;
        if (valid) end.row0(s, j, m);
    }
    __syncthreads();
    uint8_t* const dbase = dirs + P.dir_off();
    const size_t rowbytes = (size_t)B / 4;
    for (int i = 1; i <= rows; ++i) {
        const int vb = band_v(P, i - 1);
        const int org = i + P.centre() - half;                        // column of position 0 in this row
        const int plo = -org > 0 ? -org : 0;                          // positions of the columns 0 .. m (plo > phi: none)
        const int phi = m - org < B - 1 ? m - org : B - 1;
        int carry = kTrNeg;
        end.before_row(i, rows);
        for (int t = plo >> 8; plo <= phi && t <= (phi >> 8); ++t) {
            const int p0 = t * 256 + lane * 4;
            int prev[4];
            const int4 q = *(const int4*)(bufP + p0);
            prev[0] = q.x; prev[1] = q.y; prev[2] = q.z; prev[3] = q.w;
            const int upn = p0 + 4 < B ? bufP[p0 + 4] : kTrNeg;
            const int jb = org + p0;
            uint32_t hwin = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int tt = jb + c - 1;
                if (tt >= 0 && tt < m) hwin |= (uint32_t)P.h(tt) << (2 * c);
            }
            const uint32_t bits = trace_row_tile<4>(prev, upn, hwin, vb, jb, m, p0, carry, i, end.best);
            *(int4*)(bufC + p0) = make_int4(prev[0], prev[1], prev[2], prev[3]);
            dbase[(size_t)(i - 1) * rowbytes + (size_t)(p0 >> 2)] = (uint8_t)bits;
            end.after_row(prev, m - jb, i);
        }
        __syncthreads();                                              // the row is in memory before the next one reads it
        int* tmp = bufP; bufP = bufC; bufC = tmp;
    }
    end.reduce();
    return end;
}

// Walks P back from (i, j) -- to (0, 0) if P is anchored, else to row 0 -- and hands every op to `put` (far end first).  Returns
// whether the path touched the first or the last diagonal of the band (in row 0 only where P says touch_row0); j = the column it
// stopped in.
template <class Problem, class Put>
__device__ __forceinline__ bool band_walk(const Problem& P, const uint8_t* dirs, int i, int& j, Put&& put) {
    const int B = (int)P.band(), half = B / 2, c = P.centre();
    const uint8_t* const d0 = dirs + P.dir_off();
    const size_t rowbytes = (size_t)B / 4;
    bool touch = false;
    while (i > 0 || (Problem::anchored && j > 0)) {
        int p = j - i - c + half;
        if (p <= 0 || p >= B - 1) { touch = touch || i > 0 || Problem::touch_row0; p = p < 0 ? 0 : (p > B - 1 ? B - 1 : p); }      // (a path never leaves the band; the clamp keeps a read in bounds whatever the bytes say)
        uint32_t d = 2;
        if (i > 0) {
            d = j <= 0 ? 1u : (uint32_t)((d0[(size_t)(i - 1) * rowbytes + (size_t)(p >> 2)] >> (2 * (p & 3))) & 3u);
            if (d == 3) d = 2;
        }
        if (d == 0) {
            put(P.h(j - 1) == band_v(P, i - 1) ? kOpEq : kOpX);
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

// ---- affine gaps ----------------------------------------------------------------------------------------------
// Gotoh's three matrices under scores the caller chooses: match +a, mismatch -b, a gap of L bases -(o + e L).
//     E[i][q] = max(H[i-1][q] - o - e, E[i-1][q] - e)        H[i][q] = max(H[i-1][q-1] + s, E[i][q], F[i][q])
//     F[i][q] = max(H[i][q-1] - o - e, F[i][q-1] - e)  =  max_{q' < q} (Hc[q'] + e q') - o - e q,   Hc = max(diagonal, E)
// (a gap that opens out of F pays o twice and never wins): still ONE prefix maximum per row, now exclusive, over Hc + e p.  A lane keeps
// H and E of the previous row in registers; E needs both from the upper neighbour, one __shfl_down each.  Per cell 4 direction bits:
// bits 0-1 the first of diagonal (0), E (1), F (2) that attains H; bit 2 H - o >= E; bit 3 H - o >= F -- a gap that arrives at this cell
// from below (bit 2) or from the right (bit 3) was opened here, ties to opening.  Nibble p & 1 of byte p / 2, rows of B / 2 bytes.
// INVARIANT, extended: the wide sweep's second scratch rows of H and of E start uninitialised, and what lies outside the columns 0 .. m is
// never used -- affine_row_tile masks cd, and the two terms of E, by the column they stand for.
struct AfnScore { int a, b, o, e; };              // wave-uniform: a kernel argument

// One row of one tile of 64 * C cells: prev / eprev = H[i-1] / E[i-1] at the lane's positions, upn / eupn = the same at the next lane's
// first position; carry = prefix maximum of Hc + e * position over the tiles before this one.  Leaves H[i], E[i] in prev, eprev and
// returns the 4C direction bits.  The other arguments are trace_row_tile's.
template <int C>
__device__ __forceinline__ uint64_t affine_row_tile(int (&prev)[C], int (&eprev)[C], int upn, int eupn, uint32_t hwin, int vb, int jb, int m, int p0, int& carry, int i,
                                                    TraceBest& best, const AfnScore sc) {
    const int lane = (int)(threadIdx.x & 63);
    const int oe = sc.o + sc.e;
    int cd[C], en[C], loc[C];
    int run = kTrNeg;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = jb + c;
        const bool valid = j >= 0 && j <= m;
        const int sub = ((int)((hwin >> (2 * c)) & 3u) == vb) ? sc.a : -sc.b;
        const int up = c + 1 < C ? prev[c + 1] : upn;
        const int eup = c + 1 < C ? eprev[c + 1] : eupn;
        cd[c] = (j >= 1 && valid) ? prev[c] + sub : kTrNeg;           // (i-1, j-1)
        const int eo = up - oe, ee = eup - sc.e;                      // (i-1, j): the gap opens, the gap goes on
        int e = eo > ee ? eo : ee;
        if (!valid || e < kTrNeg) e = kTrNeg;
        en[c] = e;
        loc[c] = run;                                                 // exclusive: the cells of the lane before this one
        const int hc = cd[c] > e ? cd[c] : e;
        const int t = hc + sc.e * (p0 + c);
        run = t > run ? t : run;
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
    uint64_t bits = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = jb + c;
        const bool valid = j >= 0 && j <= m;
        const int mx = loc[c] > ex ? loc[c] : ex;
        int f = mx - sc.o - sc.e * (p0 + c);
        if (!valid || f < kTrNeg) f = kTrNeg;
        const int hc = cd[c] > en[c] ? cd[c] : en[c];
        int s = hc > f ? hc : f;
        if (!valid) s = kTrNeg;
        const uint32_t d = (s == cd[c] ? 0u : (s == en[c] ? 1u : 2u)) | (s - sc.o >= en[c] ? 4u : 0u) | (s - sc.o >= f ? 8u : 0u);
        bits |= (uint64_t)d << (4 * c);
        if (valid) trace_best_take(best, s, i + j, i);
        prev[c] = s;
        eprev[c] = en[c];
    }
    return bits;
}

template <int C> struct AffineDirWord;
template <> struct AffineDirWord<4> { using type = uint16_t; };
template <> struct AffineDirWord<8> { using type = uint32_t; };
template <> struct AffineDirWord<16> { using type = uint64_t; };

// The register sweep, affine: band_sweep's shape with two register rows and direction words twice as wide.
template <int C, class Problem>
__device__ __forceinline__ typename Problem::End band_sweep_affine(const Problem& P, uint8_t* dirs, const AfnScore sc) {
    using Word = typename AffineDirWord<C>::type;
    constexpr int B = 64 * C, half = B / 2;
    const int lane = (int)(threadIdx.x & 63);
    const int m = P.m(), rows = P.rows((uint32_t)B);
    const int p0 = lane * C;
    const int j0 = P.centre() + p0 - half;                            // column of the lane's first cell in row 0
    int prev[C], eprev[C];
    typename Problem::End end;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = j0 + c;
        const bool valid = j >= 0 && j <= m;
        prev[c] = valid ? P.row0(j) : kTrNeg;
        eprev[c] = kTrNeg;                                            // E[0][.] is minus infinity in every mode
        if (valid) end.row0(prev[c], j, m);
    }
    uint32_t hwin = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int t = j0 + c;
        if (t >= 0 && t < m) hwin |= (uint32_t)P.h(t) << (2 * c);
    }
    Word* const drow = (Word*)(dirs + P.dir_off()) + lane;
    const uint32_t* const vpack = P.vpack();
    uint32_t vw = 0;
    int64_t vwi = -1;
    for (int i = 1; i <= rows; ++i) {
        const int64_t gv = P.vidx(i - 1);
        if ((gv >> 4) != vwi) { vwi = gv >> 4; vw = vpack[vwi]; }
        const int vb = (int)(((vw >> ((uint32_t)(gv & 15) * 2)) & 3u) ^ P.vcomp());
        int upn = __shfl_down(prev[0], 1, 64), eupn = __shfl_down(eprev[0], 1, 64);
        if (lane == 63) { upn = kTrNeg; eupn = kTrNeg; }
        int carry = kTrNeg;
        const int jb = i + p0 - half + P.centre();
        end.before_row(i, rows);
        const uint64_t bits = affine_row_tile<C>(prev, eprev, upn, eupn, hwin, vb, jb, m, p0, carry, i, end.best, sc);
        drow[(size_t)(i - 1) * 64] = (Word)bits;
        end.after_row(prev, m - jb, i);
        const int t = jb + C - 1;                                     // slide the window, as band_sweep does
        uint32_t nb = 0;
        if (t >= 0 && t < m) nb = (uint32_t)P.h(t);
        hwin = (C == 16 ? (hwin >> 2) : ((hwin >> 2) & ((1u << (2 * (C - 1))) - 1u))) | (nb << (2 * (C - 1)));
    }
    end.reduce();
    return end;
}

// The tiled sweep, affine, any band: the previous rows of H and of E in P's scratch of 4 * B ints (H, H, E, E), swapped per row.  See
// the INVARIANT above.
template <class Problem>
__device__ __forceinline__ typename Problem::End band_sweep_affine_wide(const Problem& P, uint8_t* dirs, int* scratch, const AfnScore sc) {
    const int lane = (int)threadIdx.x;
    const int B = (int)P.band(), half = B / 2;
    const int m = P.m(), rows = P.rows(P.band());
    int* bufP = scratch + P.scr_off();
    int* bufC = bufP + B;
    int* ebufP = bufC + B;
    int* ebufC = ebufP + B;
    typename Problem::End end;
    for (int p = lane; p < B; p += 64) {
        const int j = P.centre() + p - half;
        const bool valid = j >= 0 && j <= m;
        const int s = valid ? P.row0(j) : kTrNeg;
        bufP[p] = s;
        ebufP[p] = kTrNeg;
        if (valid) end.row0(s, j, m);
    }
    __syncthreads();
    uint8_t* const dbase = dirs + P.dir_off();
    const size_t rowbytes = (size_t)B / 2;
    for (int i = 1; i <= rows; ++i) {
        const int vb = band_v(P, i - 1);
        const int org = i + P.centre() - half;                        // column of position 0 in this row
        const int plo = -org > 0 ? -org : 0;                          // positions of the columns 0 .. m (plo > phi: none)
        const int phi = m - org < B - 1 ? m - org : B - 1;
        int carry = kTrNeg;
        end.before_row(i, rows);
        for (int t = plo >> 8; plo <= phi && t <= (phi >> 8); ++t) {
            const int p0 = t * 256 + lane * 4;
            int prev[4], eprev[4];
            const int4 q = *(const int4*)(bufP + p0), qe = *(const int4*)(ebufP + p0);
            prev[0] = q.x; prev[1] = q.y; prev[2] = q.z; prev[3] = q.w;
            eprev[0] = qe.x; eprev[1] = qe.y; eprev[2] = qe.z; eprev[3] = qe.w;
            const int upn = p0 + 4 < B ? bufP[p0 + 4] : kTrNeg;
            const int eupn = p0 + 4 < B ? ebufP[p0 + 4] : kTrNeg;
            const int jb = org + p0;
            uint32_t hwin = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int tt = jb + c - 1;
                if (tt >= 0 && tt < m) hwin |= (uint32_t)P.h(tt) << (2 * c);
            }
            const uint64_t bits = affine_row_tile<4>(prev, eprev, upn, eupn, hwin, vb, jb, m, p0, carry, i, end.best, sc);
            *(int4*)(bufC + p0) = make_int4(prev[0], prev[1], prev[2], prev[3]);
            *(int4*)(ebufC + p0) = make_int4(eprev[0], eprev[1], eprev[2], eprev[3]);
            *(uint16_t*)(dbase + (size_t)(i - 1) * rowbytes + (size_t)(p0 >> 1)) = (uint16_t)bits;
            end.after_row(prev, m - jb, i);
        }
        __syncthreads();                                              // the row is in memory before the next one reads it
        int* tmp = bufP; bufP = bufC; bufC = tmp;
        tmp = ebufP; ebufP = ebufC; ebufC = tmp;
    }
    end.reduce();
    return end;
}

// band_walk over the 4-bit directions: a walk with a state in {H (0), E (1), F (2)}, from (i, j) in H.  In H the cell's source moves
// diagonally or enters a gap without moving; in E an 'I' goes up, in F a 'D' goes left, and the gap ends in the cell it arrives at when
// that cell's close bit is set.  Row 0 (anchored) is 'D' leftwards and column 0 'I' upwards whatever the state.  Clamp, touch and the
// returned column are band_walk's.
template <class Problem, class Put>
__device__ __forceinline__ bool band_walk_affine(const Problem& P, const uint8_t* dirs, int i, int& j, Put&& put) {
    const int B = (int)P.band(), half = B / 2, c = P.centre();
    const uint8_t* const d0 = dirs + P.dir_off();
    const size_t rowbytes = (size_t)B / 2;
    bool touch = false;
    uint32_t state = 0;
    while (i > 0 || (Problem::anchored && j > 0)) {
        int p = j - i - c + half;
        if (p <= 0 || p >= B - 1) { touch = touch || i > 0 || Problem::touch_row0; p = p < 0 ? 0 : (p > B - 1 ? B - 1 : p); }      // (the clamp keeps a read in bounds whatever the bytes say)
        if (i == 0) { put(kOpDel); --j; continue; }
        if (j <= 0) { put(kOpIns); --i; continue; }
        const uint32_t w = (uint32_t)(d0[(size_t)(i - 1) * rowbytes + (size_t)(p >> 1)] >> (4 * (p & 1))) & 15u;
        if ((state == 1 && (w & 4u)) || (state == 2 && (w & 8u))) state = 0;            // the gap that arrived here was opened here
        if (state == 0) {
            state = (w & 3u) == 3u ? 2u : (w & 3u);
            if (state == 0) {
                put(P.h(j - 1) == band_v(P, i - 1) ? kOpEq : kOpX);
                --i; --j;
                continue;
            }
        }
        if (state == 1) { put(kOpIns); --i; }
        else { put(kOpDel); --j; }
    }
    return touch;
}
#endif

}  // namespace bella
