// links.hpp -- the ends of two linked unitigs aligned against each other: true overlaps and CIGARs for the L lines, on gfx950
// (DESIGN.md section 26).
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h; the tests hold
// a numpy statement of it).  Everything is an integer, so the result is that statement's exactly.
//
// Pack.  k_lnk_pack writes, for every link that is aligned, two windows of 2-bit words: X, the last m bases of the oriented `from`
// unitig, and Y, the first n bases of the oriented `to` unitig -- reverse-complemented where the link's sign asks for it, so the DP
// and the walks see two forward sequences (dV = +1, comp = 0).  One thread per output word (unitig.hpp's gather splits its work the
// same way): a binary search over the windows' word offsets finds the window, 16 bases are gathered from the ASCII sequences.
//
// DP.  realign.hpp's kernels with another end: rows are Y, columns X, row 0 is 0 in every cell of the band (the start is free along
// `from`), and the end is the best cell of COLUMN m over the rows 0 .. n, ties to the smallest row (`to` starts at its first base,
// `from` ends at its last).  trace_row_tile is called as it stands with a TraceBest nobody reads; after every row the lane that holds
// column m proposes (score, i) -- rows ascend, so a lane keeps its first maximum --, and one wave reduction at the end takes the best
// proposal, ties to the smallest row.  Per row that is 2 C compares and selects on top of ~30 C instructions.
//
// Walks.  rea_walk from (i_end, m): k_lnk_count and k_lnk_write are k_rea_count and k_rea_write on a copy of the job whose n is i_end.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "realign.hpp"
#include "trace.hpp"

namespace bella {

constexpr uint32_t kLnkNone = 0xFFFFFFFFu;
constexpr uint32_t kLnkMaxBand = 4096;

// one window of the pack: `len` bases of the ASCII sequences from `src` on, forwards, or (rc) backwards and complemented
struct LnkWin {
    uint64_t src;          // the window's first base in the unitig's own direction
    uint32_t len;
    uint32_t rc;
};
struct LnkRes { int32_t score; int32_t i_end; };      // in the place of a ReaRes: the end is (i_end, m)
static_assert(sizeof(LnkRes) == sizeof(ReaRes), "a batch keeps either in one buffer");

// the proposal of one lane, and the rule between two: the larger score, then the smaller row
struct LnkEnd { int s; int i; };
BELLA_HD void lnk_end_take(LnkEnd& b, int s, int i) {
    if (s > b.s || (s == b.s && i < b.i)) { b.s = s; b.i = i; }
}

#if defined(__HIPCC__)
// woff[nwin + 1]: the windows' first words; one thread per word
__global__ void k_lnk_pack(const uint8_t* ascii, const LnkWin* wins, const uint64_t* woff, uint32_t nwin, uint64_t nwords, uint32_t* packed) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    uint32_t a = 0, b = nwin;                                         // the last window with woff <= w
    while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (woff[mid] <= w) a = mid; else b = mid;
    }
    const LnkWin win = wins[a];
    const uint64_t k0 = (w - woff[a]) * 16;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 16 && k0 + k < win.len; ++k) {
        const uint64_t t = k0 + k;
        const uint8_t ch = ascii[win.rc ? win.src + (win.len - 1 - t) : win.src + t];
        const uint32_t code = ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u;
        v |= (win.rc ? code ^ 3u : code) << (2 * k);
    }
    packed[w] = v;
}

__device__ __forceinline__ void lnk_end_reduce(LnkEnd& b) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int s = __shfl_xor(b.s, d, 64), i = __shfl_xor(b.i, d, 64);
        lnk_end_take(b, s, i);
    }
}

// band of 64 * C diagonals in registers; wavefront w runs jobs[w] (k_rea_dp's sweep; the end is a cell of column m)
template <int C>
__global__ __launch_bounds__(kTraceBlock) void k_lnk_dp(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, LnkRes* res) {
    using Word = typename TraceDirWord<C>::type;
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= njobs) return;                                           // (whole wavefronts leave)
    const int lane = (int)(threadIdx.x & 63);
    const ReaJob e = jobs[w];
    constexpr int B = 64 * C, half = B / 2;
    const int n = (int)e.n, m = e.m;
    const int p0 = lane * C;
    const int j0 = e.c + p0 - half;                                   // column of the lane's first cell in row 0
    int prev[C];
    uint32_t hwin = 0;
    LnkEnd end{kTrNeg, 0};
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = j0 + c;
        prev[c] = (j >= 0 && j <= m) ? 0 : kTrNeg;
        if (j == m) end = LnkEnd{0, 0};                               // row 0 proposes 0
        if (j >= 0 && j < m) hwin |= (uint32_t)trace_base(upacked, e.gH, 1, 0u, j) << (2 * c);
    }
    Word* const drow = (Word*)(dirs + e.dir_off) + lane;
    TraceBest unused{kTrNeg, 0, 0};
    uint32_t vw = 0;
    int64_t vwi = -1;
    for (int i = 1; i <= n; ++i) {
        const int64_t gv = e.gV + (int64_t)(i - 1);
        if ((gv >> 4) != vwi) { vwi = gv >> 4; vw = rpacked[vwi]; }
        const int vb = (int)((vw >> ((uint32_t)(gv & 15) * 2)) & 3u);
        int upn = __shfl_down(prev[0], 1, 64);
        if (lane == 63) upn = kTrNeg;
        int carry = kTrNeg;
        const uint32_t bits = trace_row_tile<C>(prev, upn, hwin, vb, i + j0, m, p0, carry, i, unused);
        drow[(size_t)(i - 1) * 64] = (Word)bits;
        const int cm = m - i - j0;                                    // the lane's cell that is column m in this row, if 0 <= cm < C
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == cm && prev[c] > end.s) end = LnkEnd{prev[c], i};
        const int t = i + j0 + C - 1;                                 // the column j - 1 of the lane's last cell in row i + 1
        uint32_t nbase = 0;
        if (t >= 0 && t < m) nbase = (uint32_t)trace_base(upacked, e.gH, 1, 0u, t);
        hwin = (C == 16 ? (hwin >> 2) : ((hwin >> 2) & ((1u << (2 * (C - 1))) - 1u))) | (nbase << (2 * (C - 1)));
    }
    lnk_end_reduce(end);
    if (lane == 0) res[w] = LnkRes{end.s, end.i};
}

// any band: k_rea_dp_wide's shape and invariant (tiles of 256 cells, the previous row in global scratch, one wavefront per block)
__global__ __launch_bounds__(64) void k_lnk_dp_wide(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, int* scratch,
                                                    LnkRes* res) {
    const uint32_t w = blockIdx.x;
    if (w >= njobs) return;
    const int lane = (int)threadIdx.x;
    const ReaJob e = jobs[w];
    const int B = (int)e.band, half = B / 2;
    const int n = (int)e.n, m = e.m;
    int* bufP = scratch + e.scr_off;
    int* bufC = bufP + B;
    LnkEnd end{kTrNeg, 0};
    for (int p = lane; p < B; p += 64) {
        const int j = e.c + p - half;
        bufP[p] = (j >= 0 && j <= m) ? 0 : kTrNeg;
        if (j == m) end = LnkEnd{0, 0};
    }
    __syncthreads();
    TraceBest unused{kTrNeg, 0, 0};
    uint8_t* const dbase = dirs + e.dir_off;
    const size_t rowbytes = (size_t)B / 4;
    for (int i = 1; i <= n; ++i) {
        const int vb = trace_base(rpacked, e.gV, 1, 0u, i - 1);
        const int org = i + e.c - half;                               // column of position 0 in this row
        const int plo = -org > 0 ? -org : 0;                          // positions of the columns 0 .. m
        const int phi = m - org < B - 1 ? m - org : B - 1;
        int carry = kTrNeg;
        if (plo <= phi) {
            for (int t = plo >> 8; t <= (phi >> 8); ++t) {
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
                    if (tt >= 0 && tt < m) hwin |= (uint32_t)trace_base(upacked, e.gH, 1, 0u, tt) << (2 * c);
                }
                const uint32_t bits = trace_row_tile<4>(prev, upn, hwin, vb, jb, m, p0, carry, i, unused);
                *(int4*)(bufC + p0) = make_int4(prev[0], prev[1], prev[2], prev[3]);
                dbase[(size_t)(i - 1) * rowbytes + (size_t)(p0 >> 2)] = (uint8_t)bits;
                const int cm = m - jb;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c == cm && prev[c] > end.s) end = LnkEnd{prev[c], i};
            }
        }
        __syncthreads();                                              // the row is in memory before the next one reads it
        int* tmp = bufP; bufP = bufC; bufC = tmp;
    }
    lnk_end_reduce(end);
    if (lane == 0) res[w] = LnkRes{end.s, end.i};
}

// the counting walk from (i_end, m); a column m that no path reaches counts as touched
__global__ void k_lnk_count(const ReaJob* jobs, const LnkRes* res, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, const uint8_t* dirs, ReaCnt* out) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= njobs) return;
    ReaCnt o{};
    ReaJob e = jobs[x];
    const LnkRes r = res[x];
    if (r.score <= kReaNoEnd || r.i_end < 0 || r.i_end > (int)e.n) { o.touch = 1; out[x] = o; return; }
    e.n = (uint32_t)r.i_end;
    TraceRuns runs;
    int qb = 0;
    const bool t = rea_walk(e, ReaRes{r.score, e.m}, rpacked, upacked, dirs, qb, runs);
    o.nops = runs.nruns;
    o.n_eq = runs.cnt[0]; o.n_x = runs.cnt[1]; o.n_ins = runs.cnt[2]; o.n_del = runs.cnt[3];
    o.touch = t ? 1u : 0u;
    o.q_begin = qb;
    out[x] = o;
}

// one thread per link with runs: ops[op_off .. op_off + nops) in the order of `to`
__global__ void k_lnk_write(const ReaJob* jobs, const LnkRes* res, const ReaCnt* cnt, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, const uint8_t* dirs,
                            uint32_t* ops) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= njobs) return;
    ReaJob e = jobs[x];
    if (e.op_off == ~0ull) return;
    const LnkRes r = res[x];
    e.n = (uint32_t)r.i_end;
    TraceEmit bw{ops, (int64_t)(e.op_off + cnt[x].nops), -1};
    int qb = 0;
    rea_walk(e, ReaRes{r.score, e.m}, rpacked, upacked, dirs, qb, bw);
    bw.flush();
}
#endif

}  // namespace bella
