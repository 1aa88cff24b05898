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
// DP.  band.hpp's sweep on realign.hpp's problem, forwards only, with another end: rows are Y, columns X, row 0
// is 0 in every cell of the band (the start is free along `from`), and the end is the best cell of COLUMN m over the rows 0 .. n, ties
// to the smallest row (`to` starts at its first base, `from` ends at its last).  LnkEnd carries a TraceBest nobody reads; after every
// row the lane that holds column m proposes (score, i) -- rows ascend, so a lane keeps its first maximum --, and one wave reduction at
// the end takes the best proposal, ties to the smallest row.  Per row that is 2 C compares and selects on top of ~30 C instructions.
//
// Walks.  k_rea_count and k_rea_write on a LnkRes: from (i_end, m).
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

#if defined(__HIPCC__)
// the end rule: the proposal of one lane, and the rule between two -- the larger score, then the smaller row
struct LnkEnd {
    TraceBest best{kTrNeg, 0, 0};                                     // (trace_row_tile's; unread)
    int s = kTrNeg, i = 0;
    __device__ __forceinline__ void take(int s2, int i2) {
        if (s2 > s || (s2 == s && i2 < i)) { s = s2; i = i2; }
    }
    __device__ __forceinline__ void row0(int, int j, int m) { if (j == m) { s = 0; i = 0; } }
    __device__ __forceinline__ void before_row(int, int) {}
    template <int C> __device__ __forceinline__ void after_row(const int (&prev)[C], int cm, int row) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == cm && prev[c] > s) { s = prev[c]; i = row; }
    }
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) take(__shfl_xor(s, d, 64), __shfl_xor(i, d, 64));
    }
    __device__ __forceinline__ LnkRes res() const { return LnkRes{s, i}; }
};
using LnkProblem = ReaProblemT<LnkEnd, true>;

// the walk starts in (i_end, m)
__device__ __forceinline__ bool rea_start(const ReaJob& e, const LnkRes& r, int& i, int& j) {
    i = r.i_end; j = e.m;
    return r.i_end >= 0 && r.i_end <= (int)e.n;
}

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
        const uint32_t code = base_code(ascii[win.rc ? win.src + (win.len - 1 - t) : win.src + t]);
        v |= (win.rc ? code ^ 3u : code) << (2 * k);
    }
    packed[w] = v;
}

// band of 64 * C diagonals in registers; wavefront w runs jobs[w]
template <int C>
__global__ __launch_bounds__(kTraceBlock) void k_lnk_dp(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, LnkRes* res) {
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= njobs) return;                                           // (whole wavefronts leave)
    const ReaJob e = jobs[w];
    const LnkEnd end = band_sweep<C>(LnkProblem{e, rpacked, upacked}, dirs);
    if ((threadIdx.x & 63) == 0) res[w] = end.res();
}

// any band; one wavefront per block
__global__ __launch_bounds__(64) void k_lnk_dp_wide(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, int* scratch,
                                                    LnkRes* res) {
    const uint32_t w = blockIdx.x;
    if (w >= njobs) return;
    const ReaJob e = jobs[w];
    const LnkEnd end = band_sweep_wide(LnkProblem{e, rpacked, upacked}, dirs, scratch);
    if (threadIdx.x == 0) res[w] = end.res();
}

struct LnkFamily {               // ReaFamily's sibling: the runs of links do not vote
    using Res = LnkRes;
    static constexpr bool votes = false;
    template <int C> static constexpr auto dp() { return k_lnk_dp<C>; }
    static constexpr auto dp_wide() { return k_lnk_dp_wide; }
};
#endif

}  // namespace bella
