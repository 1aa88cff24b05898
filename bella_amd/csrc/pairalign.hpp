// pairalign.hpp -- caller-supplied pairs of sequences aligned on the device: global, semi-global or dovetail, with their runs, on gfx950
// (DESIGN.md section 28).
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h; the tests hold
// a numpy statement of it).  Everything is an integer, so the result is that statement's exactly.
//
// Pack.  links.hpp's k_lnk_pack over the caller's ASCII: one window per (sequence, reverse-complemented or not) that a pair uses, each
// packed once however many pairs name it.  The DP and the walks see two forward sequences (dV = +1, comp = 0).
//
// DP.  band.hpp's sweep on realign.hpp's problem: rows are the query Q, columns the target T.  Three end rules:
//   global       row 0 is -q, the path starts in (0, 0) (the anchored ReaProblemT), and the end is the cell (n, m): GlbEnd -- after the
//                last row the lane that holds column m proposes its score, one wave reduction follows.  Per row that is one scalar
//                compare on top of the sweep;
//   semi-global  row 0 is 0, the end is the best cell of row n: realign.hpp's ReaEnd;
//   dovetail     row 0 is 0, the end is the best cell of column m: links.hpp's LnkEnd, and its kernels as they are.
//
// Walks.  k_rea_count and k_rea_write on the family's result; the global one walks the anchored problem, from (n, m) back to (0, 0).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "links.hpp"
#include "realign.hpp"

namespace bella {

constexpr uint32_t kPalMaxBand = BELLA_ALIGN_MAX_BAND;
constexpr uint64_t kPalMaxSeq = 1ull << 30;          // bases of one sequence: BAD_ARG from here on
constexpr uint64_t kPalMaxCells = 1ull << 27;        // n + m of one pair: every score stays far above the sweep's minus infinity (kTrNeg / 2)

struct GlbRes { int32_t score; int32_t pad; };        // in the place of a ReaRes: the end is (n, m)
static_assert(sizeof(GlbRes) == sizeof(ReaRes), "a batch keeps either in one buffer");

#if defined(__HIPCC__)
// the end rule: the score of the cell (n, m), kTrNeg when the band does not hold it
struct GlbEnd {
    TraceBest best{kTrNeg, 0, 0};                                     // (trace_row_tile's; unread)
    int s = kTrNeg;
    bool last = false;
    __device__ __forceinline__ void row0(int, int, int) {}
    __device__ __forceinline__ void before_row(int i, int rows) { last = i == rows; }
    template <int C> __device__ __forceinline__ void after_row(const int (&prev)[C], int cm, int) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (last && c == cm) s = prev[c];
    }
    __device__ __forceinline__ void reduce() {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_xor(s, d, 64); s = t > s ? t : s; }
    }
    __device__ __forceinline__ GlbRes res() const { return GlbRes{s, 0}; }
};
using GlbProblem = ReaProblemT<GlbEnd, true, true>;
using SemiProblem = ReaProblemT<ReaEnd, true>;                        // realign.hpp's alignment with V known to run forwards
template <> struct ReaWalkOf<GlbRes> { using type = GlbProblem; };

// the walk starts in (n, m)
__device__ __forceinline__ bool rea_start(const ReaJob& e, const GlbRes&, int& i, int& j) {
    i = (int)e.n; j = e.m;
    return true;
}

// band of 64 * C diagonals in registers; wavefront w runs jobs[w]
template <int C, class Problem, class Res>
__global__ __launch_bounds__(kTraceBlock) void k_pal_dp(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, Res* res) {
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= njobs) return;                                           // (whole wavefronts leave)
    const ReaJob e = jobs[w];
    const typename Problem::End end = band_sweep<C>(Problem{e, rpacked, upacked}, dirs);
    if ((threadIdx.x & 63) == 0) res[w] = end.res();
}

// any band; one wavefront per block
template <class Problem, class Res>
__global__ __launch_bounds__(64) void k_pal_dp_wide(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, int* scratch, Res* res) {
    const uint32_t w = blockIdx.x;
    if (w >= njobs) return;
    const ReaJob e = jobs[w];
    const typename Problem::End end = band_sweep_wide(Problem{e, rpacked, upacked}, dirs, scratch);
    if (threadIdx.x == 0) res[w] = end.res();
}

template <class Problem, class ResT>
struct PalFamily {               // LnkFamily's sibling (the dovetail runs as an LnkFamily): the runs do not vote
    using Res = ResT;
    static constexpr bool votes = false;
    template <int C> static constexpr auto dp() { return k_pal_dp<C, Problem, ResT>; }
    static constexpr auto dp_wide() { return k_pal_dp_wide<Problem, ResT>; }
};
using PalGlobal = PalFamily<GlbProblem, GlbRes>;
using PalSemi = PalFamily<SemiProblem, ReaRes>;
using PalDovetail = LnkFamily;

// ---- affine gaps and the caller's scores -------------------------------------------------------------------------
// band.hpp's affine sweep and walk under the same three end rules, unedited: they see H.  Only the anchored row 0 knows the scores.
struct AfnGlbProblem : GlbProblem {
    AfnScore sc;
    __device__ __forceinline__ AfnGlbProblem(const ReaJob& e, const uint32_t* r, const uint32_t* u, const AfnScore& s) : GlbProblem{e, r, u}, sc(s) {}
    __device__ __forceinline__ int row0(int j) const { return j > 0 ? -(sc.o + sc.e * j) : 0; }          // H[0][q] = F[0][q]: one gap from (0, 0)
};
template <class Problem> __device__ __forceinline__ Problem afn_problem(const ReaJob& e, const uint32_t* r, const uint32_t* u, const AfnScore&) { return Problem{e, r, u}; }
template <> __device__ __forceinline__ AfnGlbProblem afn_problem<AfnGlbProblem>(const ReaJob& e, const uint32_t* r, const uint32_t* u, const AfnScore& s) {
    return AfnGlbProblem(e, r, u, s);
}

// band of 64 * C diagonals in registers; wavefront w runs jobs[w]
template <int C, class Problem, class Res>
__global__ __launch_bounds__(kTraceBlock) void k_pal_afn_dp(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, Res* res,
                                                            const AfnScore sc) {
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= njobs) return;                                           // (whole wavefronts leave)
    const ReaJob e = jobs[w];
    const typename Problem::End end = band_sweep_affine<C>(afn_problem<Problem>(e, rpacked, upacked, sc), dirs, sc);
    if ((threadIdx.x & 63) == 0) res[w] = end.res();
}

// any band; one wavefront per block
template <class Problem, class Res>
__global__ __launch_bounds__(64) void k_pal_afn_dp_wide(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, int* scratch, Res* res,
                                                        const AfnScore sc) {
    const uint32_t w = blockIdx.x;
    if (w >= njobs) return;
    const ReaJob e = jobs[w];
    const typename Problem::End end = band_sweep_affine_wide(afn_problem<Problem>(e, rpacked, upacked, sc), dirs, scratch, sc);
    if (threadIdx.x == 0) res[w] = end.res();
}

// k_rea_count and k_rea_write over band_walk_affine
template <class Res>
__global__ void k_afn_count(const ReaJob* jobs, const Res* res, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, const uint8_t* dirs, ReaCnt* out) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= njobs) return;
    ReaCnt o{};
    const ReaJob e = jobs[x];
    const Res r = res[x];
    int i, j;
    if (!rea_start(e, r, i, j) || r.score <= kReaNoEnd) { o.touch = 1; out[x] = o; return; }
    TraceRuns runs;
    const bool t = band_walk_affine(typename ReaWalkOf<Res>::type{e, rpacked, upacked}, dirs, i, j, runs);
    o.nops = runs.nruns;
    o.n_eq = runs.cnt[0]; o.n_x = runs.cnt[1]; o.n_ins = runs.cnt[2]; o.n_del = runs.cnt[3];
    o.touch = t ? 1u : 0u;
    o.q_begin = j;
    out[x] = o;
}

template <class Res>
__global__ void k_afn_write(const ReaJob* jobs, const Res* res, const ReaCnt* cnt, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, const uint8_t* dirs,
                            uint32_t* ops) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= njobs) return;
    const ReaJob e = jobs[x];
    if (e.op_off == ~0ull) return;
    TraceEmit bw{ops, (int64_t)(e.op_off + cnt[x].nops), -1};
    int i, j;
    rea_start(e, res[x], i, j);
    band_walk_affine(typename ReaWalkOf<Res>::type{e, rpacked, upacked}, dirs, i, j, bw);
    bw.flush();
}

// for the host (BandTraits in bella_hip.hip has the linear families' values): direction bits per cell, scratch ints per job and band
// cell, the walks; the DP kernels take the scores behind the linear ones' arguments
template <class Problem, class ResT>
struct PalAfnFamily {
    using Res = ResT;
    static constexpr bool votes = false, affine = true;
    static constexpr uint32_t dir_bits = 4, scr_ints = 4;
    template <int C> static constexpr auto dp() { return k_pal_afn_dp<C, Problem, ResT>; }
    static constexpr auto dp_wide() { return k_pal_afn_dp_wide<Problem, ResT>; }
    static constexpr auto count() { return k_afn_count<ResT>; }
    static constexpr auto write() { return k_afn_write<ResT>; }
};
using PalAfnGlobal = PalAfnFamily<AfnGlbProblem, GlbRes>;
using PalAfnSemi = PalAfnFamily<SemiProblem, ReaRes>;
using PalAfnDovetail = PalAfnFamily<LnkProblem, LnkRes>;
#endif

}  // namespace bella
