// realign.hpp -- every read aligned against the current sequence of its unitig, the votes piled up in unitig coordinates, on gfx950
// (DESIGN.md section 18).
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h; the tests hold
// a numpy statement of it).  Everything is an integer, so the result is that statement's exactly.
//
// Placement.  k_rea_backbone (one thread per vertex) gives every read its first vertex; k_rea_anchor (one thread per record) gives
// every contained read the record that joins it to a backbone read over the longest span -- one 64-bit atomicMax per candidate, the key
// span << 32 | ~index, so the choice does not depend on the order the threads run in; k_rea_place (one thread per read) turns vertex or
// record into the unitig, the orientation and the window [s, e) on the current sequence.
//
// DP.  band.hpp's sweep with ReaProblem and ReaEnd: row 0 is 0 in every cell of the band (the start is free
// along the unitig), the band's diagonals are q - i - c for the read's centre diagonal c, the rows are the read's clip in its orientation
// on the unitig (reversed and complemented for orientation 1) and the columns the 2-bit pack of the unitig's bases, and the end is the
// best cell of row n alone: the running best is cleared before the last row, so the tie rule of trace_best_take (smallest i + j) is
// the smallest q.  Per row that is one scalar compare more than k_trace_dp.
// The kernel is bound by VALU issue, as k_trace_dp is: ~30 C instructions per row against one C-byte store per lane.
//
// Walks.  One thread per read from (n, q_end) up to row 0: a counting walk (runs, op totals, whether the path touched the band's first
// or last diagonal, q_begin), and once the host has laid the runs out a writing walk, backwards from the read's last run.
// Votes.  One wavefront per read over its runs, pileup.hpp's mapping (64 runs per chunk, their columns dealt to the lanes): a column of
// '=' / 'X' votes the read's base at q, 'D' votes del at q, a run of 'I' one ins vote with its first base in the junction before q.
//
// Circles (opt-in).  k_rea_place may put a read of a circular unitig on the UNROLLED circle: the window's start
// taken modulo the raw length, the window moved on by plen when it begins in the first band_max / 2 bases, so no band leaves
// [0, 2 plen].  k_rea_pack_unrolled writes such a unitig's bases twice in a row; a ReaJob names the pack offset (gH), the table's row
// base (gT) and the modulus (mt) apart; the DP and the walks see a target of m = 2 plen columns, and k_rea_vote folds a column j >= mt
// back by one subtraction.  With the switch off none of this runs: gH = gT, mt = m.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "pileup.hpp"
#include "trace.hpp"

namespace bella {

constexpr uint32_t kReaNone = 0xFFFFFFFFu;
constexpr uint64_t kReaMaxUnitig = 1ull << 30;       // bases of one unitig: column indices stay far inside an int
constexpr uint64_t kReaMaxUnrolled = 1ull << 29;     // ... of one that is aligned against twice in a row (section 19)

// one read of a DP batch, filled by the host from the read's placement
struct ReaJob {
    int64_t gH;            // first base of the unitig in the 2-bit pack (the unrolled layout when the round unrolls circles: section 19)
    int64_t gV;            // base of the packed reads that is row 1
    uint64_t dir_off;      // bytes into the direction buffer: rows 1 .. n, B / 4 bytes each
    uint64_t scr_off;      // wide kernel: ints into the scratch (2 B per read)
    uint64_t op_off;       // first run in the batch's op array; ~0: the read does not vote
    uint32_t n;            // rows: bases of the clip
    int32_t m;             // columns: bases of the unitig
    int32_t c;             // centre diagonal
    uint32_t band;
    int32_t dV;            // +1, or -1 for orientation 1
    uint32_t comp;         // 3 for orientation 1
    int32_t mt;            // rows of the unitig in the table: a vote at column j >= mt goes to row j - mt (m: never; plen on the unrolled circle)
    int64_t gT;            // first row of the unitig in the table
};
struct ReaRes { int32_t score; int32_t q_end; };
struct ReaCnt { uint32_t nops, n_eq, n_x, n_ins, n_del, touch; int32_t q_begin; uint32_t pad; };

// raw unitig coordinate -> coordinate on the current sequence; segments [lo, hi) are the unitig's, len / plen its lengths
BELLA_HD int64_t rea_map(int64_t x, const uint64_t* pos, const uint32_t* nb, const uint64_t* cpos, const uint32_t* cnb, uint64_t lo, uint64_t hi, int64_t len, int64_t plen) {
    if (x < 0) return x;
    if (x >= len) return plen + (x - len);
    uint64_t a = lo, b = hi;                                          // the last segment with pos <= x
    while (b - a > 1) {
        const uint64_t mid = a + (b - a) / 2;
        if ((int64_t)pos[mid] <= x) a = mid; else b = mid;
    }
    if (!nb[a]) return (int64_t)cpos[a];
    return (int64_t)cpos[a] + (x - (int64_t)pos[a]) * (int64_t)cnb[a] / (int64_t)nb[a];
}

#if defined(__HIPCC__)
__global__ void k_rea_backbone(const uint32_t* verts, uint32_t nseg, uint32_t* bvert) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nseg) atomicMin(bvert + (verts[i] >> 1), i);
}

// key[c] = max over the records that join the contained read c to a backbone read of span on c << 32 | ~index (0: none)
__global__ void k_rea_anchor(const bella_overlap* recs, uint32_t nrec, const uint32_t* bvert, const uint8_t* contained, const uint8_t* removed, unsigned long long* key) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nrec) return;
    const bella_overlap r = recs[x];
    const unsigned long long low = (unsigned long long)(0xFFFFFFFFu - x);
    if (contained[r.cid] == 1 && !removed[r.cid] && bvert[r.cid] == kReaNone && bvert[r.rid] != kReaNone)
        atomicMax(key + r.cid, ((unsigned long long)(uint32_t)(r.endV - r.begV) << 32) | low);
    if (contained[r.rid] == 1 && !removed[r.rid] && bvert[r.rid] == kReaNone && bvert[r.cid] != kReaNone)
        atomicMax(key + r.rid, ((unsigned long long)(uint32_t)(r.endH - r.begH) << 32) | low);
}

// rbeg / rend: the reads' clips among all bases (whole reads: roff and roff + 1).  uoff: raw unitig offsets, coffs: current ones.
__global__ void k_rea_place(uint32_t nreads, const uint64_t* roff, const uint64_t* rbeg, const uint64_t* rend, const uint32_t* bvert, const unsigned long long* key,
                            const bella_overlap* recs, const uint8_t* contained, const uint8_t* removed, const uint32_t* verts, const uint32_t* slot_utg,
                            const uint64_t* pos, const uint32_t* nb, const uint64_t* cpos, const uint32_t* cnb, const uint64_t* uvoff, const uint64_t* uoff,
                            const uint64_t* coffs, uint32_t band0, const uint8_t* circular, uint32_t band_max, uint32_t unroll, bella_realign_placement* out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nreads) return;
    bella_realign_placement P{};
    P.unitig = kReaNone; P.anchor = kReaNone; P.status = BELLA_REALIGN_NONE;
    const int64_t L = (int64_t)(roff[r + 1] - roff[r]), beg = (int64_t)(rbeg[r] - roff[r]), end = (int64_t)(rend[r] - roff[r]);
    int64_t x0 = 0;
    uint32_t o = 0, u = kReaNone;
    if (bvert[r] != kReaNone) {
        const uint32_t i = bvert[r];
        o = verts[i] & 1u; u = slot_utg[i];
        x0 = (int64_t)pos[i] - (o ? L - end : beg);
    } else if (contained[r] == 1 && !removed[r]) {
        const unsigned long long k = key[r];
        if (!k) P.status = BELLA_REALIGN_UNPLACED;
        else {
            const uint32_t idx = 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull);
            const bella_overlap rec = recs[idx];
            const bool isV = rec.cid != r;                             // the backbone read is V
            const uint32_t b = isV ? rec.cid : rec.rid;
            const int64_t Lb = (int64_t)(roff[b + 1] - roff[b]), bb = (int64_t)(rbeg[b] - roff[b]), be = (int64_t)(rend[b] - roff[b]);
            int64_t d;
            uint32_t s;
            if (isV) { d = (int64_t)rec.begV - rec.begH; s = rec.strand; }             // H' = this read, in V's frame
            else if (!rec.strand) { d = (int64_t)rec.begH - rec.begV; s = 0; }         // V = this read, in the frame of H' = H
            else { d = Lb - ((int64_t)rec.begH - rec.begV) - L; s = 1; }               // ... of H' = rc(H): mirrored by H's length
            const uint32_t i = bvert[b], ob = verts[i] & 1u;
            const int64_t x0b = (int64_t)pos[i] - (ob ? Lb - be : bb);
            u = slot_utg[i];
            x0 = ob ? x0b + (Lb - d - L) : x0b + d;
            o = ob ? s ^ 1u : s;
            P.anchor = idx;
        }
    }
    if (u != kReaNone && end > beg) {
        const int64_t n = end - beg, x = x0 + (o ? L - end : beg);
        const uint64_t lo = uvoff[u], hi = uvoff[u + 1];
        const int64_t len = (int64_t)(uoff[u + 1] - uoff[u]), plen = (int64_t)(coffs[u + 1] - coffs[u]);
        P.unitig = u; P.orient = o;
        bool unrolled = false;
        if (unroll && circular[u] && len > 0 && (uint64_t)plen < kReaMaxUnrolled) {      // section 19: on the unrolled circle, if the read cannot lap itself
            int64_t xm = x % len;
            if (xm < 0) xm += len;
            const int64_t ym = xm + n, bm = (int64_t)band_max;
            if (ym - len < len) {
                const int64_t s0 = rea_map(xm, pos, nb, cpos, cnb, lo, hi, len, plen);
                const int64_t e0 = ym < len ? rea_map(ym, pos, nb, cpos, cnb, lo, hi, len, plen) : plen + rea_map(ym - len, pos, nb, cpos, cnb, lo, hi, len, plen);
                const int64_t w = e0 - s0;
                if (w >= 0 && (n > w ? n : w) + bm <= plen) {
                    P.s = s0 < bm / 2 ? s0 + plen : s0;
                    P.e = P.s + w;
                    P.status = BELLA_REALIGN_VOTED; P.pad = 1;
                    unrolled = true;
                }
            }
        }
        if (!unrolled) {
            P.s = rea_map(x, pos, nb, cpos, cnb, lo, hi, len, plen);
            P.e = rea_map(x + n, pos, nb, cpos, cnb, lo, hi, len, plen);
            const int64_t h = (int64_t)(band0 / 2);
            P.status = (P.s < -h || P.e > plen + h || P.e < P.s) ? BELLA_REALIGN_OUTSIDE : BELLA_REALIGN_VOTED;   // (VOTED: a candidate until the DP has spoken)
        }
    }
    out[r] = P;
}

BELLA_HD uint32_t base_code(uint8_t ch) { return ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 0u; }      // ASCII -> the 2-bit code (anything else: A)

// 16 ASCII bases -> one word of the 2-bit pack
__global__ void k_rea_pack(const uint8_t* ascii, uint64_t total, uint32_t* packed) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w * 16 >= total) return;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 16 && w * 16 + k < total; ++k) v |= base_code(ascii[w * 16 + k]) << (2 * k);
    packed[w] = v;
}

// The unrolled layout (section 19): unitig u's bases start at poffs[u] and, where poffs[u + 1] - poffs[u] is twice its length, stand
// there twice in a row.  One thread per word of 16 bases; a word that straddles a seam or a unitig's end gathers from two places.
__global__ void k_rea_pack_unrolled(const uint8_t* ascii, const uint64_t* coffs, const uint64_t* poffs, uint32_t nutg, uint64_t ptotal, uint32_t* packed) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w * 16 >= ptotal) return;
    uint32_t a = 0, b = nutg;                                         // the unitig of the word's first base: the last u with poffs[u] <= g
    while (b - a > 1) {
        const uint32_t mid = a + (b - a) / 2;
        if (poffs[mid] <= w * 16) a = mid; else b = mid;
    }
    uint32_t u = a;
    uint64_t pb = poffs[u], pe = poffs[u + 1], cb = coffs[u], plen = coffs[u + 1] - cb;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 16 && w * 16 + k < ptotal; ++k) {
        const uint64_t g = w * 16 + k;
        while (g >= pe) { ++u; pb = pe; pe = poffs[u + 1]; cb = coffs[u]; plen = coffs[u + 1] - cb; }       // (g < ptotal = poffs[nutg]: u stays below nutg)
        const uint64_t j = g - pb;
        v |= base_code(ascii[cb + (j >= plen ? j - plen : j)]) << (2 * k);
    }
    packed[w] = v;
}

struct ReaEnd {                  // the best cell of the last row: trace_best_take's smallest i + j is the smallest q there
    TraceBest best{kTrNeg, 0, 0};
    __device__ __forceinline__ void row0(int, int, int) {}
    __device__ __forceinline__ void before_row(int i, int rows) { if (i == rows) best = TraceBest{kTrNeg, 0, 0}; }
    template <int C> __device__ __forceinline__ void after_row(const int (&)[C], int, int) {}
    __device__ __forceinline__ void reduce() { trace_best_reduce(best); }
    __device__ __forceinline__ ReaRes res() const { return ReaRes{best.s, best.sum - best.i}; }
};

// a ReaJob as band.hpp's problem; kForward: V is known to run forwards and uncomplemented (links.hpp), so dV and comp are constants;
// kAnchored: the path starts in (0, 0) and row 0 is -q (pairalign.hpp's global alignment), else anywhere in row 0, which is 0
template <class EndRule, bool kForward, bool kAnchored = false>
struct ReaProblemT {
    using End = EndRule;
    static constexpr bool anchored = kAnchored, touch_row0 = false;
    const ReaJob& e;
    const uint32_t *rpacked, *upacked;
    __device__ __forceinline__ int m() const { return e.m; }
    __device__ __forceinline__ int rows(uint32_t) const { return (int)e.n; }
    __device__ __forceinline__ int centre() const { return e.c; }
    __device__ __forceinline__ int row0(int j) const { return kAnchored ? -j : 0; }
    __device__ __forceinline__ int h(int64_t t) const { return trace_base(upacked, e.gH, 1, 0u, t); }
    __device__ __forceinline__ const uint32_t* vpack() const { return rpacked; }
    __device__ __forceinline__ int64_t vidx(int64_t t) const { return e.gV + (int64_t)(kForward ? 1 : e.dV) * t; }
    __device__ __forceinline__ uint32_t vcomp() const { return kForward ? 0u : e.comp; }
    __device__ __forceinline__ uint64_t dir_off() const { return e.dir_off; }
    __device__ __forceinline__ uint64_t scr_off() const { return e.scr_off; }
    __device__ __forceinline__ uint32_t band() const { return e.band; }
};
using ReaProblem = ReaProblemT<ReaEnd, false>;

// band of 64 * C diagonals in registers; wavefront w runs jobs[w]
template <int C>
__global__ __launch_bounds__(kTraceBlock) void k_rea_dp(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, ReaRes* res) {
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= njobs) return;                                           // (whole wavefronts leave)
    const ReaJob e = jobs[w];
    const ReaEnd end = band_sweep<C>(ReaProblem{e, rpacked, upacked}, dirs);
    if ((threadIdx.x & 63) == 0) res[w] = end.res();
}

// any band; one wavefront per block
__global__ __launch_bounds__(64) void k_rea_dp_wide(const ReaJob* jobs, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, uint8_t* dirs, int* scratch,
                                                    ReaRes* res) {
    const uint32_t w = blockIdx.x;
    if (w >= njobs) return;
    const ReaJob e = jobs[w];
    const ReaEnd end = band_sweep_wide(ReaProblem{e, rpacked, upacked}, dirs, scratch);
    if (threadIdx.x == 0) res[w] = end.res();
}

struct ReaFamily {               // for the host: what the DP leaves per job, the DP kernels, whether the runs vote
    using Res = ReaRes;
    static constexpr bool votes = true;
    template <int C> static constexpr auto dp() { return k_rea_dp<C>; }
    static constexpr auto dp_wide() { return k_rea_dp_wide; }
};

constexpr int kReaNoEnd = kTrNeg / 2;      // a best score at or below this: the end rule found no cell that a path from row 0 reaches

// where the walk of a job starts, and whether that is a cell of the rectangle (links.hpp has the LnkRes one)
__device__ __forceinline__ bool rea_start(const ReaJob& e, const ReaRes& r, int& i, int& j) {
    i = (int)e.n; j = r.q_end;
    return r.q_end >= 0 && r.q_end <= e.m;
}

// the problem the walks of a result see: ReaProblem, unless the result says otherwise (pairalign.hpp's global one is anchored)
template <class Res> struct ReaWalkOf { using type = ReaProblem; };

// The walks, one thread per job, from the DP's end (Res: a ReaRes or a LnkRes) back to row 0, the job's last op first.  The counting
// walk: runs, op totals, whether the path touched the first or the last diagonal of the band (an end that nothing reaches counts as
// touched), q_begin = the junction where it reached row 0.
template <class Res>
__global__ void k_rea_count(const ReaJob* jobs, const Res* res, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, const uint8_t* dirs, ReaCnt* out) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= njobs) return;
    ReaCnt o{};
    const ReaJob e = jobs[x];
    const Res r = res[x];
    int i, j;
    if (!rea_start(e, r, i, j) || r.score <= kReaNoEnd) { o.touch = 1; out[x] = o; return; }
    TraceRuns runs;
    const bool t = band_walk(typename ReaWalkOf<Res>::type{e, rpacked, upacked}, dirs, i, j, runs);
    o.nops = runs.nruns;
    o.n_eq = runs.cnt[0]; o.n_x = runs.cnt[1]; o.n_ins = runs.cnt[2]; o.n_del = runs.cnt[3];
    o.touch = t ? 1u : 0u;
    o.q_begin = j;
    out[x] = o;
}

// the writing walk, one thread per job with runs: ops[op_off .. op_off + nops) in the order of V
template <class Res>
__global__ void k_rea_write(const ReaJob* jobs, const Res* res, const ReaCnt* cnt, uint32_t njobs, const uint32_t* rpacked, const uint32_t* upacked, const uint8_t* dirs,
                            uint32_t* ops) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= njobs) return;
    const ReaJob e = jobs[x];
    if (e.op_off == ~0ull) return;
    TraceEmit bw{ops, (int64_t)(e.op_off + cnt[x].nops), -1};
    int i, j;
    rea_start(e, res[x], i, j);
    band_walk(typename ReaWalkOf<Res>::type{e, rpacked, upacked}, dirs, i, j, bw);
    bw.flush();
}

// one wavefront per read; table: nine counters per base of all unitigs.  A column j of the unrolled circle (m = 2 mt) votes in row
// j - mt once it is past the seam: one compare and one subtraction per vote.
__global__ __launch_bounds__(kPileBlock) void k_rea_vote(const ReaJob* jobs, const ReaCnt* cnt, uint32_t njobs, const uint32_t* ops, const uint32_t* rpacked, uint32_t* table,
                                                         unsigned long long* votes) {
    const uint32_t x = (uint32_t)(((uint64_t)blockIdx.x * kPileBlock + threadIdx.x) >> 6);
    if (x >= njobs) return;                                           // (whole wavefronts leave)
    const int lane = (int)(threadIdx.x & 63);
    const ReaJob e = jobs[x];
    if (e.op_off == ~0ull) return;
    const uint32_t nops = cnt[x].nops, m = (uint32_t)e.m, mt = (uint32_t)e.mt;
    const uint32_t* const po = ops + e.op_off;
    uint32_t ci = 0, cj = (uint32_t)cnt[x].q_begin;                   // where the chunk's first run starts: row (0-based base of the read), column
    uint32_t nv = 0;
    for (uint32_t c0 = 0; c0 < nops; c0 += 64) {
        const uint32_t w = c0 + lane < nops ? po[c0 + lane] : 0u;
        const uint32_t op = w & 15u, len = w >> 4;
        const uint32_t di = op != kOpDel ? len : 0u, dj = op != kOpIns ? len : 0u;
        const uint32_t ei = pile_scan_incl(di, lane), ej = pile_scan_incl(dj, lane), ec = pile_scan_incl(len, lane);
        const uint32_t si = ci + ei - di, sj = cj + ej - dj;
        const uint32_t total = __shfl(ec, 63, 64);
        for (uint32_t t0 = 0; t0 < total; t0 += 64) {
            const bool live = t0 + lane < total;
            const uint32_t t = live ? t0 + lane : total - 1;
            int r = 0;                                                // the first run whose columns end behind t
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const uint32_t en = __shfl(ec, r + s - 1, 64);
                if (en <= t) r += s;
            }
            const uint32_t rw = __shfl(w, r, 64), rend = __shfl(ec, r, 64), ri = __shfl(si, r, 64), rj = __shfl(sj, r, 64);
            if (!live) continue;
            const uint32_t rop = rw & 15u, rlen = rw >> 4;
            const uint32_t o = t - (rend - rlen);
            const uint32_t i = ri + (rop != kOpDel ? o : 0u), j = rj + (rop != kOpIns ? o : 0u);
            if (rop <= kOpX) {
                if (i < e.n && j < m) {
                    atomicAdd(table + ((uint64_t)e.gT + (j >= mt ? j - mt : j)) * kPileCounters + (uint32_t)trace_base(rpacked, e.gV, e.dV, e.comp, i), 1u);
                    ++nv;
                }
            } else if (rop == kOpIns) {                               // bases of the read only: one vote for the run, in the junction before rj
                if (o == 0 && ri < e.n && rj < m) {
                    atomicAdd(table + ((uint64_t)e.gT + (rj >= mt ? rj - mt : rj)) * kPileCounters + kPileIns + (uint32_t)trace_base(rpacked, e.gV, e.dV, e.comp, ri), 1u);
                    ++nv;
                }
            } else if (rop == kOpDel) {                               // a base of the unitig only
                if (j < m) { atomicAdd(table + ((uint64_t)e.gT + (j >= mt ? j - mt : j)) * kPileCounters + kPileDel, 1u); ++nv; }
            }
        }
        ci += __shfl(ei, 63, 64);
        cj += __shfl(ej, 63, 64);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) nv += __shfl_xor(nv, d, 64);
    if (lane == 0 && nv) atomicAdd(votes, (unsigned long long)nv);
}

// Where the segments of the sequence that was aligned against begin in the new one: scan[g] = bases emitted before position g of all
// unitig bases (k_cons_write's scan).  npos[i] / nnb[i] per vertex.
__global__ void k_rea_segpos(const uint64_t* scan, const uint64_t* cpos, const uint32_t* slot_utg, const uint64_t* uvoff, const uint64_t* coffs, uint32_t nseg, uint64_t* npos,
                             uint32_t* nnb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseg) return;
    const uint32_t u = slot_utg[i];
    const uint64_t base = scan[coffs[u]], a = scan[coffs[u] + cpos[i]];
    const uint64_t b = (uint64_t)i + 1 < uvoff[u + 1] ? scan[coffs[u] + cpos[i + 1]] : scan[coffs[u + 1]];
    npos[i] = a - base;
    nnb[i] = (uint32_t)(b - a);
}
#endif

}  // namespace bella
