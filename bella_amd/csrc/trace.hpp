// trace.hpp -- base-level alignments: banded DP with stored directions, backtrace and run-length ops on gfx950.
//
// Nothing in the reference does this (its PAF carries a score and end points only); the definition is this project's own and is
// written down in DESIGN.md section 9.  In short: an EXTENSION is a DP anchored at the seed (cell (0,0) = 0, match +1, mismatch -1,
// gap -1 linear, the X-drop's scoring) over the rectangle rows i = 0..n (bases of V) x columns j = 0..m (bases of the oriented H),
// free at the far end: it ends at the cell with the best score, ties to the smallest i + j, then the smallest i.  A pair is the left
// extension (both sequences reversed from the seed's start), the seed's k columns, and the right extension.
//
// The sweep and the backtrace are band.hpp's.  What this file brings: TraceProblem -- one pack, dH and comp on H,
// row 0 = -j around the centre diagonal 0, the rows trace_rows(n, m, B) that hold a cell of the rectangle inside the band -- and
// TraceEnd, the best cell anywhere, row 0 included.  Bands above 1,024 cells (widened extensions, tests that force the band to cover
// the rectangle) run k_trace_dp_wide.  The walks are one thread per pair: a counting walk (runs, op totals, whether the path touched
// the band edge) and, once the host has laid out the op array, a writing walk -- left part forwards, right part from the pair's end
// backwards.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "band.hpp"
#include "core.hpp"

namespace bella {

constexpr uint32_t kTrMinBand = 256, kTrRegBand = 1024;      // register kernel: C = 4, 8, 16
constexpr uint32_t kTrMaxBand = 1u << 18;                    // covers any rectangle of reads < 65,536 (2 * 65,536 = 2^17)

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

#if defined(__HIPCC__)
struct TraceEnd {                // the best cell anywhere, row 0 included
    TraceBest best{kTrNeg, 0, 0};
    __device__ __forceinline__ void row0(int s, int j, int) { trace_best_take(best, s, j, 0); }
    __device__ __forceinline__ void before_row(int, int) {}
    template <int C> __device__ __forceinline__ void after_row(const int (&)[C], int, int) {}
    __device__ __forceinline__ void reduce() { trace_best_reduce(best); }
    __device__ __forceinline__ TraceExtRes res() const { return TraceExtRes{best.s, (uint32_t)best.i, (uint32_t)(best.sum - best.i), 0u}; }
};

struct TraceProblem {
    using End = TraceEnd;
    static constexpr bool anchored = true, touch_row0 = true;
    const TraceExt& e;
    const uint32_t* packed;
    __device__ __forceinline__ int m() const { return (int)e.m; }
    __device__ __forceinline__ int rows(uint32_t B) const { return (int)trace_rows(e.n, e.m, B); }
    __device__ __forceinline__ int centre() const { return 0; }
    __device__ __forceinline__ int row0(int j) const { return -j; }
    __device__ __forceinline__ int h(int64_t t) const { return trace_base(packed, e.gH, e.dH, e.comp, t); }
    __device__ __forceinline__ const uint32_t* vpack() const { return packed; }
    __device__ __forceinline__ int64_t vidx(int64_t t) const { return e.gV + (int64_t)e.dV * t; }
    __device__ __forceinline__ uint32_t vcomp() const { return 0u; }
    __device__ __forceinline__ uint64_t dir_off() const { return e.dir_off; }
    __device__ __forceinline__ uint64_t scr_off() const { return e.scr_off; }
    __device__ __forceinline__ uint32_t band() const { return e.band; }
};

// band of 64 * C cells in registers; list[w] = the extension of wavefront w
template <int C>
__global__ __launch_bounds__(kTraceBlock) void k_trace_dp(const TraceExt* exts, const uint32_t* list, uint32_t nlist, const uint32_t* packed,
                                                          uint8_t* dirs, TraceExtRes* res) {
    const uint32_t w = (uint32_t)(((uint64_t)blockIdx.x * kTraceBlock + threadIdx.x) >> 6);
    if (w >= nlist) return;                                           // (whole wavefronts leave)
    const uint32_t slot = list[w];
    const TraceExt e = exts[slot];
    const TraceEnd end = band_sweep<C>(TraceProblem{e, packed}, dirs);
    if ((threadIdx.x & 63) == 0) res[slot] = end.res();
}

// any band; one wavefront per block
__global__ __launch_bounds__(64) void k_trace_dp_wide(const TraceExt* exts, const uint32_t* list, uint32_t nlist, const uint32_t* packed, uint8_t* dirs,
                                                      int* scratch, TraceExtRes* res) {
    const uint32_t w = blockIdx.x;
    if (w >= nlist) return;
    const uint32_t slot = list[w];
    const TraceExt e = exts[slot];
    const TraceEnd end = band_sweep_wide(TraceProblem{e, packed}, dirs, scratch);
    if (threadIdx.x == 0) res[slot] = end.res();
}

// ---- backtrace ------------------------------------------------------------------------------------------------------------------
// Walks one extension from its best cell back to the seed and hands every op to `put` (far end first).  Returns whether the path
// touched the first or the last diagonal of the band.
template <class Put>
__device__ __forceinline__ bool trace_walk(const TraceExt& e, const TraceExtRes& r, const uint32_t* packed, const uint8_t* dirs, Put&& put) {
    int j = (int)r.bj;
    return band_walk(TraceProblem{e, packed}, dirs, (int)r.bi, j, put);
}

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
