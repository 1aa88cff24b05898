// pileup.hpp -- read correction: a per-read pileup accumulated from the traced alignments, and the consensus call, on gfx950.
//
// Nothing in the reference does this (it ends at the overlap / alignment file); the definition is this project's own and is written
// down in DESIGN.md section 10.  In short: every base position of every read owns nine uint32 counters (36 bytes): base[4] = votes for
// A, C, G, T at the position, del = votes that the base is not there, ins[4] = votes for ONE base inserted in the junction just before
// the position.  A traced pair (V = read cid, H' = read rid oriented by the strand) votes on both of its reads: an aligned column votes
// the other read's base, a gap base votes `del` on the read that has the base, a gap run votes one `ins` on the read that lacks it.
// Everything is an integer sum, so the table does not depend on the order the votes arrive in.
//
// Mapping of the vote kernel.  One wavefront per pair, looping over the pair's runs 64 at a time: lane l loads run 64 c + l, three
// inclusive wave scans (bases of V, bases of H', columns) give every run its start (i, j) and its first column -- the segmented scan of
// the pair; the columns of the 64 runs are then dealt to the lanes 64 at a time (a 6-step search over the lanes' column prefix finds a
// column's run), so consecutive lanes hold consecutive columns of a run = consecutive 36-byte records of the table, whatever the run
// lengths are (at 15 % error a run is 4 columns long on average: one lane per run or one loop per run would leave the wave idle).
// The other choice, a flat list of runs balanced by bases over all pairs, needs a device-wide segmented scan and a second pass; the
// pairs of a batch are thousands and each has thousands of columns, so one wavefront per pair already fills the device.
// No LDS: the run table of a chunk lives in the lanes' registers and is read with cross-lane permutes.
//
// The consensus is three passes over the table: k_cons_decide (per position: 0, 1 or 2 bases, per-read statistics reduced per wave),
// an exclusive scan of the emit counts (hipCUB), k_cons_write (ASCII bases at their offsets) + k_cons_reads (per-read offsets).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "core.hpp"
#include "trace.hpp"

namespace bella {

constexpr int kPileCounters = 9;       // base[4], del, ins[4]
enum { kPileDel = 4, kPileIns = 5 };

// one traced pair of a batch, as the vote kernel reads it
struct PilePair {
    uint64_t rowV, rowH;   // first base of read cid / rid among all bases: row of the table and position in the packed reads
    uint64_t op_off;       // first run in the batch's op array
    uint32_t nops;
    uint32_t lenV, lenH;
    uint32_t strand;       // 1: H' = reverse complement of H
    int32_t i0, j0;        // tbegV, tbegH: where the ops start on V and on H'
};

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t pile_base(const uint32_t* packed, uint64_t g) { return (packed[g >> 4] >> ((uint32_t)(g & 15) * 2)) & 3u; }

__device__ __forceinline__ uint32_t pile_scan_incl(uint32_t x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

constexpr int kPileBlock = 256;        // four independent wavefronts

__global__ __launch_bounds__(kPileBlock) void k_pile_vote(const PilePair* pp, uint32_t npairs, const uint32_t* ops, const uint32_t* packed, uint32_t* table,
                                                          unsigned long long* votes) {
    const uint32_t q = (uint32_t)(((uint64_t)blockIdx.x * kPileBlock + threadIdx.x) >> 6);
    if (q >= npairs) return;                                          // (whole wavefronts leave)
    const int lane = (int)(threadIdx.x & 63);
    const PilePair P = pp[q];
    const uint32_t* const po = ops + P.op_off;
    const uint32_t comp = P.strand ? 3u : 0u;
    uint32_t ci = (uint32_t)P.i0, cj = (uint32_t)P.j0;               // where the chunk's first run starts
    uint32_t nv = 0;
    for (uint32_t c0 = 0; c0 < P.nops; c0 += 64) {
        const uint32_t w = c0 + lane < P.nops ? po[c0 + lane] : 0u;
        const uint32_t op = w & 15u, len = w >> 4;
        const uint32_t di = op != kOpDel ? len : 0u, dj = op != kOpIns ? len : 0u;
        const uint32_t ei = pile_scan_incl(di, lane), ej = pile_scan_incl(dj, lane), ec = pile_scan_incl(len, lane);
        const uint32_t si = ci + ei - di, sj = cj + ej - dj;          // this lane's run starts at (si, sj)
        const uint32_t total = __shfl(ec, 63, 64);
        for (uint32_t t0 = 0; t0 < total; t0 += 64) {
            const bool live = t0 + lane < total;
            const uint32_t t = live ? t0 + lane : total - 1;
            int r = 0;                                                // the first run whose columns end behind t
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const uint32_t e = __shfl(ec, r + s - 1, 64);
                if (e <= t) r += s;
            }
            const uint32_t rw = __shfl(w, r, 64), rend = __shfl(ec, r, 64), ri = __shfl(si, r, 64), rj = __shfl(sj, r, 64);
            if (!live) continue;
            const uint32_t rop = rw & 15u, rlen = rw >> 4;
            const uint32_t o = t - (rend - rlen);
            const uint32_t i = ri + (rop != kOpDel ? o : 0u), j = rj + (rop != kOpIns ? o : 0u);
            // position j of H' is position lenH - 1 - j of H on strand 1, its base the complement
            const uint64_t gH = P.rowH + (P.strand ? (uint64_t)P.lenH - 1 - j : (uint64_t)j);
            if (rop <= kOpX) {
                if (i < P.lenV && j < P.lenH) {
                    const uint32_t vb = pile_base(packed, P.rowV + i), hb = pile_base(packed, gH) ^ comp;
                    atomicAdd(table + (P.rowV + i) * kPileCounters + hb, 1u);
                    atomicAdd(table + gH * kPileCounters + (vb ^ comp), 1u);
                    nv += 2;
                }
            } else if (rop == kOpIns) {                               // a base of V only
                if (i < P.lenV) { atomicAdd(table + (P.rowV + i) * kPileCounters + kPileDel, 1u); ++nv; }
                if (o == 0) {
                    // H lacks the run: one vote into the junction before rj of H' = junction lenH - rj of H on strand 1, with the base
                    // that comes first in H's own direction (strand 1: the complement of the run's last base)
                    const uint32_t jn = P.strand ? P.lenH - rj : rj;
                    const uint32_t iv = P.strand ? ri + rlen - 1 : ri;
                    if (rj <= P.lenH && jn < P.lenH && iv < P.lenV) {
                        atomicAdd(table + (P.rowH + jn) * kPileCounters + kPileIns + (pile_base(packed, P.rowV + iv) ^ comp), 1u);
                        ++nv;
                    }
                }
            } else if (rop == kOpDel) {                               // a base of H' only
                if (j < P.lenH) { atomicAdd(table + gH * kPileCounters + kPileDel, 1u); ++nv; }
                if (o == 0 && ri < P.lenV && rj < P.lenH) {           // V lacks the run: its first base, into the junction before ri
                    atomicAdd(table + (P.rowV + ri) * kPileCounters + kPileIns + (pile_base(packed, gH) ^ comp), 1u);
                    ++nv;
                }
            }
        }
        ci += __shfl(ei, 63, 64);
        cj += __shfl(ej, 63, 64);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) nv += __shfl_xor(nv, d, 64);
    if (lane == 0 && nv) atomicAdd(votes, (unsigned long long)nv);
}

// ---- votes with every gap run at its canonical position (the test kit states it in numpy) ---------
// k_pile_vote's mapping -- one wavefront per pair, 64 runs per chunk in registers, no LDS -- on modified run records.  A gap lane
// decides its own run: the left shift sL inside the '=' run before it, the right shift sR inside the '=' run behind it (strand 1
// only: nobody else reads it), each the common suffix / prefix of S[..x) and S[..x + L) over the 2-bit bases, at most the length of
// that '=' run.  The neighbours' words come over __shfl_up / __shfl_down; the last run of the chunk before is carried in a register
// and lane 63 loads the first run of the chunk behind (where that run is a gap, lane 63 also works out what it takes from it).
// Pass L deals the columns of the left-normalised runs (the '=' run gives up sL columns, the gap lane owns L + sL: its tail is '='
// columns at the displaced coordinates) and casts the V-side votes of every pair and the H-side votes of a strand-0 pair; a strand-1
// pair deals its columns a second time (pass R, the mirror image with sR) for its H-side votes: right in V order is left in H's own
// direction.  The atomics per pair are what k_pile_vote issues.  The shift loop goes base by base: it is bounded by the length of
// one '=' run (a few bases at 15 % error; a long homopolymer in an exact overlap costs its wave that many steps once).
struct PileNormCnt { unsigned long long votes, gap_runs, shifted_runs, shifted_columns; };

// S is V (row = rowV) or H' (row = rowH; rev: position a of H' is position lenS - 1 - a of H -- the complement does not matter to a
// comparison inside S).  Both return 0 where a comparison would leave S.
__device__ __forceinline__ uint32_t pile_sbase(const uint32_t* packed, uint64_t row, uint32_t lenS, bool rev, uint32_t a) {
    return pile_base(packed, row + (rev ? lenS - 1 - a : a));
}
__device__ __forceinline__ uint32_t pile_shift_left(const uint32_t* packed, uint64_t row, uint32_t lenS, bool rev, uint32_t x, uint32_t L, uint32_t d) {
    if ((uint64_t)x + L > lenS) return 0;
    if (d > x) d = x;
    uint32_t s = 0;
    while (s < d && pile_sbase(packed, row, lenS, rev, x - 1 - s) == pile_sbase(packed, row, lenS, rev, x + L - 1 - s)) ++s;
    return s;
}
__device__ __forceinline__ uint32_t pile_shift_right(const uint32_t* packed, uint64_t row, uint32_t lenS, bool rev, uint32_t x, uint32_t L, uint32_t d) {
    if ((uint64_t)x + L >= lenS) return 0;
    if (d > lenS - x - L) d = lenS - x - L;
    uint32_t s = 0;
    while (s < d && pile_sbase(packed, row, lenS, rev, x + s) == pile_sbase(packed, row, lenS, rev, x + L + s)) ++s;
    return s;
}

__global__ __launch_bounds__(kPileBlock) void k_pile_vote_norm(const PilePair* pp, uint32_t npairs, const uint32_t* ops, const uint32_t* packed, uint32_t* table,
                                                               PileNormCnt* cnt) {
    const uint32_t q = (uint32_t)(((uint64_t)blockIdx.x * kPileBlock + threadIdx.x) >> 6);
    if (q >= npairs) return;                                          // (whole wavefronts leave)
    const int lane = (int)(threadIdx.x & 63);
    const PilePair P = pp[q];
    const uint32_t* const po = ops + P.op_off;
    const uint32_t comp = P.strand ? 3u : 0u;
    uint32_t ci = (uint32_t)P.i0, cj = (uint32_t)P.j0;               // where the chunk's first run starts
    uint32_t prev_w = 0, prev_sR = 0;                                 // the last run of the chunk before ('=' of length 0: no shift) and its right shift
    uint32_t nv = 0, n_gap = 0, n_shift = 0, n_cols = 0;
    for (uint32_t c0 = 0; c0 < P.nops; c0 += 64) {
        const uint32_t w = c0 + lane < P.nops ? po[c0 + lane] : 0u;
        const uint32_t op = w & 15u, len = w >> 4;
        uint32_t wp = __shfl_up(w, 1, 64), wn = __shfl_down(w, 1, 64);
        if (lane == 0) wp = prev_w;
        if (lane == 63) wn = c0 + 64 < P.nops ? po[c0 + 64] : 0u;
        const uint32_t di = op != kOpDel ? len : 0u, dj = op != kOpIns ? len : 0u;
        const uint32_t ei = pile_scan_incl(di, lane), ej = pile_scan_incl(dj, lane);
        const uint32_t si = ci + ei - di, sj = cj + ej - dj;          // this lane's run starts at (si, sj)
        // ---- the shifts of this lane's gap run
        const bool gap = (op == kOpIns || op == kOpDel) && len;
        uint32_t sL = 0, sR = 0;
        if (gap) {
            const bool isI = op == kOpIns;
            const uint64_t row = isI ? P.rowV : P.rowH;
            const uint32_t lenS = isI ? P.lenV : P.lenH, x = isI ? si : sj;
            const bool rev = !isI && P.strand;
            if ((wp & 15u) == kOpEq) sL = pile_shift_left(packed, row, lenS, rev, x, len, wp >> 4);
            if (P.strand && (wn & 15u) == kOpEq) sR = pile_shift_right(packed, row, lenS, rev, x, len, wn >> 4);
            const uint32_t sH = P.strand ? sR : sL;
            ++n_gap;
            n_shift += (sL ? 1u : 0u) + (sH ? 1u : 0u);
            n_cols += sL + sH;
        }
        // ---- what an '=' lane gives to the gap behind it (pass L) and to the gap before it (pass R)
        uint32_t giveL = __shfl_down(sL, 1, 64), takeR = __shfl_up(sR, 1, 64);
        if (lane == 0) takeR = prev_sR;
        if (lane == 63) {
            giveL = 0;
            const uint32_t nop = wn & 15u, nlen = wn >> 4;
            if (op == kOpEq && (nop == kOpIns || nop == kOpDel) && nlen) {               // the first run of the chunk behind is a gap: its left shift, as its own lane will find it
                const bool isI = nop == kOpIns;
                giveL = pile_shift_left(packed, isI ? P.rowV : P.rowH, isI ? P.lenV : P.lenH, !isI && P.strand, (isI ? si : sj) + len, nlen, len);
            }
        }
        for (uint32_t pass = 0; pass <= P.strand; ++pass) {
            const bool voteV = pass == 0, voteH = pass == 1 || !P.strand;
            // the lane's record of this pass: mlen columns from (ai, aj); a gap lane's first `pre` and last mlen - pre - len are '='
            const uint32_t sh = pass ? sR : sL;
            const uint32_t mlen = op == kOpEq ? len - (pass ? takeR : giveL) : len + sh;
            const uint32_t back = pass ? 0u : sh, fwd = pass && op == kOpEq ? takeR : 0u;
            const uint32_t ai = si - back + fwd, aj = sj - back + fwd, pre = pass ? sh : 0u;
            const uint32_t ec = pile_scan_incl(mlen, lane);
            const uint32_t total = __shfl(ec, 63, 64);
            for (uint32_t t0 = 0; t0 < total; t0 += 64) {
                const bool live = t0 + lane < total;
                const uint32_t t = live ? t0 + lane : total - 1;
                int r = 0;                                            // the first run whose columns end behind t
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) {
                    const uint32_t e = __shfl(ec, r + s - 1, 64);
                    if (e <= t) r += s;
                }
                const uint32_t rw = __shfl(w, r, 64), rend = __shfl(ec, r, 64), rmlen = __shfl(mlen, r, 64), ri = __shfl(ai, r, 64), rj = __shfl(aj, r, 64),
                               rpre = __shfl(pre, r, 64);
                const uint32_t rop = rw & 15u, rlen = rw >> 4;
                if (!live || rop > kOpDel) continue;
                const uint32_t o = t - (rend - rmlen);
                const bool in_gap = rop >= kOpIns && o >= rpre && o < rpre + rlen;
                if (!in_gap) {                                        // an aligned column: of an '=' / 'X' run, or one a gap jumped over
                    const uint32_t skip = rop >= kOpIns && o >= rpre ? rlen : 0u;      // behind the gap: past its bases on the side that has them
                    const uint32_t i = ri + o - skip + (rop == kOpIns ? skip : 0u), j = rj + o - skip + (rop == kOpDel ? skip : 0u);
                    if (i < P.lenV && j < P.lenH) {
                        const uint64_t gH = P.rowH + (P.strand ? (uint64_t)P.lenH - 1 - j : (uint64_t)j);
                        const uint32_t vb = pile_base(packed, P.rowV + i), hb = pile_base(packed, gH) ^ comp;
                        if (voteV) { atomicAdd(table + (P.rowV + i) * kPileCounters + hb, 1u); ++nv; }
                        if (voteH) { atomicAdd(table + gH * kPileCounters + (vb ^ comp), 1u); ++nv; }
                    }
                    continue;
                }
                const uint32_t g = o - rpre, gi = ri + rpre, gj = rj + rpre;           // column g of the gap that starts at (gi, gj)
                if (rop == kOpIns) {                                  // a base of V only
                    const uint32_t i = gi + g;
                    if (voteV && i < P.lenV) { atomicAdd(table + (P.rowV + i) * kPileCounters + kPileDel, 1u); ++nv; }
                    if (voteH && g == 0) {                            // (k_pile_vote's junction and base)
                        const uint32_t jn = P.strand ? P.lenH - gj : gj;
                        const uint32_t iv = P.strand ? gi + rlen - 1 : gi;
                        if (gj <= P.lenH && jn < P.lenH && iv < P.lenV) {
                            atomicAdd(table + (P.rowH + jn) * kPileCounters + kPileIns + (pile_base(packed, P.rowV + iv) ^ comp), 1u);
                            ++nv;
                        }
                    }
                } else {                                              // a base of H' only
                    const uint32_t j = gj + g;
                    const uint64_t gH = P.rowH + (P.strand ? (uint64_t)P.lenH - 1 - j : (uint64_t)j);
                    if (voteH && j < P.lenH) { atomicAdd(table + gH * kPileCounters + kPileDel, 1u); ++nv; }
                    if (voteV && g == 0 && gi < P.lenV && gj < P.lenH) {
                        atomicAdd(table + (P.rowV + gi) * kPileCounters + kPileIns + (pile_base(packed, gH) ^ comp), 1u);
                        ++nv;
                    }
                }
            }
        }
        ci += __shfl(ei, 63, 64);
        cj += __shfl(ej, 63, 64);
        prev_w = __shfl(w, 63, 64);
        prev_sR = __shfl(sR, 63, 64);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        nv += __shfl_xor(nv, d, 64); n_gap += __shfl_xor(n_gap, d, 64); n_shift += __shfl_xor(n_shift, d, 64); n_cols += __shfl_xor(n_cols, d, 64);
    }
    if (lane == 0) {
        if (nv) atomicAdd(&cnt->votes, (unsigned long long)nv);
        if (n_gap) atomicAdd(&cnt->gap_runs, (unsigned long long)n_gap);
        if (n_shift) atomicAdd(&cnt->shifted_runs, (unsigned long long)n_shift);
        if (n_cols) atomicAdd(&cnt->shifted_columns, (unsigned long long)n_cols);
    }
}

// table[first + x] += add[x]  (bella_hip_add_pileup: another context's counters)
__global__ void k_pile_add(uint32_t* table, const uint32_t* add, uint64_t n) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x < n) table[x] += add[x];
}

// ---- consensus ------------------------------------------------------------------------------------------------------------------
// What the rule of DESIGN.md section 10 decides at one position: the emit byte and the position's share of the statistics.
struct ConsDecision {
    uint32_t emit;                     // count | first base << 2 | second base << 4: a junction's inserted base comes before the position's own
    uint32_t sub, del, ins, cov;       // 0 / 1 each
    uint64_t depth;
};

// row: the nine counters of the position; p: its index in its read (the junction before it reads the row before: p >= 1 only); own: the
// read's base there.  The one statement of the rule on the device: k_cons_decide (read space) and k_pol_decide (unitig space) call it.
__device__ __forceinline__ ConsDecision cons_decide_at(const uint32_t* row, uint32_t p, uint32_t own, uint32_t min_depth) {
    uint32_t cb[4] = {row[0], row[1], row[2], row[3]};
    const uint32_t del = row[kPileDel];
    const uint64_t depth = (uint64_t)cb[0] + cb[1] + cb[2] + cb[3] + del;
    uint32_t n = 0, code = 0, n_ins = 0, n_del = 0, n_sub = 0, cov = 0;
    if (p >= 1) {                                                     // the junction before p
        const uint32_t* const pr = row - kPileCounters;
        const uint64_t dprev = (uint64_t)pr[0] + pr[1] + pr[2] + pr[3] + pr[kPileDel];
        const uint64_t cmin = dprev < depth ? dprev : depth;
        const uint32_t in[4] = {row[kPileIns], row[kPileIns + 1], row[kPileIns + 2], row[kPileIns + 3]};
        const uint64_t I = (uint64_t)in[0] + in[1] + in[2] + in[3];
        if (cmin >= min_depth && 2 * I > cmin + 1) {
            uint32_t best = 0;
            for (uint32_t x = 1; x < 4; ++x) if (in[x] > in[best]) best = x;
            code |= best << (2 + 2 * n);
            ++n; n_ins = 1;
        }
    }
    if (depth < min_depth) {
        code |= own << (2 + 2 * n); ++n;
    } else {
        cov = 1;
        if (2 * (uint64_t)del > depth + 1) n_del = 1;
        else {
            uint64_t wv[4];
            for (uint32_t x = 0; x < 4; ++x) wv[x] = (uint64_t)cb[x] + (x == own ? 1u : 0u);
            uint32_t best = 0;
            for (uint32_t x = 1; x < 4; ++x) if (wv[x] > wv[best]) best = x;
            if (wv[own] == wv[best]) best = own;
            code |= best << (2 + 2 * n); ++n;
            n_sub = best != own ? 1u : 0u;
        }
    }
    return ConsDecision{code | n, n_sub, n_del, n_ins, cov, depth};
}

// Per position g (a row of the table): emit[g].  Per-read statistics: a wavefront whose 64 positions lie in one read reduces across its
// lanes first.
__global__ __launch_bounds__(256) void k_cons_decide(const uint32_t* table, const uint32_t* packed, const uint64_t* roff, uint32_t nreads, uint64_t total,
                                                     uint32_t min_depth, uint8_t* emit, bella_consensus_read* stats) {
    const uint64_t g0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g0 < total;
    const uint64_t g = live ? g0 : total - 1;
    const int lane = (int)(threadIdx.x & 63);
    uint32_t lo = 0, hi = nreads;                                     // the read of g: the last r with roff[r] <= g
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (roff[mid] <= g) lo = mid; else hi = mid;
    }
    const uint32_t r = lo;
    const uint32_t p = (uint32_t)(g - roff[r]);
    const ConsDecision d = cons_decide_at(table + g * kPileCounters, p, pile_base(packed, g), min_depth);
    if (live) emit[g] = (uint8_t)d.emit;
    // statistics
    uint32_t s_sub = live ? d.sub : 0u, s_del = live ? d.del : 0u, s_ins = live ? d.ins : 0u, s_cov = live ? d.cov : 0u;
    unsigned long long s_depth = live ? d.depth : 0ull;
    const uint32_t r0 = __shfl(r, 0, 64);
    if (__all(!live || r == r0)) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            s_sub += __shfl_xor(s_sub, m, 64); s_del += __shfl_xor(s_del, m, 64); s_ins += __shfl_xor(s_ins, m, 64); s_cov += __shfl_xor(s_cov, m, 64);
            s_depth += __shfl_xor(s_depth, m, 64);
        }
        if (lane != 0) return;
    }
    bella_consensus_read* const st = stats + r;
    if (s_sub) atomicAdd(&st->substituted, s_sub);
    if (s_del) atomicAdd(&st->deleted, s_del);
    if (s_ins) atomicAdd(&st->inserted, s_ins);
    if (s_cov) atomicAdd(&st->covered, s_cov);
    if (s_depth) atomicAdd((unsigned long long*)&st->depth_sum, s_depth);
}

// scan[g] = bases emitted before position g (scan[total] = all of them)
__global__ void k_cons_write(const uint8_t* emit, const uint64_t* scan, uint64_t total, uint8_t* out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const uint32_t e = emit[g], n = e & 3u;
    const uint64_t o = scan[g];
    if (n >= 1) out[o] = (uint8_t)"ACGT"[(e >> 2) & 3u];
    if (n >= 2) out[o + 1] = (uint8_t)"ACGT"[(e >> 4) & 3u];
}

__global__ void k_cons_reads(const uint64_t* roff, const uint64_t* scan, uint32_t nreads, uint64_t* offs, bella_consensus_read* stats) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nreads) return;
    const uint64_t o = scan[roff[r]];
    offs[r] = o;
    if (r < nreads) {
        stats[r].len_before = (uint32_t)(roff[r + 1] - roff[r]);
        stats[r].len_after = (uint32_t)(scan[roff[r + 1]] - o);
    }
}
#endif

}  // namespace bella
