// polish.hpp -- unitig consensus: the pileup table's majority vote taken per position of the backbone reads, inside the unitig's own
// coordinate system, on gfx950.
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h).  Everything is
// an integer, so the result is the numpy mirror's exactly.
//
// Work is split over RAW UNITIG POSITIONS, never over unitigs or reads: one unitig spanning the genome costs what a thousand short ones
// cost, as with unitig.hpp's gather.  A tile is kPolTile = 4,096 consecutive positions (256 threads x 16).
//
// k_pol_decide.  One workgroup per tile; in step k lane t holds position 4096 tile + 256 k + t, so the lanes of a wavefront read 64
// consecutive 36-byte rows of the table (ascending for orientation 0, descending for orientation 1) and write 64 consecutive emit
// bytes.  A lane finds the segment of its first position by bisection over gseg and steps forward from there.  The rule is
// pileup.hpp's cons_decide_at; for orientation 1 the decision string is reverse-complemented inside the byte.  The per-unitig
// statistics are reduced across a wavefront whose 64 positions lie in one unitig before they go to the record; the tile's emitted-base
// count is reduced over the workgroup (one LDS word per wavefront).
// The tile counts -- not the positions -- are scanned (hipCUB, 64-bit sums).
// k_pol_segoff.  One wavefront per segment start: the tile's prefix plus the emit counts in front of the start inside its tile, read 16
// bytes per lane (a tile is 4 KB of emit bytes).  k_pol_finish turns those into ppos / pnbases / the unitig offsets / len_after.
// k_pol_write.  One workgroup per tile: a lane owns 16 consecutive positions (one 16-byte load of emit bytes), the lanes' counts are
// scanned (wave scan in registers, one LDS word per wavefront), every lane puts its <= 32 ASCII bytes into an LDS stage at their
// tile-relative offsets, shifted by the tile's output offset mod 16; after the barrier the stage goes out in 16-byte stores from
// consecutive lanes on 16-byte-aligned addresses.  The first and last 16-byte word of a tile's output range are shared with the
// neighbouring tiles and go out bytewise.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "pileup.hpp"
#include "unitig.hpp"

namespace bella {

constexpr uint32_t kPolBlock = 256;
constexpr uint32_t kPolPerLane = 16;
constexpr uint32_t kPolTile = kPolBlock * kPolPerLane;    // positions per tile; at most 2 kPolTile emitted bases

#if defined(__HIPCC__)
// sum of (byte & 3) over the first nb bytes (0 .. 4 and more) of a word of emit bytes
__device__ __forceinline__ uint32_t pol_count4(uint32_t w, uint32_t nb) {
    const uint32_t mask = nb >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nb)) - 1u);
    return ((w & 0x03030303u & mask) * 0x01010101u) >> 24;
}

// gseg[nseg + 1]: where every segment's raw bases begin among all unitig positions (k_utg_segoff); emit holds ntiles * kPolTile bytes
// (the positions behind `total` get 0); recs is zeroed on entry.  rbeg[r] / rend[r]: read r's span among all bases (whole reads: roff and
// roff + 1; clipped reads: trim.hpp's spans).
__global__ __launch_bounds__(kPolBlock) void k_pol_decide(const uint64_t* gseg, const uint32_t* verts, const uint32_t* slot_utg, uint32_t nseg, uint64_t total,
                                                          const uint64_t* roff, const uint64_t* rbeg, const uint64_t* rend, const uint32_t* packed, const uint32_t* table,
                                                          uint32_t min_depth, uint8_t* emit, bella_polish_unitig* recs, uint32_t* tile_cnt) {
    __shared__ uint32_t wsum[kPolBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * kPolTile;
    const int lane = (int)(threadIdx.x & 63);
    uint32_t s;
    {
        const uint64_t g = base + threadIdx.x < total ? base + threadIdx.x : total - 1;
        uint32_t lo = 0, hi = nseg;                                   // the last segment with gseg[s] <= g
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (gseg[mid] <= g) lo = mid; else hi = mid;
        }
        s = lo;
    }
    uint64_t beg = gseg[s], end = gseg[s + 1];
    uint32_t cnt = 0;
    for (uint32_t k = 0; k < kPolPerLane; ++k) {
        const uint64_t g0 = base + (uint64_t)k * kPolBlock + threadIdx.x;
        const bool live = g0 < total;
        const uint64_t g = live ? g0 : total - 1;
        while (g >= end && s + 1 < nseg) { ++s; beg = end; end = gseg[s + 1]; }
        const uint32_t v = verts[s], r = v >> 1;
        const uint64_t i = g - beg;
        const uint64_t row = (v & 1u) ? rend[r] - 1 - i : rbeg[r] + i;
        const uint32_t p = (uint32_t)(row - roff[r]);                 // the ORIGINAL position: the junction rule and the table know no clip
        const ConsDecision d = cons_decide_at(table + row * kPileCounters, p, pile_base(packed, row), min_depth);
        uint32_t e = d.emit;
        if (v & 1u) {                                                 // rc of the decision string: the position's base first, then the junction's
            const uint32_t n = e & 3u, b0 = ((e >> 2) & 3u) ^ 3u, b1 = ((e >> 4) & 3u) ^ 3u;
            e = n == 2 ? (2u | b1 << 2 | b0 << 4) : n == 1 ? (1u | b0 << 2) : 0u;
        }
        if (!live) e = 0;
        emit[g0] = (uint8_t)e;
        cnt += e & 3u;
        // statistics
        const uint32_t u = slot_utg[s];
        uint32_t s_sub = live ? d.sub : 0u, s_del = live ? d.del : 0u, s_ins = live ? d.ins : 0u, s_cov = live ? d.cov : 0u;
        unsigned long long s_depth = live ? d.depth : 0ull;
        const uint32_t u0 = __shfl(u, 0, 64);
        bool mine = live;
        if (__all(!live || u == u0)) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                s_sub += __shfl_xor(s_sub, m, 64); s_del += __shfl_xor(s_del, m, 64); s_ins += __shfl_xor(s_ins, m, 64); s_cov += __shfl_xor(s_cov, m, 64);
                s_depth += __shfl_xor(s_depth, m, 64);
            }
            mine = lane == 0;
        }
        if (mine) {
            bella_polish_unitig* const st = recs + u;
            if (s_sub) atomicAdd((unsigned long long*)&st->substituted, (unsigned long long)s_sub);
            if (s_del) atomicAdd((unsigned long long*)&st->deleted, (unsigned long long)s_del);
            if (s_ins) atomicAdd((unsigned long long*)&st->inserted, (unsigned long long)s_ins);
            if (s_cov) atomicAdd((unsigned long long*)&st->covered, (unsigned long long)s_cov);
            if (s_depth) atomicAdd((unsigned long long*)&st->depth_sum, s_depth);
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m, 64);
    if (lane == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// gp[i] = polished bases in front of segment i (i == nseg: all of them); tile_pref[ntiles + 1]: the exclusive scan of the tile counts
__global__ __launch_bounds__(kPolBlock) void k_pol_segoff(const uint64_t* gseg, uint32_t nseg, const uint8_t* emit, const uint64_t* tile_pref, uint64_t* gp) {
    const uint64_t i = ((uint64_t)blockIdx.x * kPolBlock + threadIdx.x) >> 6;
    if (i > nseg) return;                                             // (whole wavefronts leave)
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t g = gseg[i], t = g / kPolTile;
    const uint32_t within = (uint32_t)(g - t * kPolTile);             // emit bytes of tile t in front of g; 0 when g is a tile's first position
    const uint8_t* const e = emit + t * kPolTile;
    uint32_t c = 0;
    for (uint32_t o = lane * 16; o < within; o += 64 * 16) {
        const uint4 w = *reinterpret_cast<const uint4*>(e + o);
        const uint32_t nb = within - o;                               // valid bytes from o on (16 and more: all of them)
        c += pol_count4(w.x, nb) + pol_count4(w.y, nb > 4 ? nb - 4 : 0u) + pol_count4(w.z, nb > 8 ? nb - 8 : 0u) + pol_count4(w.w, nb > 12 ? nb - 12 : 0u);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) c += __shfl_xor(c, m, 64);
    if (lane == 0) gp[i] = tile_pref[t] + c;
}

// ppos / pnbases per segment; per unitig its offset (poffs[nutg] = the total), len_before and len_after.  uvoff[nutg + 1], uboff[nutg + 1].
__global__ void k_pol_finish(const uint64_t* gp, const uint32_t* slot_utg, const uint64_t* uvoff, const uint64_t* uboff, uint32_t nseg, uint32_t nutg, uint64_t* ppos,
                             uint32_t* pnb, uint64_t* poffs, bella_polish_unitig* recs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nseg) {
        ppos[i] = gp[i] - gp[uvoff[slot_utg[i]]];
        pnb[i] = (uint32_t)(gp[i + 1] - gp[i]);
    }
    if (i <= nutg) {
        const uint64_t o = gp[uvoff[i]];                              // (uvoff[nutg] == nseg)
        poffs[i] = o;
        if (i < nutg) {
            recs[i].len_before = uboff[i + 1] - uboff[i];
            recs[i].len_after = gp[uvoff[i + 1]] - o;
        }
    }
}

// out: 16-byte aligned, holds the total rounded up to 16
__global__ __launch_bounds__(kPolBlock) void k_pol_write(const uint8_t* emit, const uint64_t* tile_pref, uint8_t* out) {
    __shared__ uint32_t wsum[kPolBlock / 64];
    __shared__ __attribute__((aligned(16))) uint8_t stage[2 * kPolTile + 16];
    const uint64_t B = tile_pref[blockIdx.x];
    const uint32_t T = (uint32_t)(tile_pref[blockIdx.x + 1] - B);     // <= 2 kPolTile
    const uint32_t a = (uint32_t)(B & 15u);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint4 w4 = *reinterpret_cast<const uint4*>(emit + (uint64_t)blockIdx.x * kPolTile + threadIdx.x * kPolPerLane);
    const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    const uint32_t c = pol_count4(w[0], 4) + pol_count4(w[1], 4) + pol_count4(w[2], 4) + pol_count4(w[3], 4);
    const uint32_t incl = pile_scan_incl(c, (int)lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t off = a + incl - c;
    for (uint32_t q = 0; q < wave; ++q) off += wsum[q];
#pragma unroll
    for (int j = 0; j < (int)kPolPerLane; ++j) {
        const uint32_t e = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu, n = e & 3u;
        if (n >= 1) stage[off++] = (uint8_t)utg_ascii((e >> 2) & 3u);
        if (n >= 2) stage[off++] = (uint8_t)utg_ascii((e >> 4) & 3u);
    }
    __syncthreads();
    uint8_t* const dst = out + (B - a);                               // 16-byte aligned; stage[x] belongs at dst[x]
    const uint32_t lim = a + T, nwords = (lim + 15) / 16;
    for (uint32_t k = threadIdx.x; k < nwords; k += kPolBlock) {
        const uint32_t lo = k * 16 < a ? a : k * 16, hi = k * 16 + 16 < lim ? k * 16 + 16 : lim;
        if (hi - lo == 16) *reinterpret_cast<uint4*>(dst + k * 16) = *reinterpret_cast<const uint4*>(stage + k * 16);
        else for (uint32_t b = lo; b < hi; ++b) dst[b] = stage[b];    // the range's first and last word: neighbouring tiles own the rest of them
    }
}
#endif

}  // namespace bella
