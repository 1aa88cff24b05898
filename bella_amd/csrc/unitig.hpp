// unitig.hpp -- tip clipping, unitig compaction and unitig sequences on the reduced string graph, on gfx950.
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h).
// Everything is an integer, so the result is the numpy mirror's exactly.
//
// Tip round.  One thread per vertex; a start vertex (in-degree 0, out-degree >= 1) walks at most max_tip_reads steps over the round's
// snapshot (the CSR the round began with) and, when the walk stops at a fork (IN / OUT), walks it again storing 1 into the per-read hit
// byte of every chain vertex: colliding stores write the same value.  Then filter, scan, compact as the build does.
//
// Compaction.  succ / pred from mergeability (v -> w with out-degree(v) == 1 and in-degree(w) == 1).  List ranking by pointer jumping
// towards the path's head: a double-buffered (ptr, rank, dist) record of 16 bytes per vertex, ceil(log2(2 nreads)) rounds, a head points
// at itself with rank 0.  Vertices whose pointer does not rest on a head afterwards are on all-mergeable cycles: the same jumping carries
// the minimum of v and of v ^ 1 around the cycle, the minimum vertex becomes the head (its in-edge is cut) and the ranking runs once more.
// Nothing walks a chain, so a unitig as long as the genome costs the same O(log n) launches.
//
// Sequence gather.  Work is distributed over OUTPUT bases: one lane per 16 consecutive bases finds its segment (unitig vertex) by
// bisection over the global segment offsets and stores its 16 bytes with one 128-bit store, so a wavefront writes 1 KiB contiguous.  A
// lane whose 16 bases lie inside one segment takes them from two packed words with a 64-bit shift (reversed and complemented for
// orientation 1); a lane that straddles segments, or whose segments are shorter than 16 bases, takes them base by base.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "graph.hpp"

namespace bella {

constexpr uint32_t kUtgNone = 0xFFFFFFFFu;
constexpr uint32_t kUtgBasesPerLane = 16;
enum { kUcTips = 0, kUcReads, kUcCycle, kUcCount };      // device counters (uint32 each)

struct UtgRank {           // pointer jumping towards the head
    uint32_t ptr, rank;
    uint64_t dist;         // sum of the edge lens from the head
};
struct UtgMin {            // ... and around a cycle
    uint32_t ptr, mn, mn2, pad;
};

#if defined(__HIPCC__)
// ---- tip clipping ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tip_walk(const uint32_t* off, const bella_graph_edge* E, uint32_t nv, uint32_t max_tip, uint8_t* hit, uint32_t* counters) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    bool tip = false;
    if (v < nv && off[(v ^ 1u) + 1] == off[v ^ 1u] && off[v + 1] > off[v]) {
        uint32_t cur = v, n = 1;
        for (;;) {
            const uint32_t d = off[cur + 1] - off[cur];
            if (d == 0) break;                                          // END
            if (d > 1) { tip = true; break; }                           // OUT
            const uint32_t w = E[off[cur]].dst;
            if (off[(w ^ 1u) + 1] - off[w ^ 1u] != 1) { tip = true; break; }   // IN
            if (n == max_tip || n >= nv) break;                         // LONG (a chain never revisits a vertex: n < nv)
            cur = w;
            ++n;
        }
        if (tip) {
            cur = v;
            for (uint32_t i = 0; i < n; ++i) {
                hit[cur >> 1] = 1;
                if (i + 1 < n) cur = E[off[cur]].dst;
            }
        }
    }
    graph_count(counters + kUcTips, tip);
}

// ---- compaction ------------------------------------------------------------------------------------------------------------------------
// pred is all ones on entry; an in-degree-1 vertex has one writer
__global__ void k_utg_succ(const uint32_t* off, const bella_graph_edge* E, uint32_t nv, uint32_t* succ, uint32_t* pred, uint32_t* outlen, uint32_t* inlen) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    uint32_t s = kUtgNone, l = 0;
    if (off[v + 1] - off[v] == 1) {
        const bella_graph_edge e = E[off[v]];
        if (off[(e.dst ^ 1u) + 1] - off[e.dst ^ 1u] == 1) {
            s = e.dst; l = e.len;
            pred[e.dst] = v;
            inlen[e.dst] = e.len;
        }
    }
    succ[v] = s;
    outlen[v] = l;
}

__device__ __forceinline__ bool utg_is_head(const uint32_t* pred, const uint8_t* cut, uint32_t v) { return pred[v] == kUtgNone || (cut && cut[v]); }

__global__ void k_utg_rank_init(const uint32_t* pred, const uint32_t* inlen, const uint8_t* cut, uint32_t nv, UtgRank* st) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    st[v] = utg_is_head(pred, cut, v) ? UtgRank{v, 0u, 0ull} : UtgRank{pred[v], 1u, (uint64_t)inlen[v]};
}

__global__ void k_utg_rank_jump(const UtgRank* in, UtgRank* out, uint32_t nv) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const UtgRank s = in[v], q = in[s.ptr];
    out[v] = UtgRank{q.ptr, s.rank + q.rank, s.dist + q.dist};
}

// vertices whose pointer does not rest on a head: on a cycle
__global__ __launch_bounds__(256) void k_utg_cycle_count(const UtgRank* st, const uint32_t* pred, uint32_t nv, uint32_t* counters) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    graph_count(counters + kUcCycle, v < nv && pred[st[v].ptr] != kUtgNone);
}

__global__ void k_utg_min_init(const uint32_t* pred, uint32_t nv, UtgMin* st) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    st[v] = UtgMin{pred[v] == kUtgNone ? v : pred[v], v, v ^ 1u, 0u};
}

__global__ void k_utg_min_jump(const UtgMin* in, UtgMin* out, uint32_t nv) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const UtgMin s = in[v], q = in[s.ptr];
    out[v] = UtgMin{q.ptr, s.mn < q.mn ? s.mn : q.mn, s.mn2 < q.mn2 ? s.mn2 : q.mn2, 0u};
}

// the smallest vertex of every cycle becomes a head; cmin2 = the smallest vertex of the mirror cycle
__global__ void k_utg_cut(const UtgRank* rank, const UtgMin* mn, const uint32_t* pred, uint32_t nv, uint8_t* cut, uint32_t* cmin2) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const bool on_cycle = pred[rank[v].ptr] != kUtgNone;
    cut[v] = (on_cycle && mn[v].mn == v) ? 1 : 0;
    cmin2[v] = mn[v].mn2;
}

__device__ __forceinline__ bool utg_is_tail(const uint32_t* succ, const uint8_t* cut, uint32_t v) { return succ[v] == kUtgNone || (cut && cut[succ[v]]); }

__global__ void k_utg_tail(const UtgRank* st, const uint32_t* succ, const uint8_t* cut, const uint8_t* dead, uint32_t nv, uint32_t* tail_of, uint32_t* cnt_of) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || dead[v >> 1] || !utg_is_tail(succ, cut, v)) return;
    tail_of[st[v].ptr] = v;
    cnt_of[st[v].ptr] = st[v].rank + 1;
}

// emit[v] = v heads an emitted unitig; nvert[v] = its vertices (both 0 at v == nv: the scans' last element)
__global__ void k_utg_select(const uint32_t* pred, const uint8_t* cut, const uint32_t* cmin2, const uint8_t* dead, const uint32_t* tail_of, const uint32_t* cnt_of, uint32_t nv,
                             uint32_t* emit, uint32_t* nvert) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > nv) return;
    bool e = false;
    if (v < nv && !dead[v >> 1] && utg_is_head(pred, cut, v)) e = (cut && cut[v]) ? v <= cmin2[v] : v <= (tail_of[v] ^ 1u);
    emit[v] = e ? 1u : 0u;
    nvert[v] = e ? cnt_of[v] : 0u;
}

__global__ void k_utg_scatter(const UtgRank* st, const uint32_t* succ, const uint32_t* outlen, const uint32_t* inlen, const uint8_t* cut, const uint8_t* dead,
                              const uint64_t* rbeg, const uint64_t* rend, const uint32_t* emit, const uint32_t* uid, const uint32_t* voff, uint32_t nv, uint32_t* verts,
                              uint64_t* pos, uint32_t* nb, uint32_t* slot_utg, uint64_t* u_voff, uint64_t* u_len, uint8_t* u_circ) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv || dead[v >> 1]) return;
    const UtgRank s = st[v];
    const uint32_t h = s.ptr;
    if (!emit[h]) return;
    const uint32_t u = uid[h], slot = voff[h] + s.rank;
    const bool tail = utg_is_tail(succ, cut, v), circ = cut && cut[h];
    const uint32_t r = v >> 1;
    const uint32_t n = tail ? (circ ? inlen[h] : (uint32_t)(rend[r] - rbeg[r])) : outlen[v];
    verts[slot] = v;
    pos[slot] = s.dist;
    nb[slot] = n;
    slot_utg[slot] = u;
    if (v == h) { u_voff[u] = voff[h]; u_circ[u] = circ ? 1 : 0; }
    if (tail) u_len[u] = s.dist + n;
}

// gseg[slot] = where the slot's bases begin among all unitig bases; gseg[nseg] = their total
__global__ void k_utg_segoff(const uint32_t* slot_utg, const uint64_t* pos, const uint64_t* u_boff, uint32_t nseg, uint32_t nutg, uint64_t* gseg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > nseg) return;
    gseg[i] = i < nseg ? u_boff[slot_utg[i]] + pos[i] : u_boff[nutg];
}

// flag[i] = edge i is not mergeable (a link); flag[m] = 0
__global__ void k_utg_linkflag(const bella_graph_edge* E, uint32_t m, const uint32_t* succ, uint8_t* flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    flag[i] = (i < m && succ[E[i].src] != E[i].dst) ? 1 : 0;
}

__global__ void k_utg_links(const bella_graph_edge* E, const uint8_t* flag, const uint32_t* lscan, uint32_t m, const UtgRank* st, const uint32_t* uid, const uint32_t* tail_of,
                            bella_unitig_link* links) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || !flag[i]) return;
    const bella_graph_edge e = E[i];
    const uint32_t v = e.src, w = e.dst, h = st[v].ptr, t = tail_of[w];      // v ends the path that h heads; w heads the path that t ends
    bella_unitig_link l;
    l.flags = 0;
    if (h <= (v ^ 1u)) l.a = uid[h]; else { l.a = uid[v ^ 1u]; l.flags |= BELLA_UNITIG_LINK_A_MINUS; }
    if (w <= (t ^ 1u)) l.b = uid[w]; else { l.b = uid[t ^ 1u]; l.flags |= BELLA_UNITIG_LINK_B_MINUS; }
    l.ovl = e.ovl; l.rec = e.rec; l.edge = i;
    links[lscan[i]] = l;
}

// ---- sequence gather -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t utg_ascii(uint32_t code) { return (0x54474341u >> (8 * code)) & 0xFFu; }     // "ACGT"

// 16 codes (2 bits each, base j at bits 2 j) of the packed reads from base index g on
__device__ __forceinline__ uint32_t utg_codes16(const uint32_t* packed, uint64_t g) {
    const uint64_t w = g >> 4;
    const uint32_t sh = (uint32_t)(g & 15) * 2;
    const uint64_t two = (uint64_t)packed[w] | (sh ? (uint64_t)packed[w + 1] << 32 : 0ull);
    return (uint32_t)(two >> sh);
}

// out holds ceil(total / 16) * 16 bytes; packed: the loaded reads; rbeg[r] / rend[r]: where read r's span begins and ends among all
// bases (whole reads: roff and roff + 1; clipped reads: trim.hpp's spans); gseg[nseg + 1], verts[nseg], nb[nseg]
__global__ __launch_bounds__(256) void k_utg_gather(const uint64_t* gseg, const uint32_t* verts, const uint32_t* nb, uint32_t nseg, uint64_t total, const uint64_t* rbeg,
                                                    const uint64_t* rend, const uint32_t* packed, uint4* out) {
    const uint64_t lane = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t g0 = lane * kUtgBasesPerLane;
    if (g0 >= total) return;
    uint32_t lo = 0, hi = nseg;                                         // the last segment with gseg[s] <= g0
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (gseg[mid] <= g0) lo = mid; else hi = mid;
    }
    uint32_t s = lo;
    uint64_t beg = gseg[s], end = gseg[s + 1];
    uint32_t codes;
    if (g0 + kUtgBasesPerLane <= end) {                                 // all 16 bases inside one segment
        const uint32_t v = verts[s], r = v >> 1;
        const uint64_t i = g0 - beg;
        if (!(v & 1u)) codes = utg_codes16(packed, rbeg[r] + i);
        else {
            uint32_t x = utg_codes16(packed, rend[r] - 16 - i);         // bases L-1-i-15 .. L-1-i of the span, to be reversed and complemented
            x = __brev(x);
            x = ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
            codes = ~x;
        }
    } else {
        codes = 0;
        for (uint32_t j = 0; j < kUtgBasesPerLane; ++j) {
            const uint64_t g = g0 + j;
            if (g >= total) break;
            while (g >= end && s + 1 < nseg) { ++s; beg = end; end = gseg[s + 1]; }
            const uint32_t v = verts[s], r = v >> 1;
            const uint64_t i = g - beg;
            const uint64_t at = (v & 1u) ? rend[r] - 1 - i : rbeg[r] + i;
            uint32_t code = (packed[at >> 4] >> ((uint32_t)(at & 15) * 2)) & 3u;
            if (v & 1u) code ^= 3u;
            codes |= code << (2 * j);
        }
    }
    uint32_t w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t c4 = codes >> (8 * q);
        w[q] = utg_ascii(c4 & 3u) | utg_ascii((c4 >> 2) & 3u) << 8 | utg_ascii((c4 >> 4) & 3u) << 16 | utg_ascii((c4 >> 6) & 3u) << 24;
    }
    out[lane] = make_uint4(w[0], w[1], w[2], w[3]);
}
#endif

}  // namespace bella
