// graph.hpp -- string graph of the traced overlaps on gfx950: overlap classes, containment, per-vertex lists, Myers' transitive reduction.
//
// Nothing in the reference does this (it ends at the overlap / alignment file); the definition is this project's own and is written
// down in DESIGN.md section 11 and in include/bella_hip.h.  Everything is an integer, so the result is the numpy mirror's exactly.
//
// Passes.  k_graph_classify: one thread per record, the class and the record's two edge candidates (2 i and 2 i + 1: an edge's twin is
// the other candidate of its record), contained flags with ordinary atomics; with the clips of trim.hpp the record is cut first.  k_graph_filter: candidates without a contained end, their
// degrees.  The lists: two stable device radix sorts (by dst, then by src << 32 | len; a dropped candidate's key is all ones and lands
// behind the kept ones), an exclusive scan of the degrees, a gather that also records where every candidate went (pos: the twin pass
// finds an edge's twin there without a search).
//
// Mapping of the reduction.  One wavefront per vertex v, four independent wavefronts per workgroup, no workgroup barrier.  v's neighbour
// set sits in the wavefront's LDS slice: an open-addressing table dst -> slot of 2 x degree slots (at most kGraphSlots) and one mark byte
// per slot (INPLAY / ELIMINATED); the duplicate-(src, dst) check falls out of the insert.  The loop over v -> w is wave-uniform and serial
// (step 2 reads w's mark "at that moment"); the lanes stride over w's list in global memory and look x up in the table; the lists are
// ordered by len, so "stop at the first edge over the threshold" is a wave ballot.  Marks only move INPLAY -> ELIMINATED, so the lanes'
// order inside one list does not matter.  A vertex with more than kGraphLdsCap neighbours takes the same walk with its neighbour set in
// global memory: the vertex's dst values sorted (one more radix sort over the edges, only when such a vertex exists) searched by
// bisection, the marks beside them.  Degrees at 30x coverage are a few tens: 5 KB of LDS per wavefront keeps 24 wavefronts on a CU.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"

namespace bella {

constexpr uint32_t kGraphLdsCap = 512;      // neighbours the LDS table of a wavefront holds
constexpr uint32_t kGraphSlots = 1024;      // its slots (load <= 1/2)
constexpr int kGraphBlock = 256;            // four independent wavefronts
constexpr uint32_t kGraphNone = 0xFFFFFFFFu;
enum { kGrInplay = 1, kGrEliminated = 2 };
// device counters of a build (uint32 each)
enum { kGcShort = 0, kGcInternal, kGcEdgesAll, kGcEdgesKept, kGcReduced, kGcContained, kGcMaxDegree, kGcOvercap, kGcDuplicate, kGcFinal, kGcOutside, kGcCount };

struct GraphKeyDst {       // the low word of a (src << 32 | dst) key
    __host__ __device__ uint32_t operator()(const uint64_t& v) const { return (uint32_t)v; }
};

#if defined(__HIPCC__)
__device__ __forceinline__ void graph_count(uint32_t* counter, bool pred) {          // one atomic per wavefront
    const unsigned long long m = __ballot(pred);
    if (m && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1) atomicAdd(counter, (uint32_t)__popcll(m));
}

// clip == nullptr: the records as they are.  Otherwise every record is cut to its reads' clips first (trim.hpp): a
// record with an uncovered read or an emptied interval is OUTSIDE, gives no candidates and is counted; the others are classified in
// clipped coordinates with the clipped lengths.
__global__ __launch_bounds__(256) void k_graph_classify(const bella_overlap* recs, uint32_t n, const uint64_t* roff, const bella_read_clip* clip, uint32_t min_overlap,
                                                        uint32_t max_overhang, uint32_t permille, bella_graph_edge* cand, uint32_t* contained, uint32_t* counters) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    bool is_short = false, is_internal = false, is_outside = false;
    if (live) {
        const bella_overlap r = recs[i];
        int64_t l1 = (int64_t)(roff[r.cid + 1] - roff[r.cid]), l2 = (int64_t)(roff[r.rid + 1] - roff[r.rid]);
        int64_t b1 = r.begV, e1 = r.endV, b2 = r.begH, e2 = r.endH;
        const uint32_t s = r.strand ? 1u : 0u;
        if (clip) {
            const bella_read_clip c1 = clip[r.cid], c2 = clip[r.rid];
            if (c1.end == c1.beg || c2.end == c2.beg) is_outside = true;
            else {
                const int64_t cs1 = c1.beg, ce1 = c1.end, c2s = s ? l2 - (int64_t)c2.end : (int64_t)c2.beg, c2e = s ? l2 - (int64_t)c2.beg : (int64_t)c2.end;
                int64_t db = cs1 - b1 > c2s - b2 ? cs1 - b1 : c2s - b2, de = e1 - ce1 > e2 - c2e ? e1 - ce1 : e2 - c2e;
                db = db > 0 ? db : 0; de = de > 0 ? de : 0;
                b1 += db; b2 += db; e1 -= de; e2 -= de;
                if (e1 <= b1 || e2 <= b2) is_outside = true;
                else { b1 -= cs1; e1 -= cs1; b2 -= c2s; e2 -= c2s; l1 = ce1 - cs1; l2 = c2e - c2s; }
            }
        }
        const int64_t t1 = l1 - e1, t2 = l2 - e2;
        bella_graph_edge a{kGraphNone, kGraphNone, 0, 0, i, 0}, b{kGraphNone, kGraphNone, 0, 0, i, BELLA_GRAPH_EDGE_TWIN};
        const int64_t overhang = (b1 < b2 ? b1 : b2) + (t1 < t2 ? t1 : t2), maplen = e1 - b1 > e2 - b2 ? e1 - b1 : e2 - b2;
        if (is_outside) {}
        else if (e1 - b1 < (int64_t)min_overlap || e2 - b2 < (int64_t)min_overlap) is_short = true;
        else if (overhang > (int64_t)max_overhang || (uint64_t)(1000 * overhang) > (uint64_t)permille * (uint64_t)maplen) is_internal = true;
        else if (b1 <= b2 && t1 <= t2) atomicOr(contained + r.cid, 1u);
        else if (b1 >= b2 && t1 >= t2) atomicOr(contained + r.rid, 1u);
        else if (b1 > b2) {
            a.src = 2 * r.cid; a.dst = 2 * r.rid + s; a.len = (uint32_t)(b1 - b2); a.ovl = (uint32_t)(l1 - (b1 - b2));
            b.src = 2 * r.rid + (s ^ 1u); b.dst = 2 * r.cid + 1; b.len = (uint32_t)(t2 - t1); b.ovl = (uint32_t)(l2 - (t2 - t1));
        } else {
            a.src = 2 * r.rid + s; a.dst = 2 * r.cid; a.len = (uint32_t)(b2 - b1); a.ovl = (uint32_t)(l2 - (b2 - b1));
            b.src = 2 * r.cid + 1; b.dst = 2 * r.rid + (s ^ 1u); b.len = (uint32_t)(t1 - t2); b.ovl = (uint32_t)(l1 - (t1 - t2));
        }
        cand[2 * (size_t)i] = a;
        cand[2 * (size_t)i + 1] = b;
    }
    graph_count(counters + kGcShort, is_short);
    graph_count(counters + kGcInternal, is_internal);
    if (clip) graph_count(counters + kGcOutside, is_outside);
}

// candidates without a contained end: ok[e], the degree of their source, the first sort's key (dst) and value (e)
__global__ __launch_bounds__(256) void k_graph_filter(const bella_graph_edge* cand, uint32_t ncand, const uint32_t* contained, uint8_t* ok, uint32_t* deg, uint32_t* key1,
                                                      uint32_t* idx, uint32_t* counters) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    bool exists = false, kept = false;
    if (e < ncand) {
        const uint32_t src = cand[e].src, dst = cand[e].dst;
        exists = src != kGraphNone;
        kept = exists && !contained[src >> 1] && !contained[dst >> 1];
        ok[e] = kept ? 1 : 0;
        key1[e] = kept ? dst : kGraphNone;
        idx[e] = e;
        if (kept) atomicAdd(deg + src, 1u);
    }
    graph_count(counters + kGcEdgesAll, exists);
    graph_count(counters + kGcEdgesKept, kept);
}

// the second sort's key of the candidates in dst order: src << 32 | len; all ones for a dropped candidate
__global__ void k_graph_key2(const bella_graph_edge* cand, const uint8_t* ok, const uint32_t* idx, uint32_t ncand, uint64_t* key2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncand) return;
    const uint32_t e = idx[i];
    key2[i] = ok[e] ? ((uint64_t)cand[e].src << 32 | cand[e].len) : ~0ull;
}

// edges[i] = the i-th kept candidate in (src, len, dst) order; pos[candidate] = i; bykey[i] = src << 32 | dst (the over-cap path sorts these)
__global__ void k_graph_gather(const bella_graph_edge* cand, const uint32_t* idx, uint32_t m, bella_graph_edge* edges, uint32_t* pos, uint64_t* bykey) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t e = idx[i];
    const bella_graph_edge g = cand[e];
    edges[i] = g;
    pos[e] = i;
    bykey[i] = (uint64_t)g.src << 32 | g.dst;
}

__global__ void k_graph_vertex_stats(const uint32_t* off, uint32_t nv, const uint32_t* contained, uint32_t nreads, uint32_t cap, uint32_t* counters) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t deg = v < nv ? off[v + 1] - off[v] : 0u;
    if (deg) atomicMax(counters + kGcMaxDegree, deg);
    graph_count(counters + kGcOvercap, deg > cap);
    graph_count(counters + kGcContained, v < nreads && (contained[v] & 1u) != 0);      // (bit 1: uncovered, trim.hpp)
}

__device__ __forceinline__ void graph_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

// The neighbour set of one vertex, in LDS (a hash table) or in global memory (sorted dst values): find(x) = where x's mark byte lives.
struct GraphSetLds {
    uint32_t* key;
    volatile uint8_t* mark;
    uint32_t mask;
    __device__ __forceinline__ volatile uint8_t* find(uint32_t x) const {
        uint32_t h = (x * 0x9E3779B1u >> 12) & mask;
        for (;;) {
            const uint32_t k = key[h];
            if (k == x) return mark + h;
            if (k == kGraphNone) return nullptr;
            h = (h + 1) & mask;
        }
    }
};
struct GraphSetGlobal {
    const uint64_t* sorted;        // the vertex's (src << 32 | dst) keys, ascending
    volatile uint8_t* mark;
    uint32_t n;
    __device__ __forceinline__ volatile uint8_t* find(uint32_t x) const {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if ((uint32_t)sorted[mid] < x) lo = mid + 1; else hi = mid;
        }
        return lo < n && (uint32_t)sorted[lo] == x ? mark + lo : nullptr;
    }
};

// steps 2 to 4 of the reduction for the vertex whose out-edges are E[a, b); every neighbour's mark is INPLAY on entry
template <class Set>
__device__ __forceinline__ uint32_t graph_reduce_vertex(const Set& S, const uint32_t* off, const bella_graph_edge* E, uint32_t a, uint32_t b, uint32_t fuzz, int lane,
                                                        uint8_t* reduced) {
    const uint64_t L = (uint64_t)E[b - 1].len + fuzz;
    for (uint32_t e = a; e < b; ++e) {                                  // step 2: serial over w
        const uint32_t w = E[e].dst, lvw = E[e].len;
        if (*S.find(w) != kGrInplay) continue;                          // (wave-uniform)
        const uint32_t wa = off[w], wb = off[w + 1];
        for (uint32_t j0 = wa; j0 < wb; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool in = j < wb;
            const uint32_t x = in ? E[j].dst : 0u, lx = in ? E[j].len : 0u;
            const bool over = in && (uint64_t)lvw + lx > L;
            if (in && !over) {
                volatile uint8_t* const p = S.find(x);
                if (p && *p == kGrInplay) *p = kGrEliminated;
            }
            if (__ballot(over)) break;                                  // the list is ordered by len: everything behind is over too
        }
        graph_fence();                                                  // the next w reads its mark after this list's writes
    }
    for (uint32_t e = a; e < b; ++e) {                                  // step 3: whatever w's mark; index 0 and the edges shorter than fuzz
        const uint32_t w = E[e].dst;
        const uint32_t wa = off[w], wb = off[w + 1];
        for (uint32_t j0 = wa; j0 < wb; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool in = j < wb;
            const uint32_t x = in ? E[j].dst : 0u, lx = in ? E[j].len : 0u;
            const bool take = in && (j == wa || lx < fuzz);
            if (take) {
                volatile uint8_t* const p = S.find(x);
                if (p && *p == kGrInplay) *p = kGrEliminated;
            }
            if (__ballot(in && !take)) break;
        }
    }
    graph_fence();
    uint32_t nred = 0;
    for (uint32_t j = a + lane; j < b; j += 64) {                        // step 4
        const bool r = *S.find(E[j].dst) == kGrEliminated;
        reduced[j] = r ? 1 : 0;
        nred += r ? 1u : 0u;
    }
    return nred;
}

// off / E: the lists.  bykey (sorted by src << 32 | dst, same offsets) and gmark (one byte per edge): the over-cap path's neighbour sets;
// both may be null when no vertex is over the cap and force_global == 0.
__global__ __launch_bounds__(kGraphBlock) void k_graph_reduce(const uint32_t* off, const bella_graph_edge* E, uint32_t nv, uint32_t fuzz, uint32_t force_global,
                                                              const uint64_t* bykey, uint8_t* gmark, uint8_t* reduced, uint32_t* counters) {
    __shared__ uint32_t s_key[kGraphBlock / 64][kGraphSlots];
    __shared__ uint8_t s_mark[kGraphBlock / 64][kGraphSlots];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const uint32_t v = blockIdx.x * (kGraphBlock / 64) + wave;
    if (v >= nv) return;                                                // (whole wavefronts leave)
    const uint32_t a = off[v], b = off[v + 1], deg = b - a;
    if (!deg) return;
    uint32_t nred = 0;
    bool dup = false;
    if (!force_global && deg <= kGraphLdsCap) {
        uint32_t slots = 64;
        while (slots < 2 * deg) slots <<= 1;
        GraphSetLds S{s_key[wave], s_mark[wave], slots - 1};
        for (uint32_t h = lane; h < slots; h += 64) S.key[h] = kGraphNone;
        graph_fence();
        for (uint32_t j = a + lane; j < b; j += 64) {
            const uint32_t d = E[j].dst;
            uint32_t h = (d * 0x9E3779B1u >> 12) & S.mask;
            for (;;) {
                const uint32_t old = atomicCAS(S.key + h, kGraphNone, d);
                if (old == kGraphNone) { S.mark[h] = kGrInplay; break; }
                if (old == d) { dup = true; break; }
                h = (h + 1) & S.mask;
            }
        }
        graph_fence();
        if (!__ballot(dup)) nred = graph_reduce_vertex(S, off, E, a, b, fuzz, lane, reduced);
    } else {
        GraphSetGlobal S{bykey + a, gmark + a, deg};
        for (uint32_t j = lane; j < deg; j += 64) {
            S.mark[j] = kGrInplay;
            if (j && (uint32_t)S.sorted[j] == (uint32_t)S.sorted[j - 1]) dup = true;
        }
        graph_fence();
        if (!__ballot(dup)) nred = graph_reduce_vertex(S, off, E, a, b, fuzz, lane, reduced);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) nred += __shfl_xor(nred, d, 64);
    if (lane == 0 && nred) atomicAdd(counters + kGcReduced, nred);
    if (dup) atomicOr(counters + kGcDuplicate, 1u);
}

// an edge stays when neither it nor its twin (the other candidate of its record) was reduced
__global__ void k_graph_symmetric(const bella_graph_edge* E, uint32_t m, const uint32_t* pos, const uint8_t* reduced, uint8_t* keep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    if (i == m) { keep[m] = 0; return; }                                // (the scan's last element)
    const uint32_t t = pos[(2 * E[i].rec + (E[i].flags & BELLA_GRAPH_EDGE_TWIN)) ^ 1u];
    keep[i] = (reduced[i] | reduced[t]) ? 0 : 1;
}

// scan[i] = kept edges before i: the final edges, and the final offsets of the vertices
__global__ void k_graph_compact(const bella_graph_edge* E, const uint8_t* keep, const uint32_t* scan, uint32_t m, bella_graph_edge* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && keep[i]) out[scan[i]] = E[i];
}
__global__ void k_graph_new_offsets(const uint32_t* off, const uint32_t* scan, uint32_t nv, uint32_t* out) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v <= nv) out[v] = scan[off[v]];
}

// What a round of tip clipping (unitig.hpp) and of bubble popping (bubble.hpp) share once it has marked its reads in `hit`:
// removed |= hit, and the round's reads into the stage's counter
__global__ __launch_bounds__(256) void k_graph_mark_reads(const uint8_t* hit, uint32_t nr, uint8_t* removed, uint32_t* counter) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    const bool h = r < nr && hit[r];
    if (h) removed[r] = 1;
    graph_count(counter, h);
}

// keep[i] = neither end of edge i was hit and (ekill != NULL) the edge was not killed itself; keep[m] = 0 (the scan's last element)
__global__ void k_graph_keep_filter(const bella_graph_edge* E, uint32_t m, const uint8_t* hit, const uint8_t* ekill, uint8_t* keep) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    keep[i] = (i < m && !(hit[E[i].src >> 1] | hit[E[i].dst >> 1] | (ekill ? ekill[i] : 0))) ? 1 : 0;
}

// Weak-overlap removal: edge v -> w is weak iff 1000 ovl < permille best(v), best(v) = the ovl of the first edge of
// v's list (the list is ordered by len and its edges share the source read's length).  One thread per edge: its own weakness, then its
// twin's, found by a serial scan of the list of dst ^ 1 as k_bub_apply finds it (a handful of edges after the reduction; at most the
// degree of a hub); ekill[j] = either.  Every byte has one writer.  Thread j < nv also counts vertex j when it is a fork.
enum { kWcForks = 0, kWcWeak, kWcRemoved, kWcCount };                  // device counters (uint32 each)
__device__ __forceinline__ bool graph_is_weak(uint32_t ovl, uint32_t best, uint32_t permille) { return 1000ull * ovl < (uint64_t)permille * best; }
__global__ __launch_bounds__(256) void k_graph_weak(const uint32_t* off, const bella_graph_edge* E, uint32_t m, uint32_t nv, uint32_t permille, uint8_t* ekill,
                                                    uint32_t* counters) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    bool weak = false, gone = false;
    if (j < m) {
        const uint32_t s = E[j].src, d = E[j].dst;
        weak = graph_is_weak(E[j].ovl, E[off[s]].ovl, permille);
        bool twin_weak = false;
        const uint32_t ta = off[d ^ 1u], tb = off[(d ^ 1u) + 1];
        for (uint32_t q = ta; q < tb; ++q)
            if (E[q].dst == (s ^ 1u)) { twin_weak = graph_is_weak(E[q].ovl, E[ta].ovl, permille); break; }
        gone = weak | twin_weak;
        ekill[j] = gone ? 1 : 0;
    }
    graph_count(counters + kWcForks, j < nv && off[j + 1] - off[j] >= 2);
    graph_count(counters + kWcWeak, weak);
    graph_count(counters + kWcRemoved, gone);
}
#endif

}  // namespace bella
