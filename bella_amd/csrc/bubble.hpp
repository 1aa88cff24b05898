// bubble.hpp -- bubble popping on the reduced string graph, on gfx950.
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h) and follows
// miniasm's asg_pop_bubble.  Everything is an integer, so the result is the numpy mirror's exactly.
//
// A round.  k_bub_sources lists the vertices with two or more out-edges (in any order: a source's result does not depend on the others).
// k_bub_detect and k_bub_apply give one source to one wavefront, four independent wavefronts per workgroup, no workgroup barrier: the
// shape of the reduction kernel.  The visited set of the Kahn traversal sits in the wavefront's LDS slice (BubWave, 9,984 bytes): an
// open-addressing table vertex -> record of 512 slots and at most 256 records (r, d, c, D, p), the stack of ready records and, for the
// apply pass, one byte per record for the kept path.  The pop loop is wave-uniform and serial; the lanes stride over the popped vertex's
// out-edges.  The edges of one vertex have distinct dst, so every lane owns the record it updates and only the table insert is atomic;
// new records and stack slots are numbered by ballot.  Which ready vertex is popped first does not change (t, visited, d, c, D, p)
// (DESIGN.md section 13), so the order the lanes push in is free.
//
// k_bub_detect: a canonical success (s < t ^ 1) claims the reads of its interior with atomicMin(claim[read], s).  k_bub_apply runs the
// same traversal again -- it is deterministic and reads a few hundred bytes of CSR per source, where keeping every source's visited set
// from the first pass would take 6 KB of global memory per source and a pass to write and one to read it -- tests the claims and, for an
// accepted bubble, stores 1 into hit[read] of the interior off the kept path and into ekill[edge] of every edge inside the bubble that is
// not a path edge, and of its twin.  Plain stores: colliding writes store the same value.  Then filter, scan, compact as the tip rounds.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "graph.hpp"

namespace bella {

constexpr uint32_t kBubSlots = 512;         // the table of a wavefront (load <= 5 / 8: 256 records and the 64 keys of one refused batch)
constexpr uint32_t kBubRecords = BELLA_MAX_BUBBLE_READS + 1;
constexpr int kBubBlock = 256;              // four independent wavefronts
enum { kBcSources = 0, kBcFound, kBcPopped, kBcReads, kBcCount };      // device counters (uint32 each)

struct BubWave {                            // the LDS slice of one wavefront
    uint64_t D[kBubRecords];                // length of the best path
    uint32_t key[kBubSlots];                // vertex, or all ones
    uint32_t vtx[kBubRecords], r[kBubRecords], d[kBubRecords];
    uint16_t slot[kBubSlots];               // key's record
    uint16_t p[kBubRecords], c[kBubRecords], stack[kBubRecords];      // p: the predecessor's record
    uint8_t onk[kBubRecords];               // the record is on the kept path (apply)
};
static_assert(sizeof(BubWave) == 9984, "the LDS slice of a wavefront");

#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t bub_hash(uint32_t x) { return (x * 0x9E3779B1u >> 12) & (kBubSlots - 1); }

// the record of x, or -1
__device__ __forceinline__ int bub_find(const BubWave& W, uint32_t x) {
    uint32_t h = bub_hash(x);
    for (;;) {
        const uint32_t k = W.key[h];
        if (k == x) return (int)W.slot[h];
        if (k == kGraphNone) return -1;
        h = (h + 1) & (kBubSlots - 1);
    }
}

// detect(s) of DESIGN.md section 13 for the whole wavefront: -> the record of t (n = the records, s is record 0), or -1.  max_reads <=
// BELLA_MAX_BUBBLE_READS.  Every branch that leaves is wave-uniform.
__device__ __forceinline__ int bub_detect(BubWave& W, const uint32_t* off, const bella_graph_edge* E, uint32_t s, uint32_t max_reads, uint32_t max_dist, int lane, uint32_t& n_out) {
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t h = lane; h < kBubSlots; h += 64) W.key[h] = kGraphNone;
    graph_fence();
    if (lane == 0) {
        const uint32_t h = bub_hash(s);
        W.key[h] = s; W.slot[h] = 0;
        W.vtx[0] = s; W.r[0] = 0; W.d[0] = 0; W.c[0] = 0; W.D[0] = 0; W.p[0] = 0;
        W.stack[0] = 0;
    }
    graph_fence();
    uint32_t n = 1, sp = 1, pending = 0;
    while (sp) {
        const uint32_t vi = W.stack[--sp];
        const uint32_t v = W.vtx[vi], dv = W.d[vi], cv = W.c[vi];
        const uint64_t Dv = W.D[vi];
        const uint32_t a = off[v], b = off[v + 1];
        if (a == b) return -1;                                          // a tip inside
        for (uint32_t j0 = a; j0 < b; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool in = j < b;
            const uint32_t w = in ? E[j].dst : kGraphNone, l = in ? E[j].len : 0u;
            const bool bad = in && (w == s || (uint64_t)dv + l > max_dist);
            bool fresh = false;
            uint32_t h = 0;
            if (in && !bad) {
                h = bub_hash(w);
                for (;;) {
                    const uint32_t old = atomicCAS(&W.key[h], kGraphNone, w);
                    if (old == kGraphNone) { fresh = true; break; }
                    if (old == w) break;
                    h = (h + 1) & (kBubSlots - 1);
                }
            }
            if (__ballot(bad)) return -1;                               // a cycle through s; too far
            const unsigned long long fm = __ballot(fresh);
            const uint32_t nf = (uint32_t)__popcll(fm);
            if (n + nf - 1 > max_reads) return -1;                      // too many reads (so n + nf <= kBubRecords below)
            uint32_t wi = 0;
            if (fresh) {
                wi = n + (uint32_t)__popcll(fm & below);
                W.slot[h] = (uint16_t)wi;
                W.vtx[wi] = w; W.r[wi] = off[(w ^ 1u) + 1] - off[w ^ 1u] - 1u;
                W.d[wi] = dv + l; W.c[wi] = (uint16_t)(cv + 1); W.D[wi] = Dv + l; W.p[wi] = (uint16_t)vi;
            } else if (in) {
                wi = W.slot[h];
                if (dv + l < W.d[wi]) W.d[wi] = dv + l;
                const uint32_t cw = W.c[wi];
                const uint64_t Dw = W.D[wi];
                if (cv + 1 > cw || (cv + 1 == cw && (Dv + l > Dw || (Dv + l == Dw && v < W.vtx[W.p[wi]])))) {
                    W.c[wi] = (uint16_t)(cv + 1); W.D[wi] = Dv + l; W.p[wi] = (uint16_t)vi;
                }
                W.r[wi] -= 1u;
            }
            n += nf; pending += nf;
            graph_fence();
            if (__ballot(in && bub_find(W, w ^ 1u) >= 0)) return -1;    // both orientations of a read (w == s ^ 1 included)
            const bool ready = in && W.r[wi] == 0;
            const unsigned long long rm = __ballot(ready);
            if (ready) W.stack[sp + (uint32_t)__popcll(rm & below)] = (uint16_t)wi;
            sp += (uint32_t)__popcll(rm); pending -= (uint32_t)__popcll(rm);
            graph_fence();
        }
        if (sp == 1 && pending == 0) { n_out = n; return (int)W.stack[0]; }
    }
    return -1;                                                          // an in-edge from outside keeps some vertex waiting
}

// list[0 .. counters[kBcSources]) = the vertices with two or more out-edges, in any order
__global__ __launch_bounds__(256) void k_bub_sources(const uint32_t* off, uint32_t nv, uint32_t* list, uint32_t* counters) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    const bool src = v < nv && off[v + 1] - off[v] >= 2;
    const unsigned long long m = __ballot(src);
    if (!m) return;
    const int first = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(counters + kBcSources, (uint32_t)__popcll(m));
    base = __shfl(base, first, 64);
    if (src) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = v;
}

// claim[nreads] is all ones on entry
__global__ __launch_bounds__(kBubBlock) void k_bub_detect(const uint32_t* off, const bella_graph_edge* E, const uint32_t* list, uint32_t max_reads, uint32_t max_dist,
                                                          uint32_t* claim, uint32_t* counters) {
    __shared__ BubWave s_w[kBubBlock / 64];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const uint32_t i = blockIdx.x * (kBubBlock / 64) + wave;
    if (i >= counters[kBcSources]) return;                              // (whole wavefronts leave)
    BubWave& W = s_w[wave];
    const uint32_t s = list[i];
    uint32_t n = 0;
    const int ti = bub_detect(W, off, E, s, max_reads, max_dist, lane, n);
    if (ti < 0 || s >= (W.vtx[ti] ^ 1u)) return;                        // not found; the mirror side acts
    for (uint32_t k = 1 + lane; k < n; k += 64)
        if (k != (uint32_t)ti) atomicMin(claim + (W.vtx[k] >> 1), s);
    if (lane == 0) atomicAdd(counters + kBcFound, 1u);
}

// hit[nreads] and ekill[nedges] are zero on entry
__global__ __launch_bounds__(kBubBlock) void k_bub_apply(const uint32_t* off, const bella_graph_edge* E, const uint32_t* list, uint32_t max_reads, uint32_t max_dist,
                                                         const uint32_t* claim, uint8_t* hit, uint8_t* ekill, uint32_t* counters) {
    __shared__ BubWave s_w[kBubBlock / 64];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const uint32_t i = blockIdx.x * (kBubBlock / 64) + wave;
    if (i >= counters[kBcSources]) return;
    BubWave& W = s_w[wave];
    const uint32_t s = list[i];
    uint32_t n = 0;
    const int ti = bub_detect(W, off, E, s, max_reads, max_dist, lane, n);
    if (ti < 0 || s >= (W.vtx[ti] ^ 1u)) return;
    bool lost = false;
    for (uint32_t k = 1 + lane; k < n; k += 64) {
        W.onk[k] = 0;
        if (k != (uint32_t)ti && claim[W.vtx[k] >> 1] != s) lost = true;
    }
    if (__ballot(lost)) return;                                         // a bubble with a smaller source holds one of the reads
    graph_fence();
    if (lane == 0) {                                                    // the kept path: t, p(t), ... s
        W.onk[0] = 1;
        for (uint32_t k = (uint32_t)ti; k != 0; k = W.p[k]) W.onk[k] = 1;
    }
    graph_fence();
    for (uint32_t k = 1 + lane; k < n; k += 64)
        if (!W.onk[k]) hit[W.vtx[k] >> 1] = 1;
    for (uint32_t k = 0; k < n; ++k) {                                  // every edge inside the bubble that is not a path edge, and its twin
        const uint32_t v = W.vtx[k], a = off[v], b = off[v + 1];
        for (uint32_t j = a + lane; j < b; j += 64) {
            const uint32_t w = E[j].dst;
            const int wi = bub_find(W, w);
            if (wi < 0 || (wi != 0 && W.onk[wi] && W.p[wi] == k)) continue;
            ekill[j] = 1;
            for (uint32_t q = off[w ^ 1u], qe = off[(w ^ 1u) + 1]; q < qe; ++q)
                if (E[q].dst == (v ^ 1u)) { ekill[q] = 1; break; }
        }
    }
    if (lane == 0) atomicAdd(counters + kBcPopped, 1u);
}
#endif

}  // namespace bella
