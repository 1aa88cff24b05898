// trim.hpp -- coverage trimming of the reads before the string graph on gfx950: every read is clipped to its longest stretch that at
// least min_depth overlap records cover (the stage is miniasm's ma_hit_sub, the cut of the records ma_hit_cut).
//
// Nothing in the reference does this.  Everything is an integer, so the result is the numpy mirror's exactly.
//
// Passes.  k_trim_events: one thread per record, its (at most) two shrunk intervals as four 64-bit keys read << 32 | pos << 1 | is_start;
// a skipped interval writes all ones, which sort behind every real key.  One device radix sort of the keys.  k_trim_offsets: where every
// read's events begin among the sorted keys (a bisection per read).  k_trim_sweep: one wavefront per read, four independent wavefronts
// per workgroup, no workgroup barrier, no LDS, no atomics.  The lanes take the read's events 64 at a time; a shuffle scan of +1 / -1
// gives the running depth, the carry stays in a register.  Depth is judged after ALL events of a position, so a lane is decisive only
// where the next key has another position (an end sorts before a start of the same position; both are counted before anyone looks).  Among
// the decisive lanes a region starts where depth >= min_depth follows a lane below it and ends at the next lane below it: two ballots.
// A lane that ends a region finds its start with a shuffle from the last start lane below it (or the start carried from an earlier
// chunk); the best (length, -start), the number of regions and the largest depth are reduced over the lanes and carried across chunks.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"

namespace bella {

constexpr int kTrimBlock = 256;             // four independent wavefronts
constexpr uint64_t kTrimNoEvent = ~0ull;

// the shrunk interval of [b, e) on a read of l bases: false when nothing is left
__host__ __device__ inline bool trim_shrink(int64_t b, int64_t e, int64_t l, int64_t end_clip, int64_t* s, int64_t* t) {
    *s = b <= end_clip ? b : b + end_clip;
    *t = l - e <= end_clip ? e : e - end_clip;
    return *t > *s;
}

#if defined(__HIPCC__)
// keys[4 i .. 4 i + 3]: V's start and end, H's start and end (H in its own coordinates); nint += the intervals written
__global__ __launch_bounds__(256) void k_trim_events(const bella_overlap* recs, uint32_t n, const uint64_t* roff, uint32_t end_clip, uint32_t min_span, uint64_t* keys,
                                                     uint32_t* nint) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t made = 0;
    if (i < n) {
        const bella_overlap r = recs[i];
        const int64_t l1 = (int64_t)(roff[r.cid + 1] - roff[r.cid]), l2 = (int64_t)(roff[r.rid + 1] - roff[r.rid]);
        const int64_t b1 = r.begV, e1 = r.endV, b2 = r.strand ? l2 - r.endH : r.begH, e2 = r.strand ? l2 - r.begH : r.endH;
        uint64_t k[4] = {kTrimNoEvent, kTrimNoEvent, kTrimNoEvent, kTrimNoEvent};
        if (e1 - b1 >= (int64_t)min_span && e2 - b2 >= (int64_t)min_span) {
            int64_t s, t;
            if (trim_shrink(b1, e1, l1, end_clip, &s, &t)) {
                k[0] = (uint64_t)r.cid << 32 | (uint64_t)s << 1 | 1u;
                k[1] = (uint64_t)r.cid << 32 | (uint64_t)t << 1;
                ++made;
            }
            if (trim_shrink(b2, e2, l2, end_clip, &s, &t)) {
                k[2] = (uint64_t)r.rid << 32 | (uint64_t)s << 1 | 1u;
                k[3] = (uint64_t)r.rid << 32 | (uint64_t)t << 1;
                ++made;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) keys[4 * (size_t)i + j] = k[j];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) made += __shfl_xor(made, d, 64);
    if ((threadIdx.x & 63) == 0 && made) atomicAdd(nint, made);         // (a statistic; the clips need no atomics)
}

// evoff[r] = the first sorted key of read r or a later one, r in [0, nreads]; all-ones keys lie behind evoff[nreads]
__global__ void k_trim_offsets(const uint64_t* keys, uint64_t nkeys, uint32_t nreads, uint32_t* evoff) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > nreads) return;
    const uint64_t want = (uint64_t)r << 32;
    uint64_t lo = 0, hi = nkeys;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    evoff[r] = (uint32_t)lo;
}

__global__ __launch_bounds__(kTrimBlock) void k_trim_sweep(const uint64_t* keys, const uint32_t* evoff, uint32_t nreads, uint32_t min_depth, uint32_t min_span,
                                                           bella_read_clip* clip) {
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t r = blockIdx.x * (kTrimBlock / 64) + (threadIdx.x >> 6);
    if (r >= nreads) return;                                            // (whole wavefronts leave)
    const uint32_t a = evoff[r], b = evoff[r + 1];
    int32_t carry = 0;                                                  // depth behind the chunks so far
    uint32_t open_start = 0, nregions = 0, max_depth = 0;
    bool prev_cov = false;                                              // the last decisive lane so far had depth >= min_depth
    uint64_t best = 0;                                                  // len << 32 | ~start of the best region so far (0: none)
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (uint32_t c0 = a; c0 < b; c0 += 64) {
        const uint32_t j = c0 + (uint32_t)lane;
        const bool in = j < b;
        const uint64_t key = in ? keys[j] : 0ull;
        const uint64_t next = (in && j + 1 < b) ? keys[j + 1] : kTrimNoEvent;
        const uint32_t pos = (uint32_t)key >> 1;
        int32_t depth = in ? ((key & 1u) ? 1 : -1) : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t up = __shfl_up(depth, d, 64);
            if (lane >= d) depth += up;
        }
        depth += carry;
        carry = __shfl(depth, 63, 64);
        const bool decisive = in && (next >> 1) != (key >> 1);
        const bool cov = decisive && depth >= (int32_t)min_depth;
        const unsigned long long D = __ballot(decisive), C = __ballot(cov);
        const unsigned long long dbelow = D & below;
        const bool before = dbelow ? ((C >> (63 - __clzll((long long)dbelow))) & 1ull) != 0 : prev_cov;
        const bool starts = cov && !before, ends = decisive && !cov && before;
        const unsigned long long S = __ballot(starts), E = __ballot(ends);
        const unsigned long long sbelow = S & below;
        const uint32_t from = __shfl(pos, sbelow ? 63 - __clzll((long long)sbelow) : lane, 64);
        const uint32_t start = sbelow ? from : open_start;
        uint64_t mine = ends ? ((uint64_t)(pos - start) << 32 | (0xFFFFFFFFu - start)) : 0ull;
        uint32_t dmax = decisive ? (uint32_t)depth : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = __shfl_xor(mine, d, 64);
            mine = o > mine ? o : mine;
            const uint32_t od = __shfl_xor(dmax, d, 64);
            dmax = od > dmax ? od : dmax;
        }
        best = mine > best ? mine : best;
        max_depth = dmax > max_depth ? dmax : max_depth;
        nregions += (uint32_t)__popcll(E);
        if (S) open_start = __shfl(pos, 63 - __clzll((long long)S), 64);
        if (D) prev_cov = ((C >> (63 - __clzll((long long)D))) & 1ull) != 0;
    }
    if (lane == 0) {
        const uint32_t len = (uint32_t)(best >> 32), start = 0xFFFFFFFFu - (uint32_t)best;
        bella_read_clip out{0, 0, nregions, max_depth};
        if (best && len >= min_span) { out.beg = start; out.end = start + len; }
        clip[r] = out;
    }
}

// the device flag word of a build with clips: bit 1 for an uncovered read (bit 0, contained, is set by the classification)
__global__ void k_trim_flags(const bella_read_clip* clip, uint32_t nreads, uint32_t* flags) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nreads) flags[r] = clip[r].end == clip[r].beg ? 2u : 0u;
}

// begs[r] / ends[r]: where read r's clipped bases begin and end among all bases
__global__ void k_trim_spans(const bella_read_clip* clip, const uint64_t* roff, uint32_t nreads, uint64_t* begs, uint64_t* ends) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nreads) { begs[r] = roff[r] + clip[r].beg; ends[r] = roff[r] + clip[r].end; }
}
#endif

}  // namespace bella
