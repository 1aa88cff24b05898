// recorrect.hpp -- read correction rounds: for every overlap record, each read's raw clip aligned against the current corrected sequence
// of the other read, the votes piled up in corrected coordinates, one more consensus; on gfx950.
//
// Nothing in the reference does this; the definition is this project's own (include/bella_hip.h; the tests hold a
// numpy statement of it).  Everything is an integer, so the result is that statement's exactly.
//
// The DP, the walks and the vote are realign.hpp's kernels, called as they stand: a ReaJob knows a query clip, a target sequence, a centre
// diagonal and a table row base, and nothing about unitigs.  What is here is what section 18 leaves to the host, because there the jobs
// are the reads of a few unitigs and here they are two per record -- millions at 100k reads:
//   k_rec_anchors   one thread per anchor: where every 256th raw base of a read lies in its corrected sequence (the emit scan).
//   k_rec_place     one thread per job: the query clip, the window [s, e) through the anchors, the centre diagonal; a bella_recorrect_job
//                   and a ReaJob without its batch fields.
//   k_rec_bytes     direction bytes of the pending jobs at band B (n B / 4); an exclusive scan (hipCUB) gives the prefix.
//   k_rec_cut       one thread: the end of the batch that starts at b -- a binary search in the prefix for the budget.
//   k_rec_gather    one thread per job of the batch: its ReaJob with dir_off / scr_off / band filled in.
//   k_rec_settle    one thread per job after the counting walk: the record's alignment fields and status, whether it goes on to the next
//                   band, its runs if it votes; the status counts by atomics (one per wavefront after the compiler's coalescing).
//   k_rec_opoff     the voters' op_off from the scan of their run counts.
// The lists (the jobs that take part, the jobs that touched) are compacted on the device with hipcub::DeviceSelect::Flagged; the host
// reads one count per list, two words per batch (its end and its direction bytes) and one per batch for the runs.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "../../include/bella_hip.h"
#include "realign.hpp"

namespace bella {

constexpr uint32_t kRecStep = BELLA_RECORRECT_ANCHOR_STEP;
constexpr uint32_t kRecMaxBatch = 1u << 20;          // jobs of one DP launch

// anchors of a read of L raw bases
BELLA_HD uint64_t rec_nanchors(uint64_t L) { return (L + kRecStep - 1) / kRecStep + 1; }

// P_r(x), 0 <= x <= L: rea_map over the segments pos = 256 j, nb = min(256, L - 256 j), cpos = a[j], cnb = a[j + 1] - a[j]
BELLA_HD int64_t rec_map(int64_t x, int64_t L, const uint64_t* a, int64_t plen) {
    if (x >= L) return plen;
    const int64_t j = x / (int64_t)kRecStep, p = j * (int64_t)kRecStep;
    const int64_t nb = L - p < (int64_t)kRecStep ? L - p : (int64_t)kRecStep;
    return (int64_t)a[j] + (x - p) * (int64_t)(a[j + 1] - a[j]) / nb;
}

struct RecCounts { unsigned long long band_capped, low_identity, voted; };

#if defined(__HIPCC__)
// out[g], g = aoff[r] + j: scan[off[r] + x] - scan[off[r]] with x = old[g] (a later round: the old anchor) or min(256 j, length) (round 1:
// off = the raw offsets).  scan: the emit scan over all positions of the sequences that were decided on.
__global__ void k_rec_anchors(const uint64_t* off, const uint64_t* scan, const uint64_t* aoff, const uint64_t* old, uint32_t nreads, uint64_t nanch, uint64_t* out) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nanch) return;
    uint32_t lo = 0, hi = nreads;                                     // the read of g: the last r with aoff[r] <= g (every read has an anchor)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (aoff[mid] <= g) lo = mid; else hi = mid;
    }
    const uint64_t b = off[lo], len = off[lo + 1] - b;
    uint64_t x = old ? old[g] : (g - aoff[lo]) * kRecStep;
    if (x > len) x = len;
    out[g] = scan[b + x] - scan[b];
}

// job 2 x + side of record x.  roff: raw offsets, coffs: current ones, aoff / anch: the anchors of the current sequences.
__global__ void k_rec_place(const bella_overlap* recs, uint32_t nrec, const uint64_t* roff, const uint64_t* coffs, const uint64_t* aoff, const uint64_t* anch,
                            bella_recorrect_job* out, ReaJob* jobs, uint8_t* live) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * nrec) return;
    const bella_overlap r = recs[t >> 1];
    const uint32_t side = t & 1u;
    const int64_t LH = (int64_t)(roff[r.rid + 1] - roff[r.rid]);
    bella_recorrect_job J{};
    J.record = t >> 1; J.side = side; J.orient = r.strand;
    int64_t wb, we;
    if (!side) {
        J.target = r.cid; J.query = r.rid;
        J.qbeg = (uint32_t)(r.strand ? LH - r.endH : r.begH); J.qend = (uint32_t)(r.strand ? LH - r.begH : r.endH);
        wb = r.begV; we = r.endV;
    } else {
        J.target = r.rid; J.query = r.cid;
        J.qbeg = (uint32_t)r.begV; J.qend = (uint32_t)r.endV;
        wb = r.strand ? LH - r.endH : r.begH; we = r.strand ? LH - r.begH : r.endH;
    }
    const int64_t L = (int64_t)(roff[J.target + 1] - roff[J.target]), plen = (int64_t)(coffs[J.target + 1] - coffs[J.target]);
    const int64_t n = (int64_t)J.qend - J.qbeg;
    const uint64_t* const a = anch + aoff[J.target];
    J.s = rec_map(wb, L, a, plen); J.e = rec_map(we, L, a, plen);
    const bool on = plen > 0 && n > 0;
    J.status = on ? BELLA_REALIGN_VOTED : BELLA_REALIGN_NONE;         // (VOTED: a candidate until the DP has spoken)
    ReaJob j{};
    j.gH = j.gT = (int64_t)coffs[J.target];
    j.gV = (int64_t)(roff[J.query] + (J.orient ? J.qend - 1 : J.qbeg));
    j.op_off = ~0ull;
    j.n = (uint32_t)n; j.m = j.mt = (int32_t)plen;
    const int64_t slack = (J.e - J.s) - n;
    j.c = (int32_t)(J.s + (slack >= 0 ? slack / 2 : -((-slack + 1) / 2)));      // floor
    j.dV = J.orient ? -1 : 1; j.comp = J.orient ? 3u : 0u;
    out[t] = J; jobs[t] = j; live[t] = on ? 1 : 0;
}

__global__ void k_rec_bytes(const uint32_t* pend, uint32_t np, const ReaJob* base, uint32_t B, uint64_t* bytes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > np) return;
    bytes[i] = i < np ? (uint64_t)base[pend[i]].n * (B / 4) : 0;     // (one more, so that the scan ends with the total)
}

// The batch that starts at pending job b: ctl[0] = its end, the largest e <= min(np, b + maxjobs) with pre[e] - pre[b] <= budget (at least
// b + 1: one job always goes), ctl[1] = its direction bytes.  One thread.
__global__ void k_rec_cut(const uint64_t* pre, uint32_t np, uint32_t b, uint64_t budget, uint32_t maxjobs, uint64_t* ctl) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t lo = b + 1, hi = np - b > maxjobs ? b + maxjobs : np;    // the answer lies in [lo, hi]
    const uint64_t base = pre[b];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (pre[mid] - base <= budget) lo = mid; else hi = mid - 1;
    }
    ctl[0] = lo;
    ctl[1] = pre[lo] - base;
}

__global__ void k_rec_gather(const uint32_t* pend, uint32_t b0, uint32_t nj, const ReaJob* base, const uint64_t* pre, uint32_t B, ReaJob* out) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nj) return;
    ReaJob j = base[pend[b0 + x]];
    j.dir_off = pre[b0 + x] - pre[b0];
    j.scr_off = (uint64_t)x * 2 * B;
    j.op_off = ~0ull;
    j.band = B;
    out[x] = j;
}

// touch[b0 + x] = the job goes on to the next band; vnops[x] = its runs if it votes (0 otherwise; vnops[nj] = 0 for the scan's total)
__global__ void k_rec_settle(const uint32_t* pend, uint32_t b0, uint32_t nj, const ReaRes* res, const ReaCnt* cnt, uint32_t B, uint32_t band_max, uint32_t min_identity,
                             bella_recorrect_job* out, uint8_t* touch, uint32_t* vnops, RecCounts* counts) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x > nj) return;
    if (x == nj) { vnops[x] = 0; return; }
    bella_recorrect_job& J = out[pend[b0 + x]];
    const ReaCnt k = cnt[x];
    const bool ended = k.nops > 0;
    J.band = B;
    J.n_eq = k.n_eq; J.n_x = k.n_x; J.n_ins = k.n_ins; J.n_del = k.n_del;
    J.score = ended ? res[x].score : 0;
    J.q_begin = ended ? k.q_begin : 0; J.q_end = ended ? res[x].q_end : 0;
    uint32_t again = 0, nv = 0;
    if (k.touch) {
        if (B < band_max) again = 1;
        else { J.status = BELLA_REALIGN_BAND_CAPPED; atomicAdd(&counts->band_capped, 1ull); }
    } else if (1000ull * k.n_eq < (uint64_t)min_identity * ((uint64_t)k.n_eq + k.n_x + k.n_ins + k.n_del)) {
        J.status = BELLA_REALIGN_LOW_IDENTITY; atomicAdd(&counts->low_identity, 1ull);
    } else {
        J.status = BELLA_REALIGN_VOTED; atomicAdd(&counts->voted, 1ull);
        nv = k.nops;
    }
    touch[b0 + x] = (uint8_t)again;
    vnops[x] = nv;
}

// the voters of a batch: where their runs go.  kept: the runs kept before this batch (keep_ops), or ~0: the records carry no op_off
__global__ void k_rec_opoff(const uint32_t* pend, uint32_t b0, uint32_t nj, const uint32_t* vnops, const uint64_t* opscan, uint64_t kept, ReaJob* jobs,
                            bella_recorrect_job* out) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= nj || !vnops[x]) return;
    jobs[x].op_off = opscan[x];
    bella_recorrect_job& J = out[pend[b0 + x]];
    J.nops = vnops[x];
    J.op_off = kept == ~0ull ? 0 : kept + opscan[x];
}
#endif

}  // namespace bella
