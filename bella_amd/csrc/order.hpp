// order.hpp -- the reference's output order inside a column, for many columns at a time (gfx950).
//
// LocalSpGEMM emits a column's pairs in the SLOT ORDER of its per-column open-addressing table (include/overlap.hpp:289-304
// table of 2^n >= max(16, nnz) slots, :321-333 hash key*107 with linear probing, :343-361 compaction in slot order).  That order is
// a function of (key, first product index) of the column's pairs alone: keys enter the table in the order of their first
// products.  The row kernels (spgemm.hpp) therefore leave their records in the order of THEIR grouping table with the first product
// index in the cid field, and the kernels here compute the slot order and move every record to its final place -- the pass over
// the records that used to be a plain compaction (the reference's "combine step", overlap.hpp:732-745).
//
// The order is reproduced with parallel atomicMin insertion of (first product << 16 | record index): an entry with an earlier
// first product displaces a later one, which resumes probing; the fixed point is exactly the layout sequential insertion produces
// (tests/test_core_host.py proves it under random interleavings).  The insertion cascades are chains of dependent LDS round trips:
// one WAVEFRONT per column (tables of up to 1,024 slots) keeps 24 independent columns in flight on a CU, which is what hides them;
// larger columns take a workgroup each.
//
// A wavefront reads its column's records ONCE, whole (16 bytes a record, NI = HT / 64 records a lane, all loads in flight together), and
// keeps them in registers through the rounds.  The ranks are then written by RECORD (rnk[record], where the gather form writes
// ord[rank]), every lane reads the ranks of its own records, and the records go out in windows of W ranks: scattered 16-byte LDS
// writes into the bytes of the two tables, which are dead by then (W = 6 HT / 16: 384 records at HT = 1,024, 192 at HT = 512; no LDS
// is added), read back in rank order and stored with 1 KB of consecutive bytes per store instruction.  The form it replaces
// (BELLA_ORDER_ONCE below keeps it per instance) loaded {key, first product} -- 8 of every 16 bytes, so whole lines -- and gathered
// the whole record by rank afterwards: every record came in from beyond L2 twice.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bella_hip.h"
#include "core.hpp"
#include "slotorder.hpp"
#include "util.hpp"

namespace bella {

constexpr uint32_t kOrderWaveHt = 1024;                    // largest table a single wavefront orders (4 KB + 2 KB of LDS)
constexpr uint32_t kOrderLdsHt = 16384;                    // largest table a workgroup holds in LDS (64 KB + 32 KB)
constexpr uint32_t kOrderBlock = 256;
constexpr uint32_t kOrderBigGrid = 512;                    // persistent workgroups of k_order_block
constexpr uint32_t kOrderOneLaunchMax = 32768;             // columns of a pass up to which ONE wavefront-per-column launch takes all table sizes (BELLA_TUNE_ORDER_SPLIT)
constexpr uint64_t kOrderWsBytes = (uint64_t)6 * 65536;    // global tables of one workgroup for columns with more than 16,384 pairs

struct OrderArgs {
    const uint64_t* flopptr;     // where a column's records stand in tmp_pairs
    const uint64_t* colptrC;     // ... and where they go
    const uint32_t* nnzC;        // pairs per column (| kOrderedBit: already in slot order, cid already the column)
    const uint32_t* flops;       // products per column: the first product indices (insertion times) lie below it
    uint32_t nreads, i0, stride, nown;
    const bella_pair* tmp_pairs;
    const bella_pair_ext* tmp_ext;
    bella_pair* pairs;
    bella_pair_ext* ext;
    uint64_t* totals;            // totals[0] = nnz(C)
    uint32_t* nbig;              // columns left to k_order_block
    uint32_t* biglist;
    uint8_t* ws;                 // kOrderWsBytes per workgroup of k_order_block
};

__device__ __forceinline__ void order_copy_record(const OrderArgs& a, uint64_t from, uint64_t to, uint32_t cid) {
    uint4 rec = *(const uint4*)(a.tmp_pairs + from);
    asm volatile("" : "+v"(rec.y));                          // (keeps the load ONE 16-byte load: the compiler splits it around the word that is replaced)
    rec.y = cid;
    *(uint4*)(a.pairs + to) = rec;
    if (a.ext) a.ext[to] = a.tmp_ext[from];
}

// The two table scans of a wavefront-ordered column, lane-INTERLEAVED (lane l takes slots 64 b + l): a block of 64 slots is one
// conflict-free LDS access and one ballot, where the chunked form of slotorder.hpp (lane l takes ht / 64 consecutive slots) puts all
// lanes of a 32-lane group on two of the 32 banks (stride 16 words at ht = 1,024).  (Round 5: the kernel's time did not change -- 0.597 ms
// for the 50 M records of the 100k set either way: it moves 2.4 GB at 4 TB/s, the copy ceiling of these boxes being 5 TB/s.  Measured and
// not kept: the records read ONCE, whole, into registers and scattered to their ranks with 16-byte GLOBAL stores -- 1.6 GB instead of
// 2.4 GB, but 0.67 ms: scattered 16-byte stores cost more than scattered 16-byte loads.  The read-once form of k_order_wave scatters
// in LDS instead and keeps the global stores coalesced.)
// nf[s] = first empty slot at or after s, cyclically; false: the table is full
__device__ __forceinline__ bool wave_next_free(const uint32_t* T2, uint16_t* nf, uint32_t ht) {
    const uint32_t lane = lane_id();
    const uint32_t nb = (ht + 63u) >> 6;
    uint32_t carry = 0xFFFFFFFFu;                             // first empty slot above the current block; after the first sweep: of the whole table
#pragma unroll 1
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (uint32_t b = nb; b-- > 0;) {
            const uint32_t s = (b << 6) + lane;
            const bool empty = s < ht && T2[s] == kEmpty;
            const unsigned long long m = __ballot(empty);
            if (sweep == 1 && s < ht) {
                const unsigned long long up = m >> lane;      // empty slots of this block at or after mine
                nf[s] = (uint16_t)(up ? s + (uint32_t)__ffsll((long long)up) - 1u : carry);
            }
            if (m) carry = (b << 6) + (uint32_t)__ffsll((long long)m) - 1u;
        }
        if (carry == 0xFFFFFFFFu) return false;
    }
    return true;
}
// ord[rank] = record index of the rank-th occupied slot (the slot order itself)
__device__ __forceinline__ void wave_rank_slots(const uint32_t* T2, uint16_t* ord, uint32_t ht) {
    const uint32_t lane = lane_id();
    const uint32_t nb = (ht + 63u) >> 6;
    uint32_t base = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t s = (b << 6) + lane;
        const uint32_t it = s < ht ? T2[s] : kEmpty;
        const unsigned long long m = __ballot(it != kEmpty);
        if (it != kEmpty) ord[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)(it & 0xFFFFu);
        base += (uint32_t)__popcll(m);
    }
}

// rnk[record] = rank of the record's slot among the occupied ones: the slot order, told to the lane that HOLDS the record
__device__ __forceinline__ void wave_rank_records(const uint32_t* T2, uint16_t* rnk, uint32_t ht) {
    const uint32_t lane = lane_id();
    const uint32_t nb = (ht + 63u) >> 6;
    uint32_t base = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t s = (b << 6) + lane;
        const uint32_t it = s < ht ? T2[s] : kEmpty;
        const unsigned long long m = __ballot(it != kEmpty);
        if (it != kEmpty) rnk[it & 0xFFFFu] = (uint16_t)(base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
        base += (uint32_t)__popcll(m);
    }
}

// a value all lanes of the wavefront hold, told to the compiler (it then keeps it, and what is computed from it, in scalar registers)
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform(uint64_t v) { return (uint64_t)uniform((uint32_t)v) | (uint64_t)uniform((uint32_t)(v >> 32)) << 32; }

// round_bound (slotorder.hpp) for the tables a wavefront orders: at most 1,024 slots, and insertion times below 2^16 (columns with 65,536
// products and more arrive in order, wide.hpp), so the product fits 32 bits -- the same bound without the 64-bit division, whose
// intermediate values sat on top of the records held in registers
__device__ __forceinline__ uint32_t round_bound_wave(uint32_t r, uint32_t ht, uint32_t d, uint32_t tmax) {
    const uint32_t keep = r + 2 < 32 ? ht >> (r + 2) : 0u;
    if (keep < 32u || tmax > 0x10000u) return tmax;
    const uint32_t b = tmax * (ht - keep) / d;
    return b >= tmax ? tmax : b;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // a record in four CONSECUTIVE registers, as an operand the empty asm can name whole

// BELLA_ORDER_ONCE: which instances of k_order_wave read every record ONCE (bit 0: <512,0>, bit 1: <1024,512>, bit 2: <1024,0>); the
// others load {key, first product} for the insertion and gather the whole record by rank afterwards (every line comes in twice).
// Default 3: the two instances that share a large pass (100k reads: 130.7 -> 113.0 us and 385.8 -> 299.8 us per pass, the gather form
// built from this same file).  The single launch of a small pass keeps the gather form: 10k reads, 0.3 M records in columns of 30
// pairs on average, 13.2 us against 17.6 us -- a lane holds 16 records' registers and issues 16 loads for a column that fills half a
// block of 64, and the records fit the cache, so the second fetch costs nothing there.  profiles/r08_order_pass.md has the runs.
#ifndef BELLA_ORDER_ONCE
#define BELLA_ORDER_ONCE 3
#endif
template <uint32_t HT, uint32_t HTLO>
constexpr bool order_reads_once() { return ((BELLA_ORDER_ONCE) >> (HT == 512 ? 0 : HTLO ? 1 : 2)) & 1; }

// one wavefront per column: tables of HTLO < ht <= HT slots (HT <= kOrderWaveHt; two instances share the columns: the small one keeps
// fewer records per lane in registers and half the LDS, so more of its columns are in flight per CU).  The instance with HTLO == 0
// also copies the columns that are in order already and lists the ones above kOrderWaveHt for k_order_block.
template <uint32_t HT, uint32_t HTLO>
__global__ __launch_bounds__(kOrderBlock) __attribute__((amdgpu_waves_per_eu(HT == 512 ? 8 : 6))) void k_order_wave(OrderArgs a) {
    constexpr bool ONCE = order_reads_once<HT, HTLO>();
    __shared__ __attribute__((aligned(16))) uint8_t s_tab[kOrderBlock / 64][6 * HT];   // per wavefront: T2 (4 B a slot), then ord (2 B a slot)
    const uint32_t j0 = blockIdx.x * (kOrderBlock / 64) + wave_id();
    const uint32_t lane = lane_id();
    if (HTLO == 0 && j0 == 0 && lane == 0) a.totals[0] = a.colptrC[a.nreads];   // nnz(C): read back once with the control block
    if (j0 >= a.nown) return;
    const uint32_t i = a.i0 + j0 * a.stride;
    // everything the column needs from its descriptors in ONE round trip (each of these is wave-uniform, so the compiler waits for
    // it where it is loaded: loaded one after the other they are four dependent trips to HBM per column)
    uint32_t nz = a.nnzC[i];
    uint64_t src = a.flopptr[i], dst = a.colptrC[i];
    uint32_t tmax = a.flops[i];
    asm volatile("" : "+v"(nz), "+v"(src), "+v"(dst), "+v"(tmax));   // (all four are issued before the first is waited for)
    nz = uniform(nz); tmax = uniform(tmax); src = uniform(src); dst = uniform(dst);   // ... and live in scalar registers from here on
    const uint32_t d = nz & ~kOrderedBit;
    if (!d) return;
    if (nz & kOrderedBit) {
        if (HTLO == 0) for (uint32_t r = lane; r < d; r += 64) order_copy_record(a, src + r, dst + r, i);
        return;
    }
    const uint32_t ht = pow2_at_least(16u, d);
    if (ht > kOrderWaveHt) {
        if (HTLO == 0 && lane == 0) a.biglist[atomicAdd(a.nbig, 1u)] = i;
        return;
    }
    if (ht > HT || ht <= HTLO) return;                       // the other instance's column
    uint32_t* T2 = (uint32_t*)s_tab[wave_id()];
    uint16_t* ord = (uint16_t*)(s_tab[wave_id()] + 4 * HT);  // next-free table during the rounds, then the ranks
    for (uint32_t s = lane; s < ht; s += 64) T2[s] = kEmpty;
    constexpr uint32_t NI = HT / 64;                         // records per lane
    // ONCE: the record stays WHOLE in four consecutive registers (what a 16-byte LDS write takes): x = key, y = first product during
    // the rounds and the record's rank after them, z and w wait for the placement
    u32x4 rec[ONCE ? NI : 1];
    uint32_t key_[ONCE ? 1 : NI], fp_[ONCE ? 1 : NI];
    auto key = [&](uint32_t u) -> uint32_t { if constexpr (ONCE) return rec[u].x; else return key_[u]; };
    auto fp = [&](uint32_t u) -> uint32_t { if constexpr (ONCE) return rec[u].y; else return fp_[u]; };
#pragma unroll
    for (uint32_t u = 0; u < NI; ++u) {
        const uint32_t j = lane + 64 * u;
        if constexpr (ONCE) {
            // (lanes beyond the column read its last record again: a load under a condition, lane mask or scalar branch alike, made the
            // compiler wait for it on the spot and copy words out of the four registers)
            rec[u] = *(const u32x4*)(a.tmp_pairs + src + (j < d ? j : d - 1));
        } else {
            key_[u] = 0; fp_[u] = 0xFFFFFFFFu;
            if (j < d) { const uint2 kf = *(const uint2*)(a.tmp_pairs + src + j); key_[u] = kf.x; fp_[u] = kf.y; }   // {key, first product}
        }
    }
    if constexpr (ONCE) {                                    // (ONE 16-byte load each, all NI issued before the first is waited for)
#pragma unroll
        for (uint32_t u = 0; u < NI; ++u) {
            asm volatile("" : "+v"(rec[u]));
            if (lane + 64 * u >= d) rec[u].y = 0xFFFFFFFFu;   // no record: in no round and in no window
        }
    }
    group_sync<64>();
    uint32_t prev = 0;
    for (uint32_t rd = 0;; ++rd) {                            // rounds by insertion time (slotorder.hpp)
        const uint32_t bound = round_bound_wave(rd, ht, d, tmax);
        if (rd) { (void)wave_next_free(T2, ord, ht); group_sync<64>(); }
        // (home and item are made anew in every round, from a multiplier and a shift the compiler cannot see through: held over the
        // rounds they are three more registers per record, 48 at NI = 16, which is what set this kernel's allocation)
        const uint32_t mask = ht - 1;
        uint32_t mul = 107u, sh = 16u, ln = lane;
        asm volatile("" : "+v"(mul), "+v"(sh), "+v"(ln));
#pragma unroll
        for (uint32_t u = 0; u < NI; ++u) {
            if (fp(u) < prev || fp(u) >= bound) continue;
            const uint32_t home = (key(u) * mul) & mask, item = (fp(u) << sh) | (ln + 64 * u);
            if (rd) slot_insert<true>(T2, ord, mask, home, item);
            else slot_insert<false>(T2, ord, mask, home, item);
        }
        group_sync<64>();
        if (bound >= tmax) break;
        prev = bound;
    }
    if constexpr (ONCE) {
        // Every lane learns the ranks of ITS records (they take the place of the first products, which are dead), and the records
        // go to their places in windows of W ranks through the bytes of the two tables, which are dead as well: scattered 16-byte
        // LDS writes, then whole windows read back in rank order, so that every global store instruction writes 1 KB of consecutive
        // bytes as the gather's stores do.  (Scattering the global stores themselves was measured in round 5, see above: slower.)
        wave_rank_records(T2, ord, ht);
        group_sync<64>();
        uint32_t ln = lane;
        asm volatile("" : "+v"(ln));                          // (the record indices are not held over the rounds either)
#pragma unroll
        for (uint32_t u = 0; u < NI; ++u) { const uint32_t j = ln + 64 * u; rec[u].y = j < d ? ord[j] : 0xFFFFFFFFu; }
        group_sync<64>();
        if (a.ext) {                                          // diagnostics (off in timed runs): read in order, scattered by rank
            asm volatile("" : "+v"(ln));
#pragma unroll
            for (uint32_t u = 0; u < NI; ++u) { const uint32_t j = ln + 64 * u; if (j < d) a.ext[dst + rec[u].y] = a.tmp_ext[src + j]; }
        }
        constexpr uint32_t W = 6 * HT / 16;                   // records the 6 * HT bytes of T2 and ord hold
        u32x4* stage = (u32x4*)s_tab[wave_id()];
        for (uint32_t w0 = 0; w0 < d; w0 += W) {
#pragma unroll
            for (uint32_t u = 0; u < NI; ++u) {
                uint32_t o = rec[u].y - w0;                   // (0xFFFFFFFF, no record: outside of every window)
                asm volatile("" : "+v"(o));                   // (or the compiler keeps 16 * rank of every record over the windows)
                if (o < W) stage[o] = rec[u];                 // the rank travels in the cid field ...
            }
            group_sync<64>();
            const uint32_t n = d - w0 < W ? d - w0 : W;       // the last window is partial
#pragma unroll
            for (uint32_t v = 0; v < W / 64; ++v) {
                const uint32_t r = lane + 64 * v;
                if (r < n) { u32x4 o = stage[r]; asm volatile("" : "+v"(o)); o.y = i; *(u32x4*)(a.pairs + dst + w0 + r) = o; }   // ... which gets the column here
            }
            group_sync<64>();
        }
        return;
    }
    wave_rank_slots(T2, ord, ht);
    group_sync<64>();
    {   // four records in flight per lane
        uint32_t r = lane;
        for (; r + 192 < d; r += 256) {
            uint4 rec[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) rec[u] = *(const uint4*)(a.tmp_pairs + src + ord[r + 64 * u]);
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) { asm volatile("" : "+v"(rec[u].y)); rec[u].y = i; *(uint4*)(a.pairs + dst + r + 64 * u) = rec[u]; }
            if (a.ext) {
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) a.ext[dst + r + 64 * u] = a.tmp_ext[src + ord[r + 64 * u]];
            }
        }
        for (; r < d; r += 64) order_copy_record(a, src + ord[r], dst + r, i);
    }
}

// one workgroup per column (persistent): the columns k_order_wave listed
__global__ __launch_bounds__(kOrderBlock) void k_order_block(OrderArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    __shared__ uint32_t scr[16];
    const uint32_t nbig = *a.nbig;
    const uint32_t tid = threadIdx.x;
    for (uint32_t x = blockIdx.x; x < nbig; x += gridDim.x) {
        const uint32_t i = a.biglist[x];
        const uint32_t d = a.nnzC[i] & ~kOrderedBit;
        const uint64_t src = a.flopptr[i], dst = a.colptrC[i];
        const uint32_t ht = pow2_at_least(16u, d);
        uint32_t* T2;
        uint16_t* ord;
        if (ht <= kOrderLdsHt) { T2 = (uint32_t*)smem; ord = (uint16_t*)(smem + (size_t)4 * kOrderLdsHt); }
        else { uint8_t* w = a.ws + (uint64_t)blockIdx.x * kOrderWsBytes; T2 = (uint32_t*)w; ord = (uint16_t*)(w + (size_t)4 * 65536); }
        for (uint32_t s = tid; s < ht; s += kOrderBlock) T2[s] = kEmpty;
        __syncthreads();
        const uint32_t tmax = a.flops[i];
        uint32_t prev = 0;
        for (uint32_t rd = 0;; ++rd) {                        // rounds by insertion time (slotorder.hpp); ord doubles as the next-free table
            const uint32_t bound = round_bound(rd, ht, d, tmax);
            if (rd) { (void)build_next_free<(int)kOrderBlock>(T2, ord, ht, scr); __syncthreads(); }
            for (uint32_t j = tid; j < d; j += kOrderBlock) {
                const uint2 kf = *(const uint2*)(a.tmp_pairs + src + j);
                if (kf.y < prev || kf.y >= bound) continue;
                const uint32_t home = (kf.x * 107u) & (ht - 1), item = (kf.y << 16) | j;
                if (rd) slot_insert<true>(T2, ord, ht - 1, home, item);
                else slot_insert<false>(T2, ord, ht - 1, home, item);
            }
            __syncthreads();
            if (bound >= tmax) break;
            prev = bound;
        }
        {
            const uint32_t c = (ht + kOrderBlock - 1) / kOrderBlock;
            const uint32_t lo = tid * c < ht ? tid * c : ht, hi = lo + c < ht ? lo + c : ht;
            uint32_t occ = 0;
            for (uint32_t s = lo; s < hi; ++s) occ += T2[s] != kEmpty ? 1u : 0u;
            uint32_t tot;
            uint32_t rank = block_excl_scan<kOrderBlock / 64>(occ, scr, &tot);
            for (uint32_t s = lo; s < hi; ++s) {
                const uint32_t it = T2[s];
                if (it != kEmpty) ord[rank++] = (uint16_t)(it & 0xFFFFu);
            }
        }
        __syncthreads();
        for (uint32_t r = tid; r < d; r += kOrderBlock) order_copy_record(a, src + ord[r], dst + r, i);
        __syncthreads();
    }
}

}  // namespace bella
