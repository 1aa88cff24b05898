// bella_hip.hip -- libbella_hip.so: context, memory, launch sequencing and the C ABI (include/bella_hip.h).
// gfx950 only.  No CPU execution path: every entry point either runs the HIP kernels or returns an error.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <array>
#include <cmath>
#include <initializer_list>
#include <iterator>
#include <map>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bella_hip.h"
#include "assemble.hpp"
#include "clip.hpp"
#include "comm.hpp"
#include "core.hpp"
#include "fastq.hpp"
#include "graph.hpp"
#include "trim.hpp"
#include "kcount.hpp"
#include "logan.hpp"
#include "order.hpp"
#include "pileup.hpp"
#include "polish.hpp"
#include "realign.hpp"
#include "links.hpp"
#include "pairalign.hpp"
#include "recorrect.hpp"
#include "spgemm.hpp"
#include "trace.hpp"
#include "unitig.hpp"
#include "bubble.hpp"
#include "util.hpp"
#include "wide.hpp"
#include "writer.hpp"
#include "xdrop.hpp"
#include "xdrop_packed.hpp"

using namespace bella;

namespace {

// Large device buffers a context gives up are kept on a free list and handed to the next request they fit, instead of going back to the
// driver: hipMalloc hands out freshly freed VRAM only after the driver has wiped it, and a phase that frees tens of GB right before
// the next one asks for as much waits about a second for that (200k reads: assembly 1.05 s instead of 60 ms, first pass 0.75 s
// instead of 15 ms).  Same synchronisation as hipFree (the device is idle when a buffer changes hands); what is pooled counts as free
// memory wherever the library sizes something by it, and goes back to the driver when an allocation fails or the context is destroyed.
// An ARENA (bella_hip_reserve): one slab taken from the driver up front, from which the buffers below are cut.  The first hipMalloc
// of a multi-GB buffer costs ~30 ms per GB on this stack (the driver maps and wipes the pages): at 100k reads the first k-mer count paid
// 850 ms for its 30 GB of sort buffers and the first assembly 210 ms, against 47 and 21 ms of kernels.  A process that will run the
// pipeline reserves once; every stage then finds its memory in place.  First fit over an offset-ordered free list with coalescing.
struct Arena {
    char* base = nullptr;
    size_t size = 0, in_use = 0, peak = 0;
    std::map<size_t, size_t> holes;                             // offset -> length of the free ranges
    static size_t round(size_t n) { return (n + 4095) & ~(size_t)4095; }
    bool owns(const void* p) const { return base && (const char*)p >= base && (const char*)p < base + size; }
    size_t free_bytes() const { return size - in_use; }
    // the largest single buffer the slab can still give (first fit over a fragmented free list: the sum of the holes is not it)
    size_t largest_hole() const { size_t m = 0; for (const auto& h : holes) m = std::max(m, h.second); return m; }
    void* take(size_t n) {
        n = round(n);
        for (auto it = holes.begin(); it != holes.end(); ++it)
            if (it->second >= n) {
                const size_t off = it->first, len = it->second;
                holes.erase(it);
                if (len > n) holes.emplace(off + n, len - n);
                in_use += n;
                peak = std::max(peak, in_use);
                return base + off;
            }
        return nullptr;
    }
    void give(void* p, size_t n) {
        n = round(n);
        in_use -= n;
        size_t off = (size_t)((char*)p - base);
        auto nx = holes.lower_bound(off);
        if (nx != holes.begin()) { auto pv = std::prev(nx); if (pv->first + pv->second == off) { off = pv->first; n += pv->second; holes.erase(pv); } }
        if (nx != holes.end() && off + n == nx->first) { n += nx->second; holes.erase(nx); }
        holes.emplace(off, n);
    }
};
struct BufPool {
    std::vector<std::pair<void*, size_t>> free;
    size_t bytes = 0;
    Arena arena;
};
constexpr size_t kPoolMinBytes = 128ull << 20, kPoolMaxBytes = 160ull << 30;
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    BufPool* pool = nullptr;     // where the buffer goes when it is released (set by ensure_bytes)
};

// Column tiers by product count.  A column runs in one 512-thread workgroup with 14.5 B of LDS per product (19 B with the
// half-size key tables of pair-rich inputs); tiers whose workgroups need the same share of a CU's 160 KB (1/4, 1/3, 1/2, all of
// it) form one LDS class = ONE launch that walks its tiers' lists from the largest columns down.  Last: the global-workspace
// tier.  BELLA_HIP_TIERS=a,b,c (read once per context; tuning aid / tests) overrides the LDS caps.
constexpr uint32_t kNumTiers = 15;  // at most
constexpr uint32_t kDefaultTiers = 14;
const uint32_t kTierCapsDefault[kNumTiers] = {384, 689, 1000, 1394, 2048, 2752, 3712, 4600, 5568, 8192, 11008, 65535, 65535, 65535};
const uint32_t kTierCapsHalf[kNumTiers] = {300, 526, 800, 1064, 1600, 2105, 2789, 3500, 4096, 6144, 8192, 11008, 65535, 65535};
constexpr uint32_t kFullTableMaxCap = 300;               // pair-rich inputs: the smallest tier holds as many pairs as products
constexpr uint32_t kHalfTableMaxCap = 4096;              // above: quarter-size key tables on any input
// LDS classes: the share of a CU's 160 KB a column's workgroup needs, and the workgroup size that goes with it.  A column costs
// a fixed ~18 us of latency (three dependent memory round trips, ~16 barriers) plus time per product: small columns get small
// workgroups so that 16 or 8 of them share a CU; where only one or two columns fit a CU they get 1024 threads -- every class
// keeps the CU's 32 wavefront slots filled.
constexpr uint32_t kNumClasses = 6;
const size_t kClassLds[kNumClasses] = {10240, 20480, 40160, 54608, 81920, 163840};   // 16, 8, 4, 3, 2, 1 workgroups per CU
#ifndef BELLA_CLASS_BLOCKS
#define BELLA_CLASS_BLOCKS {128, 256, 512, 512, 1024, 1024}
#endif
const int kClassBlock[kNumClasses] = BELLA_CLASS_BLOCKS;   // measured (tools/ab_blocks.sh): DESIGN.md 4.1
#ifndef BELLA_LONG_LIST_MAX_CAP
#define BELLA_LONG_LIST_MAX_CAP 2752
#endif
constexpr uint32_t kLongListMaxCap = BELLA_LONG_LIST_MAX_CAP;   // long-list inputs: LDS tiers above this many products are closed
constexpr uint32_t kMidToWideMin = 16;      // columns above the LDS tiers in one pass from which on they take the sort-based path
constexpr uint32_t kRerunGrid = 256;        // persistent workgroups of the rerun launch (columns an LDS tier handed over)
constexpr uint32_t kGlobalGrid = 1024;      // persistent workgroups of the global path (1024 threads each: latency-bound, two resident per CU)
constexpr uint32_t kAsmGrid = 128;

struct CastU64 {
    __host__ __device__ uint64_t operator()(const uint32_t& v) const { return (uint64_t)v; }
};
struct CastU8 {
    __host__ __device__ uint32_t operator()(const uint8_t& v) const { return (uint32_t)v; }
};
struct CountU64 {                                        // pair counts: without the "already in slot order" mark
    __host__ __device__ uint64_t operator()(const uint32_t& v) const { return (uint64_t)(v & ~kOrderedBit); }
};

// Which results of the pipeline's stages a context holds: one bit per stage, from the reads to the polished unitigs.
// drop / changed / made / has / need (below) are the only code that touches `valid`.  The stages up to the traces keep their results in
// members of the context (device buffers, mostly), PILE and CONS too; those of the stages that follow the alignment are here, one member
// per stage, on the host: the graph is small next to what it was made from, and a stage uploads what it reads.
enum Stage : uint32_t { READS, TUPLES, PANEL, MATRIX, PAIRS, ALNS, TRACES, BATCH_OPS, RECORDS, TRIM, GRAPH, UNITIGS, POLISH, REALIGN, PILE, CONS, RECORRECT, LINKS, kStages };
struct StageState {
    uint32_t valid = 1u << RECORDS;          // one bit per Stage (the records are always there: possibly none)
    std::vector<bella_overlap> records;      // accumulated by bella_hip_graph_add_overlaps (graph.hpp)
    struct Trim {                            // the clips of the last bella_hip_graph_trim, 16 bytes per read (trim.hpp; section 15).  A graph
        std::vector<bella_read_clip> clips;  // in the context was always built in the trim state the context is in now
        bella_trim_stats stats{};
    } trim;
    struct Graph {                           // the last build's result, as bella_hip_graph_clean, _pop_bubbles and _cut_weak left it (sections 11 to 13, 17)
        std::vector<uint32_t> off;
        std::vector<bella_graph_edge> edges;
        std::vector<uint8_t> contained, removed;
        bella_graph_stats stats{};
        bella_unitig_stats clean{};          // the clean's part of bella_unitig_stats (rounds .. edges_removed, clean_ms)
        bella_bubble_stats bubbles{};
        bella_weak_stats weak{};
    } graph;
    struct Unitigs {                         // the last bella_hip_graph_unitigs (unitig.hpp; section 12)
        std::vector<uint64_t> voff, pos, len, boff;
        std::vector<uint32_t> verts, nb;
        std::vector<uint8_t> circ, bases;
        std::vector<bella_unitig_link> links;
        bella_unitig_stats stats{};          // the unitigs' part
    } unitigs;
    struct Polish {                          // the last bella_hip_graph_polish_unitigs (polish.hpp; section 14)
        std::vector<uint64_t> offs, pos;
        std::vector<uint32_t> nb;
        std::vector<uint8_t> bases;
        std::vector<bella_polish_unitig> recs;
        bella_polish_stats stats{};
    } polish;
    struct Realign {                         // the last round of bella_hip_graph_realign_unitigs (realign.hpp; section 18): a Polish in shape
        std::vector<uint64_t> offs, pos;
        std::vector<uint32_t> nb;
        std::vector<uint8_t> bases;
        std::vector<bella_polish_unitig> recs;
        std::vector<bella_realign_placement> placements;
        std::vector<uint32_t> ops, table;    // kept for the tests only (keep_ops)
        bella_realign_stats stats{};
        uint64_t wrapped = 0;                // voters that reach across an origin (section 19); apart from the stats, whose struct keeps its size
    } realign;
    struct Recorrect {                       // the last round of bella_hip_recorrect (recorrect.hpp; section 20).  Sequences, per-read
        uint64_t total = 0, njobs = 0;       // statistics, anchors and job records stay on the device, with the context (rc_*)
        std::vector<uint32_t> ops, table;    // kept for the tests only (keep_ops)
        bella_recorrect_stats stats{};
    } recorrect;
    struct Links {                           // the last bella_hip_graph_align_links (links.hpp; section 26): one record per link of the unitigs,
        std::vector<bella_link_aln> alns;    // and the runs of the ALIGNED ones
        std::vector<uint32_t> ops;
        bella_link_stats stats{};
    } links;
    // READS .. BATCH_OPS, PILE and CONS (pileup.hpp; section 10) are members of the context: only their bits are here
};

}  // namespace

struct bella_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    uint32_t debug = 0;

    // reads
    uint32_t nreads = 0;
    uint64_t total_bases = 0;
    Buf packed, roff;
    // B (reference layout) and device layout
    uint32_t nkmers = 0, kmer_size = 0;
    uint64_t nnz = 0;
    std::vector<std::string> names;      // read names when the reads came through bella_hip_load_fastq
    std::vector<uint32_t> host_lens;
    uint64_t kc_ntuples = 0;             // TUPLES: the device-resident tuples + dictionary of bella_hip_count_kmers
    uint32_t kc_nkmers = 0, kc_k = 0;
    std::vector<uint64_t> kc_stats;      // what the host decided for the last count (bella_hip_get_count_stats)
    uint32_t kc_bfirst = 0, kc_brows = 0; // the read block the device-resident tuples cover (all reads unless counted distributed)
    Buf kc_nk, kc_koff, kc_hist, kc_keys, kc_alt, kc_runlen, kc_flag, kc_slot, kc_nruns, kc_dcode, kc_dcount, kc_hkey, kc_hval, kc_found,
        kc_tstart, kc_cursor, kc_sel, kc_ringo, kc_ringp, kc_opos, kc_oid, kc_opos2, kc_oid2;
    Buf Bptr, Bk, Bpos, Bent, rowF, Aent, Aent2, Aov, Arow, Bloc;
    bool have_rowlists = false;          // Aent2 / Arow hold the row lists of the current layout
    bool want_rowlists = false;          // BELLA_TUNE_ROW_LISTS: build them with the next layouts (when they fit)
    uint32_t part_first = 0, part_stride = 1;
    uint32_t layout_first = 0, layout_stride = 1;   // the partition the current layout was built for (B' / row lists: owned columns only)
    uint64_t owned_nnz = 0;              // nonzeros of the owned columns (what the current layout was built from)
    uint64_t live_nnz = 0;               // B' entries of the current layout: those with a later read (all of them with BELLA_TUNE_COMPACT_B 1)
    uint64_t sym_sig[6] = {};            // what flops / nnzC were last cleared for
    uint64_t layout_gen = 0;             // bumped by every build of the device layout
    uint32_t range_lo = 0, range_hi = 0xFFFFFFFFu;   // stage: the contiguous column range computed by the next passes
    uint32_t panel_first = 0, panel_rows = 0;
    uint64_t panel_nnz = 0;
    // assembly temporaries
    Buf t_kmer, t_read, t_pos, tstart, Bk_tmp, Bpos_tmp, rowcnt, asm_ws, asm_cls;
    Buf lk_key, lk_key2, lk_val, lk_val2, w, wscan, lk_rinfo;
    // overlap
    uint64_t flops = 0, npairs = 0;
    uint32_t pair_ratio1024 = 1024;   // max over sampled columns of 1024 * pairs/products
    bool long_list_sample = false;    // the sampled columns TOGETHER hold >= 64 products per pair
#ifdef BELLA_DEV_PROF
    Buf prof;
#endif
    Buf flopsr, flopptr, nnzC, colptrC, rowlists, tiercaps, tmp_pairs, tmp_ext, pairs, ext, sortscr, ws,
        status, cubtmp, plist_hv, overflow, ctl, retry, orderlist, order_ws;
    bool order_attr = false;
    Buf w_f, w_off, w_key, w_key2, w_idx, w_idx2, w_hv, w_ovfl, w_plist, w_scr, w_rlen, w_rstart, w_rrank, w_redo, w_segfirst,
        w_toff, w_table, w_nruns, w_desc, w_gtab, w_gcount, w_gbase, w_rfirst, w_aent2, w_aov;
    uint32_t n_wide = 0;
    uint32_t n_retry = 0;
    uint32_t n_overflow = 0;
    // alignment
    uint64_t nalns = 0;
    Buf alns, seeds, xest, xest2, xids, xorder, xres, xstate, xlive, lg_res, lg_redo, lg_scratch;
    // traced alignments of the last bella_hip_trace_pairs (records index-aligned with the pairs; the ops stay on the host)
    std::vector<bella_trace> traces;
    std::vector<uint32_t> trace_ops;
    std::vector<uint32_t> batch_ops;     // runs of the last bella_hip_trace_batch
    bella_trace_stats trace_stats{};
    std::vector<uint32_t> pal_ops;       // runs of the last bella_hip_align_sequences (pairalign.hpp; section 28): no stage, the sequences were the caller's
    bella_align_stats pal_stats{};
    Buf tr_exts, tr_lists, tr_res, tr_pres, tr_opoff, tr_dirs, tr_scr, tr_ops;
    bool trace_ops_kept = true;          // false: the last call piled its runs up on the device and did not stage them (keep_ops == 0)
    // read correction (pileup.hpp): the table of the loaded reads, and the last consensus
    uint64_t cons_total = 0;
    bella_vote_stats vote_stats{};       // the last voting call (section 21)
    bella_clip_stats clip_stats{};       // the last clipping call (clip.hpp; section 24)
    Buf pile, pile_pairs, pile_cnt, pile_tmp, cons_emit, cons_scan, cons_out, cons_offs, cons_stats;
    // correction rounds (recorrect.hpp; section 20): the anchors' offsets (one list per read), the consensus's anchors, and the last round
    uint64_t rc_nanch = 0;
    Buf rc_aoff, cons_anch, rc_out, rc_offs, rc_stats, rc_anch, rc_jobs;
    StageState as;                       // overlap records, clips, graph, unitigs, polish; which of all the stages' results are valid
    bella_timings tm{};
    hipEvent_t ev[12]{};
    uint32_t* pinned = nullptr;          // 128 host words the per-pass read backs land in
    Stager stager;                       // pinned bounce buffers of the large host <-> device copies
    bella_ingest_stats ingest{};         // of the last bella_hip_load_fastq
    int caps_state = 0;
    ncclComm_t comm = nullptr;           // communicator of bella_hip_comm_init (one rank per context)
    const Rccl* api = nullptr;           // its transport: RCCL (comm.hpp: rccl()) or the in-process one (loopback())
    int comm_ranks = 0, comm_rank = 0;
    Buf comm_meta;
    bool pass_known = false;             // tier lengths and product total of the last pass (valid for pass_sig)
    uint64_t pass_sig[6] = {};
    uint32_t pass_tcnt[20] = {};
    uint64_t pass_products = 0;
    uint64_t pass_wide_products[2] = {};  // ... of the last tier's columns and of the wide columns (what wide.hpp's path will hold)
    bool pass_rare_free = false;         // the last pass on pass_sig needed no rerun, no overflow fold, no wide column
    bool pass_big_free = false;          // ... and had no column with more than 1,024 pairs (k_order_block)
    uint32_t tier_caps[kNumTiers] = {};  // ascending LDS caps, last = 65535 (global-workspace tier); per context
    uint32_t ntiers = 0;
    bool tiers_from_env = false;         // custom tier table (bella_hip_set_tuning)
    uint64_t kcount_budget = 1ull << 30, wide_budget = 1ull << 30;   // items per pass of the counting sort / of the wide-column path
    bool lane_order_ok = true;           // k_lane_order_selftest at init
    uint64_t xdrop_class_min = 4ull * 4096 * 64;   // extensions of a batch from which on the slices run it as four classes (BELLA_TUNE_XDROP_CLASS_MIN)
    BufPool pool;                        // released device buffers waiting for the next request they fit
    uint32_t layout_inline = 0;          // the device layout holds B' entries in the INLINE form (util.hpp); 0 / 1
    bool layout_products = false;        // the device layout holds B' with one entry per PRODUCT (assemble.hpp: k_layout_compact_products)
    // which path the last assembly took (bella_hip_get_assemble_stats): the reads per table class of the last assemble_rows_device, the
    // list order of the last build_layout and whether its place pass went through the radix pass
    uint32_t asm_class_count[kAsmClasses] = {};
    bool layout_first_app = false, layout_place_sorted = false;
    // layout and path choices (bella_hip_set_tuning; the matching bella_hip_set_debug bits of earlier rounds are still read as aliases)
    uint32_t tune_layout_order = 0;      // BELLA_TUNE_LAYOUT_ORDER: 0 lists of A' in k-mer order, 1 in order of first appearance in B'
    uint32_t tune_inline = 0;            // BELLA_TUNE_INLINE_ENTRIES: 0 by the size of A' against the last-level cache, 1 never, 2 always
    uint32_t tune_row_path = 0;          // BELLA_TUNE_ROW_PATH: 0 LDS tiers, 1 every column on the global-workspace (repairing) path
    uint32_t tune_compact_b = 0;         // BELLA_TUNE_COMPACT_B: 0 the layout drops the B' entries that have no later read, 1 keeps them
    uint32_t tune_product_entries = 0;   // BELLA_TUNE_PRODUCT_ENTRIES: 0 one B' entry per product when it stays within 12 B per owned nonzero, 1 never, 2 always
    uint32_t tune_order_split = kOrderOneLaunchMax;   // BELLA_TUNE_ORDER_SPLIT: owned columns of a pass above which k_order_wave runs as two instances
    uint64_t tune_round_budget = 0;      // BELLA_TUNE_ROUND_BUDGET: direction bytes of a batch of a realignment / correction round; 0 by the free memory (round_budget)
    uint64_t tune_xdrop_batch = 0;       // BELLA_TUNE_XDROP_BATCH: extensions of a batch of the X-drop slices, as given; 0 by the free memory (run_xdrop)
    uint32_t tune_dist_layout = 2;       // BELLA_TUNE_DIST_LAYOUT: bella_hip_allgather_panels forms A' by k-mer id ranges over the communicator's ranks
                                         // (1: always, 0: never, 2 = default: on the in-process transport only -- over RCCL the path has not run on
                                         // more than one device yet, and its extra 20 B per nonzero of traffic want a measurement first)
    bool dist_agreed = false;            // ... and every rank of the communicator said it can (bella_hip_allgather_panels asks)
    bool layout_dist = false;            // ... and the current layout was built that way
    uint64_t tune_cache_bytes = 192ull << 20;   // BELLA_TUNE_CACHE_BYTES: A' above this size counts as "larger than the last-level cache"
    uint32_t xdrop_variant = 1;          // 0: one launch in length-sorted order; 1 (default): slices with compaction; 2: packed kernel in pair order; 3: scalar statement
    size_t lds_attr[40] = {};             // largest dynamic-LDS size already granted to each row-kernel instantiation
    hipStream_t side[kNumTiers + 1]{};   // independent tier launches / fold instances run concurrently
    hipEvent_t fork = nullptr, join[kNumTiers + 1]{};
};

namespace {

int fail(bella_ctx* c, int code, const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    if (c) c->err = b;
    return code;
}

#define HIPCHK(c, call)                                                                                           \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return fail(c, BELLA_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define KCHK(c) HIPCHK(c, hipGetLastError())
#define NCCLCHK(c, call)                                                                                          \
    do {                                                                                                          \
        ncclResult_t r_ = (call);                                                                                 \
        if (r_ != ncclSuccess)                                                                                    \
            return fail(c, BELLA_ERR_HIP, "%s failed: %s", #call, c->api && c->api->GetErrorString ? c->api->GetErrorString(r_) : "RCCL error"); \
    } while (0)

void release(Buf& b);
void trim_pool(BufPool& pl) {
    for (auto& q : pl.free) (void)hipFree(q.first);
    pl.free.clear();
    pl.bytes = 0;
}
int ensure_bytes(bella_ctx* c, Buf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return 0;
    release(b);
    BufPool& pl = c->pool;
    b.pool = &pl;
    const size_t want = bytes + bytes / 16 + 256;
    int best = -1;                                              // best fit on the free list: at least `want`, at most about twice that
    for (int i = 0; i < (int)pl.free.size(); ++i)
        if (pl.free[i].second >= want && pl.free[i].second <= 2 * want + (64ull << 20) && (best < 0 || pl.free[i].second < pl.free[best].second)) best = i;
    if (best >= 0) {
        b.p = pl.free[best].first; b.cap = pl.free[best].second;
        pl.bytes -= b.cap;
        pl.free.erase(pl.free.begin() + best);
        return 0;
    }
    if (pl.arena.base) {                                        // the reserved slab first (bella_hip_reserve): no trip to the driver
        void* q = pl.arena.take(want);
        if (q) { b.p = q; b.cap = Arena::round(want); return 0; }
    }
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess && !pl.free.empty()) {                  // what the free list holds back may be what is missing
        (void)hipGetLastError();
        trim_pool(pl);
        e = hipMalloc(&b.p, want);
    }
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(c, BELLA_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return 0;
}
#define ENSURE(c, buf, bytes)                  \
    do {                                       \
        int r_ = ensure_bytes(c, buf, bytes);  \
        if (r_) return r_;                     \
    } while (0)

void release(Buf& b) {
    if (b.p) {
        BufPool* pl = b.pool;
        if (pl && pl->arena.owns(b.p)) {
            (void)hipDeviceSynchronize();                       // (as below: nothing in flight touches the range when it changes hands)
            pl->arena.give(b.p, b.cap);
        } else if (pl && b.cap >= kPoolMinBytes && pl->free.size() < 32 && pl->bytes + b.cap <= kPoolMaxBytes) {
            (void)hipDeviceSynchronize();                       // (what hipFree does: nothing in flight touches the buffer when it changes hands)
            pl->free.emplace_back(b.p, b.cap);
            pl->bytes += b.cap;
        } else {
            (void)hipFree(b.p);
        }
    }
    b.p = nullptr;
    b.cap = 0;
}

// A function's own device buffer: a Buf that is released when its scope ends, on every way out.  reset() gives it up earlier (where peak
// memory or what the pool holds afterwards depends on the point); give_to() hands the allocation to a Buf the context owns.
struct TmpBuf : Buf {
    TmpBuf() = default;
    TmpBuf(const TmpBuf&) = delete;
    TmpBuf& operator=(const TmpBuf&) = delete;
    ~TmpBuf() { release(*this); }
    void reset() { release(*this); }
    void swap(TmpBuf& o) { std::swap<Buf>(*this, o); }
    void give_to(Buf& dst) { release(dst); dst = *this; p = nullptr; cap = 0; }
};

template <class T>
T* ptr(const Buf& b) { return (T*)b.p; }

inline unsigned nblk(uint64_t n, unsigned per = 256) { return (unsigned)((n + per - 1) / per); }

int read_status(bella_ctx* c, uint32_t* out) {
    HIPCHK(c, hipMemcpyAsync(out, c->status.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int status_to_error(bella_ctx* c, uint32_t st) {
    if (st & 4u) return fail(c, BELLA_ERR_BAD_BASE, "reads must be upper-case ACGT only");
    if (st & 8u) return fail(c, BELLA_ERR_TUPLE_ORDER, "tuples must be grouped by non-decreasing read id < nreads");
    if (st & 16u) return fail(c, BELLA_ERR_READ_TOO_LONG, "a read has >= 65536 tuples");
    if (st & 32u) return fail(c, BELLA_ERR_BAD_ARG, "k-mer id >= nkmers");
    if (st & 64u) return fail(c, BELLA_ERR_BAD_ARG, "a k-mer occurs in more than 16383 reads");
    if (st & 128u) return fail(c, BELLA_ERR_BAD_ARG, "a tuple's position + k exceeds the length of its read");
    if (st & 2u) return fail(c, BELLA_ERR_ROW_TOO_LARGE, "an output column has >= 65536 products");
    return 0;
}

// hipCUB's two-phase call, written once: `fn(tmp, bytes)` is asked for its size with tmp == nullptr, the context's scratch grows to
// that (plus `slack`), and the call runs.  CUB(c, function, its arguments after the first two) returns from the caller on failure, like HIPCHK.
template <class Fn>
int cub_call(bella_ctx* c, const char* what, int line, Fn&& fn, size_t slack = 0) {
    size_t tb = 0;
    hipError_t e = fn(nullptr, tb);
    if (e == hipSuccess) {
        ENSURE(c, c->cubtmp, tb + slack);
        e = fn(c->cubtmp.p, tb);
    }
    if (e != hipSuccess) return fail(c, BELLA_ERR_HIP, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), __FILE__, line);
    return 0;
}
#define CUB_SLACK(c, slack, fn, ...)                                                                                         \
    do {                                                                                                                     \
        int r_ = cub_call(c, #fn, __LINE__, [&](void* t_, size_t& n_) { return fn(t_, n_, __VA_ARGS__); }, slack);           \
        if (r_) return r_;                                                                                                   \
    } while (0)
#define CUB(c, fn, ...) CUB_SLACK(c, 0, fn, __VA_ARGS__)

// exclusive scans (rocPRIM through hipCUB: plumbing, not a hot op)
int scan_u32(bella_ctx* c, const uint32_t* in, uint32_t* out, uint64_t n) {
    CUB(c, hipcub::DeviceScan::ExclusiveSum, in, out, (int)n, c->stream);
    return 0;
}
int scan_u32_to_u64(bella_ctx* c, const uint32_t* in, uint64_t* out, uint64_t n) {
    hipcub::TransformInputIterator<uint64_t, CastU64, const uint32_t*> it(in, CastU64());
    CUB(c, hipcub::DeviceScan::ExclusiveSum, it, out, (int)n, c->stream);
    return 0;
}
int scan_u8_to_u32(bella_ctx* c, const uint8_t* in, uint32_t* out, uint64_t n) {
    hipcub::TransformInputIterator<uint32_t, CastU8, const uint8_t*> it(in, CastU8());
    CUB(c, hipcub::DeviceScan::ExclusiveSum, it, out, (int)n, c->stream);
    return 0;
}

float ev_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

// a function's own timing events: create(n) makes the first n of a, b, d, e; all of them go with the scope
struct EventSet {
    hipEvent_t a = nullptr, b = nullptr, d = nullptr, e = nullptr;
    ~EventSet() { for (hipEvent_t x : {a, b, d, e}) if (x) (void)hipEventDestroy(x); }
    int create(bella_ctx* c, int n) {
        hipEvent_t* const all[4] = {&a, &b, &d, &e};
        for (int i = 0; i < n; ++i) HIPCHK(c, hipEventCreate(all[i]));
        return 0;
    }
};

// The ABI's sized structs: struct_size in, at most struct_size bytes out.  take_params: the caller's struct over `p` (which holds the
// defaults) when there is one -- longer than this library's is fine, shorter is refused; put_sized: a result struct, cut to the caller's size.
template <class P>
int take_params(bella_ctx* c, P& p, const P* given, const char* name) {
    if (!given) return 0;
    if (given->struct_size < sizeof(P)) return fail(c, BELLA_ERR_BAD_ARG, "%s: struct_size %u is too small", name, given->struct_size);
    p = *given;
    return 0;
}
template <class S>
int put_sized(void* out, uint64_t struct_size, const S& s) {
    std::memcpy(out, &s, (size_t)std::min<uint64_t>(struct_size, sizeof(S)));
    return 0;
}

// ---- stage state --------------------------------------------------------------------------------------------------
// What is built directly from each stage.  changed(s): s has other contents now, so everything built from it goes, and what was built
// from that; drop(s): s goes too (a stage drops itself when it starts and comes back with made(s) when it has succeeded).
constexpr uint32_t stage_bit(Stage s) { return 1u << s; }
constexpr uint32_t kBuiltFrom[kStages] = {
    /* READS   */ stage_bit(TUPLES) | stage_bit(PANEL) | stage_bit(MATRIX) | stage_bit(TRIM) | stage_bit(GRAPH) | stage_bit(PILE),
    /* TUPLES  */ 0,                         // (a recount keeps the matrix: its B was copied out of the tuples)
    /* PANEL   */ 0,
    /* MATRIX  */ stage_bit(PAIRS),
    /* PAIRS   */ stage_bit(ALNS),
    /* ALNS    */ stage_bit(TRACES),
    /* TRACES  */ 0,                         // (bella_hip_graph_add_traced copies records out)
    /* BATCH_OPS */ 0,                       // (the runs of a bella_hip_trace_batch, whose pairs were the caller's)
    /* RECORDS */ stage_bit(TRIM) | stage_bit(GRAPH),
    /* TRIM    */ stage_bit(GRAPH),
    /* GRAPH   */ stage_bit(UNITIGS),
    /* UNITIGS */ stage_bit(POLISH) | stage_bit(LINKS),
    /* POLISH  */ stage_bit(REALIGN) | stage_bit(LINKS),
    /* REALIGN */ stage_bit(LINKS),          // (a round reads the round before and replaces it: realign_round says changed(REALIGN))
    /* PILE    */ stage_bit(CONS) | stage_bit(POLISH),
    /* CONS    */ stage_bit(RECORRECT),
    /* RECORRECT */ 0,                       // (a round reads the round before and replaces it)
    /* LINKS   */ 0,
};
void drop(bella_ctx* c, Stage s);
void changed(bella_ctx* c, Stage s) {
    for (uint32_t d = 0; d < kStages; ++d)
        if (kBuiltFrom[s] & (1u << d)) drop(c, (Stage)d);
}
void drop(bella_ctx* c, Stage s) {
    c->as.valid &= ~stage_bit(s);
    changed(c, s);
}
void made(bella_ctx* c, Stage s) { c->as.valid |= stage_bit(s); }
bool has(const bella_ctx* c, Stage s) { return (c->as.valid & stage_bit(s)) != 0; }
// the precondition of a call that reads stage s
int need(bella_ctx* c, Stage s) {
    static const char* const first[kStages] = {"set_reads first", "count_kmers first", "assemble_panel first", "set_B / assemble_tuples first",
                                               "overlap first", "align_pairs first", "trace_pairs first", "trace_batch first",
                                               "", "bella_hip_graph_trim first", "bella_hip_graph_build first", "bella_hip_graph_unitigs first",
                                               "bella_hip_graph_polish_unitigs first", "bella_hip_graph_realign_unitigs first", "bella_hip_pileup_reset first", "bella_hip_consensus first",
                                               "bella_hip_recorrect first", "bella_hip_graph_align_links first"};
    return has(c, s) ? 0 : fail(c, BELLA_ERR_STATE, "%s", first[s]);
}

// a stage's result struct for the caller: get(state) is the struct
template <class Get>
int get_stats(bella_ctx* c, Stage s, void* out, uint64_t struct_size, Get get) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, s)) return r;
    return put_sized(out, struct_size, get(c->as));
}
// ... and one of its arrays, when the caller wants it
template <class T>
void copy_out(void* dst, const std::vector<T>& v) {
    if (dst && !v.empty()) std::memcpy(dst, v.data(), sizeof(T) * v.size());
}

// the accumulated records / the clips on the device, for the length of one stage call (a trim exists and there are reads when the
// clips are asked for)
int upload_records(bella_ctx* c, Buf& recs) {
    const size_t bytes = sizeof(bella_overlap) * c->as.records.size();
    ENSURE(c, recs, bytes);
    if (bytes) HIPCHK(c, c->stager.h2d(recs.p, c->as.records.data(), bytes, c->stream));
    return 0;
}
int upload_clips(bella_ctx* c, Buf& clips) {
    const size_t bytes = sizeof(bella_read_clip) * c->as.trim.clips.size();
    ENSURE(c, clips, bytes);
    HIPCHK(c, c->stager.h2d(clips.p, c->as.trim.clips.data(), bytes, c->stream));
    return 0;
}

// A text file one of the writers fills: opened with a 4 MB buffer; close(ok) is the writer's result -- `ok` and the close itself.  Both
// ways to fail are reported on stderr under the writer's name.
struct TextFile {
    const char *who, *path;
    FILE* f;
    std::vector<char> buf;
    TextFile(const char* who_, const char* path_, const char* mode) : who(who_), path(path_), f(std::fopen(path_, mode)), buf((size_t)4 << 20) {
        if (f) std::setvbuf(f, buf.data(), _IOFBF, buf.size());
        else fprintf(stderr, "%s: cannot open %s\n", who, path);
    }
    ~TextFile() { if (f) (void)std::fclose(f); }
    int close(bool ok) {
        if (std::fclose(f) != 0) ok = false;
        f = nullptr;
        if (!ok) { fprintf(stderr, "%s: writing %s failed\n", who, path); return BELLA_ERR_BAD_ARG; }
        return 0;
    }
};

// the row pointers the passes index B' with: the rows of the context's own columns (build_layout; the other rows are empty)
inline const uint32_t* layout_bptr(const bella_ctx* c) { return ptr<uint32_t>(c->Bloc); }

// B (Bptr/Bk/Bpos on device) -> Bent / Aent   (see assemble.hpp): one stable radix sort of the entries by k-mer id (the runs are
// the k-mer lists of A', ascending read id) and coalesced segmented passes; 32 B of temporaries per nonzero.
// The layout follows the context's partition (bella_hip_set_partition): A' is whole, B' entries -- and the optional row lists --
// exist for the owned columns only, so the per-column part of the work and of the memory is 1/stride of the whole.
// The large working buffers of k-mer counting (the sort's two key arrays and the tile arrays: 29 GB at 100k reads) stay with the context
// when the call returns and go when the next stage starts (assembly, device layout): a second count finds them in place, a pipeline's
// peak is what it was -- and no call frees tens of GB only for the next one to ask for them again at once (hipMalloc right after a
// hipFree of that size was measured at ~1 s on ROCm 7.2, against microseconds otherwise).
void release_count_scratch(bella_ctx* c) {
    release(c->kc_keys); release(c->kc_alt); release(c->kc_runlen); release(c->kc_flag); release(c->kc_slot);
}

// (bella_hip_allgather_panels with BELLA_TUNE_DIST_LAYOUT: the formation of A' shared over the ranks; defined behind the collectives)
int layout_dist(bella_ctx* c, uint64_t nown_nnz, uint32_t rmask, uint32_t inl, int kbits, uint32_t** ekey_out, uint64_t** eval_out,
                uint32_t** fkey_out, uint64_t** fval_out);
void layout_dist_fail(bella_ctx* c);
bool layout_dist_eligible(const bella_ctx* c);

// collective: every rank of the context's communicator is inside this call (bella_hip_allgather_panels) -- the only caller that may
// take the shared formation of A'
int build_layout(bella_ctx* c, bool collective = false) {
    release_count_scratch(c);
    const uint64_t nnz = c->nnz;
    const uint32_t nk = c->nkmers;
    const uint32_t pf = c->part_first, ps = c->part_stride;
    if (nnz >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "nnz(A) must be < 2^32 (KMERINDEX uint32, main.cpp:60)");
    drop(c, MATRIX);
    c->have_rowlists = false;
    c->layout_inline = 0;
    c->layout_products = false;
    c->layout_first_app = false;
    c->layout_place_sorted = false;
    c->live_nnz = 0;
    c->tm.expand_ms = 0.f;
    // shared formation of A' (layout_dist): every rank agreed to it in bella_hip_allgather_panels, so a rank that fails BEFORE it gets
    // there still says so in the formation's metadata exchange -- the others leave instead of waiting for it
    const bool dist = collective && c->dist_agreed;
    struct Bail { bella_ctx* c; bool armed; ~Bail() { if (armed) layout_dist_fail(c); } } bail{c, dist};
    if (dist && (c->debug & 262144u)) return fail(c, BELLA_ERR_STATE, "debug bit 18: this rank fails before its share of the formation");
    if (!dist) {                                                   // (shared: the sort buffers are sized by the rank's share)
        ENSURE(c, c->lk_key, 4 * nnz);
        ENSURE(c, c->lk_key2, 4 * nnz);
        ENSURE(c, c->lk_val, 8 * nnz);
        ENSURE(c, c->lk_val2, 8 * nnz);
    }
    ENSURE(c, c->lk_rinfo, 8 * ((size_t)c->nreads + 1));
    // (w also holds one word per READ: the owned rows' lengths of a partitioned layout, the rows' product counts of the row lists --
    // a matrix with fewer nonzeros than reads must not shrink it below that)
    ENSURE(c, c->w, 4 * std::max<uint64_t>(nnz + 1, (uint64_t)c->nreads + 2));
    ENSURE(c, c->wscan, 4 * std::max<uint64_t>(nnz + 1, (uint64_t)c->nreads + 2));
    ENSURE(c, c->Aent, 8 * nnz + 64);
    HIPCHK(c, hipMemsetAsync(c->status.p, 0, 4, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    // the context's own row pointers: all rows, or the owned ones (the others keep no entries)
    uint64_t nown_nnz = nnz;
    c->layout_first = pf; c->layout_stride = ps;
    ENSURE(c, c->Bloc, 4 * ((size_t)c->nreads + 2));
    if (ps > 1) {
        uint32_t* len = ptr<uint32_t>(c->w);
        k_layout_own_lengths<<<nblk((uint64_t)c->nreads + 1), 256, 0, c->stream>>>(ptr<uint32_t>(c->Bptr), c->nreads, pf, ps, len);
        KCHK(c);
        int rc = scan_u32(c, len, ptr<uint32_t>(c->Bloc), (uint64_t)c->nreads + 1);
        if (rc) return rc;
        uint32_t n32 = 0;
        HIPCHK(c, hipMemcpyAsync(&n32, ptr<uint32_t>(c->Bloc) + c->nreads, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        nown_nnz = n32;
    } else {
        HIPCHK(c, hipMemcpyAsync(c->Bloc.p, c->Bptr.p, 4 * ((size_t)c->nreads + 1), hipMemcpyDeviceToDevice, c->stream));
    }
    c->owned_nnz = 0;
    uint32_t ratio1024 = 1024;
    uint64_t rowF_total = 0;                                       // the products of the owned rows, once rowF has been scanned in 64 bits ...
    bool rowF_scanned = false;                                     // ... into lk_rinfo
    c->long_list_sample = false;
    const uint32_t* Bloc = ptr<uint32_t>(c->Bloc);                 // the rows of the owned columns
    // (buffers only ever grow; a context that goes from a whole layout to a partition's gives the difference back)
    if (c->Bent.cap > 16 * nown_nnz + (1u << 20)) release(c->Bent);
    ENSURE(c, c->Bent, 8 * nown_nnz);
    const bool first_app = c->tune_layout_order == 1 || (c->debug & 1024u);
    c->layout_dist = dist;
    if (nnz || dist) {
        int kbits = 1;
        while (kbits < 32 && (1ull << kbits) < (uint64_t)nk) ++kbits;
        const uint32_t rmask = c->nreads <= (1u << 30) ? 0x3FFFFFFFu : 0x7FFFFFFFu;   // read id field of the sort value
        // Default: the lists of A' stay in k-mer order (= the sorted order itself; nothing to scatter, scan or look up) and every pass
        // expands B' x A' itself: the fastest ONE-SHOT call (layout + first pass).  BELLA_TUNE_LAYOUT_ORDER 1 (tests): the lists in
        // order of first appearance in B' (the owner row of a list streams it; three more random-access passes here).
        const uint32_t by_kmer = first_app ? 0u : 1u;
        c->layout_first_app = first_app;
        // entries whose k-mer has exactly one later read carry that read (util.hpp: INLINE form) when bit 31 of the list index and bit 30
        // of a read id are free -- and when A' is larger than the last-level cache (256 MB): the form saves a line from HBM per such
        // entry and pass (row kernels 4.03 -> 3.69 ms at 100k reads, A' = 1.6 GB), but where the gather is a cache hit it only adds a
        // branch (10k reads, A' = 92 MB: 0.360 -> 0.367 ms per step).  BELLA_TUNE_INLINE_ENTRIES 1: the plain form everywhere, as for inputs
        // beyond those bounds; 2: the inline form on any size
        const bool inl_pays = 8ull * nnz > c->tune_cache_bytes || c->tune_inline == 2 || (c->debug & 65536u);
        const uint32_t inl = rmask == 0x3FFFFFFFu && nnz < 0x80000000ull && inl_pays && c->tune_inline != 1 && !(c->debug & 32768u) ? 1u : 0u;
        c->layout_inline = inl;
        uint32_t* ekey = nullptr;                                  // the nown_nnz B' entries of this context's rows {own index, entry}, any order ...
        uint64_t* eval = nullptr;
        const uint32_t* skey = nullptr;                            // ... and two free buffers of that size for the partition pass below
        const uint64_t* sval = nullptr;
        if (dist) {
            uint32_t *fk = nullptr; uint64_t* fv = nullptr;
            bail.armed = false;                                    // (from here on layout_dist speaks for this rank)
            int rcd = layout_dist(c, nown_nnz, rmask, inl, kbits, &ekey, &eval, &fk, &fv);
            if (rcd) return rcd;
            skey = fk; sval = fv;
        } else {
        k_layout_prep<<<nblk(c->nreads, kWaves), kBlock, 0, c->stream>>>(ptr<uint32_t>(c->Bptr), ptr<uint32_t>(c->Bk), ptr<uint16_t>(c->Bpos), c->nreads,
                                                                        ptr<uint32_t>(c->packed), ptr<uint64_t>(c->roff), c->kmer_size, nk,
                                                                        ptr<uint32_t>(c->lk_key), ptr<uint64_t>(c->lk_val),
                                                                        first_app ? ptr<uint32_t>(c->w) : nullptr, ptr<uint32_t>(c->status));
        KCHK(c);
        // bad input (k-mer id out of range, k-mer past the end of its read) stops here: the passes below trust the keys
        uint32_t st0 = 0;
        int rc0 = read_status(c, &st0);
        if (rc0) return rc0;
        rc0 = status_to_error(c, st0);
        if (rc0) return rc0;
        hipcub::DoubleBuffer<uint32_t> dk(ptr<uint32_t>(c->lk_key), ptr<uint32_t>(c->lk_key2));
        hipcub::DoubleBuffer<uint64_t> dv(ptr<uint64_t>(c->lk_val), ptr<uint64_t>(c->lk_val2));
        CUB(c, hipcub::DeviceRadixSort::SortPairs, dk, dv, (uint64_t)nnz, 0, kbits, c->stream);
        skey = dk.Current();
        sval = dv.Current();
        if (!by_kmer) {
            k_layout_heads<<<nblk(nnz), 256, 0, c->stream>>>(skey, sval, nnz, ptr<uint32_t>(c->Bptr), rmask, ptr<uint32_t>(c->w), ptr<uint32_t>(c->status));
            KCHK(c);
            int rc = scan_u32(c, ptr<uint32_t>(c->w), ptr<uint32_t>(c->wscan), nnz);
            if (rc) return rc;
        }
        ekey = dk.Alternate();                                     // (the sort's other buffers are free now)
        eval = dv.Alternate();
        uint32_t* counter = ptr<uint32_t>(c->status) + 7;
        HIPCHK(c, hipMemsetAsync(counter, 0, 4, c->stream));
        uint2* rinfo = ptr<uint2>(c->lk_rinfo);
        k_layout_rinfo<<<nblk(c->nreads), 256, 0, c->stream>>>(Bloc, ptr<uint64_t>(c->roff), c->nreads, rinfo);
        KCHK(c);
        k_layout_emit<<<nblk(nnz, ps > 1 ? kLayoutEmitPartBlock : 256), ps > 1 ? kLayoutEmitPartBlock : 256, 0, c->stream>>>(skey, sval, nnz, ptr<uint32_t>(c->Bptr), Bloc, ptr<uint32_t>(c->wscan), ptr<uint32_t>(c->packed),
                                                        ptr<uint64_t>(c->roff), c->kmer_size, rmask, ptr<uint2>(c->Aent), ekey, eval, by_kmer, pf, ps, counter,
                                                        ptr<uint32_t>(c->status), inl, rinfo);
        KCHK(c);
        {   // a k-mer in more than 16,383 reads overflows the count field of the B' entries: stop before anything trusts them
            uint32_t st1 = 0;
            int rc1 = read_status(c, &st1);
            if (rc1) return rc1;
            rc1 = status_to_error(c, st1);
            if (rc1) return rc1;
        }
        }   // !dist
        if (nown_nnz) {   // one radix pass on the top 8 bits of the entry index: B' is then written region by region
            int ebits = 1;
            while (ebits < 32 && (1ull << ebits) < nown_nnz) ++ebits;
            hipcub::DoubleBuffer<uint32_t> ek(ekey, const_cast<uint32_t*>(skey));
            hipcub::DoubleBuffer<uint64_t> ev(eval, const_cast<uint64_t*>(sval));
            if (ebits > 12) CUB(c, hipcub::DeviceRadixSort::SortPairs, ek, ev, (uint64_t)nown_nnz, ebits - 8, ebits, c->stream);
            c->layout_place_sorted = ebits > 12;
            k_layout_place<<<((nblk(nown_nnz) + 7u) / 8u) * 8u, 256, 0, c->stream>>>(ek.Current(), ev.Current(), nown_nnz, ptr<uint2>(c->Bent));
            KCHK(c);
        }
        c->owned_nnz = nown_nnz;
        c->live_nnz = nown_nnz;
        ENSURE(c, c->rowF, 4 * ((size_t)c->nreads + 2));
        if (!nown_nnz) HIPCHK(c, hipMemsetAsync(c->rowF.p, 0, 4 * ((size_t)c->nreads + 2), c->stream));
        if (nown_nnz) {
            // one pass over the rows of B': the rows' products (rowF: what estimateFLOP returns, kept like a row pointer) and their live
            // entries; then B' without the entries that have no later read (assemble.hpp: k_layout_live / k_layout_compact): new row
            // pointers by a scan of the live counts, the live entries moved in their order; from here on Bloc indexes the compacted B'
            const bool compact = !c->tune_compact_b;
            uint32_t* len = ptr<uint32_t>(c->w);
            uint32_t* bnew = ptr<uint32_t>(c->wscan);
            k_layout_live<<<nblk((uint64_t)c->nreads + 1, kWaves), kBlock, 0, c->stream>>>(Bloc, ptr<uint2>(c->Bent), c->nreads, inl, compact ? len : nullptr,
                                                                                         ptr<uint32_t>(c->rowF));
            KCHK(c);
            // One entry per PRODUCT (assemble.hpp: k_layout_compact_products) instead of one per live entry: the row pointers are the scan
            // of rowF, the LDS-tier row kernels then have no expansion phase.  Not next to the row lists (they replace B' in the pass); the
            // products must fit a 32-bit row pointer; and 8 B per product may not exceed 12 B per owned nonzero -- that keeps B' inside the
            // 13 B per owned nonzero the layout promises, and long-list inputs (HiFi-like, ~14 products per nonzero), which get the row
            // lists anyway, on the per-entry form.  If the buffer cannot be had (debug bit 11: tests, as if), the per-entry form stands.
            // (both scans -- live entries, products -- and both totals before ONE wait: an input that stays on the per-entry form pays no
            // host round trip for having been asked; the row lists below start from the same 64-bit scan)
            uint32_t live = 0;
            if (compact) {
                int rc = scan_u32(c, len, bnew, (uint64_t)c->nreads + 1);
                if (rc) return rc;
                HIPCHK(c, hipMemcpyAsync(&live, bnew + c->nreads, 4, hipMemcpyDeviceToHost, c->stream));
            }
            // (auto additionally asks that A' be larger than the last-level cache, the rule of the inline entries: at 10k reads, A' = 92 MB,
            // the form saves no time and its longer B' -- there 1.67 x the live entries -- costs 2 % of the step)
            const bool ask_products = compact && c->tune_product_entries != 1 &&
                                      (c->tune_product_entries == 2 || (!c->want_rowlists && 8ull * nnz > c->tune_cache_bytes));
            if (ask_products) {
                int rc = scan_u32_to_u64(c, ptr<uint32_t>(c->rowF), ptr<uint64_t>(c->lk_rinfo), (uint64_t)c->nreads + 1);   // (rowF[nreads] = 0)
                if (rc) return rc;
                HIPCHK(c, hipMemcpyAsync(&rowF_total, ptr<uint64_t>(c->lk_rinfo) + c->nreads, 8, hipMemcpyDeviceToHost, c->stream));
                rowF_scanned = true;
            }
            if (compact) HIPCHK(c, hipStreamSynchronize(c->stream));
            if (ask_products) {
                Buf& start = c->lk_rinfo;                          // (free since k_layout_emit) the 64-bit scan of rowF: the new row pointers, and their total
                const uint64_t F = rowF_total;
                const bool small = 8ull * F <= 12ull * nown_nnz || c->tune_product_entries == 2;
                if (F && F < 0xFFFFFFF0ull && small && !(c->debug & 2048u)) {
                    TmpBuf out;
                    if (!ensure_bytes(c, out, 8 * (size_t)F)) {
                        k_layout_compact_products<<<c->nreads, 64, 0, c->stream>>>(Bloc, ptr<uint64_t>(start), bnew, ptr<uint2>(c->Bent), c->nreads, inl,
                                                                                   ptr<uint2>(out));
                        if (hipGetLastError() != hipSuccess) return fail(c, BELLA_ERR_HIP, "k_layout_compact_products failed to launch");
                        HIPCHK(c, hipMemcpyAsync(c->Bloc.p, bnew, 4 * ((size_t)c->nreads + 1), hipMemcpyDeviceToDevice, c->stream));
                        HIPCHK(c, hipStreamSynchronize(c->stream));
                        out.give_to(c->Bent);
                        c->live_nnz = F;
                        c->layout_products = true;
                    } else c->err.clear();
                }
            }
            if (compact && !c->layout_products) {
                TmpBuf out;
                ENSURE(c, out, 8 * (size_t)live);
                k_layout_compact<<<nblk(c->nreads, kWaves), kBlock, 0, c->stream>>>(Bloc, bnew, ptr<uint2>(c->Bent), c->nreads, inl, ptr<uint2>(out));
                if (hipGetLastError() != hipSuccess) return fail(c, BELLA_ERR_HIP, "k_layout_compact failed to launch");
                HIPCHK(c, hipMemcpyAsync(c->Bloc.p, bnew, 4 * ((size_t)c->nreads + 1), hipMemcpyDeviceToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                out.give_to(c->Bent);                              // (the uncompacted B' goes here, not at the end of the call)
                c->live_nnz = live;
            }
        }
        // pairs/products on a sample of (owned) columns -> key-table budget of the LDS tiers (see k_sample_pair_ratio), and: is this a
        // long-list input (HiFi-like: at most one pair in 64 products)?
        const size_t bitmap_bytes = 4 * (((size_t)c->nreads + 31) / 32);
        uint32_t samp[2] = {0, 0};
        if (c->owned_nnz && bitmap_bytes <= 128 * 1024) {
            HIPCHK(c, hipMemsetAsync(ptr<uint32_t>(c->status) + 6, 0, 16, c->stream));   // [6] max ratio, [8] pairs, [9] products / 64 of the sample
            const uint32_t ncols = c->nreads / ps + 1;                  // owned columns: first + j * stride
            const uint32_t nsample = ncols < 512 ? ncols : 512;
            const uint32_t step = (ncols / nsample ? ncols / nsample : 1) * ps;
            HIPCHK(c, hipFuncSetAttribute((const void*)k_sample_pair_ratio, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bitmap_bytes));
            k_sample_pair_ratio<<<nsample, kBlock, bitmap_bytes, c->stream>>>(Bloc, ptr<uint2>(c->Bent), ptr<uint2>(c->Aent),
                                                                             c->nreads, pf, step, ptr<uint32_t>(c->status) + 6, inl);
            KCHK(c);
            HIPCHK(c, hipMemcpyAsync(&ratio1024, ptr<uint32_t>(c->status) + 6, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(samp, ptr<uint32_t>(c->status) + 8, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        // Long-list inputs send most of their columns to the path above the LDS tiers, which groups a column's products in LDS from a
        // product list -- expanded per batch and per pass when the layout has none.  The same expansion once, here, costs a one-shot
        // call nothing and every further pass less: such inputs get the row lists whenever they fit.
        c->long_list_sample = samp[1] > 0 && samp[0] <= samp[1];     // >= 64 products per pair on the sample
        const bool auto_lists = c->long_list_sample && !(c->debug & 1u) && c->tune_row_path != 1 && c->lane_order_ok;
        if (by_kmer && (c->want_rowlists || auto_lists) && c->nreads <= (1u << 30)) {
            // row lists (BELLA_TUNE_ROW_LISTS): products per owned row -> row starts -> the tails of the lists copied in product order.
            // Optional in every respect: if they do not fit next to what a pass needs, or an allocation fails, the layout stands without them.
            int rc = ensure_bytes(c, c->Arow, 8 * ((size_t)c->nreads + 2));
            uint64_t F = 0;
            if (!rc && rowF_scanned) {                             // (the compaction above already scanned rowF in 64 bits and knows the total)
                HIPCHK(c, hipMemcpyAsync(c->Arow.p, c->lk_rinfo.p, 8 * ((size_t)c->nreads + 1), hipMemcpyDeviceToDevice, c->stream));
                F = rowF_total;
            } else if (!rc) {
                rc = scan_u32_to_u64(c, ptr<uint32_t>(c->rowF), ptr<uint64_t>(c->Arow), (uint64_t)c->nreads + 1);   // (rowF[nreads] = 0)
                if (rc) return rc;
                HIPCHK(c, hipMemcpyAsync(&F, ptr<uint64_t>(c->Arow) + c->nreads, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
            size_t mfree = 0, mtotal = 0;
            HIPCHK(c, hipMemGetInfo(&mfree, &mtotal));
            // (released buffers and the reserved slab count as free for this purpose -- the slab by its largest HOLE: the lists are one
            // buffer, and a fragmented slab that cannot give it would send the request to the driver next to the slab's 55 % of VRAM)
            mfree += c->pool.bytes + c->pool.arena.largest_hole();
            // 10 bytes per product for the lists; a pass over all owned columns then needs about 60 more per product (records twice,
            // product lists, scratch, diagnostics) -- the lists are only built when both fit (debug bit 11: tests, "no room")
            const bool fits = (double)F * 70.0 + 1e8 <= (double)mfree && !(c->debug & 2048u);
            if (!rc && fits) {
                HIPCHK(c, hipEventRecord(c->ev[10], c->stream));
                rc = ensure_bytes(c, c->Aent2, 8 * F + 64);
                if (!rc) rc = ensure_bytes(c, c->Aov, 2 * F + 64);
                if (!rc) {
                    const uint32_t grid = c->nreads < 4096u ? c->nreads : 4096u;
                    if (grid) k_layout_rowlists<<<grid, kRowListBlock, 0, c->stream>>>(Bloc, ptr<uint2>(c->Bent), ptr<uint2>(c->Aent), ptr<uint64_t>(c->Arow),
                                                                                     ptr<uint64_t>(c->roff), nullptr, c->nreads, ptr<uint2>(c->Aent2), ptr<uint16_t>(c->Aov), inl);
                    KCHK(c);
                    HIPCHK(c, hipEventRecord(c->ev[11], c->stream));
                    HIPCHK(c, hipEventSynchronize(c->ev[11]));
                    c->tm.expand_ms = ev_ms(c->ev[10], c->ev[11]);
                    c->have_rowlists = true;
                }
            }
            if (!c->have_rowlists) { release(c->Aent2); release(c->Aov); release(c->Arow); c->err.clear(); }
        }
    }
    if (!c->have_rowlists) { release(c->Aent2); release(c->Aov); release(c->Arow); }
    if (!nnz) {
        HIPCHK(c, hipMemsetAsync(c->Bloc.p, 0, 4 * ((size_t)c->nreads + 2), c->stream));
        ENSURE(c, c->rowF, 4 * ((size_t)c->nreads + 2));
        HIPCHK(c, hipMemsetAsync(c->rowF.p, 0, 4 * ((size_t)c->nreads + 2), c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
    uint32_t st = 0;
    int rc = read_status(c, &st);
    if (rc) return rc;
    rc = status_to_error(c, st);
    if (rc) return rc;
    c->pair_ratio1024 = ratio1024;
    // assembly temporaries are large (tens of bytes per nonzero): give them back
    release(c->lk_key); release(c->lk_key2); release(c->lk_val); release(c->lk_val2); release(c->w); release(c->wscan); release(c->lk_rinfo);
    c->tm.layout_ms = ev_ms(c->ev[4], c->ev[5]);
    made(c, MATRIX);
    c->layout_gen++;
    return 0;
}

// Xavier's scores are int8: the rule of align_pairs and of xdrop_batch (the LOGAN-scoring calls have no such bound)
int check_xavier_xdrop(bella_ctx* c, const bella_params* p) {
    if (p->xdrop > 127) return fail(c, BELLA_ERR_BAD_ARG, "params.xdrop must fit Xavier's int8 scores (<= 127)");
    return 0;
}

int check_params(bella_ctx* c, const bella_params* p) {
    if (!p) return fail(c, BELLA_ERR_BAD_ARG, "params is NULL");
    if (p->kmer_size != c->kmer_size)
        return fail(c, BELLA_ERR_BAD_ARG, "params.kmer_size (%u) differs from the matrix's (%u)", p->kmer_size, c->kmer_size);
    // (bin_size == 0 is legal: chain.hpp:114 compares |overlap difference| < binSize, so no two products ever share a bin)
    if (!p->skip_alignment) {
        if (int r = check_xavier_xdrop(c, p)) return r;
        if (!(p->error_rate >= 0.0 && p->error_rate <= 1.0) || !(p->delta_chernoff >= 0.0 && p->delta_chernoff <= 1.0))
            return fail(c, BELLA_ERR_BAD_ARG, "params.error_rate and params.delta_chernoff must lie in [0, 1]");
    }
    return 0;
}

}  // namespace

extern "C" {

int bella_hip_abi_version(void) { return BELLA_HIP_ABI_VERSION; }

int bella_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* bella_hip_strerror(int code) {
    switch (code) {
        case BELLA_OK: return "ok";
        case BELLA_ERR_NO_DEVICE: return "no gfx950 HIP device";
        case BELLA_ERR_HIP: return "HIP runtime error";
        case BELLA_ERR_BAD_ARG: return "bad argument";
        case BELLA_ERR_BAD_BASE: return "read contains a character other than ACGT";
        case BELLA_ERR_READ_TOO_LONG: return "read too long for 16-bit positions";
        case BELLA_ERR_TUPLE_ORDER: return "tuples not grouped by read";
        case BELLA_ERR_STATE: return "call order violated";
        case BELLA_ERR_ROW_TOO_LARGE: return "output column too large";
        case BELLA_ERR_BINS: return "more than 16 overlap bins";
        case BELLA_ERR_NOMEM: return "out of device memory";
    }
    return "unknown error";
}

const char* bella_hip_last_error(const bella_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int bella_hip_init(int device, bella_ctx** out) {
    if (!out) return BELLA_ERR_BAD_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return BELLA_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return BELLA_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BELLA_ERR_NO_DEVICE;
    bella_ctx* c = new bella_ctx();
    c->device = device;
    c->ntiers = 0;
    for (uint32_t t = 0; t < kNumTiers; ++t) { c->tier_caps[t] = kTierCapsDefault[t]; c->ntiers = t + 1; if (kTierCapsDefault[t] == 65535) break; }
    hipError_t he = hipSetDevice(device);
    if (he == hipSuccess) he = hipStreamCreate(&c->stream);
    for (auto& e : c->ev) if (he == hipSuccess) he = hipEventCreate(&e);
    {   // side streams 0 / 1 carry the classes of the largest columns: their workgroups go first whenever a CU has room
        int least = 0, greatest = 0;
        if (he == hipSuccess) he = hipDeviceGetStreamPriorityRange(&least, &greatest);
        int si = 0;
        for (auto& st : c->side) {
            // (the last one carries the host-driven sort-based path of wide.hpp next to the class launches: its small kernels and
            // copies must not queue behind the classes' workgroups)
            if (he == hipSuccess) he = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, si < 2 || si == kNumTiers ? greatest : least);
            ++si;
        }
    }
    if (he == hipSuccess) he = hipEventCreateWithFlags(&c->fork, hipEventDisableTiming);
    for (auto& e : c->join) if (he == hipSuccess) he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (he != hipSuccess) { bella_hip_destroy(c); return BELLA_ERR_HIP; }
    if (hipHostMalloc((void**)&c->pinned, 512, hipHostMallocDefault) != hipSuccess) { delete c; return BELLA_ERR_NOMEM; }
    if (ensure_bytes(c, c->status, 256)) { delete c; return BELLA_ERR_NOMEM; }
    (void)hipMemset(c->status.p, 0, 256);
    {   // the LDS tiers of the row kernels rely on lane-ordered same-address LDS atomics (spgemm.hpp, phase S): checked once per context
        uint32_t bad = 1;
        k_lane_order_selftest<<<1, 64, 0, c->stream>>>(ptr<uint32_t>(c->status) + 12);
        if (hipMemcpyAsync(&bad, ptr<uint32_t>(c->status) + 12, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) bad = 1;
        c->lane_order_ok = bad == 0;
        c->tm.lane_order = c->lane_order_ok ? 1u : 2u;
    }
    *out = c;
    return 0;
}

void bella_hip_destroy(bella_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm && c->api) { (void)c->api->CommDestroy(c->comm); c->comm = nullptr; }
    release(c->comm_meta);
    Buf* all[] = {&c->packed, &c->roff, &c->Bptr, &c->Bk, &c->Bpos, &c->Bent, &c->rowF, &c->Aent, &c->Aent2, &c->Aov, &c->Arow, &c->Bloc, &c->t_kmer, &c->t_read, &c->t_pos,
                  &c->tstart, &c->Bk_tmp, &c->Bpos_tmp, &c->rowcnt, &c->asm_ws, &c->asm_cls, &c->lk_key, &c->lk_key2, &c->lk_val, &c->lk_val2, &c->lk_rinfo,
                  &c->w, &c->wscan, &c->flopsr, &c->flopptr, &c->nnzC, &c->colptrC,
                  &c->rowlists, &c->tiercaps, &c->tmp_pairs, &c->tmp_ext, &c->pairs, &c->ext, &c->sortscr, &c->ws,
                  &c->status, &c->cubtmp, &c->alns, &c->seeds, &c->plist_hv, &c->overflow, &c->ctl, &c->retry, &c->orderlist, &c->order_ws, &c->w_f, &c->w_off, &c->w_key, &c->w_key2, &c->w_idx, &c->w_idx2, &c->w_hv, &c->w_ovfl,
                  &c->w_plist, &c->w_scr, &c->w_rlen, &c->w_rstart, &c->w_rrank, &c->w_redo, &c->w_segfirst, &c->w_toff, &c->w_table, &c->w_nruns, &c->w_desc, &c->w_gtab, &c->w_gcount, &c->w_gbase, &c->w_rfirst, &c->w_aent2, &c->w_aov, &c->kc_nk, &c->kc_koff, &c->kc_hist, &c->kc_keys, &c->kc_alt, &c->kc_runlen,
                  &c->kc_flag, &c->kc_slot, &c->kc_nruns, &c->kc_dcode, &c->kc_dcount, &c->kc_hkey, &c->kc_hval, &c->kc_found, &c->kc_tstart, &c->kc_cursor, &c->kc_sel, &c->kc_ringo, &c->kc_ringp, &c->kc_opos, &c->kc_oid, &c->kc_opos2, &c->kc_oid2, &c->xest, &c->xest2, &c->xids, &c->xorder, &c->xres, &c->xstate, &c->xlive, &c->lg_res, &c->lg_redo, &c->lg_scratch,
                  &c->tr_exts, &c->tr_lists, &c->tr_res, &c->tr_pres, &c->tr_opoff, &c->tr_dirs, &c->tr_scr, &c->tr_ops,
                  &c->pile, &c->pile_pairs, &c->pile_cnt, &c->pile_tmp, &c->cons_emit, &c->cons_scan, &c->cons_out, &c->cons_offs, &c->cons_stats,
                  &c->rc_aoff, &c->cons_anch, &c->rc_out, &c->rc_offs, &c->rc_stats, &c->rc_anch, &c->rc_jobs};
    for (Buf* b : all) release(*b);
    trim_pool(c->pool);
    if (c->pool.arena.base) { (void)hipFree(c->pool.arena.base); c->pool.arena = Arena(); }
    for (auto& e : c->ev) (void)hipEventDestroy(e);
    for (auto& st : c->side) (void)hipStreamDestroy(st);
    (void)hipEventDestroy(c->fork);
    for (auto& e : c->join) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    if (c->pinned) (void)hipHostFree(c->pinned);
    c->stager.destroy();
    delete c;
}

int bella_hip_set_tuning(bella_ctx* c, uint32_t what, const uint64_t* values, uint32_t n) {
    if (!c || (n && !values)) return BELLA_ERR_BAD_ARG;
    switch (what) {
        case BELLA_TUNE_LDS_TIERS: {                               // ascending product capacities of the LDS tiers, each in [64, 11008]; n = 0: defaults
            uint32_t caps[kNumTiers];
            uint32_t m = 0;
            for (uint32_t q = 0; q < n && m + 1 < kNumTiers; ++q) {
                const uint64_t v = values[q];
                if (v < 64 || v > 11008 || (m && v <= caps[m - 1])) return fail(c, BELLA_ERR_BAD_ARG, "tier caps must ascend within [64, 11008]");
                caps[m++] = (uint32_t)v;
            }
            if (m) {
                for (uint32_t t = 0; t < m; ++t) c->tier_caps[t] = caps[t];
                c->tier_caps[m] = 65535;
                c->ntiers = m + 1;
                c->tiers_from_env = true;
            } else {
                c->ntiers = 0;
                for (uint32_t t = 0; t < kNumTiers; ++t) { c->tier_caps[t] = kTierCapsDefault[t]; c->ntiers = t + 1; if (kTierCapsDefault[t] == 65535) break; }
                c->tiers_from_env = false;
            }
            c->caps_state = 0;
            c->pass_known = false;
            return 0;
        }
        case BELLA_TUNE_KCOUNT_BUDGET: c->kcount_budget = n && values[0] ? values[0] : (1ull << 30); return 0;
        case BELLA_TUNE_WIDE_BUDGET: c->wide_budget = n && values[0] ? values[0] : (1ull << 30); return 0;
        case BELLA_TUNE_XDROP_VARIANT:
            if (n && values[0] > 3) return fail(c, BELLA_ERR_BAD_ARG, "x-drop variant 0..3");   // (validated before it is stored)
            c->xdrop_variant = n ? (uint32_t)values[0] : 1u;
            return 0;
        case BELLA_TUNE_XDROP_CLASS_MIN: c->xdrop_class_min = n ? values[0] : 4ull * 4096 * 64; return 0;
        case BELLA_TUNE_ROW_LISTS:
            if (n && values[0] > 1) return fail(c, BELLA_ERR_BAD_ARG, "row lists: 0 or 1");
            c->want_rowlists = n && values[0] == 1;
            return 0;
        case BELLA_TUNE_LAYOUT_ORDER:
            if (n && values[0] > 1) return fail(c, BELLA_ERR_BAD_ARG, "layout order: 0 (k-mer order) or 1 (first appearance)");
            c->tune_layout_order = n ? (uint32_t)values[0] : 0u;
            return 0;
        case BELLA_TUNE_INLINE_ENTRIES:
            if (n && values[0] > 2) return fail(c, BELLA_ERR_BAD_ARG, "inline entries: 0 (by size), 1 (never) or 2 (always)");
            c->tune_inline = n ? (uint32_t)values[0] : 0u;
            return 0;
        case BELLA_TUNE_ROW_PATH:
            if (n && values[0] > 1) return fail(c, BELLA_ERR_BAD_ARG, "row path: 0 (LDS tiers) or 1 (global workspace)");
            c->tune_row_path = n ? (uint32_t)values[0] : 0u;
            c->pass_known = false;
            return 0;
        case BELLA_TUNE_DIST_LAYOUT:
            if (n && values[0] > 2) return fail(c, BELLA_ERR_BAD_ARG, "distributed layout: 0 (never), 1 (always) or 2 (on the in-process transport only)");
            c->tune_dist_layout = n ? (uint32_t)values[0] : 2u;
            return 0;
        case BELLA_TUNE_CACHE_BYTES:
            c->tune_cache_bytes = n && values[0] ? values[0] : (192ull << 20);
            return 0;
        case BELLA_TUNE_COMPACT_B:
            if (n && values[0] > 1) return fail(c, BELLA_ERR_BAD_ARG, "compact B': 0 (drop the entries without a later read) or 1 (keep them)");
            c->tune_compact_b = n ? (uint32_t)values[0] : 0u;
            return 0;
        case BELLA_TUNE_PRODUCT_ENTRIES:
            if (n && values[0] > 2) return fail(c, BELLA_ERR_BAD_ARG, "product entries: 0 (by size), 1 (never) or 2 (always)");
            c->tune_product_entries = n ? (uint32_t)values[0] : 0u;
            c->pass_known = false;
            return 0;
        case BELLA_TUNE_ORDER_SPLIT:
            c->tune_order_split = n ? (uint32_t)(values[0] < 0xFFFFFFFFull ? values[0] : 0xFFFFFFFFull) : kOrderOneLaunchMax;
            return 0;
        case BELLA_TUNE_ROUND_BUDGET: c->tune_round_budget = n ? values[0] : 0; return 0;
        case BELLA_TUNE_XDROP_BATCH: c->tune_xdrop_batch = n ? values[0] : 0; return 0;
    }
    return fail(c, BELLA_ERR_BAD_ARG, "unknown tuning parameter %u", what);
}

// Released buffers the context keeps for reuse (BufPool) go back to the driver: for hosts that share the device with other allocators
// (another context, RCCL, PyTorch) and would rather have the memory than the faster next stage.  The reserved slab is not touched.
int bella_hip_trim(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    trim_pool(c->pool);
    return 0;
}

// One slab from the driver, up front (see Arena): bytes == 0 gives an existing, unused slab back.  A larger request replaces an unused
// slab; while buffers live in the slab it stays as it is (BELLA_ERR_STATE).  What does not fit the slab later goes to hipMalloc as before.
int bella_hip_reserve(bella_ctx* c, uint64_t bytes, double* ms) {
    if (!c) return BELLA_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    Arena& a = c->pool.arena;
    if (ms) *ms = 0.0;
    if (a.base && a.in_use) return bytes <= a.size ? 0 : fail(c, BELLA_ERR_STATE, "the reserved slab is in use (%zu of %zu bytes)", a.in_use, a.size);
    if (a.base && bytes && bytes <= a.size) return 0;
    if (a.base) { HIPCHK(c, hipDeviceSynchronize()); (void)hipFree(a.base); a = Arena(); }
    if (!bytes) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    void* q = nullptr;
    trim_pool(c->pool);
    const size_t sz = Arena::round((size_t)bytes);
    hipError_t e = hipMalloc(&q, sz);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(c, BELLA_ERR_NOMEM, "hipMalloc(%zu) for the reserved slab failed: %s", sz, hipGetErrorString(e)); }
    // touch it now: the driver maps (and wipes) pages on first use, which is the cost this call exists to take out of the stages
    e = hipMemsetAsync(q, 0, sz, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(q); return fail(c, BELLA_ERR_HIP, "reserve: %s", hipGetErrorString(e)); }
    a.base = (char*)q; a.size = sz; a.in_use = 0; a.peak = 0;
    a.holes.clear();
    a.holes.emplace(0, sz);
    if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int bella_hip_set_debug(bella_ctx* c, uint32_t flags) {
    if (!c) return BELLA_ERR_BAD_ARG;
    c->debug = flags;
    return 0;
}

int bella_hip_set_column_range(bella_ctx* c, uint32_t first, uint32_t count) {
    if (!c) return BELLA_ERR_BAD_ARG;
    c->range_lo = first;
    c->range_hi = (uint64_t)first + count > 0xFFFFFFFFull ? 0xFFFFFFFFu : first + count;
    changed(c, MATRIX);
    return 0;
}

int bella_hip_set_partition(bella_ctx* c, uint32_t first, uint32_t stride) {
    if (!c || stride == 0 || first >= stride) return fail(c, BELLA_ERR_BAD_ARG, "partition needs 0 <= first < stride");
    c->part_first = first;
    c->part_stride = stride;
    changed(c, MATRIX);
    return 0;
}

// the reads onto the device: `fill(pinned, o, n)` produces bytes [o, o + n) of the concatenated bases (Stager::h2d_fill)
extern "C++" {
template <typename Fill>
static int set_reads_impl(bella_ctx* c, const uint64_t* offsets, uint32_t nreads, Fill&& fill) {
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t total = offsets[nreads];
    for (uint32_t r = 0; r < nreads; ++r) {
        if (offsets[r + 1] < offsets[r]) return fail(c, BELLA_ERR_BAD_ARG, "offsets must be non-decreasing");
        if (offsets[r + 1] - offsets[r] >= 65536ull)
            return fail(c, BELLA_ERR_READ_TOO_LONG, "read %u has %llu bases; positions are 16 bit (common.h:122-126)", r,
                        (unsigned long long)(offsets[r + 1] - offsets[r]));
    }
    const uint64_t nwords = (total + 15) / 16;
    ENSURE(c, c->packed, 4 * (nwords + 16));
    ENSURE(c, c->roff, 8 * ((size_t)nreads + 1));
    TmpBuf raw;
    ENSURE(c, raw, total);
    if (total) HIPCHK(c, c->stager.h2d_fill(raw.p, total, c->stream, fill));
    HIPCHK(c, hipMemcpyAsync(c->roff.p, offsets, 8 * ((size_t)nreads + 1), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->packed.p, 0, 4 * (nwords + 16), c->stream));
    HIPCHK(c, hipMemsetAsync(c->status.p, 0, 4, c->stream));
    if (nwords) {
        k_pack_reads<<<nblk(nwords), 256, 0, c->stream>>>(ptr<uint8_t>(raw), total, ptr<uint32_t>(c->packed), nwords,
                                                          ptr<uint32_t>(c->status));
        KCHK(c);
    }
    uint32_t st = 0;
    int rc = read_status(c, &st);
    if (rc) return rc;
    raw.reset();
    rc = status_to_error(c, st);
    if (rc) return rc;
    c->nreads = nreads;
    c->total_bases = total;
    c->names.clear();
    c->host_lens.resize(nreads);
    for (uint32_t r = 0; r < nreads; ++r) c->host_lens[r] = (uint32_t)(offsets[r + 1] - offsets[r]);
    for (Buf* b : {&c->pile, &c->cons_out, &c->cons_offs, &c->cons_stats, &c->rc_aoff, &c->cons_anch, &c->rc_out, &c->rc_offs, &c->rc_stats, &c->rc_anch, &c->rc_jobs})
        release(*b);                                                  // (the pileup belongs to the reads it was sized for)
    c->as.records.clear();                                            // (so do the overlap records)
    changed(c, READS);                                                // (... and everything else but the runs of a trace_batch)
    made(c, READS);
    return 0;
}

}  // extern "C++"

int bella_hip_set_reads(bella_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads) {
    if (!c || !offsets || (nreads && !bases)) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    return set_reads_impl(c, offsets, nreads, [bases](void* pinned, size_t o, size_t n) { Stager::par_memcpy(pinned, bases + o, n); });
}

// ---- FASTQ ingest (fastq.hpp) ---------------------------------------------------------------------------------------------
// The file is mapped and indexed on all cores; the bases go mapping -> pinned buffer -> device one 64 MB chunk at a time, the
// gather of chunk i+1 overlapping the transfer of chunk i.  The concatenated bases never exist on the host.
// One file or several: the reference's -f names a LIST of FASTQ files whose reads are numbered through in list order
// (kmercount.hpp:82-105 GetFiles, main.cpp:339-423).  Every file is mapped and indexed for itself; the base stream of the set is the
// files' streams back to back, and a chunk that spans a file boundary is gathered from both sides.
int bella_hip_load_fastq_list(bella_ctx* c, const char* const* paths, uint32_t nfiles, uint32_t* nreads, uint64_t* nbases) {
    if (!c || (nfiles && !paths)) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    std::vector<FastqIndex> ix(nfiles);
    std::vector<uint64_t> first(nfiles + 1, 0);                 // first[f]: where file f's bases start in the set's base stream
    std::vector<uint64_t> offsets(1, 0);
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t file_bytes = 0, total_reads = 0;
    unsigned threads = 1;
    for (uint32_t f = 0; f < nfiles; ++f) {
        if (!paths[f]) return fail(c, BELLA_ERR_BAD_ARG, "null path");
        if (ix[f].build(paths[f], err)) return fail(c, BELLA_ERR_BAD_ARG, "%s", err.c_str());
        total_reads += ix[f].names.size();
        if (total_reads >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "more than 2^32 reads");
        first[f + 1] = first[f] + ix[f].nbases();
        for (uint32_t r = 0; r < ix[f].nreads(); ++r) offsets.push_back(first[f] + ix[f].offsets[r + 1]);
        file_bytes += (uint64_t)ix[f].file.n;
        threads = std::max(threads, ix[f].threads);
    }
    const auto t1 = std::chrono::steady_clock::now();
    int rc = set_reads_impl(c, offsets.data(), (uint32_t)total_reads, [&](void* pinned, size_t o, size_t n) {
        uint32_t f = (uint32_t)(std::upper_bound(first.begin(), first.end(), (uint64_t)o) - first.begin()) - 1;
        uint8_t* dst = (uint8_t*)pinned;
        while (n) {
            while (f + 1 < nfiles && first[f + 1] <= o) ++f;    // (files without bases)
            const size_t take = (size_t)std::min<uint64_t>(n, first[f + 1] - o);
            ix[f].gather_parallel(dst, o - first[f], take);
            dst += take; o += take; n -= take;
        }
    });
    if (rc) return rc;
    const auto t2 = std::chrono::steady_clock::now();
    c->ingest = {file_bytes, c->total_bases, c->nreads, threads, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                 std::chrono::duration<double, std::milli>(t2 - t1).count()};
    c->names.clear();
    c->names.reserve(total_reads);
    for (uint32_t f = 0; f < nfiles; ++f)
        for (auto& nm : ix[f].names) c->names.push_back(std::move(nm));
    if (nreads) *nreads = c->nreads;
    if (nbases) *nbases = c->total_bases;
    return 0;
}

int bella_hip_load_fastq(bella_ctx* c, const char* path, uint32_t* nreads, uint64_t* nbases) {
    if (!c || !path) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    return bella_hip_load_fastq_list(c, &path, 1, nreads, nbases);
}

int bella_hip_get_ingest_stats(bella_ctx* c, bella_ingest_stats* out) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    *out = c->ingest;
    return 0;
}

int bella_hip_get_read_names(bella_ctx* c, char* buf, uint64_t buflen, uint64_t* offsets, uint64_t* needed) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (!has(c, READS) || c->names.size() != c->nreads) return fail(c, BELLA_ERR_STATE, "the reads were not loaded with bella_hip_load_fastq");
    uint64_t tot = 0;
    for (const auto& n : c->names) tot += n.size() + 1;
    if (needed) *needed = tot;
    if (!buf) return 0;
    if (buflen < tot) return fail(c, BELLA_ERR_BAD_ARG, "name buffer too small: %llu < %llu", (unsigned long long)buflen, (unsigned long long)tot);
    uint64_t o = 0;
    for (size_t r = 0; r < c->names.size(); ++r) {
        if (offsets) offsets[r] = o;
        std::memcpy(buf + o, c->names[r].c_str(), c->names[r].size() + 1);          // NUL-terminated, back to back
        o += c->names[r].size() + 1;
    }
    if (offsets) offsets[c->names.size()] = o;
    return 0;
}

int bella_hip_get_read_lengths(bella_ctx* c, uint32_t* lens) {
    if (!c || !lens) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, READS)) return r;
    std::memcpy(lens, c->host_lens.data(), 4 * (size_t)c->nreads);
    return 0;
}

// The end of an assembly entry point: its times; the temporaries of assemble_rows_device go back where rows were assembled, and the tuple
// buffers where the tuples were the caller's (those of a count stay: bella_hip_get_tuples, the next panel)
static int assembly_done(bella_ctx* c, bool rows, bool host_tuples) {
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[1]));
    c->tm.assemble_ms = ev_ms(c->ev[0], c->ev[1]);
    if (rows) c->tm.rows_ms = ev_ms(c->ev[0], c->ev[6]);
    if (host_tuples) { release(c->t_kmer); release(c->t_read); release(c->t_pos); }
    if (rows) { release(c->Bk_tmp); release(c->Bpos_tmp); release(c->asm_ws); }
    return 0;
}

int bella_hip_set_B(bella_ctx* c, uint16_t kmer_size, uint32_t nkmers, const uint32_t* colptr, const uint32_t* rowids,
                    const uint16_t* values) {
    if (!c || !colptr) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (kmer_size < 1 || kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32] (MAX_KMER_SIZEK, kmercode/common.h:13)");
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, TUPLES); drop(c, PANEL); drop(c, MATRIX);
    if (colptr[0] != 0) return fail(c, BELLA_ERR_BAD_ARG, "colptr[0] must be 0");
    for (uint32_t r = 0; r < c->nreads; ++r) {
        if (colptr[r + 1] < colptr[r]) return fail(c, BELLA_ERR_BAD_ARG, "colptr must be non-decreasing (column %u)", r);
        if (colptr[r + 1] - colptr[r] >= 65536u) return fail(c, BELLA_ERR_READ_TOO_LONG, "column %u has >= 65536 entries", r);
    }
    const uint64_t nnz = colptr[c->nreads];
    if (nnz && (!rowids || !values)) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    ENSURE(c, c->Bptr, 4 * ((size_t)c->nreads + 1));
    ENSURE(c, c->Bk, 4 * nnz);
    ENSURE(c, c->Bpos, 2 * nnz);
    HIPCHK(c, hipMemcpyAsync(c->Bptr.p, colptr, 4 * ((size_t)c->nreads + 1), hipMemcpyHostToDevice, c->stream));
    if (nnz) {
        HIPCHK(c, c->stager.h2d(c->Bk.p, rowids, 4 * nnz, c->stream));
        HIPCHK(c, c->stager.h2d(c->Bpos.p, values, 2 * nnz, c->stream));
    }
    c->nkmers = nkmers;
    c->nnz = nnz;
    c->kmer_size = kmer_size;
    int rc = build_layout(c);
    if (rc) return rc;
    return assembly_done(c, false, false);
}

// tuples of the reads first .. first+nr-1 -> their rows of B (CSR: c->Bptr local offsets, c->Bk, c->Bpos), on device
// t_kmer == nullptr: the tuples are already on the device (bella_hip_count_kmers), `toff` tuples into the buffers
static int assemble_rows_device(bella_ctx* c, uint32_t first, uint32_t nr, uint64_t ntuples, const uint32_t* t_kmer,
                                const uint32_t* t_read, const uint16_t* t_pos, uint64_t* nnz_out, uint64_t toff = 0) {
    release_count_scratch(c);
    if (t_kmer || !ntuples) {
        ENSURE(c, c->t_kmer, 4 * ntuples);
        ENSURE(c, c->t_read, 4 * ntuples);
        ENSURE(c, c->t_pos, 2 * ntuples);
    }
    ENSURE(c, c->tstart, 8 * ((size_t)nr + 2));
    ENSURE(c, c->Bk_tmp, 4 * ntuples);
    ENSURE(c, c->Bpos_tmp, 2 * ntuples);
    ENSURE(c, c->rowcnt, 4 * ((size_t)nr + 2));
    ENSURE(c, c->Bptr, 4 * ((size_t)nr + 2));
    const uint64_t ws_stride = ((uint64_t)8 * (asm_dedup_slots(65536) + 1) + (uint64_t)6 * 65536 + 255) & ~(uint64_t)255;
    ENSURE(c, c->asm_cls, 4 * ((size_t)kAsmClasses * (nr + 1) + 16));
    if (ntuples && t_kmer) {                          // nullptr: the tuples are already there (bella_hip_count_kmers)
        HIPCHK(c, c->stager.h2d(c->t_kmer.p, t_kmer, 4 * ntuples, c->stream));
        HIPCHK(c, c->stager.h2d(c->t_read.p, t_read, 4 * ntuples, c->stream));
        HIPCHK(c, c->stager.h2d(c->t_pos.p, t_pos, 2 * ntuples, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    HIPCHK(c, hipMemsetAsync(c->status.p, 0, 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rowcnt.p, 0, 4 * ((size_t)nr + 2), c->stream));
    uint32_t* const cls_lists = ptr<uint32_t>(c->asm_cls);
    uint32_t* const cls_counts = cls_lists + (size_t)kAsmClasses * (nr + 1);
    HIPCHK(c, hipMemsetAsync(cls_counts, 0, 4 * 8, c->stream));
    k_tuple_bounds<<<nblk(ntuples + 1), 256, 0, c->stream>>>(ptr<uint32_t>(c->t_read) + toff, ntuples, first, nr, ptr<uint64_t>(c->tstart),
                                                             ptr<uint32_t>(c->status));
    KCHK(c);
    if (nr) {
        k_asm_classify<<<nblk(nr), 256, 0, c->stream>>>(ptr<uint64_t>(c->tstart), nr, cls_lists, cls_counts, ptr<uint32_t>(c->rowcnt), ptr<uint32_t>(c->status));
        KCHK(c);
    }
    uint32_t st = 0;
    uint32_t ccount[8] = {};
    HIPCHK(c, hipMemcpyAsync(ccount, cls_counts, sizeof(ccount), hipMemcpyDeviceToHost, c->stream));
    int rc = read_status(c, &st);
    if (rc) return rc;
    rc = status_to_error(c, st);
    if (rc) return rc;
    for (uint32_t q = 0; q < kAsmClasses; ++q) c->asm_class_count[q] = ccount[q];
    AsmArgs a;
    a.t_kmer = ptr<uint32_t>(c->t_kmer) + toff;
    a.t_pos = ptr<uint16_t>(c->t_pos) + toff;
    a.tstart = ptr<uint64_t>(c->tstart);
    a.nreads = nr;
    a.Bk_tmp = ptr<uint32_t>(c->Bk_tmp);
    a.Bpos_tmp = ptr<uint16_t>(c->Bpos_tmp);
    a.rowcnt = ptr<uint32_t>(c->rowcnt);
    a.ws_stride = ws_stride;
    a.status = ptr<uint32_t>(c->status);
#ifdef BELLA_ASM_CLOCK
    static unsigned long long* d_aclk = nullptr;
    if (!d_aclk) (void)hipMalloc(&d_aclk, 64 * 8);
    (void)hipMemsetAsync(d_aclk, 0, 64 * 8, c->stream);
    a.clk = d_aclk;
#endif
    {
        // one launch per LDS class (table sizes <= 1024, 2048, 4096, 8192 slots: 256, 512, 1024, 1024 threads), then the global tables
        struct Cls { uint32_t hi; int blk; void (*kern)(AsmArgs); };
        const Cls cls[4] = {{1024u, 256, k_asm_rows_lds<256>}, {2048u, 512, k_asm_rows_lds<512>}, {4096u, 1024, k_asm_rows_lds<1024>},
                            {8192u, 1024, k_asm_rows_lds<1024>}};
        for (int q = 0; q < 4; ++q) {
            if (!ccount[q]) continue;
            HIPCHK(c, hipFuncSetAttribute((const void*)cls[q].kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)asm_lds_bytes(kAsmLdsSlots)));
            a.list = cls_lists + (size_t)q * nr; a.nlist = ccount[q];
#ifdef BELLA_ASM_CLOCK
            a.clk = d_aclk + 8 * q;
#endif
            cls[q].kern<<<ccount[q], cls[q].blk, asm_lds_bytes(cls[q].hi), c->stream>>>(a);
            KCHK(c);
        }
        if (ccount[4]) {
            ENSURE(c, c->asm_ws, ws_stride * kAsmGrid);
            a.ws = ptr<uint8_t>(c->asm_ws);
            a.list = cls_lists + (size_t)4 * nr; a.nlist = ccount[4];
            k_asm_rows_global<<<ccount[4] < kAsmGrid ? ccount[4] : kAsmGrid, 1024, 0, c->stream>>>(a);
            KCHK(c);
        }
    }
#ifdef BELLA_ASM_CLOCK
    {
        unsigned long long hh[64];
        (void)hipMemcpyAsync(hh, d_aclk, 64 * 8, hipMemcpyDeviceToHost, c->stream);
        (void)hipStreamSynchronize(c->stream);
        for (int q = 0; q < 4; ++q) {
            const unsigned long long* h = hh + 8 * q;
            unsigned long long tot = 0;
            for (int i = 0; i < 6; ++i) tot += h[i];
            if (!tot) continue;
            std::fprintf(stderr, "[asm clock] class %d reads %u:", q, ccount[q]);
            const char* nm[6] = {"head+init", "insert", "dup", "rounds", "scan", "emit"};
            for (int i = 0; i < 6; ++i) std::fprintf(stderr, " %s %.1f%%", nm[i], 100.0 * (double)h[i] / (double)tot);
            std::fprintf(stderr, " | cycles per read %.0f\n", (double)tot / ccount[q]);
        }
    }
#endif
    rc = scan_u32(c, ptr<uint32_t>(c->rowcnt), ptr<uint32_t>(c->Bptr), (uint64_t)nr + 1);
    if (rc) return rc;
    uint32_t nnz32 = 0;
    HIPCHK(c, hipMemcpyAsync(&nnz32, ptr<uint32_t>(c->Bptr) + nr, 4, hipMemcpyDeviceToHost, c->stream));
    rc = read_status(c, &st);
    if (rc) return rc;
    rc = status_to_error(c, st);
    if (rc) return rc;
    const uint64_t nnz = nnz32;
    ENSURE(c, c->Bk, 4 * nnz);
    ENSURE(c, c->Bpos, 2 * nnz);
    if (nr) {
        k_compact_B<<<nblk(nr, kWaves), kBlock, 0, c->stream>>>(ptr<uint64_t>(c->tstart), ptr<uint32_t>(c->Bptr), nr,
                                                                ptr<uint32_t>(c->Bk_tmp), ptr<uint16_t>(c->Bpos_tmp),
                                                                ptr<uint32_t>(c->Bk), ptr<uint16_t>(c->Bpos));
        KCHK(c);
    }
    HIPCHK(c, hipEventRecord(c->ev[6], c->stream));            // rows_ms = ev[0] .. ev[6]
    *nnz_out = nnz;
    return 0;
}

int bella_hip_assemble_tuples(bella_ctx* c, uint16_t kmer_size, uint32_t nkmers, uint64_t ntuples, const uint32_t* t_kmer,
                              const uint32_t* t_read, const uint16_t* t_pos) {
    if (!c || (ntuples && (!t_kmer || !t_read || !t_pos))) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (kmer_size < 1 || kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    if (ntuples >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "tuple count must be < 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, TUPLES); drop(c, PANEL); drop(c, MATRIX);
    uint64_t nnz = 0;
    int rc = assemble_rows_device(c, 0, c->nreads, ntuples, t_kmer, t_read, t_pos, &nnz);
    if (rc) return rc;
    c->nkmers = nkmers;
    c->nnz = nnz;
    c->kmer_size = kmer_size;
    rc = build_layout(c);
    if (rc) return rc;
    return assembly_done(c, true, true);
}

// ---- k-mer counting, dictionary, tuples (kcount.hpp) ----------------------------------------------------------------------
static int grow_keep(bella_ctx* c, Buf& b, size_t need, size_t used) {
    if (b.cap >= need) return 0;
    TmpBuf nb;
    ENSURE(c, nb, need + need / 4);
    if (used) HIPCHK(c, hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    nb.give_to(b);
    return 0;
}

// dist: collective over the context's communicator -- rank r counts the canonical words of ITS range of histogram bins over all
// reads (1/N of the sort), the partial dictionaries (ascending, so their concatenation in rank order is the whole ascending
// dictionary) are exchanged with one grouped send/recv, and tuples are generated for the reads bfirst .. bfirst + brows - 1 only
static int comm_agree(bella_ctx* c, int local_rc);
static int comm_sync(bella_ctx* c, const char* what);

// what a count asks of the reads and of its arguments (mode: 0 all k-mers, 1 syncmers, 2 minimizers; the read block the tuples are for)
static int count_args(bella_ctx* c, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t mode, uint32_t window, uint32_t bfirst,
                      uint32_t brows) {
    if (int r = need(c, READS)) return r;
    if (kmer_size < 1 || kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    if (lower < 2 || upper < lower || upper > 65535) return fail(c, BELLA_ERR_BAD_ARG, "need 2 <= lower <= upper <= 65535");
    if (mode == 2 && (window < 1 || window > 65535)) return fail(c, BELLA_ERR_BAD_ARG, "minimizer window must be in [1,65535]");
    if (mode == 1 && kmer_size <= kSmerLen) return fail(c, BELLA_ERR_BAD_ARG, "syncmer selection needs k > 5 (smerlen, syncmer.hpp:45)");
    if ((uint64_t)bfirst + brows > c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "read block exceeds the read set");
    return 0;
}

constexpr uint32_t kCountStatsHead = 8;                            // bella_hip_get_count_stats: words before the passes

static int count_kmers_impl(bella_ctx* c, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t mode, uint32_t window,
                            uint32_t* nkmers_out, uint64_t* ntuples_out, uint64_t* ndistinct_out, bool dist = false, uint32_t bfirst = 0,
                            uint32_t brows = 0) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (!dist) {                                                   // the tuples are for all reads (dist: the entry point has made the checks)
        bfirst = 0; brows = c->nreads;
        if (int r = count_args(c, kmer_size, lower, upper, mode, window, bfirst, brows)) return r;
    }
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, TUPLES);
    const uint32_t nr = c->nreads, k = kmer_size;
    static const int dev_marks = getenv("BELLA_DEV_KCMARKS") ? atoi(getenv("BELLA_DEV_KCMARKS")) : 0;   // 1: stage times (synchronising), 2: host time only
    auto tmark0 = std::chrono::steady_clock::now();
    auto mark = [&](const char* what) {
        if (!dev_marks) return;
        if (dev_marks == 1) (void)hipStreamSynchronize(c->stream);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[kc] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - tmark0).count());
        tmark0 = t;
    };
    const int NR = dist ? c->comm_ranks : 1, me = dist ? c->comm_rank : 0;
    if (dist && !c->comm) return fail(c, BELLA_ERR_STATE, "bella_hip_comm_init first");
    // Local phase (histogram, sort passes, partial dictionary): a rank that fails here still takes part in the status exchange below,
    // so that all ranks leave the call together instead of waiting for it in the dictionary exchange.
    const uint8_t* d_sel = nullptr;
    uint64_t nk_total = 0, ndistinct = 0, nocc = 0;                // reliable k-mers, distinct k-mers, occurrences of reliable k-mers so far
    uint32_t *occ_pos = nullptr, *occ_id = nullptr, *occ_pos2 = nullptr, *occ_id2 = nullptr;   // the list of occurrences and what it is sorted against
    bool fast = false, one_pass_all = false;
    uint32_t pb = 0, gb = 0;
    uint64_t npos = 0, table_slots = 0;                            // positions of the read set; slots of the look-up table (0: none built)
    std::vector<uint64_t> pass_stats;                              // per pass: first bin, end bin, words, tiles of the run kernels
    int rc = [&]() -> int {
    const unsigned rgrid = nr < 16384u ? (nr ? nr : 1u) : 16384u;
    ENSURE(c, c->kc_nk, 4 * ((size_t)nr + 2));
    ENSURE(c, c->kc_koff, 8 * ((size_t)nr + 2));
    ENSURE(c, c->kc_hist, 8 * kCountBins);
    ENSURE(c, c->kc_found, 4 * ((size_t)nr + 2));
    ENSURE(c, c->kc_tstart, 8 * ((size_t)nr + 2));
    ENSURE(c, c->kc_nruns, 16);
    ENSURE(c, c->kc_cursor, 16);
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    k_kmers_per_read<<<nblk((uint64_t)nr + 1), 256, 0, c->stream>>>(ptr<uint64_t>(c->roff), nr, k, ptr<uint32_t>(c->kc_nk));
    KCHK(c);
    int rc = scan_u32_to_u64(c, ptr<uint32_t>(c->kc_nk), ptr<uint64_t>(c->kc_koff), (uint64_t)nr + 1);
    if (rc) return rc;
    // ntot = koff[nr] is needed before the histogram in minimizer mode (the selection flags are per position)
    uint64_t ntot = 0;
    HIPCHK(c, hipMemcpyAsync(&ntot, ptr<uint64_t>(c->kc_koff) + nr, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (mode == 2) {
        const uint32_t cap = window + 2;
        ENSURE(c, c->kc_sel, ntot + 16);
        ENSURE(c, c->kc_ringo, 8 * (size_t)cap * (nr ? nr : 1));
        ENSURE(c, c->kc_ringp, 4 * (size_t)cap * (nr ? nr : 1));
        HIPCHK(c, hipMemsetAsync(c->kc_sel.p, 0, ntot + 16, c->stream));
        k_minimizer_select<<<nblk(nr ? nr : 1, 64), 64, 0, c->stream>>>(ptr<uint32_t>(c->packed), ptr<uint64_t>(c->roff), ptr<uint32_t>(c->kc_nk),
                                                                    ptr<uint64_t>(c->kc_koff), nr, k, window, cap, ptr<uint64_t>(c->kc_ringo),
                                                                    ptr<uint32_t>(c->kc_ringp), ptr<uint8_t>(c->kc_sel));
        KCHK(c);
        d_sel = ptr<uint8_t>(c->kc_sel);
        release(c->kc_ringo); release(c->kc_ringp);
    }
    // Words with their positions (kcount.hpp): when the word's 2k bits and a global position index fit 64 bits together -- and the
    // positions that make tuples are the positions that are counted (not so in syncmer mode) -- every sorted word still knows where it
    // came from and the reliable ones leave (position, id) on a list that one more sort turns into the tuples: no hash table over the
    // dictionary, no look-up per position (which was a third of this call).  Not across ranks (a rank only sorts its share of the words).
    {
        int posbits = 1;
        while (posbits < 63 && (1ull << posbits) < ntot) ++posbits;
        fast = NR == 1 && mode != 1 && 2 * (int)k + posbits <= 64 && posbits <= 32 && !(c->debug & 16384u);   // debug bit 14: tests, the look-up path
        pb = fast ? (uint32_t)posbits : 0u;
        npos = ntot;
    }
    uint64_t budget = c->kcount_budget;
    if (budget > 0x7FFF0000ull) budget = 0x7FFF0000ull;               // rocPRIM item counts are 32-bit
    uint64_t hist[kCountBins] = {};
    if (mode == 0 && NR == 1 && ntot <= budget) {
        hist[0] = ntot;                                                // one pass over every position: no histogram needed to size it
        one_pass_all = true;
    } else {
    HIPCHK(c, hipMemsetAsync(c->kc_hist.p, 0, 8 * kCountBins, c->stream));
    k_code_hist<<<rgrid, kBlock, 0, c->stream>>>(ptr<uint32_t>(c->packed), ptr<uint64_t>(c->roff), ptr<uint32_t>(c->kc_nk), nr, k, mode,
                                                 ptr<uint64_t>(c->kc_koff), d_sel, (unsigned long long*)c->kc_hist.p);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(hist, c->kc_hist.p, sizeof(hist), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    // passes = runs of consecutive bins holding at most `budget` k-mers (28 bytes of HBM per k-mer in flight)
    // this rank's bins: consecutive, balanced by their word counts (every rank derives the same split from the same histogram)
    uint32_t bin_lo = 0, bin_hi = kCountBins;
    if (NR > 1) {
        uint64_t tot = 0;
        for (uint32_t b = 0; b < kCountBins; ++b) tot += hist[b];
        auto cut = [&](int r) -> uint32_t {                       // first bin of rank r
            if (r <= 0) return 0u;
            if (r >= NR) return kCountBins;
            const uint64_t want = tot / (uint64_t)NR * (uint64_t)r;
            uint64_t acc = 0;
            uint32_t b = 0;
            while (b < kCountBins && acc + hist[b] / 2 < want) acc += hist[b++];
            return b;
        };
        bin_lo = cut(me);
        bin_hi = cut(me + 1);
    }
    std::vector<uint32_t> pass_lo, pass_hi;
    std::vector<uint64_t> pass_n;
    if (one_pass_all) { pass_lo.push_back(0); pass_hi.push_back(kCountBins); pass_n.push_back(ntot); }
    else
    for (uint32_t b = bin_lo; b < bin_hi;) {
        uint64_t n = hist[b];
        if (n > 0x7FFF0000ull) return fail(c, BELLA_ERR_NOMEM, "k-mer counting: one bin of canonical k-mers holds %llu words", (unsigned long long)n);
        uint32_t e = b + 1;
        while (e < bin_hi && n + hist[e] <= budget) n += hist[e++];
        pass_lo.push_back(b); pass_hi.push_back(e); pass_n.push_back(n);
        b = e;
    }
    const bool single = pass_n.size() == 1 && mode == 0 && NR == 1;    // every position contributes: word j of read r has a fixed place
    // (with the positions in the keys the run kernels handle groups of four neighbouring words: the sort may leave out the word's
    // two lowest bits, and does when that saves it a pass of eight bits -- 32 instead of 34 bits for k = 17)
    gb = fast && 2 * k >= 10 && (2 * k + 7) / 8 > (2 * k - 2 + 7) / 8 ? 2u : 0u;
    for (size_t p = 0; p < pass_n.size(); ++p) {
        const uint64_t np = pass_n[p];
        const uint64_t st[4] = {pass_lo[p], pass_hi[p], np, fast && np ? (uint64_t)nblk(np, kRunTile) : 0ull};
        pass_stats.insert(pass_stats.end(), st, st + 4);
        if (!np) continue;
        ENSURE(c, c->kc_keys, 8 * np);
        ENSURE(c, c->kc_alt, 8 * np);
        ENSURE(c, c->kc_runlen, 4 * (np + 64));                    // (fast path: per-tile arrays, two of ntile + 8 words each -- np / 2048 tiles)
        ENSURE(c, c->kc_flag, 4 * (np + 64));
        ENSURE(c, c->kc_slot, 4 * (np + 64));
        if (!single) HIPCHK(c, hipMemsetAsync(c->kc_cursor.p, 0, 8, c->stream));
        k_emit_codes<<<rgrid, kBlock, 0, c->stream>>>(ptr<uint32_t>(c->packed), ptr<uint64_t>(c->roff), ptr<uint32_t>(c->kc_nk),
                                                      ptr<uint64_t>(c->kc_koff), nr, k, mode, pass_lo[p], pass_hi[p], d_sel, ptr<uint64_t>(c->kc_keys),
                                                      single ? nullptr : (unsigned long long*)c->kc_cursor.p, pb);
        KCHK(c);
        mark("alloc + emit codes");
        hipcub::DoubleBuffer<uint64_t> db(ptr<uint64_t>(c->kc_keys), ptr<uint64_t>(c->kc_alt));
        // At the limit of the positions-in-the-keys path the word ends in bit 63.  For up to merge_sort_limit items rocPRIM sorts by
        // merging under a comparator that masks the bit range, and builds the mask's upper end as (1 << end_bit) - 1: a shift by the
        // key's width when end_bit is 64, which leaves the mask of the bits BELOW begin_bit -- the keys came back ordered by their
        // position fields (k = 25 with 16,384 positions: 3 of 40 reliable k-mers found).  Such a pass sorts on all 64 bits: the plain
        // comparator.  Words still stand group by group (inside a group now by low bits, then position: the run kernels count per low
        // bits in any interleaving), and a pass of that size costs the same either way.  Larger passes take the radix path.
        const int end_bit = (int)pb + 2 * (int)k;
        const bool whole_key = end_bit == 64 && pb + gb > 0 && np <= ::rocprim::radix_sort_config<>::merge_sort_limit;
        CUB(c, hipcub::DeviceRadixSort::SortKeys, db, (int)np, whole_key ? 0 : (int)(pb + gb), end_bit, c->stream);
        uint64_t* sorted = db.Current();
        mark("sort");
        if (fast) {
            // runs of equal words, tile by tile: reliable runs per tile -> scan over the tiles = the ids of this pass -> every reliable
            // word's id to its position, the dictionary entries from the runs' first words (kcount.hpp)
            const unsigned ntile = nblk(np, kRunTile);
            uint32_t* tile_rel = ptr<uint32_t>(c->kc_runlen);       // (ntile + 1 each; 4 (np + 64) bytes are there)
            uint32_t* tile_words = tile_rel + ntile + 8;
            uint32_t* tile_heads = ptr<uint32_t>(c->kc_flag);
            uint32_t* tile_base = ptr<uint32_t>(c->kc_slot);
            uint32_t* tile_wbase = tile_base + ntile + 8;
            HIPCHK(c, hipMemsetAsync(tile_rel + ntile, 0, 4, c->stream));
            HIPCHK(c, hipMemsetAsync(tile_words + ntile, 0, 4, c->stream));
            k_run_count<<<ntile, kRunBlock, 0, c->stream>>>(sorted, np, pb, gb, lower, upper, mode != 0, tile_rel, tile_heads, tile_words);
            KCHK(c);
            rc = scan_u32(c, tile_rel, tile_base, (uint64_t)ntile + 1);
            if (rc) return rc;
            rc = scan_u32(c, tile_words, tile_wbase, (uint64_t)ntile + 1);
            if (rc) return rc;
            {
                hipcub::TransformInputIterator<uint64_t, CastU64, const uint32_t*> hit(tile_heads, CastU64());
                CUB(c, hipcub::DeviceReduce::Sum, hit, ptr<uint64_t>(c->kc_cursor), (int)ntile, c->stream);
            }
            uint32_t nrel = 0, nwords = 0;
            uint64_t nruns = 0;
            HIPCHK(c, hipMemcpyAsync(&nrel, tile_base + ntile, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&nwords, tile_wbase + ntile, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(&nruns, c->kc_cursor.p, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            mark("run count + scans");
            if (nk_total + nrel >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "more than 2^32 reliable k-mers");
            if (nocc + nwords >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "tuple count must be < 2^32");
            rc = grow_keep(c, c->kc_dcode, 8 * (nk_total + nrel), 8 * nk_total);
            if (rc) return rc;
            rc = grow_keep(c, c->kc_dcount, 2 * (nk_total + nrel), 2 * nk_total);
            if (rc) return rc;
            // the list of occurrences: with one pass (the usual case) it goes into the sort's free buffer (8 np bytes: positions, then
            // ids) and is later sorted against the buffer of the sorted words, which nobody reads after this kernel -- no allocation;
            // with several passes it grows in buffers of its own
            uint32_t *op = nullptr, *oi = nullptr;
            if (pass_n.size() == 1) {
                uint64_t* freebuf = sorted == ptr<uint64_t>(c->kc_keys) ? ptr<uint64_t>(c->kc_alt) : ptr<uint64_t>(c->kc_keys);
                op = (uint32_t*)freebuf; oi = op + np;
                occ_pos = op; occ_id = oi; occ_pos2 = (uint32_t*)sorted; occ_id2 = occ_pos2 + np;
            } else {
                rc = grow_keep(c, c->kc_opos, 4 * (nocc + nwords) + 16, 4 * nocc);
                if (rc) return rc;
                rc = grow_keep(c, c->kc_oid, 4 * (nocc + nwords) + 16, 4 * nocc);
                if (rc) return rc;
                op = ptr<uint32_t>(c->kc_opos) + nocc; oi = ptr<uint32_t>(c->kc_oid) + nocc;
                occ_pos = ptr<uint32_t>(c->kc_opos); occ_id = ptr<uint32_t>(c->kc_oid); occ_pos2 = nullptr; occ_id2 = nullptr;
            }
            mark("grow dict + list");
            k_run_assign<<<ntile, kRunBlock, 0, c->stream>>>(sorted, np, pb, gb, lower, upper, mode != 0, tile_base, tile_wbase, (uint32_t)nk_total, op, oi,
                                                             ptr<uint64_t>(c->kc_dcode) + nk_total, ptr<uint16_t>(c->kc_dcount) + nk_total);
            KCHK(c);
            mark("run assign");
            nocc += nwords;
            nk_total += nrel;
            ndistinct += nruns;
            continue;
        }
        uint64_t* run_code = sorted == ptr<uint64_t>(c->kc_keys) ? ptr<uint64_t>(c->kc_alt) : ptr<uint64_t>(c->kc_keys);
        CUB(c, hipcub::DeviceRunLengthEncode::Encode, sorted, run_code, ptr<uint32_t>(c->kc_runlen), ptr<uint32_t>(c->kc_nruns), (int)np, c->stream);
        uint32_t nruns = 0;
        HIPCHK(c, hipMemcpyAsync(&nruns, c->kc_nruns.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        k_flag_reliable<<<nblk((uint64_t)nruns + 1), 256, 0, c->stream>>>(ptr<uint32_t>(c->kc_runlen), nruns, lower, upper, mode != 0, ptr<uint32_t>(c->kc_flag));
        KCHK(c);
        rc = scan_u32(c, ptr<uint32_t>(c->kc_flag), ptr<uint32_t>(c->kc_slot), (uint64_t)nruns + 1);
        if (rc) return rc;
        uint32_t nrel = 0;
        HIPCHK(c, hipMemcpyAsync(&nrel, ptr<uint32_t>(c->kc_slot) + nruns, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nk_total + nrel >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "more than 2^32 reliable k-mers");
        rc = grow_keep(c, c->kc_dcode, 8 * (nk_total + nrel), 8 * nk_total);
        if (rc) return rc;
        rc = grow_keep(c, c->kc_dcount, 2 * (nk_total + nrel), 2 * nk_total);
        if (rc) return rc;
        if (nruns) {
            k_write_dict<<<nblk(nruns), 256, 0, c->stream>>>(run_code, ptr<uint32_t>(c->kc_runlen), ptr<uint32_t>(c->kc_flag), ptr<uint32_t>(c->kc_slot),
                                                             nruns, mode != 0, ptr<uint64_t>(c->kc_dcode) + nk_total, ptr<uint16_t>(c->kc_dcount) + nk_total);
            KCHK(c);
        }
        nk_total += nrel;
        ndistinct += nruns;
    }
    return 0;
    }();
    if (NR > 1) rc = comm_agree(c, rc);
    if (rc) return rc;
    mark("passes");
    if (NR > 1) {
        // partial dictionaries -> the whole dictionary on every rank
        ENSURE(c, c->comm_meta, 8 * 4 * ((size_t)NR + 1));
        uint64_t mine[4] = {nk_total, ndistinct, 0, 0};
        uint64_t* d_meta = ptr<uint64_t>(c->comm_meta);
        HIPCHK(c, hipMemcpyAsync(d_meta + 4 * (size_t)NR, mine, sizeof(mine), hipMemcpyHostToDevice, c->stream));
        NCCLCHK(c, c->api->AllGather(d_meta + 4 * (size_t)NR, d_meta, 4, ncclUint64, c->comm, c->stream));
        std::vector<uint64_t> meta(4 * (size_t)NR);
        HIPCHK(c, hipMemcpyAsync(meta.data(), d_meta, 8 * 4 * (size_t)NR, hipMemcpyDeviceToHost, c->stream));
        { const int sr = comm_sync(c, "dictionary sizes"); if (sr) return sr; }
        std::vector<uint64_t> off((size_t)NR + 1, 0);
        uint64_t nd_all = 0;
        for (int r = 0; r < NR; ++r) { off[r + 1] = off[r] + meta[4 * r]; nd_all += meta[4 * r + 1]; }
        TmpBuf ncode, ncount;
        int r2 = off[NR] >= 0xFFFFFFF0ull ? fail(c, BELLA_ERR_BAD_ARG, "more than 2^32 reliable k-mers") : 0;
        if (!r2) r2 = ensure_bytes(c, ncode, 8 * off[NR]);
        if (!r2) r2 = ensure_bytes(c, ncount, 2 * off[NR] + 16);
        r2 = comm_agree(c, r2);                                    // all ranks hold their receive buffers, or all leave
        if (r2) return r2;
        hipError_t he = hipSuccess;
        if (nk_total) {
            he = hipMemcpyAsync(ptr<uint64_t>(ncode) + off[me], c->kc_dcode.p, 8 * nk_total, hipMemcpyDeviceToDevice, c->stream);
            if (he == hipSuccess) he = hipMemcpyAsync(ptr<uint8_t>(ncount) + 2 * off[me], c->kc_dcount.p, 2 * nk_total, hipMemcpyDeviceToDevice, c->stream);
        }
        ncclResult_t nr2 = c->api->GroupStart();
        for (int p2 = 0; p2 < NR && nr2 == ncclSuccess; ++p2) {
            if (p2 == me) continue;
            const uint64_t pn = meta[4 * p2];
            if (nk_total) {
                nr2 = c->api->Send(c->kc_dcode.p, nk_total, ncclUint64, p2, c->comm, c->stream);
                if (nr2 == ncclSuccess) nr2 = c->api->Send(c->kc_dcount.p, 2 * nk_total, ncclUint8, p2, c->comm, c->stream);
            }
            if (pn && nr2 == ncclSuccess) {
                nr2 = c->api->Recv(ptr<uint64_t>(ncode) + off[p2], pn, ncclUint64, p2, c->comm, c->stream);
                if (nr2 == ncclSuccess) nr2 = c->api->Recv(ptr<uint8_t>(ncount) + 2 * off[p2], 2 * pn, ncclUint8, p2, c->comm, c->stream);
            }
        }
        {   // the group is closed on every path
            const ncclResult_t ge = c->api->GroupEnd();
            if (nr2 == ncclSuccess) nr2 = ge;
        }
        if (he == hipSuccess && nr2 == ncclSuccess) { const int sr = comm_sync(c, "dictionary exchange"); if (sr) return sr; }
        if (nr2 != ncclSuccess || he != hipSuccess)
            return fail(c, BELLA_ERR_HIP, "dictionary exchange failed: %s", nr2 != ncclSuccess ? (c->api->GetErrorString ? c->api->GetErrorString(nr2) : "RCCL error") : hipGetErrorString(he));
        ncode.give_to(c->kc_dcode); ncount.give_to(c->kc_dcount);
        nk_total = off[NR];
        ndistinct = nd_all;
    }
    uint32_t* ids_rel = nullptr;
    const unsigned bgrid = brows < 16384u ? (brows ? brows : 1u) : 16384u;
    uint64_t nt = 0;
    if (fast) {
        // the list of occurrences, sorted by position = the tuples in the reference's order (main.cpp:393-416); where each read's begin
        const uint32_t* spos = occ_pos;
        const uint32_t* sid = occ_id;
        if (nocc) {
            if (!occ_pos2) {
                ENSURE(c, c->kc_opos2, 4 * nocc + 16);
                ENSURE(c, c->kc_oid2, 4 * nocc + 16);
                occ_pos2 = ptr<uint32_t>(c->kc_opos2); occ_id2 = ptr<uint32_t>(c->kc_oid2);
            }
            hipcub::DoubleBuffer<uint32_t> dk(occ_pos, occ_pos2);
            hipcub::DoubleBuffer<uint32_t> dv(occ_id, occ_id2);
            CUB(c, hipcub::DeviceRadixSort::SortPairs, dk, dv, (uint64_t)nocc, 0, (int)pb, c->stream);
            spos = dk.Current();
            sid = dv.Current();
            mark("sort occurrences");
        }
        uint32_t* first = ptr<uint32_t>(c->kc_found);              // (nr + 2 words)
        k_occ_bounds<<<nblk((uint64_t)brows + 1), 256, 0, c->stream>>>(spos, nocc, ptr<uint64_t>(c->kc_koff) + bfirst, brows, first, ptr<uint64_t>(c->kc_tstart));
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(&nt, ptr<uint64_t>(c->kc_tstart) + brows, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ENSURE(c, c->t_kmer, 4 * nt);
        ENSURE(c, c->t_read, 4 * nt);
        ENSURE(c, c->t_pos, 2 * nt);
        if (brows && nt) {
            k_write_tuples_sorted<<<bgrid, kBlock, 0, c->stream>>>(spos, sid, ptr<uint64_t>(c->kc_koff) + bfirst, first, brows, bfirst, ptr<uint32_t>(c->t_kmer),
                                                                   ptr<uint32_t>(c->t_read), ptr<uint16_t>(c->t_pos));
            KCHK(c);
        }
    } else {
    // countsreliable: open addressing at load factor <= 1/2
    uint64_t slots = 1024;
    while (slots < 2 * nk_total) slots <<= 1;
    table_slots = slots;
    ENSURE(c, c->kc_hkey, 8 * slots);
    ENSURE(c, c->kc_hval, 4 * slots);
    k_hash_fill<<<nblk(slots), 256, 0, c->stream>>>(ptr<uint64_t>(c->kc_hkey), slots);
    KCHK(c);
    if (nk_total) {
        k_hash_build<<<nblk(nk_total), 256, 0, c->stream>>>(ptr<uint64_t>(c->kc_dcode), (uint32_t)nk_total, ptr<uint64_t>(c->kc_hkey),
                                                            ptr<uint32_t>(c->kc_hval), slots - 1);
        KCHK(c);
    }
    // ids of every position and tuples (main.cpp:393-416) of the reads bfirst .. bfirst + brows - 1 (all reads unless distributed)
    uint64_t kb[2] = {0, 0};                                          // koff[bfirst], koff[bfirst + brows]
    HIPCHK(c, hipMemcpyAsync(&kb[0], ptr<uint64_t>(c->kc_koff) + bfirst, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&kb[1], ptr<uint64_t>(c->kc_koff) + bfirst + brows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nblockpos = kb[1] - kb[0];
    ENSURE(c, c->kc_keys, 4 * nblockpos);
    ids_rel = ptr<uint32_t>(c->kc_keys) - kb[0];                      // the kernels index ids with the absolute position koff[r] + j
    const uint8_t* sel_rel = d_sel;
    k_lookup_ids<<<bgrid, kBlock, 0, c->stream>>>(ptr<uint32_t>(c->packed), ptr<uint64_t>(c->roff) + bfirst, ptr<uint32_t>(c->kc_nk) + bfirst,
                                                  ptr<uint64_t>(c->kc_koff) + bfirst, brows, k, ptr<uint64_t>(c->kc_hkey), ptr<uint32_t>(c->kc_hval),
                                                  slots - 1, sel_rel, ids_rel, ptr<uint32_t>(c->kc_found));
    KCHK(c);
    HIPCHK(c, hipMemsetAsync(ptr<uint32_t>(c->kc_found) + brows, 0, 4, c->stream));
    rc = scan_u32_to_u64(c, ptr<uint32_t>(c->kc_found), ptr<uint64_t>(c->kc_tstart), (uint64_t)brows + 1);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(&nt, ptr<uint64_t>(c->kc_tstart) + brows, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nt >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "tuple count must be < 2^32");
    ENSURE(c, c->t_kmer, 4 * nt);
    ENSURE(c, c->t_read, 4 * nt);
    ENSURE(c, c->t_pos, 2 * nt);
    k_write_tuples<<<bgrid, kBlock, 0, c->stream>>>(ids_rel, ptr<uint32_t>(c->kc_nk) + bfirst, ptr<uint64_t>(c->kc_koff) + bfirst,
                                                    ptr<uint64_t>(c->kc_tstart), brows, bfirst, ptr<uint32_t>(c->t_kmer), ptr<uint32_t>(c->t_read),
                                                    ptr<uint16_t>(c->t_pos));
    KCHK(c);
    }
    mark("tuples");
    HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[1]));
    c->tm.kcount_ms = ev_ms(c->ev[0], c->ev[1]);
    release(c->kc_hkey); release(c->kc_hval); release(c->kc_sel);
    release(c->kc_opos); release(c->kc_oid); release(c->kc_opos2); release(c->kc_oid2);
    c->kc_ntuples = nt;
    c->kc_nkmers = (uint32_t)nk_total;
    c->kc_k = k;
    c->kc_bfirst = bfirst;
    c->kc_brows = brows;
    {
        const uint64_t head[kCountStatsHead] = {fast ? 1ull : 0ull, pb, gb, pass_stats.size() / 4, table_slots, mode, npos, c->kcount_budget};
        c->kc_stats.assign(head, head + kCountStatsHead);
        c->kc_stats.insert(c->kc_stats.end(), pass_stats.begin(), pass_stats.end());
    }
    made(c, TUPLES);
    if (nkmers_out) *nkmers_out = (uint32_t)nk_total;
    if (ntuples_out) *ntuples_out = nt;
    if (ndistinct_out) *ndistinct_out = ndistinct;
    return 0;
}

int bella_hip_count_kmers(bella_ctx* c, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t* nkmers, uint64_t* ntuples,
                          uint64_t* ndistinct) {
    return count_kmers_impl(c, kmer_size, lower, upper, 0, 0, nkmers, ntuples, ndistinct);
}

int bella_hip_count_kmers_dist(bella_ctx* c, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t selector, uint32_t window,
                               uint32_t first_read, uint32_t nreads_block, uint32_t* nkmers, uint64_t* ntuples, uint64_t* ndistinct) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (!c->comm) return fail(c, BELLA_ERR_STATE, "bella_hip_comm_init first");
    // argument and state errors are local: the rank still takes part in a status exchange, so that its peers leave the call with it
    // instead of waiting for it in the dictionary exchange
    int rc = 0;
    if (selector > 2) rc = fail(c, BELLA_ERR_BAD_ARG, "selector: 0 = all k-mers, 1 = syncmers, 2 = minimizers");
    else rc = count_args(c, kmer_size, lower, upper, selector, window, first_read, nreads_block);
    if (hipSetDevice(c->device) != hipSuccess && !rc) rc = fail(c, BELLA_ERR_HIP, "hipSetDevice failed");
    const std::string local_err = c->err;
    rc = comm_agree(c, rc);
    if (rc) { if (!local_err.empty()) c->err = local_err; return rc; }
    return count_kmers_impl(c, kmer_size, lower, upper, selector, window, nkmers, ntuples, ndistinct, true, first_read, nreads_block);
}

int bella_hip_count_syncmers(bella_ctx* c, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t* nkmers, uint64_t* ntuples,
                             uint64_t* ndistinct) {
    return count_kmers_impl(c, kmer_size, lower, upper, 1, 0, nkmers, ntuples, ndistinct);
}

int bella_hip_count_minimizers(bella_ctx* c, uint16_t kmer_size, uint32_t window, uint32_t lower, uint32_t upper, uint32_t* nkmers,
                               uint64_t* ntuples, uint64_t* ndistinct) {
    return count_kmers_impl(c, kmer_size, lower, upper, 2, window, nkmers, ntuples, ndistinct);
}

int bella_hip_get_dictionary(bella_ctx* c, uint64_t* codes, uint16_t* counts) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TUPLES)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (codes && c->kc_nkmers) HIPCHK(c, hipMemcpyAsync(codes, c->kc_dcode.p, 8 * (size_t)c->kc_nkmers, hipMemcpyDeviceToHost, c->stream));
    if (counts && c->kc_nkmers) HIPCHK(c, hipMemcpyAsync(counts, c->kc_dcount.p, 2 * (size_t)c->kc_nkmers, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bella_hip_get_count_stats(bella_ctx* c, uint64_t* values, uint32_t capacity, uint32_t* nvalues) {
    if (!c || !nvalues || (capacity && !values)) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TUPLES)) return r;
    const size_t n = c->kc_stats.size();
    for (size_t i = 0; i < n && i < capacity; ++i) values[i] = c->kc_stats[i];
    *nvalues = (uint32_t)n;
    return 0;
}

int bella_hip_get_assemble_stats(bella_ctx* c, uint64_t* values, uint32_t capacity, uint32_t* nvalues) {
    if (!c || !nvalues || (capacity && !values)) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, MATRIX)) return r;
    uint64_t v[kAsmClasses + 4];
    for (uint32_t q = 0; q < kAsmClasses; ++q) v[q] = c->asm_class_count[q];
    v[kAsmClasses] = c->layout_inline;
    v[kAsmClasses + 1] = c->layout_products ? 1u : 0u;
    v[kAsmClasses + 2] = c->layout_first_app ? 1u : 0u;
    v[kAsmClasses + 3] = c->layout_place_sorted ? 1u : 0u;
    const uint32_t n = kAsmClasses + 4;
    for (uint32_t i = 0; i < n && i < capacity; ++i) values[i] = v[i];
    *nvalues = n;
    return 0;
}

int bella_hip_get_tuples(bella_ctx* c, uint32_t* t_kmer, uint32_t* t_read, uint16_t* t_pos) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TUPLES)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = c->kc_ntuples;
    if (t_kmer && n) HIPCHK(c, hipMemcpyAsync(t_kmer, c->t_kmer.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (t_read && n) HIPCHK(c, hipMemcpyAsync(t_read, c->t_read.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (t_pos && n) HIPCHK(c, hipMemcpyAsync(t_pos, c->t_pos.p, 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bella_hip_assemble_counted(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TUPLES)) return r;
    if (c->kc_bfirst != 0 || c->kc_brows != c->nreads) return fail(c, BELLA_ERR_STATE, "the tuples cover a read block only: assemble_counted_panel + allgather_panels");
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, PANEL); drop(c, MATRIX);
    uint64_t nnz = 0;
    int rc = assemble_rows_device(c, 0, c->nreads, c->kc_ntuples, nullptr, nullptr, nullptr, &nnz);
    if (rc) return rc;
    c->nkmers = c->kc_nkmers;
    c->nnz = nnz;
    c->kmer_size = (uint16_t)c->kc_k;
    rc = build_layout(c);
    if (rc) return rc;
    return assembly_done(c, true, false);
}

int bella_hip_assemble_panel(bella_ctx* c, uint16_t kmer_size, uint32_t nkmers, uint32_t first_read, uint32_t nreads_panel,
                             uint64_t ntuples, const uint32_t* t_kmer, const uint32_t* t_read, const uint16_t* t_pos) {
    if (!c || (ntuples && (!t_kmer || !t_read || !t_pos))) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (kmer_size < 1 || kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    if ((uint64_t)first_read + nreads_panel > c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "panel exceeds the read set");
    if (ntuples >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "tuple count must be < 2^32");
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, TUPLES); drop(c, PANEL); drop(c, MATRIX);
    uint64_t nnz = 0;
    int rc = assemble_rows_device(c, first_read, nreads_panel, ntuples, t_kmer, t_read, t_pos, &nnz);
    if (rc) return rc;
    if (int r = assembly_done(c, true, true)) return r;
    c->nkmers = nkmers;
    c->kmer_size = kmer_size;
    c->panel_first = first_read;
    c->panel_rows = nreads_panel;
    c->panel_nnz = nnz;
    made(c, PANEL);
    return 0;
}

// a row-block panel straight from the reference's CSC arrays of B (the caller holds the whole matrix on the host and gives every
// context its block: the blocks then travel device to device, bella_hip_allgather_panels)
int bella_hip_set_B_panel(bella_ctx* c, uint16_t kmer_size, uint32_t nkmers, uint32_t first_read, uint32_t nreads_panel, const uint32_t* colptr,
                          const uint32_t* rowids, const uint16_t* values) {
    if (!c || !colptr) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (kmer_size < 1 || kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    if ((uint64_t)first_read + nreads_panel > c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "panel exceeds the read set");
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, TUPLES); drop(c, PANEL); drop(c, MATRIX);
    const uint32_t* cp = colptr + first_read;                      // colptr: the whole matrix's [nreads + 1]
    std::vector<uint32_t> cnt((size_t)nreads_panel + 2, 0);
    for (uint32_t r = 0; r < nreads_panel; ++r) {
        if (cp[r + 1] < cp[r]) return fail(c, BELLA_ERR_BAD_ARG, "colptr must be non-decreasing (column %u)", first_read + r);
        if (cp[r + 1] - cp[r] >= 65536u) return fail(c, BELLA_ERR_READ_TOO_LONG, "column %u has >= 65536 entries", first_read + r);
        cnt[r] = cp[r + 1] - cp[r];
    }
    const uint64_t nnz = (uint64_t)cp[nreads_panel] - cp[0];
    if (nnz && (!rowids || !values)) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    ENSURE(c, c->rowcnt, 4 * ((size_t)nreads_panel + 2));
    ENSURE(c, c->Bk, 4 * nnz);
    ENSURE(c, c->Bpos, 2 * nnz);
    HIPCHK(c, hipMemcpyAsync(c->rowcnt.p, cnt.data(), 4 * ((size_t)nreads_panel + 2), hipMemcpyHostToDevice, c->stream));
    if (nnz) {
        HIPCHK(c, c->stager.h2d(c->Bk.p, rowids + cp[0], 4 * nnz, c->stream));
        HIPCHK(c, c->stager.h2d(c->Bpos.p, values + cp[0], 2 * nnz, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));                    // cnt is a host vector
    c->nkmers = nkmers;
    c->kmer_size = kmer_size;
    c->panel_first = first_read;
    c->panel_rows = nreads_panel;
    c->panel_nnz = nnz;
    made(c, PANEL);
    return 0;
}

int bella_hip_assemble_counted_panel(bella_ctx* c, uint32_t first_read, uint32_t nreads_panel) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TUPLES)) return r;
    if ((uint64_t)first_read + nreads_panel > c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "panel exceeds the read set");
    if (first_read < c->kc_bfirst || (uint64_t)first_read + nreads_panel > (uint64_t)c->kc_bfirst + c->kc_brows)
        return fail(c, BELLA_ERR_BAD_ARG, "the device-resident tuples cover the reads %u .. %u only", c->kc_bfirst, c->kc_bfirst + c->kc_brows);
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, PANEL); drop(c, MATRIX);
    uint64_t t0 = 0, t1 = 0;                                       // the panel's tuples are contiguous: tstart of its first / last read
    const uint32_t rel = first_read - c->kc_bfirst;
    HIPCHK(c, hipMemcpyAsync(&t0, ptr<uint64_t>(c->kc_tstart) + rel, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&t1, ptr<uint64_t>(c->kc_tstart) + rel + nreads_panel, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t nnz = 0;
    int rc = assemble_rows_device(c, first_read, nreads_panel, t1 - t0, nullptr, nullptr, nullptr, &nnz, t0);
    if (rc) return rc;
    if (int r = assembly_done(c, true, false)) return r;
    c->nkmers = c->kc_nkmers;
    c->kmer_size = (uint16_t)c->kc_k;
    c->panel_first = first_read;
    c->panel_rows = nreads_panel;
    c->panel_nnz = nnz;
    made(c, PANEL);
    return 0;
}

int bella_hip_panel_device_ptrs(bella_ctx* c, uint32_t* first_read, uint32_t* nreads_panel, uint64_t* nnz, const void** d_rowcnt,
                                const void** d_rowids, const void** d_values) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, PANEL)) return r;
    if (first_read) *first_read = c->panel_first;
    if (nreads_panel) *nreads_panel = c->panel_rows;
    if (nnz) *nnz = c->panel_nnz;
    if (d_rowcnt) *d_rowcnt = c->rowcnt.p;
    if (d_rowids) *d_rowids = c->Bk.p;
    if (d_values) *d_values = c->Bpos.p;
    return 0;
}

int bella_hip_set_B_device(bella_ctx* c, uint16_t kmer_size, uint32_t nkmers, const uint32_t* d_colptr, const uint32_t* d_rowids,
                           const uint16_t* d_values, uint64_t nnz) {
    if (!c || !d_colptr || (nnz && (!d_rowids || !d_values))) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (kmer_size < 1 || kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, MATRIX);
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    // the sources may alias our own panel buffers: stage through fresh allocations
    TmpBuf nBptr, nBk, nBpos;
    ENSURE(c, nBptr, 4 * ((size_t)c->nreads + 2));
    ENSURE(c, nBk, 4 * nnz);
    ENSURE(c, nBpos, 2 * nnz);
    HIPCHK(c, hipMemcpyAsync(nBptr.p, d_colptr, 4 * ((size_t)c->nreads + 1), hipMemcpyDeviceToDevice, c->stream));
    if (nnz) HIPCHK(c, hipMemcpyAsync(nBk.p, d_rowids, 4 * nnz, hipMemcpyDeviceToDevice, c->stream));
    if (nnz) HIPCHK(c, hipMemcpyAsync(nBpos.p, d_values, 2 * nnz, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    nBptr.give_to(c->Bptr); nBk.give_to(c->Bk); nBpos.give_to(c->Bpos);
    drop(c, PANEL);
    c->nkmers = nkmers;
    c->nnz = nnz;
    c->kmer_size = kmer_size;
    int rc = build_layout(c);
    if (rc) return rc;
    return assembly_done(c, false, false);
}

// ---- multi-GPU: RCCL communicator + panel all-gather -------------------------------------------------------------------------
int bella_hip_comm_available(void) { return rccl().ok() ? 1 : 0; }

static int comm_id_impl(const Rccl& api, uint8_t id[BELLA_HIP_COMM_ID_BYTES]) {
    if (!id) return BELLA_ERR_BAD_ARG;
    if (!api.ok()) return BELLA_ERR_STATE;
    ncclUniqueId u;
    static_assert(sizeof(u) == BELLA_HIP_COMM_ID_BYTES, "ncclUniqueId size");
    if (api.GetUniqueId(&u) != ncclSuccess) return BELLA_ERR_HIP;
    std::memcpy(id, &u, sizeof(u));
    return 0;
}
int bella_hip_comm_id(uint8_t id[BELLA_HIP_COMM_ID_BYTES]) { return comm_id_impl(rccl(), id); }
int bella_hip_comm_id_local(uint8_t id[BELLA_HIP_COMM_ID_BYTES]) { return comm_id_impl(loopback(), id); }

// Wait for what the collective calls put on the stream -- with a deadline (BELLA_HIP_COMM_TIMEOUT_S, default 120 s): a peer that never
// arrives must not hang the process.  On expiry the communicator is aborted (ncclCommAbort, where the transport has it) and the call
// fails like any other error: the caller falls back (bench.py, bella_amd/dist.py: the torch.distributed exchange).
static int comm_sync(bella_ctx* c, const char* what) {
    const double limit = loop_timeout_s();                      // BELLA_HIP_COMM_TIMEOUT_S, default 120 (comm.hpp)
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) { (void)hipGetLastError(); return fail(c, BELLA_ERR_HIP, "%s: %s", what, hipGetErrorString(q)); }
        (void)hipGetLastError();
        if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(200));
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
            if (c->comm && c->api && c->api->CommAbort) { (void)c->api->CommAbort(c->comm); c->comm = nullptr; c->comm_ranks = 0; }
            return fail(c, BELLA_ERR_STATE, "%s: no completion within %.0f s (a peer did not arrive); the communicator was aborted", what, limit);
        }
    }
}

// Every entry point of the transport once, right after the communicator exists (all ranks are inside bella_hip_comm_init together): an
// all-gather of the ranks' numbers and a grouped send/recv to the rank ITSELF -- a missing symbol, an ABI mismatch or a communicator
// that does not move data fails HERE, at init, not inside the first exchange of a run.
static int comm_selftest(bella_ctx* c) {
    const int N = c->comm_ranks, me = c->comm_rank;
    // (sized here, once, for every later use -- the status exchanges and the metadata lines of the shared formation of A': no collective
    // entry point can find itself without the buffer its peers are waiting to hear from it through)
    ENSURE(c, c->comm_meta, 8 * (((size_t)N + 3) * ((size_t)N + 1) + 4 * ((size_t)N + 1)) + 8 * 4 * ((size_t)N + 1) + 64);
    uint64_t* d = ptr<uint64_t>(c->comm_meta);
    const uint64_t mine[4] = {0xBE11A000ull + (uint64_t)me, ~(uint64_t)me, 0, 0};
    HIPCHK(c, hipMemsetAsync(d, 0, 8 * 4 * ((size_t)N + 1) + 64, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + 4 * (size_t)N, mine, 16, hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, c->api->AllGather(d + 4 * (size_t)N, d, 1, ncclUint64, c->comm, c->stream));
    ncclResult_t r = c->api->GroupStart();
    if (r == ncclSuccess) r = c->api->Send(d + 4 * (size_t)N + 1, 1, ncclUint64, me, c->comm, c->stream);
    if (r == ncclSuccess) r = c->api->Recv(d + 4 * (size_t)N + 2, 1, ncclUint64, me, c->comm, c->stream);
    const ncclResult_t ge = c->api->GroupEnd();
    if (r == ncclSuccess) r = ge;
    if (r != ncclSuccess) return fail(c, BELLA_ERR_HIP, "communicator self-test: %s", c->api->GetErrorString ? c->api->GetErrorString(r) : "RCCL error");
    std::vector<uint64_t> got((size_t)N + 4, 0);
    HIPCHK(c, hipMemcpyAsync(got.data(), d, 8 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(got.data() + N, d + 4 * (size_t)N, 24, hipMemcpyDeviceToHost, c->stream));
    int rc = comm_sync(c, "communicator self-test");
    if (rc) return rc;
    for (int q = 0; q < N; ++q)
        if (got[(size_t)q] != 0xBE11A000ull + (uint64_t)q) return fail(c, BELLA_ERR_STATE, "communicator self-test: the all-gather delivered %llx for rank %d", (unsigned long long)got[(size_t)q], q);
    if (got[(size_t)N + 2] != ~(uint64_t)me) return fail(c, BELLA_ERR_STATE, "communicator self-test: send/recv to self delivered %llx", (unsigned long long)got[(size_t)N + 2]);
    return 0;
}

static int comm_init_impl(bella_ctx* c, const Rccl& api, int nranks, int rank, const uint8_t id[BELLA_HIP_COMM_ID_BYTES]) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, BELLA_ERR_BAD_ARG, "bad communicator arguments");
    if (!api.ok()) return fail(c, BELLA_ERR_STATE, "librccl could not be loaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm && c->api) { (void)c->api->CommDestroy(c->comm); c->comm = nullptr; }
    c->api = &api;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    NCCLCHK(c, api.CommInitRank(&c->comm, nranks, u, rank));
    c->comm_ranks = nranks;
    c->comm_rank = rank;
    const int rc = comm_selftest(c);
    if (rc) {                                                    // a communicator that fails its self-test is not kept
        if (c->comm) { (void)(api.CommAbort ? api.CommAbort(c->comm) : api.CommDestroy(c->comm)); c->comm = nullptr; }
        c->comm_ranks = 0;
    }
    return rc;
}
int bella_hip_comm_init(bella_ctx* c, int nranks, int rank, const uint8_t id[BELLA_HIP_COMM_ID_BYTES]) {
    return comm_init_impl(c, rccl(), nranks, rank, id);
}
int bella_hip_comm_init_local(bella_ctx* c, int nranks, int rank, const uint8_t id[BELLA_HIP_COMM_ID_BYTES]) {
    return comm_init_impl(c, loopback(), nranks, rank, id);
}

int bella_hip_comm_destroy(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (c->comm && c->api) { (void)c->api->CommDestroy(c->comm); c->comm = nullptr; }
    c->comm_ranks = 0;
    return 0;
}

// Collective agreement: every rank contributes its local status; if any rank failed, ALL return an error here, together (a rank
// that left a collective entry point on a local error would leave its peers waiting in the next exchange).
static int comm_agree(bella_ctx* c, int local_rc) {
    const int N = c->comm_ranks;
    if (ensure_bytes(c, c->comm_meta, 8 * 4 * ((size_t)N + 1))) local_rc = local_rc ? local_rc : BELLA_ERR_NOMEM;
    if (!c->comm_meta.p) return local_rc ? local_rc : BELLA_ERR_NOMEM;      // (nothing to exchange through: cannot happen after the first call)
    uint64_t* d_meta = ptr<uint64_t>(c->comm_meta);
    const uint64_t mine = local_rc ? 1 : 0;
    std::vector<uint64_t> all((size_t)N, 0);
    hipError_t e = hipMemcpyAsync(d_meta + 4 * (size_t)N, &mine, 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    ncclResult_t r = c->api->AllGather(d_meta + 4 * (size_t)N, d_meta, 1, ncclUint64, c->comm, c->stream);
    if (r != ncclSuccess) return local_rc ? local_rc : fail(c, BELLA_ERR_HIP, "status exchange failed");
    if (e == hipSuccess) e = hipMemcpyAsync(all.data(), d_meta, 8 * (size_t)N, hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return local_rc ? local_rc : fail(c, BELLA_ERR_HIP, "status exchange: %s", hipGetErrorString(e));
    { const int sr = comm_sync(c, "status exchange"); if (sr) return local_rc ? local_rc : sr; }
    if (local_rc) return local_rc;
    for (int q = 0; q < N; ++q)
        if (all[(size_t)q]) return fail(c, BELLA_ERR_STATE, "rank %d failed inside the collective call; all ranks leave it", q);
    return 0;
}

// ---- the formation of A' shared over the ranks (BELLA_TUNE_DIST_LAYOUT; kernels: assemble.hpp) ---------------------------------------
// Every rank holds the whole exchanged matrix B (6 B per nonzero) and computes the columns i % N == rank.  Replicated, the device layout
// sorts ALL entries by k-mer on every rank to form A' (prep + sort: 7.7 of a rank's 11.4 ms at N = 8, 100k reads).  Here rank g keeps the
// entries whose k-mer id lies in the g-th N-th of the id space, sorts those, emits ITS slice of A' (in place in the whole array) and
// the B' entries of ALL rows for those k-mers; then two grouped exchanges: the slices of A' (all-gather: 8 B per nonzero) and the B'
// entries to the owners of their rows (all-to-all: 12 B per nonzero).  Same layout as the replicated one, entry for entry.
extern "C++" {
namespace {
// what a rank needs for the shared formation (asked of every rank in bella_hip_allgather_panels; taken only if all can)
bool layout_dist_eligible(const bella_ctx* c) {
    const bool first_app = c->tune_layout_order == 1 || (c->debug & 1024u);
    const bool wanted = c->tune_dist_layout == 1 || (c->tune_dist_layout == 2 && c->api == &loopback());
    return wanted && c->comm && c->api && c->comm_ranks > 1 && (uint32_t)c->comm_ranks <= kOwnerMax &&
           c->part_stride == (uint32_t)c->comm_ranks && c->part_first == (uint32_t)c->comm_rank && !first_app && c->nreads <= (1u << 30);
}
// a rank that failed before its formation began: its line of the metadata exchange says so (the ranks inside layout_dist read it and leave)
void layout_dist_fail(bella_ctx* c) {
    const size_t N = (size_t)c->comm_ranks, W = N + 3;
    if (ensure_bytes(c, c->comm_meta, 8 * (W * (N + 1) + 4 * (N + 1))) || !c->comm_meta.p) return;
    uint64_t* d_meta = ptr<uint64_t>(c->comm_meta);
    std::vector<uint64_t> line(W, 0);
    line[0] = 1;
    if (hipMemcpyAsync(d_meta + W * N, line.data(), 8 * W, hipMemcpyHostToDevice, c->stream) != hipSuccess) return;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return;
    if (c->api->AllGather(d_meta + W * N, d_meta, W, ncclUint64, c->comm, c->stream) != ncclSuccess) return;
    (void)comm_sync(c, "layout metadata");
}
int layout_dist(bella_ctx* c, uint64_t nown_nnz, uint32_t rmask, uint32_t inl, int kbits, uint32_t** ekey_out, uint64_t** eval_out,
                uint32_t** fkey_out, uint64_t** fval_out) {
    const int N = c->comm_ranks, me = c->comm_rank;
    const uint32_t nr = c->nreads, nk = c->nkmers;
    const uint64_t nnz = c->nnz;
    const uint32_t klo = (uint32_t)((uint64_t)nk * (uint64_t)me / (uint64_t)N), khi = (uint32_t)((uint64_t)nk * (uint64_t)(me + 1) / (uint64_t)N);
    const uint32_t M = (nr + (uint32_t)N - 1) / (uint32_t)N;      // rows per owner, at most
    const size_t W = (size_t)N + 3;                               // words of a rank's line of the metadata exchange
    TmpBuf pbuf, sbuf, hbuf;                                      // owner-major row lengths + their scan; per-owner counters and cursors
    // (1) this rank's entries: per row how many, where they go, how many for the rows of each rank.  Host synchronisations of the
    // whole formation: this read-back, the metadata exchange, the end of the data exchange, the closing agreement.
    int rc = ensure_bytes(c, pbuf, 4 * ((size_t)N * M + 2));
    if (!rc) rc = ensure_bytes(c, sbuf, 4 * ((size_t)N * M + 2));
    if (!rc) rc = ensure_bytes(c, hbuf, 8 * 2 * (size_t)kOwnerMax);
    if (!rc) rc = ensure_bytes(c, c->comm_meta, 8 * (W * ((size_t)N + 1) + 4 * ((size_t)N + 1)));
    uint32_t* cnt = ptr<uint32_t>(c->w);
    uint32_t* rowbase = ptr<uint32_t>(c->wscan);
    unsigned long long* hist = ptr<unsigned long long>(hbuf);
    std::vector<uint64_t> line(W, 0);                             // {failed, entries of my slice, entries of my rows, entries for the rows of rank 0 .. N-1}
    uint32_t nsel32 = 0;
    if (!rc) rc = [&]() -> int {
        HIPCHK(c, hipMemsetAsync(hist, 0, 8 * 2 * (size_t)kOwnerMax, c->stream));
        k_range_rowcount<<<nblk((uint64_t)nr + 1, kWaves), kBlock, 0, c->stream>>>(ptr<uint32_t>(c->Bptr), ptr<uint32_t>(c->Bk), nr, klo, khi, cnt, nk,
                                                                                   ptr<uint32_t>(c->status));
        KCHK(c);
        k_owner_hist_rows<<<nblk(nr ? nr : 1), 256, 0, c->stream>>>(cnt, nr, (uint32_t)N, hist);
        KCHK(c);
        const int sr = scan_u32(c, cnt, rowbase, (uint64_t)nr + 1);
        if (sr) return sr;
        HIPCHK(c, hipMemcpyAsync(&nsel32, rowbase + nr, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(line.data() + 3, hist, 8 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
        // a k-mer id beyond the dictionary belongs to no rank's range: the slices would not add up and every rank would report a
        // STATE error; the rank that sees it reports the bad input instead (status bit 32, as the replicated formation does)
        uint32_t st0 = 0;
        const int r0 = read_status(c, &st0);
        if (r0) return r0;
        return status_to_error(c, st0);
    }();
    const uint64_t nsel = nsel32;
    // (2) buffers for the rank's share: what it sorts (nsel) and what it receives (nown_nnz)
    const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(nsel, nown_nnz), 1);
    if (!rc) rc = ensure_bytes(c, c->lk_key, 4 * cap);
    if (!rc) rc = ensure_bytes(c, c->lk_key2, 4 * cap);
    if (!rc) rc = ensure_bytes(c, c->lk_val, 8 * cap);
    if (!rc) rc = ensure_bytes(c, c->lk_val2, 8 * cap);
    // (3) every rank's line to every rank: all take the same decision from the same table
    if (!c->comm_meta.p) return rc ? rc : BELLA_ERR_NOMEM;        // (nothing to exchange through: cannot happen after the first collective call)
    uint64_t* d_meta = ptr<uint64_t>(c->comm_meta);
    line[0] = rc ? 1 : 0; line[1] = nsel; line[2] = nown_nnz;
    std::vector<uint64_t> T(W * (size_t)N, 0);
    {
        hipError_t e = hipMemcpyAsync(d_meta + W * (size_t)N, line.data(), 8 * W, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        const ncclResult_t r = c->api->AllGather(d_meta + W * (size_t)N, d_meta, W, ncclUint64, c->comm, c->stream);
        if (r != ncclSuccess) return rc ? rc : fail(c, BELLA_ERR_HIP, "layout metadata exchange failed");
        if (e == hipSuccess) e = hipMemcpyAsync(T.data(), d_meta, 8 * W * (size_t)N, hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) return rc ? rc : fail(c, BELLA_ERR_HIP, "layout metadata exchange: %s", hipGetErrorString(e));
        const int sr = comm_sync(c, "layout metadata");
        if (sr) return rc ? rc : sr;
    }
    if (rc) return rc;
    std::vector<uint64_t> abase((size_t)N + 1, 0), roffs((size_t)N + 1, 0), ooff((size_t)N + 1, 0);
    for (int p = 0; p < N; ++p) {
        if (T[W * (size_t)p]) return fail(c, BELLA_ERR_STATE, "rank %d failed inside the collective call; all ranks leave it", p);
        abase[(size_t)p + 1] = abase[(size_t)p] + T[W * (size_t)p + 1];
    }
    if (abase[(size_t)N] != nnz)
        return fail(c, BELLA_ERR_STATE, "the ranks' slices hold %llu of %llu entries (different matrices or dictionaries?)",
                    (unsigned long long)abase[(size_t)N], (unsigned long long)nnz);
    for (int q = 0; q < N; ++q) {                                 // (every rank checks every rank's rows: the same verdict everywhere)
        uint64_t got = 0;
        for (int p = 0; p < N; ++p) got += T[W * (size_t)p + 3 + (size_t)q];
        if (got != T[W * (size_t)q + 2])
            return fail(c, BELLA_ERR_STATE, "the ranks hold %llu entries for the rows of rank %d, its rows have %llu", (unsigned long long)got, q,
                        (unsigned long long)T[W * (size_t)q + 2]);
    }
    auto S = [&](int p, int q) { return T[W * (size_t)p + 3 + (size_t)q]; };    // entries rank p holds for the rows of rank q
    for (int p = 0; p < N; ++p) { roffs[(size_t)p + 1] = roffs[(size_t)p] + S(p, me); ooff[(size_t)p + 1] = ooff[(size_t)p] + S(me, p); }
    // (4) my entries in k-mer order
    hipcub::DoubleBuffer<uint32_t> dk(ptr<uint32_t>(c->lk_key), ptr<uint32_t>(c->lk_key2));
    hipcub::DoubleBuffer<uint64_t> dv(ptr<uint64_t>(c->lk_val), ptr<uint64_t>(c->lk_val2));
    // (valid buffers of the agreed sizes whatever happens below: a rank whose passes fail still moves its -- then meaningless -- share)
    uint32_t *okey = ptr<uint32_t>(c->lk_key2), *rkey = ptr<uint32_t>(c->lk_key);
    uint64_t *oval = ptr<uint64_t>(c->lk_val2), *rval = ptr<uint64_t>(c->lk_val);
    rc = [&]() -> int {
        if (nsel) {
            k_layout_prep_range<<<nblk(nr, kWaves), kBlock, 0, c->stream>>>(ptr<uint32_t>(c->Bptr), ptr<uint32_t>(c->Bk), ptr<uint16_t>(c->Bpos), nr,
                                                                           ptr<uint32_t>(c->packed), ptr<uint64_t>(c->roff), c->kmer_size, nk, klo, khi,
                                                                           rowbase, dk.Current(), dv.Current(), ptr<uint32_t>(c->status));
            KCHK(c);
            CUB(c, hipcub::DeviceRadixSort::SortPairs, dk, dv, (uint64_t)nsel, 0, kbits, c->stream);
        }
        // (5) where a row starts in ITS owner's B': owner-major lengths, one scan
        uint2* rinfo = ptr<uint2>(c->lk_rinfo);
        k_owner_lengths<<<nblk((uint64_t)N * M + 1), 256, 0, c->stream>>>(ptr<uint32_t>(c->Bptr), nr, (uint32_t)N, M, ptr<uint32_t>(pbuf));
        KCHK(c);
        const int sr = scan_u32(c, ptr<uint32_t>(pbuf), ptr<uint32_t>(sbuf), (uint64_t)N * M + 1);
        if (sr) return sr;
        k_layout_rinfo_owner<<<nblk(nr ? nr : 1), 256, 0, c->stream>>>(ptr<uint32_t>(sbuf), ptr<uint64_t>(c->roff), nr, (uint32_t)N, M, rinfo);
        KCHK(c);
        // (6) my slice of A' (in place in the whole array) and the B' entries of all rows for my k-mers, each into its owner's range
        okey = dk.Alternate(); oval = dv.Alternate();
        rkey = dk.Current(); rval = dv.Current();                 // (the sorted arrays are free after this pass: what the rank receives goes there)
        if (nsel) {
            HIPCHK(c, hipMemcpyAsync(hist + kOwnerMax, ooff.data(), 8 * (size_t)N, hipMemcpyHostToDevice, c->stream));
            k_layout_emit<<<nblk(nsel, kLayoutEmitPartBlock), kLayoutEmitPartBlock, 0, c->stream>>>(
                dk.Current(), dv.Current(), nsel, ptr<uint32_t>(c->Bptr), ptr<uint32_t>(c->Bloc), ptr<uint32_t>(c->wscan), ptr<uint32_t>(c->packed),
                ptr<uint64_t>(c->roff), c->kmer_size, rmask, ptr<uint2>(c->Aent), okey, oval, 1u, (uint32_t)me, (uint32_t)N, nullptr, ptr<uint32_t>(c->status),
                inl, rinfo, (uint32_t)abase[(size_t)me], hist + kOwnerMax);
            KCHK(c);
        }
        return 0;
    }();
    // A rank that could not launch its passes still takes part in the exchange (the sizes are agreed: nobody waits); its error leaves
    // with the closing agreement.
    // (7) the two exchanges, one group: B' entries to their owners, slices of A' into place
    hipError_t he = hipSuccess;
    ncclResult_t nr2 = ncclSuccess;
    {
        if (S(me, me)) {
            he = hipMemcpyAsync(rkey + roffs[(size_t)me], okey + ooff[(size_t)me], 4 * (size_t)S(me, me), hipMemcpyDeviceToDevice, c->stream);
            if (he == hipSuccess) he = hipMemcpyAsync(rval + roffs[(size_t)me], oval + ooff[(size_t)me], 8 * (size_t)S(me, me), hipMemcpyDeviceToDevice, c->stream);
        }
        uint64_t* A64 = ptr<uint64_t>(c->Aent);
        nr2 = c->api->GroupStart();
        for (int p = 0; p < N && nr2 == ncclSuccess; ++p) {
            if (p == me) continue;
            const uint64_t to = S(me, p), from = S(p, me), theirs = T[W * (size_t)p + 1];
            if (to) {
                nr2 = c->api->Send(okey + ooff[(size_t)p], to, ncclUint32, p, c->comm, c->stream);
                if (nr2 == ncclSuccess) nr2 = c->api->Send(oval + ooff[(size_t)p], to, ncclUint64, p, c->comm, c->stream);
            }
            if (from && nr2 == ncclSuccess) {
                nr2 = c->api->Recv(rkey + roffs[(size_t)p], from, ncclUint32, p, c->comm, c->stream);
                if (nr2 == ncclSuccess) nr2 = c->api->Recv(rval + roffs[(size_t)p], from, ncclUint64, p, c->comm, c->stream);
            }
            if (nsel && nr2 == ncclSuccess) nr2 = c->api->Send(A64 + abase[(size_t)me], nsel, ncclUint64, p, c->comm, c->stream);
            if (theirs && nr2 == ncclSuccess) nr2 = c->api->Recv(A64 + abase[(size_t)p], theirs, ncclUint64, p, c->comm, c->stream);
        }
        {
            const ncclResult_t ge = c->api->GroupEnd();           // the group is closed on every path
            if (nr2 == ncclSuccess) nr2 = ge;
        }
    }
    uint32_t st = 0;
    if (he == hipSuccess && nr2 == ncclSuccess) he = hipMemcpyAsync(&st, ptr<uint32_t>(c->status), 4, hipMemcpyDeviceToHost, c->stream);
    if (nr2 != ncclSuccess || he != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        if (!rc) rc = fail(c, BELLA_ERR_HIP, "layout exchange failed: %s", nr2 != ncclSuccess ? (c->api->GetErrorString ? c->api->GetErrorString(nr2) : "RCCL error") : hipGetErrorString(he));
    } else {
        const int sr = comm_sync(c, "layout exchange");
        if (!rc) rc = sr;
        if (!rc) rc = status_to_error(c, st);
    }
    rc = comm_agree(c, rc);                                       // all ranks hold the layout's inputs, or all leave
    if (rc) return rc;
    *ekey_out = rkey; *eval_out = rval; *fkey_out = okey; *fval_out = oval;
    return 0;
}
}  // namespace
}  // extern "C++"

int bella_hip_allgather_panels(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (!c->comm) return fail(c, BELLA_ERR_STATE, "bella_hip_comm_init first");
    HIPCHK(c, hipSetDevice(c->device));
    const int N = c->comm_ranks, me = c->comm_rank;
    c->dist_agreed = false;
    // a rank without a panel still takes part in the status exchange: all ranks leave the call together
    int rc = comm_agree(c, need(c, PANEL));
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    // who holds what: {first read, rows, nnz} of every rank
    ENSURE(c, c->comm_meta, 8 * 4 * ((size_t)N + 1));
    // (the fourth word also says whether this rank can take the shared formation of A': all must, or none does)
    uint64_t mine[4] = {c->panel_first, c->panel_rows, c->panel_nnz, (uint64_t)c->nkmers | (layout_dist_eligible(c) ? 1ull << 32 : 0ull)};
    uint64_t* d_meta = ptr<uint64_t>(c->comm_meta);
    HIPCHK(c, hipMemcpyAsync(d_meta + 4 * (size_t)N, mine, sizeof(mine), hipMemcpyHostToDevice, c->stream));
    NCCLCHK(c, c->api->AllGather(d_meta + 4 * (size_t)N, d_meta, 4, ncclUint64, c->comm, c->stream));
    std::vector<uint64_t> meta(4 * (size_t)N);
    HIPCHK(c, hipMemcpyAsync(meta.data(), d_meta, 8 * 4 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
    rc = comm_sync(c, "panel sizes");
    if (rc) return rc;
    // (the checks below see the same numbers on every rank: all ranks fail them together)
    std::vector<uint64_t> roff((size_t)N + 1, 0), eoff((size_t)N + 1, 0);
    c->dist_agreed = true;
    for (int r = 0; r < N; ++r) {
        if (!(meta[4 * r + 3] >> 32)) c->dist_agreed = false;
        meta[4 * r + 3] &= 0xFFFFFFFFull;
        if (meta[4 * r] != roff[r]) return fail(c, BELLA_ERR_BAD_ARG, "panels must be consecutive read blocks in rank order (rank %d starts at %llu, expected %llu)",
                                                r, (unsigned long long)meta[4 * r], (unsigned long long)roff[r]);
        if (meta[4 * r + 3] != meta[3]) return fail(c, BELLA_ERR_BAD_ARG, "rank %d counted a different k-mer dictionary", r);
        roff[r + 1] = roff[r] + meta[4 * r + 1];
        eoff[r + 1] = eoff[r] + meta[4 * r + 2];
    }
    if (roff[N] != c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "the panels cover %llu of %u reads", (unsigned long long)roff[N], c->nreads);
    const uint64_t nnz = eoff[N];
    if (nnz >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "nnz(A) must be < 2^32");
    TmpBuf nCnt, nBk, nBpos, nBptr;
    rc = ensure_bytes(c, nCnt, 4 * ((size_t)c->nreads + 2));
    if (!rc) rc = ensure_bytes(c, nBptr, 4 * ((size_t)c->nreads + 2));
    if (!rc) rc = ensure_bytes(c, nBk, 4 * nnz);
    if (!rc) rc = ensure_bytes(c, nBpos, 2 * nnz + 16);
    rc = comm_agree(c, rc);                                       // all ranks hold the full arrays, or all leave
    if (rc) return rc;
    // one grouped exchange: to every peer my block, from every peer its block, straight to its place in the full arrays
    uint32_t* cnt = ptr<uint32_t>(nCnt);
    uint32_t* bk = ptr<uint32_t>(nBk);
    uint8_t* bpos = ptr<uint8_t>(nBpos);
    hipError_t he = hipMemsetAsync(cnt + c->nreads, 0, 8, c->stream);
    if (he == hipSuccess && c->panel_rows) he = hipMemcpyAsync(cnt + roff[me], c->rowcnt.p, 4 * (size_t)c->panel_rows, hipMemcpyDeviceToDevice, c->stream);
    if (he == hipSuccess && c->panel_nnz) he = hipMemcpyAsync(bk + eoff[me], c->Bk.p, 4 * (size_t)c->panel_nnz, hipMemcpyDeviceToDevice, c->stream);
    if (he == hipSuccess && c->panel_nnz) he = hipMemcpyAsync(bpos + 2 * eoff[me], c->Bpos.p, 2 * (size_t)c->panel_nnz, hipMemcpyDeviceToDevice, c->stream);
    ncclResult_t nr2 = ncclSuccess;
    if (N > 1) {
        nr2 = c->api->GroupStart();
        for (int p = 0; p < N && nr2 == ncclSuccess; ++p) {
            if (p == me) continue;
            const uint64_t prow = meta[4 * p + 1], pnnz = meta[4 * p + 2];
            if (c->panel_rows) nr2 = c->api->Send(c->rowcnt.p, c->panel_rows, ncclUint32, p, c->comm, c->stream);
            if (prow && nr2 == ncclSuccess) nr2 = c->api->Recv(cnt + roff[p], prow, ncclUint32, p, c->comm, c->stream);
            if (c->panel_nnz && nr2 == ncclSuccess) {
                nr2 = c->api->Send(c->Bk.p, c->panel_nnz, ncclUint32, p, c->comm, c->stream);
                if (nr2 == ncclSuccess) nr2 = c->api->Send(c->Bpos.p, 2 * c->panel_nnz, ncclUint8, p, c->comm, c->stream);
            }
            if (pnnz && nr2 == ncclSuccess) {
                nr2 = c->api->Recv(bk + eoff[p], pnnz, ncclUint32, p, c->comm, c->stream);
                if (nr2 == ncclSuccess) nr2 = c->api->Recv(bpos + 2 * eoff[p], 2 * pnnz, ncclUint8, p, c->comm, c->stream);
            }
        }
        const ncclResult_t ge = c->api->GroupEnd();               // the group is closed on every path
        if (nr2 == ncclSuccess) nr2 = ge;
    }
    if (nr2 != ncclSuccess || he != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        return fail(c, BELLA_ERR_HIP, "panel exchange failed: %s", nr2 != ncclSuccess ? (c->api->GetErrorString ? c->api->GetErrorString(nr2) : "RCCL error") : hipGetErrorString(he));
    }
    rc = scan_u32(c, cnt, ptr<uint32_t>(nBptr), (uint64_t)c->nreads + 1);
    if (!rc) rc = comm_sync(c, "panel exchange");
    nCnt.reset();
    if (rc) return rc;
    nBptr.give_to(c->Bptr); nBk.give_to(c->Bk); nBpos.give_to(c->Bpos);
    drop(c, PANEL); drop(c, MATRIX);
    c->nnz = nnz;
    rc = build_layout(c, true);
    if (rc) return rc;
    return assembly_done(c, false, false);                        // (assemble_ms: exchange + layout)
}

int bella_hip_get_B(bella_ctx* c, uint64_t* nnz, uint32_t* colptr, uint32_t* rowids, uint16_t* values) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, MATRIX)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (nnz) *nnz = c->nnz;
    if (colptr) HIPCHK(c, hipMemcpyAsync(colptr, c->Bptr.p, 4 * ((size_t)c->nreads + 1), hipMemcpyDeviceToHost, c->stream));
    if (rowids && c->nnz) HIPCHK(c, hipMemcpyAsync(rowids, c->Bk.p, 4 * c->nnz, hipMemcpyDeviceToHost, c->stream));
    if (values && c->nnz) HIPCHK(c, hipMemcpyAsync(values, c->Bpos.p, 2 * c->nnz, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

__global__ void k_wide_sizes(const uint32_t* cols, const uint32_t* flops, uint32_t nw, uint32_t* wf) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > nw) return;
    wf[s] = s < nw ? flops[cols[s]] : 0u;
}

// columns with >= 65536 products: expand -> sort by (column, partner) -> pairs -> slot order -> serial fold (wide.hpp)
// T: the batch's products (run_wide has the columns' sizes on the host: no second trip for their sum)
// A batch runs in two parts: wide_batch_begin enqueues everything up to the point where the host must know the batch's pair count (the
// columns' sizes, the row lists if the layout has none, the first grouping pass and the copy of its totals into pinned memory) and
// returns without waiting -- run_spgemm enqueues it BEFORE the LDS classes' row kernels, so that the first grouping pass starts with
// them instead of behind their queue --; wide_batch_finish waits for the totals and enqueues the rest.
struct WideBatch {
    WideArgs a{};
    uint32_t nw = 0;
    uint64_t T = 0;
    int rbits = 1, seg_bits = 1;
    bool tried_group = false;
};
constexpr uint32_t kPinWide = 112;                                  // c->pinned[112 ..]: pairs of the batch, overflow flag, runs of the sort-based path
static int wide_batch_begin(bella_ctx* c, const SpgemmArgs& sa, uint32_t nw, const uint32_t* d_cols, uint64_t T, WideBatch& wb) {
    wb.nw = nw; wb.T = T;
    ENSURE(c, c->w_f, 4 * ((size_t)nw + 2));
    ENSURE(c, c->w_off, 8 * ((size_t)nw + 2));
    ENSURE(c, c->w_nruns, 16);
    k_wide_sizes<<<nblk((uint64_t)nw + 1), 256, 0, c->stream>>>(d_cols, ptr<uint32_t>(c->flopsr), nw, ptr<uint32_t>(c->w_f));
    KCHK(c);
    int rc = scan_u32_to_u64(c, ptr<uint32_t>(c->w_f), ptr<uint64_t>(c->w_off), (uint64_t)nw + 1);
    if (rc) return rc;
    if (T >= 0x7FFF0000ull) return fail(c, BELLA_ERR_ROW_TOO_LARGE, "the columns with >= 65536 products hold %llu products together (limit 2^31)",
                                        (unsigned long long)T);
    ENSURE(c, c->w_plist, 8 * (T + 64)); ENSURE(c, c->w_scr, 2 * T);
    ENSURE(c, c->w_segfirst, 4 * ((size_t)nw + 2));
    ENSURE(c, c->w_toff, 8 * ((size_t)nw + 2));
    WideArgs& a = wb.a;
    a.cols = d_cols; a.nw = nw; a.woff = ptr<uint64_t>(c->w_off);
    a.Bptr = sa.Bptr; a.Bent = sa.Bent; a.inl = sa.inl; a.Aent = sa.Aent; a.Aent2 = sa.Aent2; a.Aov = sa.Aov; a.Arow = sa.Arow; a.roff = sa.roff; a.packed = sa.packed; a.flopptr = sa.flopptr;
    a.k = sa.k; a.binSize = sa.binSize;
    a.plist = ptr<uint2>(c->w_plist); a.plist_pad = T; a.sort_scratch = ptr<uint16_t>(c->w_scr);
    a.tmp_pairs = sa.tmp_pairs; a.tmp_ext = sa.tmp_ext; a.nnzC = sa.nnzC; a.status = sa.ctl + kCtlStatus;
    while ((1ull << wb.rbits) < (uint64_t)c->nreads) ++wb.rbits;   // a partner read id fits rbits bits
    a.rbits = (uint32_t)wb.rbits;
    while ((1u << wb.seg_bits) < nw) ++wb.seg_bits;
    a.key32 = wb.rbits + wb.seg_bits <= 32 && !(c->debug & 64u) ? 1u : 0u;   // debug bit 6: tests, 64-bit keys on any input
    a.R_first = nullptr;
    // wide columns with few partners (HiFi-like input): group in LDS, two streaming passes over the columns' products (wide.hpp) --
    // unless a column's partners do not fit the table, the lane-order self-test failed, or debug bit 12 asks for the sort-based path
    // (tests).  The products are read from the row lists; a layout without them (the default) expands the BATCH's columns into a
    // temporary list first (10 bytes per product of the batch, k_layout_rowlists on the batch's columns).
    bool lists = c->have_rowlists;
    if (!lists && c->lane_order_ok && !(c->debug & 4096u) && c->nreads <= (1u << 30)) {
        if (!ensure_bytes(c, c->w_aent2, 8 * T + 64) && !ensure_bytes(c, c->w_aov, 2 * T + 64)) {
            k_layout_rowlists<<<nw < 4096u ? nw : 4096u, kRowListBlock, 0, c->stream>>>(sa.Bptr, sa.Bent, sa.Aent, ptr<uint64_t>(c->w_off), sa.roff, d_cols, nw,
                                                                                        ptr<uint2>(c->w_aent2), ptr<uint16_t>(c->w_aov), sa.inl);
            KCHK(c);
            a.Aent2 = ptr<uint2>(c->w_aent2); a.Aov = ptr<uint16_t>(c->w_aov); a.Arow = nullptr;
            lists = true;
        } else {
            c->err.clear();                                        // (no room: the sort-based path expands for itself)
            release(c->w_aent2); release(c->w_aov);
        }
    }
    if (lists && c->lane_order_ok && !(c->debug & 4096u)) {
        ENSURE(c, c->w_gtab, sizeof(uint4) * (size_t)nw * kWideGroupSlots);
        ENSURE(c, c->w_gcount, 4 * ((size_t)nw + 4));
        ENSURE(c, c->w_gbase, 4 * ((size_t)nw + 4));
        a.gtab = ptr<uint4>(c->w_gtab); a.gcount = ptr<uint32_t>(c->w_gcount); a.gbase = ptr<uint32_t>(c->w_gbase);
        HIPCHK(c, hipMemsetAsync(a.gcount + nw, 0, 8, c->stream));          // the scan's last element and the overflow flag
        k_wide_group1<<<nw < 4096u ? nw : 4096u, kWideGroup1Block, 0, c->stream>>>(a);
        KCHK(c);
        rc = scan_u32(c, ptr<uint32_t>(c->w_gcount), ptr<uint32_t>(c->w_gbase), (uint64_t)nw + 1);
        if (rc) return rc;
        // (8 bytes into pinned memory: the pairs of the batch and the overflow flag; the slot-order tables are sized on the device)
        HIPCHK(c, hipMemcpyAsync(c->pinned + kPinWide, ptr<uint32_t>(c->w_gbase) + nw, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->pinned + kPinWide + 1, ptr<uint32_t>(c->w_gcount) + nw + 1, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->join[kNumTiers - 3], c->stream));
        // The append pass needs nothing from the host (the table images and the batch's product count): it follows at once and leaves by
        // itself if a column's partners did not fit the table (the flag); the host meanwhile waits for the totals and prepares the
        // kernels that need the pair count on a second stream.
        k_wide_group2_chunks<<<nw < 8192u ? nw : 8192u, kWideGroup2Block, 0, c->stream>>>(a);
        KCHK(c);
        wb.tried_group = true;
    }
    return 0;
}

// sync_at_end: another batch follows (its buffers may be reallocated: the kernels of this one must be done)
static int wide_batch_finish(bella_ctx* c, WideBatch& wb, bool sync_at_end) {
    WideArgs& a = wb.a;
    const uint32_t nw = wb.nw;
    const uint64_t T = wb.T;
    hipStream_t const s2 = c->side[kNumTiers - 1];
    uint32_t np = 0;
    bool grouped = false;
    int rc = 0;
    // slot-order tables (pow2 >= max(16, pairs) slots per column: at most 16 nw + 2 np in all), ranks, descriptors by class: small kernels
    auto tables_and_descriptors = [&](hipStream_t st) -> int {
        const uint64_t tab_cap = 16ull * nw + 2ull * np;
        ENSURE(c, c->w_table, 8 * tab_cap);
        a.table = ptr<uint64_t>(c->w_table); a.toff = ptr<uint64_t>(c->w_toff);
        k_wide_toff<<<1, 1024, 0, st>>>(a.seg_first, nw, ptr<uint64_t>(c->w_toff));
        KCHK(c);
        k_wide_table_fill<<<nblk(tab_cap), 256, 0, st>>>(a.table, tab_cap);
        KCHK(c);
        if (np) {
            k_wide_insert<<<nblk(np), 256, 0, st>>>(a);
            KCHK(c);
        }
        k_wide_ranks<<<nw < 1024u ? nw : 1024u, kBlock, 0, st>>>(a);
        KCHK(c);
        if (np) {
            ENSURE(c, c->w_redo, 4 * ((size_t)np + 4));
            a.redo = ptr<uint32_t>(c->w_redo);
            HIPCHK(c, hipMemsetAsync(a.redo + np, 0, 16, st));    // (the redo count and the three class counts of k_wide_desc)
            ENSURE(c, c->w_desc, 3 * sizeof(WidePairAddr) * (size_t)np);
            a.desc = (WidePairAddr*)c->w_desc.p;
            k_wide_desc<<<nblk(np), 256, 0, st>>>(a);
            KCHK(c);
        }
        return 0;
    };
    if (wb.tried_group) {
        HIPCHK(c, hipEventSynchronize(c->join[kNumTiers - 3]));      // (the totals are there; the append pass is running)
        if (c->pinned[kPinWide + 1] == 0) {
            np = c->pinned[kPinWide];
            ENSURE(c, c->w_rlen, 4 * ((size_t)np + 1)); ENSURE(c, c->w_rstart, 4 * ((size_t)np + 2)); ENSURE(c, c->w_rrank, 4 * ((size_t)np + 1));
            ENSURE(c, c->w_rfirst, 4 * ((size_t)np + 1));
            ENSURE(c, c->w_key2, 8 * ((size_t)np + 1));
            a.R_len_w = ptr<uint32_t>(c->w_rlen); a.R_start_w = ptr<uint32_t>(c->w_rstart); a.R_key_w = c->w_key2.p;
            a.R_first = ptr<uint32_t>(c->w_rfirst);
            a.R_key = c->w_key2.p; a.R_len = ptr<uint32_t>(c->w_rlen); a.R_start = ptr<uint32_t>(c->w_rstart); a.npairs = np;
            a.R_rank = ptr<uint32_t>(c->w_rrank);
            a.seg_first = ptr<uint32_t>(c->w_gbase);                 // first pair of every column = the prefix sums of the pair counts
            grouped = true;
            if (np) {
                // NEXT to the append pass (which wide_batch_begin enqueued), on a stream of their own: the pairs' keys / lists / first
                // products (from the table images) and the small kernels that only need those -- tables, slot-order insertion, ranks,
                // descriptors
                HIPCHK(c, hipStreamWaitEvent(s2, c->join[kNumTiers - 3], 0));
                k_wide_pairs<<<nw < 8192u ? nw : 8192u, kWideGroup2Block, 0, s2>>>(a);
                KCHK(c);
                rc = tables_and_descriptors(s2);
                if (rc) return rc;
                HIPCHK(c, hipEventRecord(c->join[kNumTiers - 2], s2));
                HIPCHK(c, hipStreamWaitEvent(c->stream, c->join[kNumTiers - 2], 0));
            } else {
                rc = tables_and_descriptors(c->stream);
                if (rc) return rc;
            }
        }
    }
    {   // bella_timings.wide_batches: which of the two ran, batch by batch (two saturating 16-bit counts)
        const uint32_t sh = grouped ? 0u : 16u;
        if (((c->tm.wide_batches >> sh) & 0xFFFFu) != 0xFFFFu) c->tm.wide_batches += 1u << sh;
    }
    if (!grouped) {
        // the sort-based path: 38 bytes per product of the batch in flight (only allocated when this path runs)
        const int rbits = wb.rbits, seg_bits = wb.seg_bits;
        ENSURE(c, c->w_key, 8 * T); ENSURE(c, c->w_key2, 8 * T);
        ENSURE(c, c->w_idx, 4 * T); ENSURE(c, c->w_idx2, 4 * T);
        ENSURE(c, c->w_hv, 8 * T);
        ENSURE(c, c->w_rlen, 4 * (T + 1)); ENSURE(c, c->w_rstart, 4 * (T + 2)); ENSURE(c, c->w_rrank, 4 * T);
        a.R_first = nullptr;
        a.W_key = c->w_key.p; a.W_idx = ptr<uint32_t>(c->w_idx); a.W_rec = ptr<uint2>(c->w_hv);
        k_wide_expand<<<nw < 2048u ? nw : 2048u, kWideExpandBlock, 0, c->stream>>>(a);
        KCHK(c);
        // sort by (column, partner read) over the meaningful bits, run-length encode into pairs; u32 keys when they fit
        auto sort_and_encode = [&](auto key_tag) -> int {
            using K = decltype(key_tag);
            hipcub::DoubleBuffer<K> dk((K*)c->w_key.p, (K*)c->w_key2.p);
            hipcub::DoubleBuffer<uint32_t> dv(ptr<uint32_t>(c->w_idx), ptr<uint32_t>(c->w_idx2));
            CUB(c, hipcub::DeviceRadixSort::SortPairs, dk, dv, (int)T, 0, rbits + seg_bits, c->stream);
            a.S_key = dk.Current(); a.S_idx = dv.Current();
            K* rkey = dk.Current() == (K*)c->w_key.p ? (K*)c->w_key2.p : (K*)c->w_key.p;
            CUB(c, hipcub::DeviceRunLengthEncode::Encode, (const K*)a.S_key, rkey, ptr<uint32_t>(c->w_rlen), ptr<uint32_t>(c->w_nruns), (int)T, c->stream);
            a.R_key = rkey;
            return 0;
        };
        {
            const int rc2 = a.key32 ? sort_and_encode(uint32_t{}) : sort_and_encode(uint64_t{});
            if (rc2) return rc2;
        }
        HIPCHK(c, hipMemcpyAsync(c->pinned + kPinWide + 2, c->w_nruns.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        np = c->pinned[kPinWide + 2];
        HIPCHK(c, hipMemsetAsync(ptr<uint32_t>(c->w_rlen) + np, 0, 4, c->stream));
        rc = scan_u32(c, ptr<uint32_t>(c->w_rlen), ptr<uint32_t>(c->w_rstart), (uint64_t)np + 1);
        if (rc) return rc;
        a.R_len = ptr<uint32_t>(c->w_rlen); a.R_start = ptr<uint32_t>(c->w_rstart); a.npairs = np;
        a.R_rank = ptr<uint32_t>(c->w_rrank); a.seg_first = ptr<uint32_t>(c->w_segfirst);
        k_wide_gather<<<nblk(T), 256, 0, c->stream>>>(a, T);
        KCHK(c);
        k_wide_segments<<<nblk((uint64_t)np + 1), 256, 0, c->stream>>>(a);
        KCHK(c);
        rc = tables_and_descriptors(c->stream);
        if (rc) return rc;
    }
    if (np) {
        // one workgroup per pair (closed-form fold); what it leaves over (lists of >= 32768 products, > 16 bins) to the serial fold
#ifdef BELLA_WF_CLOCK
        static unsigned long long* d_clk = nullptr;
        if (!d_clk) (void)hipMalloc(&d_clk, 64);
        (void)hipMemsetAsync(d_clk, 0, 64, c->stream);
        a.clk = d_clk;
#endif
        // (three instances by list length, wide.hpp: the class counts are on the device, workgroups beyond a class's pairs leave at once)
        // The instances run side by side (other pairs, other lists; the redo list and its counter take atomics): the short lists on a
        // stream of their own, so that one instance's last pairs do not hold up the next one's first.
        HIPCHK(c, hipEventRecord(c->fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(s2, c->fork, 0));
        k_wide_fold_wg<kWideFoldBlockLarge, kWideFoldMid, kGridBucketsLarge, 1, 6><<<np < 16384u ? np : 16384u, kWideFoldBlockLarge, 0, c->stream>>>(a);
        KCHK(c);
        k_wide_fold_wg<kWideFoldBlockSmall, kWideFoldSmall, 2048, 0, 6><<<np < 16384u ? np : 16384u, kWideFoldBlockSmall, 0, s2>>>(a);
        KCHK(c);
        k_wide_fold_wg<kWideFoldBlockLarge, kWideFoldLdsLarge, kGridBucketsLarge, 2, 4><<<np < 4096u ? np : 4096u, kWideFoldBlockLarge, 0, c->stream>>>(a);
        KCHK(c);
        HIPCHK(c, hipEventRecord(c->join[kNumTiers - 1], s2));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->join[kNumTiers - 1], 0));
#ifdef BELLA_WF_CLOCK
        {
            unsigned long long h[8];
            (void)hipMemcpyAsync(h, d_clk, 64, hipMemcpyDeviceToHost, c->stream);
            (void)hipStreamSynchronize(c->stream);
            unsigned long long tot = 0;
            for (int i = 0; i < 8; ++i) tot += h[i];
            std::fprintf(stderr, "[wf clock] pairs %u:", np);
            for (int i = 0; i < 8; ++i) std::fprintf(stderr, " p%d %.1f%%", i, 100.0 * (double)h[i] / (double)tot);
            std::fprintf(stderr, " | cycles per pair %.0f\n", (double)tot / np);
        }
#endif
        k_wide_fold<<<nblk(np, 64), 64, 0, c->stream>>>(a);
        KCHK(c);
    }
    if (sync_at_end) HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
static int run_wide_batch(bella_ctx* c, const SpgemmArgs& sa, uint32_t nw, const uint32_t* d_cols, uint64_t T, bool sync_at_end) {
    WideBatch wb;
    int rc = wide_batch_begin(c, sa, nw, d_cols, T, wb);
    if (rc) return rc;
    return wide_batch_finish(c, wb, sync_at_end);
}

// batches of wide columns holding at most `budget` products each (38 bytes of HBM per product in flight)
// Tall: the products of all nw columns (known from the symbolic kernels' control block): when they fit one batch -- the usual case -- the
// columns' sizes need not come to the host at all
static int run_wide(bella_ctx* c, const SpgemmArgs& sa, uint32_t nw, const uint32_t* d_cols, uint64_t Tall) {
    if (Tall && Tall <= c->wide_budget) return run_wide_batch(c, sa, nw, d_cols, Tall, false);
    ENSURE(c, c->w_f, 4 * ((size_t)nw + 2));
    k_wide_sizes<<<nblk((uint64_t)nw + 1), 256, 0, c->stream>>>(d_cols, ptr<uint32_t>(c->flopsr), nw, ptr<uint32_t>(c->w_f));
    KCHK(c);
    std::vector<uint32_t> wf((size_t)nw + 1);
    HIPCHK(c, hipMemcpyAsync(wf.data(), c->w_f.p, 4 * ((size_t)nw + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t budget = c->wide_budget;
    for (uint32_t b = 0; b < nw;) {
        uint64_t t = wf[b];
        uint32_t e = b + 1;
        while (e < nw && t + wf[e] <= budget) t += wf[e++];
        int rc = run_wide_batch(c, sa, e - b, d_cols + b, t, e < nw);
        if (rc) return rc;
        b = e;
    }
    return 0;
}

// The pass's partition must lie inside the one the layout was built for (B' only holds the owned columns): a whole layout serves any
// partition; otherwise the layout is rebuilt from the resident B for the partition now set.
static int layout_for_partition(bella_ctx* c) {
    if (c->layout_stride == 1 || (c->layout_stride == c->part_stride && c->layout_first == c->part_first)) return 0;
    const bella_timings keep = c->tm;
    int rc = build_layout(c);
    const float lm = c->tm.layout_ms, em = c->tm.expand_ms;
    c->tm = keep;
    c->tm.layout_ms = lm; c->tm.expand_ms = em;
    return rc;
}

static int run_spgemm(bella_ctx* c, const bella_params* p, uint32_t* status_out, int depth = 0) {
    const uint32_t nr = c->nreads;
    const bool force_global = (c->debug & 1u) != 0 || c->tune_row_path == 1 || !c->lane_order_ok;   // (self-test failed: every column on the repairing path)
    const bool want_ext = (c->debug & 2u) == 0;
    const uint64_t ws_stride = (row_mem_bytes(65535, 65535, false) + 255) & ~(size_t)255;
    ENSURE(c, c->flopsr, 4 * ((size_t)nr + 2));
    ENSURE(c, c->flopptr, 8 * ((size_t)nr + 2));
    ENSURE(c, c->nnzC, 4 * ((size_t)nr + 2));
    ENSURE(c, c->colptrC, 8 * ((size_t)nr + 2));
    ENSURE(c, c->rowlists, (16 * (size_t)kNumTiers + 4) * nr + 64);   // tier descriptor lists, then the list of wide columns
    ENSURE(c, c->tiercaps, 4 * kNumTiers);
    ENSURE(c, c->ctl, 4 * kCtlWords);
    ENSURE(c, c->ws, ws_stride * kGlobalGrid);
    ENSURE(c, c->retry, 4 * ((size_t)nr + 1));
    ENSURE(c, c->orderlist, 4 * ((size_t)nr + 1));
    ENSURE(c, c->order_ws, kOrderWsBytes * kOrderBigGrid);
    if (!c->order_attr) {
        HIPCHK(c, hipFuncSetAttribute((const void*)k_order_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)6 * kOrderLdsHt)));
        c->order_attr = true;
    }
    {   // temp storage of the pass's one scan (colptrC), so that nothing is allocated between the kernels
        size_t tb1 = 0;
        hipcub::TransformInputIterator<uint64_t, CountU64, const uint32_t*> it(ptr<uint32_t>(c->nnzC), CountU64());
        HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, it, ptr<uint64_t>(c->colptrC), (int)nr + 1, c->stream));
        ENSURE(c, c->cubtmp, tb1 + 256);
    }

    uint32_t caps[kNumTiers] = {};
    const bool half_tables = !(c->pair_ratio1024 * 5 < 1024);
    const uint32_t* tier_caps = (half_tables && !c->tiers_from_env) ? kTierCapsHalf : c->tier_caps;
    uint32_t g_ntiers = c->ntiers;
    if (!c->tiers_from_env)
        for (g_ntiers = 1; tier_caps[g_ntiers - 1] != 65535; ++g_ntiers) {}
    // Long-list inputs (at most one pair in 64 products on the assembly-time sample: HiFi-like sets): the fold of a pair is
    // quadratic in its list inside the row kernels and has a position grid on the sort-based path, so the larger LDS tiers are
    // closed and their columns take that path with the columns above the tiers.
    // (either every sampled column is like that, or the sample as a whole: since round 6 the path above the tiers is the faster one for
    // such columns even when a few short-list columns stand among them -- HiFi-like 10k reads, -u 40: 6.35 -> 5.9 ms per pass)
    const bool long_lists = !force_global && !c->tiers_from_env && (c->pair_ratio1024 < 16 || c->long_list_sample);
    for (uint32_t t = 0; t < g_ntiers; ++t)
        caps[t] = (force_global || (long_lists && tier_caps[t] > kLongListMaxCap)) && t + 1 < g_ntiers ? 0 : tier_caps[t];
    const int want_state = (force_global ? 2 : 1) + (half_tables ? 2 : 0) + (long_lists ? 4 : 0);
    const uint64_t psig[6] = {c->layout_gen, ((uint64_t)c->part_first << 32) | c->part_stride, ((uint64_t)c->range_lo << 32) | c->range_hi, nr,
                              (uint64_t)want_state, (uint64_t)g_ntiers};
    const bool warm = c->pass_known && std::memcmp(psig, c->pass_sig, sizeof(psig)) == 0;
    // Rarely needed kernels: the rerun of columns whose pair count overflowed an LDS tier's key table or whose lists came out of
    // order (list and count produced on the device), and the serial fold of pairs with > 16 final bins.  Whether a pass needs them
    // is again a function of the operands: a warm pass whose predecessor needed neither leaves them out and checks the counters
    // in the final control block (should they be non-zero after all, the pass is run again with them).
    const bool skip_rare = warm && c->pass_rare_free && !(c->debug & 4u);
    const bool skip_big = warm && c->pass_big_free && !(c->debug & 4u);
    uint32_t launches = 0;
    int rc = 0;
    uint32_t* const ctl_host = c->pinned + 32;
#define EVREC(i) HIPCHK(c, hipEventRecord(c->ev[i], c->stream))
    struct Launch { int lo, hi; size_t lds; uint32_t rows; int cls; };
    Launch ln[kNumTiers];
    int nl = 0;
    auto enqueue = [&]() -> int {
    EVREC(2);
    c->tm.wide_batches = 0;                                    // (counted by wide_batch_finish)
    if (c->caps_state != want_state) {                         // the tier caps only change with the operands or the debug switch
        HIPCHK(c, hipMemcpyAsync(c->tiercaps.p, caps, sizeof(caps), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));            // caps[] is a stack array
        c->caps_state = want_state;
    }
    // one control block per pass (counters, tier lengths, status, totals): one fill, one read back
    uint32_t* d_ctl = ptr<uint32_t>(c->ctl);
    // the columns of this context: i0 + j * stride, j < nown.  The symbolic kernels only visit those; the entries of all other
    // columns in flops / nnzC are zero from the one clear made when the operands, the partition or the stage changed.
    const uint32_t hi = c->range_hi < nr ? c->range_hi : nr;
    uint32_t i0 = c->range_lo + (c->part_first + c->part_stride - c->range_lo % c->part_stride) % c->part_stride;
    const uint32_t nown = i0 < hi ? (hi - i0 + c->part_stride - 1) / c->part_stride : 0;
    if (!nown) i0 = 0;
    {
        const uint64_t sig[6] = {(uint64_t)(uintptr_t)c->flopsr.p, (uint64_t)(uintptr_t)c->nnzC.p, c->layout_gen, ((uint64_t)c->part_first << 32) | c->part_stride,
                                 ((uint64_t)c->range_lo << 32) | c->range_hi, nr};
        if (std::memcmp(sig, c->sym_sig, sizeof(sig)) != 0) {
            HIPCHK(c, hipMemsetAsync(c->flopsr.p, 0, 4 * ((size_t)nr + 2), c->stream));
            HIPCHK(c, hipMemsetAsync(c->nnzC.p, 0, 4 * ((size_t)nr + 2), c->stream));
            std::memcpy(c->sym_sig, sig, sizeof(sig));
        }
    }
    // (the control block is cleared by the first kernel of the pass)
    if (nown && c->have_rowlists) {
        k_row_flops_rl<<<nblk(nown), kBlock, 0, c->stream>>>(ptr<uint64_t>(c->Arow), i0, c->part_stride, nown, ptr<uint32_t>(c->flopsr), ptr<uint32_t>(c->nnzC), d_ctl);
        KCHK(c);
    } else if (nown) {
        k_row_flops<<<nblk(nown), kBlock, 0, c->stream>>>(ptr<uint32_t>(c->rowF), i0, c->part_stride, nown,
                                                          ptr<uint32_t>(c->flopsr), ptr<uint32_t>(c->nnzC), d_ctl);
        KCHK(c);
    } else {
        HIPCHK(c, hipMemsetAsync(d_ctl, 0, 4 * kCtlWords, c->stream));
    }
    k_tier_lists<<<nblk(nown ? nown : 1), kBlock, 0, c->stream>>>(ptr<uint32_t>(c->flopsr), nr, i0, c->part_stride, nown, ptr<uint32_t>(c->tiercaps), g_ntiers,
                                                  layout_bptr(c), ptr<uint64_t>(c->roff), ptr<uint4>(c->rowlists),
                                                  (uint32_t*)(ptr<uint4>(c->rowlists) + (size_t)kNumTiers * nr), d_ctl + kCtlTierCnt,
                                                  (unsigned long long*)(d_ctl + kCtlTotals) + 1, ptr<uint64_t>(c->flopptr),
                                                  c->have_rowlists ? ptr<uint64_t>(c->Arow) : nullptr);
    KCHK(c);
    // The host needs two things from the symbolic kernels before it can launch the row kernels: the tiers' lengths (exact grids)
    // and the product total (buffer sizes).  Both are functions of the operands, the partition and the stage only, so they are
    // read back (96 bytes into pinned memory, one host round trip) the first time a pass runs on them and remembered; later
    // passes on the same operands enqueue everything without waiting.  The final control block is checked against them.
    uint32_t* const tcnt = c->pass_tcnt;
    if (!warm) {
        c->pass_known = false;
        HIPCHK(c, hipMemcpyAsync(c->pinned, d_ctl + kCtlTierCnt, 4 * (kCtlTotals + 8 - kCtlTierCnt), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memcpy(c->pass_tcnt, c->pinned, sizeof(c->pass_tcnt));
        std::memcpy(&c->pass_products, c->pinned + (kCtlTotals - kCtlTierCnt) + 2, 8);
        std::memcpy(c->pass_wide_products, c->pinned + (kCtlTotals - kCtlTierCnt) + 4, 16);
        std::memcpy(c->pass_sig, psig, sizeof(psig));
    }
    // the product-sized buffers follow THIS pass's product count (a column partition or a stage only pays for its share; the
    // reference sizes its stages from the same number, overlap.hpp:365-404,682-710); they only ever grow
    const uint64_t Fub = c->pass_products;
    ENSURE(c, c->tmp_pairs, sizeof(bella_pair) * Fub);
    if (want_ext) ENSURE(c, c->tmp_ext, sizeof(bella_pair_ext) * Fub);
    ENSURE(c, c->plist_hv, 8 * Fub);
    ENSURE(c, c->overflow, 16 * ((Fub >> 4) + 64));   // a pair on this list has > 16 products
    ENSURE(c, c->sortscr, 2 * Fub);
    ENSURE(c, c->pairs, sizeof(bella_pair) * Fub);     // nnz(C) <= products
    if (want_ext) ENSURE(c, c->ext, sizeof(bella_pair_ext) * Fub);
    EVREC(3);

    SpgemmArgs a;
    a.Bptr = layout_bptr(c);
    a.Bent = ptr<uint2>(c->Bent);
    a.inl = c->layout_inline;
    a.Aent = ptr<uint2>(c->Aent);
    a.Aent2 = c->have_rowlists ? ptr<uint2>(c->Aent2) : nullptr;
    a.Aov = c->have_rowlists ? ptr<uint16_t>(c->Aov) : nullptr;
    a.Arow = c->have_rowlists ? ptr<uint64_t>(c->Arow) : nullptr;
    a.roff = ptr<uint64_t>(c->roff);
    a.packed = ptr<uint32_t>(c->packed);
    a.flopptr = ptr<uint64_t>(c->flopptr);
    a.flops = ptr<uint32_t>(c->flopsr);
    a.tmp_pairs = ptr<bella_pair>(c->tmp_pairs);
    a.tmp_ext = want_ext ? ptr<bella_pair_ext>(c->tmp_ext) : nullptr;
    a.nnzC = ptr<uint32_t>(c->nnzC);
    a.plist = ptr<uint2>(c->plist_hv);
    a.overflow = ptr<uint4>(c->overflow);
    a.ctl = ptr<uint32_t>(c->ctl);
    a.retry = ptr<uint32_t>(c->retry);
    a.nrows_dev = nullptr;
    a.ws = ptr<uint8_t>(c->ws);
    a.ws_stride = ws_stride;
    a.nrows = 0;
    a.k = p->kmer_size;
    a.binSize = p->bin_size;
    a.inject_unordered = (c->debug & 4u) ? 1 : 0;
#ifdef BELLA_DEV_PROF
    ENSURE(c, c->prof, 8 * 10 * kNumTiers);
    HIPCHK(c, hipMemsetAsync(c->prof.p, 0, 8 * 10 * kNumTiers, c->stream));
    a.prof = nullptr;
    a.stop_phase = getenv("BELLA_DEV_STOP") ? atoi(getenv("BELLA_DEV_STOP")) : -1;
#endif
    // LDS classes: consecutive tiers whose workgroups take the same share of a CU; one launch per class (largest class first, on
    // side streams so that the classes overlap; the class of the smallest columns, which finishes last, on the main stream), and
    // the global-workspace tier.
    auto dcap_of = [&](uint32_t cap) -> uint32_t {
        const bool half = (half_tables || (c->debug & 16u)) && cap <= kHalfTableMaxCap;     // debug bit 4: tests
        // pair-rich inputs: the smallest columns are almost all chance pairs (one product each): their tier gets a full-size table
        if (half_tables && cap <= kFullTableMaxCap) return cap;
        return half ? cap / 2 : cap / 4;
    };
    nl = 0;
    {
        int cls_prev = -1;
        for (int t = 0; t + 1 < (int)g_ntiers; ++t) {
            const size_t lds = row_mem_bytes(tier_caps[t], dcap_of(tier_caps[t]), true);
            int cls = (int)kNumClasses - 1;
            for (int k2 = 0; k2 < (int)kNumClasses; ++k2)
                if (lds <= kClassLds[k2]) { cls = k2; break; }
            if (cls != cls_prev || nl == 0) { ln[nl++] = Launch{t, t, lds, 0, cls}; cls_prev = cls; }
            ln[nl - 1].hi = t;
            ln[nl - 1].lds = lds;                                 // the class is carved for its largest tier
            ln[nl - 1].rows += tcnt[t];
        }
    }
    // Streams: at most four run concurrently on this device (hardware queues), and a workgroup of the whole-CU class only starts
    // on an EMPTY CU.  So the whole-CU class (few columns, if any) is launched first, on side stream 0, and takes its CUs before the
    // others arrive; then the next classes go to the remaining side streams, the global-workspace tier to side stream 2, and the
    // class of the smallest columns (it finishes last) stays on the main stream.
    int main_l = -1;
    for (int l = 0; l < nl; ++l) if (ln[l].rows) { main_l = l; break; }
    // The columns above the LDS tiers (<= 65,535 products): a handful runs on the global-workspace path next to the LDS classes; when
    // a pass has many of them (HiFi-like inputs, deep coverage) they join the wide columns on the sort-based path of wide.hpp, which
    // works at HBM speed instead of L2 latency (debug bit 5: tests, any number of them).
    const uint32_t n_mid = tcnt[g_ntiers - 1];
    const bool mid_to_wide = !force_global && n_mid != 0 && (n_mid >= kMidToWideMin || (c->debug & 32u));
    const bool global_tier = n_mid != 0 && !mid_to_wide;
    bool used[3] = {};
    auto side_stream = [&](int which) -> int {                    // first use: make the stream wait for what the main stream did so far
        // (the fork point is ev[3], recorded on the main stream right after the symbolic kernels: no event of its own)
        if (!used[which]) { HIPCHK(c, hipStreamWaitEvent(c->side[which], c->ev[3], 0)); used[which] = true; }
        return 0;
    };
    a.rowlist = nullptr;
    a.nrows_dev = nullptr;
    a.nreads = nr;
    int nside = 0;                                                // classes launched off the main stream so far
    auto launch_class = [&](int l, bool on_main) -> int {
        hipStream_t sst = c->stream;
        if (!on_main) {
            const int which = nside;                              // 0, 1, 2: one class each
            int r2 = side_stream(which);
            if (r2) return r2;
            sst = c->side[which];
            nside++;
        }
        a.rowlist = nullptr;
        a.nrows_dev = nullptr;
        a.rowdesc = ptr<uint4>(c->rowlists);
        a.tier_lo = (uint32_t)ln[l].lo;
        a.tier_hi = (uint32_t)ln[l].hi;
        a.tcount_valid = ln[l].hi - ln[l].lo <= 3 ? 1u : 0u;
        for (int k2 = 0; k2 < 4; ++k2) a.tcount[k2] = ln[l].lo + k2 <= ln[l].hi ? tcnt[ln[l].lo + k2] : 0u;
        a.nrows = ln[l].rows;
        a.cap = tier_caps[ln[l].hi];
        a.dcap = dcap_of(a.cap);
        const size_t lds = ln[l].lds;
        const int blk = (c->debug & 8u) ? 512 : kClassBlock[ln[l].cls];     // debug bit 3: tests, 512 threads everywhere
        int ki;
        void (*kern)(SpgemmArgs);
        const bool rl = c->have_rowlists;
        const bool pe = c->layout_products && !rl;                // B' with one entry per product: the instantiations without an expansion phase
#define BELLA_ROWS_KERN(NX, B) (rl ? k_spgemm_rows_lds<NX, B, true> : pe ? k_spgemm_rows_lds<NX, B, false, true> : k_spgemm_rows_lds<NX, B, false>)
        if (blk == 512) {
            ki = a.cap <= 8 * 512 ? 0 : a.cap <= 16 * 512 ? 1 : 2;
            kern = ki == 0 ? BELLA_ROWS_KERN(8, 512) : ki == 1 ? BELLA_ROWS_KERN(16, 512) : BELLA_ROWS_KERN(22, 512);
        } else if (blk == 1024) {
            ki = a.cap <= 4 * 1024 ? 3 : a.cap <= 8 * 1024 ? 4 : 5;
            kern = ki == 3 ? BELLA_ROWS_KERN(4, 1024) : ki == 4 ? BELLA_ROWS_KERN(8, 1024) : BELLA_ROWS_KERN(11, 1024);
        } else if (blk == 256 && a.cap <= 6 * 256) {              // cap <= 1394 <= 6 * 256
            ki = 6;
            kern = BELLA_ROWS_KERN(6, 256);
        } else if (blk == 256) {                                  // cap <= 2752 <= 11 * 256
            ki = 7;
            kern = BELLA_ROWS_KERN(11, 256);
        } else if (blk == 128) {                                  // cap <= 689 <= 6 * 128
            ki = 8;
            kern = BELLA_ROWS_KERN(6, 128);
        } else if (a.cap <= 11 * 64) {                            // ONE wavefront per column (no workgroup barriers): cap <= 689 <= 11 * 64
            ki = 18;
            kern = BELLA_ROWS_KERN(11, 64);
        } else {                                                  // cap <= 1394 <= 22 * 64
            ki = 19;
            kern = BELLA_ROWS_KERN(22, 64);
        }
#undef BELLA_ROWS_KERN
        if (rl) ki += ki >= 18 ? 2 : 9;
        else if (pe) ki += ki >= 18 ? 13 : 22;
        if (lds > c->lds_attr[ki]) {                             // once per kernel and size, not per launch
            HIPCHK(c, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            c->lds_attr[ki] = lds;
        }
#ifdef BELLA_DEV_PROF
        a.prof = (unsigned long long*)c->prof.p + 10 * l;
        {   // development builds only: leave classes out (timing experiments; the results are then incomplete)
            static const int skip = getenv("BELLA_DEV_SKIP_CLASSES") ? atoi(getenv("BELLA_DEV_SKIP_CLASSES")) : 0;
            if (skip & (1 << l)) { a.prof = nullptr; return 0; }
        }
#endif
        kern<<<ln[l].rows, blk, lds, sst>>>(a);
#ifdef BELLA_DEV_PROF
        a.prof = nullptr;
#endif
        KCHK(c);
        launches++;
        return 0;
    };
    // The wide path's first part goes BEFORE the row kernels when it is a large part of the pass (long-list inputs: HiFi-like reads with
    // a raised -u): its small kernels and the first grouping pass start at once instead of behind the classes' queues (five streams on
    // four hardware queues: every small kernel waited ~40 us for its turn, 0.3 ms before the first grouping pass began), the rest
    // follows when the classes are enqueued.  Otherwise (a few wide columns in a pass of LDS columns) the classes go first as before.
    c->n_wide = tcnt[g_ntiers] + (mid_to_wide ? n_mid : 0);
    uint32_t* const widelist = (uint32_t*)(ptr<uint4>(c->rowlists) + (size_t)kNumTiers * nr);
    const uint64_t wide_products = c->pass_wide_products[1] + (mid_to_wide ? c->pass_wide_products[0] : 0);
    auto wide_columns = [&]() -> int {                             // (the columns above the LDS tiers join the wide columns' list)
        if (mid_to_wide) {
            k_desc_cols<<<nblk(n_mid), 256, 0, c->stream>>>(ptr<uint4>(c->rowlists) + (size_t)(g_ntiers - 1) * nr, n_mid, widelist + tcnt[g_ntiers]);
            if (hipGetLastError() != hipSuccess) return fail(c, BELLA_ERR_HIP, "k_desc_cols launch failed");
        }
        return 0;
    };
    WideBatch wide_batch;
    bool wide_begun = false;
    if (c->n_wide && wide_products && wide_products <= c->wide_budget && wide_products * 4 >= c->pass_products) {
        hipStream_t const main_stream = c->stream, wst = c->side[kNumTiers];
        HIPCHK(c, hipStreamWaitEvent(wst, c->ev[3], 0));
        c->stream = wst;
        int rw = wide_columns();
        if (!rw) rw = wide_batch_begin(c, a, c->n_wide, widelist, wide_products, wide_batch);
        c->stream = main_stream;
        if (rw) { (void)hipStreamSynchronize(wst); return rw; }
        wide_begun = true;
    }
    auto whole_cu = [&](int l) { return 2 * ln[l].lds > kClassLds[kNumClasses - 1]; };
    // the whole-CU class (few columns, if any) goes FIRST, on a side stream of its own: its workgroups take their CUs before the other
    // classes' workgroups arrive, and those fill the rest of the chip next to it instead of waiting behind it
    int nwhole = 0;
    for (int l = nl - 1; l >= 0; --l)
        if (ln[l].rows && whole_cu(l) && l != main_l && nwhole == 0) { rc = launch_class(l, false); if (rc) return rc; nwhole++; }
        else if (ln[l].rows && whole_cu(l) && l != main_l) { rc = launch_class(l, true); if (rc) return rc; }
    if (global_tier) {                                            // the columns above the LDS tiers (or all of them: debug bit 0)
        hipStream_t sst = c->stream;
        if (main_l >= 0) { rc = side_stream(2); if (rc) return rc; sst = c->side[2]; }      // (launch_class uses sides 0, 1 then)
        a.rowdesc = ptr<uint4>(c->rowlists) + (size_t)(g_ntiers - 1) * nr;
        a.nrows = tcnt[g_ntiers - 1];
        a.cap = tier_caps[g_ntiers - 1];
        a.dcap = a.cap;
        const unsigned grid = a.nrows < kGlobalGrid ? a.nrows : kGlobalGrid;
        if (c->have_rowlists) k_spgemm_rows_global<true><<<grid, kGlobalBlock, 0, sst>>>(a);
        else k_spgemm_rows_global<false><<<grid, kGlobalBlock, 0, sst>>>(a);
        KCHK(c);
        launches++;
    }
    {   // the three largest remaining classes each get a side stream; what is left (the classes of the smallest columns) runs on
        // the main stream, larger class first
        int side_left = 3 - nwhole - (global_tier ? 1 : 0);
        for (int l = nl - 1; l >= 0; --l) {
            if (!ln[l].rows || (whole_cu(l) && l != main_l)) continue;
            int later = 0;                                        // non-empty classes below this one
            for (int m2 = 0; m2 < l; ++m2) later += ln[m2].rows ? 1 : 0;
            const bool on_main = l == main_l || side_left == 0 || later == 0;
            if (!on_main) side_left--;
            rc = launch_class(l, on_main);
            if (rc) return rc;
        }
    }
    // The columns of the sort-based path (wide.hpp) are other columns than the LDS classes': the path -- host-driven, several
    // synchronisations -- runs on a stream of its own NEXT to the class launches above instead of after them (HiFi-like input with a
    // raised -u, 10k reads: the classes take 1.35 ms of a pass whose wide path takes 8.7)
    if (c->n_wide) {
        hipStream_t const main_stream = c->stream, wst = c->side[kNumTiers];
        c->stream = wst;                                           // (everything run_wide enqueues, allocates for and waits on)
        int rw = 0;
        if (wide_begun) rw = wide_batch_finish(c, wide_batch, false);
        else {
            HIPCHK(c, hipStreamWaitEvent(wst, c->ev[3], 0));
            rw = wide_columns();
            if (!rw) rw = run_wide(c, a, c->n_wide, widelist, wide_products);
        }
        c->stream = main_stream;
        if (rw) { (void)hipStreamSynchronize(wst); return rw; }
        HIPCHK(c, hipEventRecord(c->join[kNumTiers], wst));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->join[kNumTiers], 0));
    }
    for (int w = 0; w < 3; ++w)
        if (used[w]) {
            HIPCHK(c, hipEventRecord(c->join[w], c->side[w]));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->join[w], 0));
        }
    FoldArgs fa;
    fa.ctl = a.ctl;
    fa.overflow = a.overflow;
    fa.flopptr = a.flopptr;
    fa.plist = a.plist;
    fa.roff = a.roff;
    fa.packed = a.packed;
    fa.tmp_pairs = a.tmp_pairs;
    fa.tmp_ext = a.tmp_ext;
    fa.sort_scratch = ptr<uint16_t>(c->sortscr);
    fa.k = a.k;
    fa.binSize = a.binSize;
    auto rerun_columns = [&]() -> int {
        a.rowlist = ptr<uint32_t>(c->retry);
        a.rowdesc = nullptr;
        a.nrows_dev = ptr<uint32_t>(c->ctl) + kCtlRetry;
        if (c->have_rowlists) k_spgemm_rows_global<true><<<kRerunGrid, kGlobalBlock, 0, c->stream>>>(a);
        else k_spgemm_rows_global<false><<<kRerunGrid, kGlobalBlock, 0, c->stream>>>(a);   // (the list is usually empty or a handful of columns)
        KCHK(c);
        return 0;
    };
    auto finish = [&]() -> int {                                  // colptrC, slot order + move to the final place, the pass's host round trip
        if ((uint64_t)nr + 1 <= kScanSingleMax) {
            k_scan_counts<<<1, 1024, 0, c->stream>>>(ptr<uint32_t>(c->nnzC), ptr<uint64_t>(c->colptrC), nr + 1);
            KCHK(c);
        } else {
            hipcub::TransformInputIterator<uint64_t, CountU64, const uint32_t*> it(ptr<uint32_t>(c->nnzC), CountU64());
            size_t tb = c->cubtmp.cap;
            HIPCHK(c, hipcub::DeviceScan::ExclusiveSum(c->cubtmp.p, tb, it, ptr<uint64_t>(c->colptrC), (int)nr + 1, c->stream));
        }
        EVREC(6);
        if (nr) {
            OrderArgs oa;
            oa.flopptr = ptr<uint64_t>(c->flopptr); oa.colptrC = ptr<uint64_t>(c->colptrC); oa.nnzC = ptr<uint32_t>(c->nnzC);
            oa.flops = ptr<uint32_t>(c->flopsr);
            oa.nreads = nr; oa.i0 = i0; oa.stride = c->part_stride; oa.nown = nown;
            oa.tmp_pairs = ptr<bella_pair>(c->tmp_pairs); oa.tmp_ext = want_ext ? ptr<bella_pair_ext>(c->tmp_ext) : nullptr;
            oa.pairs = ptr<bella_pair>(c->pairs); oa.ext = want_ext ? ptr<bella_pair_ext>(c->ext) : nullptr;
            oa.totals = (uint64_t*)(d_ctl + kCtlTotals);
            oa.nbig = d_ctl + kCtlOrderBig; oa.biglist = ptr<uint32_t>(c->orderlist); oa.ws = ptr<uint8_t>(c->order_ws);
            // two instances share the columns by table size (the small one keeps more columns in flight per CU: tuned at 100k reads);
            // on a small pass the second launch costs more than it buys (10k reads: two launches and the gap between them for 0.3 M
            // records), so one instance takes all tables up to 1,024 slots there
            if (nown <= c->tune_order_split) {
                k_order_wave<kOrderWaveHt, 0><<<nblk(nown ? nown : 1, kOrderBlock / 64), kOrderBlock, 0, c->stream>>>(oa);
                KCHK(c);
            } else {
                k_order_wave<512, 0><<<nblk(nown ? nown : 1, kOrderBlock / 64), kOrderBlock, 0, c->stream>>>(oa);
                KCHK(c);
                k_order_wave<kOrderWaveHt, 512><<<nblk(nown ? nown : 1, kOrderBlock / 64), kOrderBlock, 0, c->stream>>>(oa);
                KCHK(c);
            }
            // columns with more than 1,024 pairs: a warm pass whose predecessor had none leaves the kernel out and checks the count in the
            // final control block (like the rerun and overflow kernels above)
            if (!skip_big) {
                k_order_block<<<kOrderBigGrid, kOrderBlock, (size_t)6 * kOrderLdsHt, c->stream>>>(oa);
                KCHK(c);
            }
        }
        EVREC(7);
        HIPCHK(c, hipMemcpyAsync(ctl_host, d_ctl, 4 * kCtlWords, hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    if (!skip_rare) { rc = rerun_columns(); if (rc) return rc; }
    EVREC(5);
    // the row kernels fold every pair themselves; only pairs that end with > 16 bins are left (their count stays on the device)
    if (!skip_rare) { k_fold_overflow<<<256, 64, 0, c->stream>>>(fa); KCHK(c); EVREC(8); }
    return finish();
    };   // enqueue
#undef EVREC
    // (Capturing the warm pass into a hipGraph and replaying it was measured: 0.54 ms per step against 0.41 ms for these direct
    // launches at 10k reads -- the multi-branch graph replays slower on ROCm 7.2 than the host can issue the launches.)
    rc = enqueue();
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((skip_rare && (ctl_host[kCtlRetry] || ctl_host[kCtlOverflow])) || (skip_big && ctl_host[kCtlOrderBig])) {   // the pass needed the kernels it left out: once more, with them
        c->pass_rare_free = false;
        c->pass_big_free = false;
        if (depth > 0) return fail(c, BELLA_ERR_STATE, "internal: rare kernels still skipped");
        return run_spgemm(c, p, status_out, depth + 1);
    }
    const uint32_t* const tcnt = c->pass_tcnt;
    const uint64_t Fub = c->pass_products;
    uint64_t P = 0, F = 0;
    std::memcpy(&P, ctl_host + kCtlTotals, 8);
    std::memcpy(&F, ctl_host + kCtlTotals + 2, 8);
    rc = status_to_error(c, ctl_host[kCtlStatus] & ~1u);
    if (rc) return rc;
    *status_out = ctl_host[kCtlStatus];
    c->n_overflow = ctl_host[kCtlOverflow];
    c->n_retry = ctl_host[kCtlRetry];
    c->npairs = P;
    c->flops = F;
    if (F != Fub || std::memcmp(ctl_host + kCtlTierCnt, tcnt, 4 * (g_ntiers + 1)) != 0) {
        c->pass_known = false;
        return fail(c, BELLA_ERR_STATE, "internal: product total %llu / tier lengths differ from the ones the pass was sized with (%llu)",
                    (unsigned long long)F, (unsigned long long)Fub);
    }
    c->pass_known = true;
    c->pass_rare_free = c->n_retry == 0 && c->n_overflow == 0 && c->n_wide == 0;
    c->pass_big_free = ctl_host[kCtlOrderBig] == 0;
    c->tm.symbolic_ms = ev_ms(c->ev[2], c->ev[3]);
    c->tm.spgemm_ms = ev_ms(c->ev[3], c->ev[5]);
    c->tm.fold_ms = skip_rare ? 0.f : ev_ms(c->ev[5], c->ev[8]);
    c->tm.compact_ms = ev_ms(c->ev[6], c->ev[7]);
    c->tm.overlap_total_ms = ev_ms(c->ev[2], c->ev[7]);
    c->tm.spgemm_launches = launches;
    c->tm.retry_columns = c->n_retry;
    c->tm.overflow_pairs = c->n_overflow;
#ifdef BELLA_DEV_PROF
    {
        unsigned long long ph[10 * kNumTiers];
        HIPCHK(c, hipMemcpy(ph, c->prof.p, sizeof(ph), hipMemcpyDeviceToHost));
        static const char* nm[9] = {"expand", "gather+insert", "count-scan", "scatter+singles", "rank/overlay", "parents", "walks", "emit", "head (descriptor + first entries + table init)"};
        for (int l = 0; l < nl; ++l) {
            const unsigned long long* q = ph + 10 * l;
            if (!q[9]) continue;
            double tot = 1e-9;
            for (int n = 0; n < 9; ++n) tot += (double)q[n];
            fprintf(stderr, "[bella_hip prof] class cap %u (%llu columns, %.0f cycles each):", tier_caps[ln[l].hi], q[9], tot / (double)q[9]);
            for (int n = 0; n < 9; ++n) fprintf(stderr, " %s %.1f%%", nm[n], 100.0 * (double)q[n] / tot);
            fprintf(stderr, "\n");
        }
    }
#endif
    return 0;
}

// the columns of this context under the current partition and stage: i0 + j * stride, j < nown
static uint32_t owned_columns(const bella_ctx* c, uint32_t* i0_out) {
    const uint32_t nr = c->nreads;
    const uint32_t hi = c->range_hi < nr ? c->range_hi : nr;
    uint32_t i0 = c->range_lo + (c->part_first + c->part_stride - c->range_lo % c->part_stride) % c->part_stride;
    const uint32_t nown = i0 < hi ? (hi - i0 + c->part_stride - 1) / c->part_stride : 0;
    if (!nown) i0 = 0;
    if (i0_out) *i0_out = i0;
    return nown;
}

int bella_hip_overlap(bella_ctx* c, const bella_params* p, uint64_t* npairs, uint64_t* flops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, MATRIX)) return r;
    int rc = check_params(c, p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, PAIRS);
    rc = layout_for_partition(c);
    if (rc) return rc;
    uint32_t st = 0;
    rc = run_spgemm(c, p, &st);
    if (rc == BELLA_ERR_NOMEM && c->have_rowlists) {
        // the row lists are optional: give their memory to the pass and let it expand the products itself
        (void)hipDeviceSynchronize();
        release(c->Aent2); release(c->Aov); release(c->Arow);
        c->have_rowlists = false;
        c->layout_gen++;
        c->pass_known = false;
        rc = run_spgemm(c, p, &st);
    }
    if (rc) { (void)hipDeviceSynchronize(); return rc; }     // side-stream kernels of the pass may still be in flight
    if (st & 1u) return fail(c, BELLA_ERR_BINS, "internal: > 16 bins without sort scratch");
    made(c, PAIRS);
    c->tm.numeric_passes++;
    c->tm.numeric_columns += owned_columns(c, nullptr);
    if (npairs) *npairs = c->npairs;
    if (flops) *flops = c->flops;
    return 0;
}

// the symbolic phase alone (spgemm.hpp: k_count_pairs)
int bella_hip_count_pairs(bella_ctx* c, const bella_params* p, uint64_t* colptrC, uint64_t* npairs, uint64_t* flops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, MATRIX)) return r;
    int rc = check_params(c, p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = layout_for_partition(c);
    if (rc) return rc;
    const uint32_t nr = c->nreads;
    ENSURE(c, c->flopsr, 4 * ((size_t)nr + 2));
    ENSURE(c, c->nnzC, 4 * ((size_t)nr + 2));
    ENSURE(c, c->colptrC, 8 * ((size_t)nr + 2));
    ENSURE(c, c->ctl, 4 * kCtlWords);
    std::memset(c->sym_sig, 0, sizeof(c->sym_sig));          // (the next numeric pass clears flops / nnzC for itself)
    changed(c, MATRIX);
    HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    HIPCHK(c, hipMemsetAsync(c->flopsr.p, 0, 4 * ((size_t)nr + 2), c->stream));
    HIPCHK(c, hipMemsetAsync(c->nnzC.p, 0, 4 * ((size_t)nr + 2), c->stream));
    HIPCHK(c, hipMemsetAsync(c->ctl.p, 0, 4 * kCtlWords, c->stream));
    uint32_t i0 = 0;
    const uint32_t nown = owned_columns(c, &i0);
    if (!colptrC && !npairs) {
        // estimateFLOP alone (overlap.hpp:157-202): the products per column were summed when the operands were laid out (rowF), no gather at all
        if (nown && c->have_rowlists) {
            k_row_flops_rl<<<nblk(nown), kBlock, 0, c->stream>>>(ptr<uint64_t>(c->Arow), i0, c->part_stride, nown, ptr<uint32_t>(c->flopsr), ptr<uint32_t>(c->nnzC), ptr<uint32_t>(c->ctl));
            KCHK(c);
        } else if (nown) {
            k_row_flops<<<nblk(nown), kBlock, 0, c->stream>>>(ptr<uint32_t>(c->rowF), i0, c->part_stride, nown, ptr<uint32_t>(c->flopsr),
                                                              ptr<uint32_t>(c->nnzC), ptr<uint32_t>(c->ctl));
            KCHK(c);
        }
        hipcub::TransformInputIterator<uint64_t, CastU64, const uint32_t*> it(ptr<uint32_t>(c->flopsr), CastU64());
        uint64_t* d_sum = ptr<uint64_t>(c->colptrC);
        CUB_SLACK(c, 256, hipcub::DeviceReduce::Sum, it, d_sum, (int)nr + 1, c->stream);
        uint64_t F = 0;
        HIPCHK(c, hipMemcpyAsync(&F, d_sum, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (flops) *flops = F;
        return 0;
    }
    if (nown) {
        CountArgs a;
        a.Bptr = layout_bptr(c); a.Bent = ptr<uint2>(c->Bent); a.Aent = ptr<uint2>(c->Aent); a.inl = c->layout_inline;
        a.Aent2 = c->have_rowlists ? ptr<uint2>(c->Aent2) : nullptr;
        a.Arow = c->have_rowlists ? ptr<uint64_t>(c->Arow) : nullptr;
        a.i0 = i0; a.stride = c->part_stride; a.nown = nown;
        a.words = (nr + 31) / 32;
        a.nnzC = ptr<uint32_t>(c->nnzC); a.flops = ptr<uint32_t>(c->flopsr);
        a.totals = (unsigned long long*)(ptr<uint32_t>(c->ctl) + kCtlTotals);
        const size_t map_bytes = 4 * (size_t)a.words;
        const bool in_lds = map_bytes <= 150 * 1024 && !(c->debug & 8192u);   // debug bit 13: tests, bitmaps in global memory
        if (in_lds) {
            // as many workgroups per CU as the bitmaps allow (at most 4 x 512 threads)
            const uint32_t per_cu = (uint32_t)std::min<size_t>(4, (160 * 1024) / (map_bytes + 64));
            const uint32_t grid = std::min<uint32_t>(nown, 256u * (per_cu ? per_cu : 1u));
            HIPCHK(c, hipFuncSetAttribute((const void*)k_count_pairs<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)map_bytes));
            a.gmap = nullptr;
            k_count_pairs<true><<<grid, kCountBlock, map_bytes, c->stream>>>(a);
        } else {
            const uint32_t grid = std::min<uint32_t>(nown, 1024u);
            ENSURE(c, c->ws, map_bytes * grid);
            a.gmap = ptr<uint32_t>(c->ws);
            k_count_pairs<false><<<grid, kCountBlock, 0, c->stream>>>(a);
        }
        KCHK(c);
    }
    {
        hipcub::TransformInputIterator<uint64_t, CountU64, const uint32_t*> it(ptr<uint32_t>(c->nnzC), CountU64());
        CUB_SLACK(c, 256, hipcub::DeviceScan::ExclusiveSum, it, ptr<uint64_t>(c->colptrC), (int)nr + 1, c->stream);
    }
    HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    uint64_t tot[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(tot, ptr<uint32_t>(c->ctl) + kCtlTotals, 16, hipMemcpyDeviceToHost, c->stream));
    if (colptrC) HIPCHK(c, hipMemcpyAsync(colptrC, c->colptrC.p, 8 * ((size_t)nr + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tm.symbolic_ms = ev_ms(c->ev[2], c->ev[3]);
    c->tm.symbolic_passes++;
    if (npairs) *npairs = tot[0];
    if (flops) *flops = tot[1];
    return 0;
}

static int get_memory_impl(bella_ctx* c, bella_memory* m);
// (the struct grew from 64 to 72 bytes between ABI versions 4 and 5 with no size handshake.)  The sized form writes at most
// struct_size bytes: a caller built against an older, shorter bella_memory gets the fields it knows and nothing behind its struct.
int bella_hip_get_memory_sized(bella_ctx* c, void* out, uint64_t struct_size) {
    if (!c || !out || struct_size < 8) return BELLA_ERR_BAD_ARG;
    bella_memory m{};
    const int rc = get_memory_impl(c, &m);
    if (rc) return rc;
    return put_sized(out, struct_size, m);
}
int bella_hip_get_memory(bella_ctx* c, bella_memory* m) { return get_memory_impl(c, m); }
static int get_memory_impl(bella_ctx* c, bella_memory* m) {
    if (!c || !m) return BELLA_ERR_BAD_ARG;
    auto sum = [](std::initializer_list<const Buf*> l) { uint64_t t = 0; for (const Buf* b : l) t += b->cap; return t; };
    m->reads_bytes = sum({&c->packed, &c->roff});
    m->matrix_bytes = sum({&c->Bptr, &c->Bk, &c->Bpos});
    m->layout_A_bytes = sum({&c->Aent});
    m->layout_B_bytes = sum({&c->Bent, &c->rowF, &c->Bloc});
    m->rowlist_bytes = sum({&c->Aent2, &c->Aov, &c->Arow});
    m->pass_bytes = sum({&c->flopsr, &c->flopptr, &c->nnzC, &c->colptrC, &c->rowlists, &c->tiercaps, &c->tmp_pairs, &c->tmp_ext, &c->pairs, &c->ext, &c->sortscr, &c->ws,
                         &c->cubtmp, &c->plist_hv, &c->overflow, &c->ctl, &c->retry, &c->orderlist, &c->order_ws, &c->w_f, &c->w_off, &c->w_key, &c->w_key2, &c->w_idx,
                         &c->w_idx2, &c->w_hv, &c->w_ovfl, &c->w_plist, &c->w_scr, &c->w_rlen, &c->w_rstart, &c->w_rrank, &c->w_redo, &c->w_segfirst, &c->w_toff, &c->w_table,
                         &c->w_nruns, &c->w_desc, &c->w_gtab, &c->w_gcount, &c->w_gbase, &c->w_rfirst, &c->w_aent2, &c->w_aov});
    m->other_bytes = sum({&c->t_kmer, &c->t_read, &c->t_pos, &c->tstart, &c->Bk_tmp, &c->Bpos_tmp, &c->rowcnt, &c->asm_ws, &c->asm_cls, &c->lk_key, &c->lk_key2, &c->lk_val,
                          &c->lk_val2, &c->lk_rinfo, &c->w, &c->wscan, &c->kc_nk, &c->kc_koff, &c->kc_hist, &c->kc_keys, &c->kc_alt, &c->kc_runlen, &c->kc_flag, &c->kc_slot, &c->kc_nruns,
                          &c->kc_dcode, &c->kc_dcount, &c->kc_hkey, &c->kc_hval, &c->kc_found, &c->kc_tstart, &c->kc_cursor, &c->kc_sel, &c->kc_ringo, &c->kc_ringp, &c->kc_opos, &c->kc_oid, &c->kc_opos2, &c->kc_oid2, &c->alns,
                          &c->seeds, &c->xest, &c->xest2, &c->xids, &c->xorder, &c->xres, &c->xstate, &c->xlive, &c->lg_res, &c->lg_redo, &c->lg_scratch, &c->status, &c->comm_meta});
    m->other_bytes += c->pool.bytes;                               // (released buffers waiting for the next request they fit)
    const bool layout = has(c, MATRIX);
    m->owned_nnz = layout ? c->owned_nnz : 0;
    m->layout_shared = layout && c->layout_dist;
    m->live_nnz = layout ? c->live_nnz : 0;
    return 0;
}

int bella_hip_get_pairs(bella_ctx* c, bella_pair* pairs, bella_pair_ext* ext, uint64_t* colptrC) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, PAIRS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (pairs && c->npairs)
        HIPCHK(c, c->stager.d2h(pairs, c->pairs.p, sizeof(bella_pair) * c->npairs, c->stream));
    if (ext && c->npairs) {
        if (c->debug & 2u) return fail(c, BELLA_ERR_STATE, "pair_ext output disabled by debug flag");
        HIPCHK(c, c->stager.d2h(ext, c->ext.p, sizeof(bella_pair_ext) * c->npairs, c->stream));
    }
    if (colptrC)
        HIPCHK(c, hipMemcpyAsync(colptrC, c->colptrC.p, 8 * ((size_t)c->nreads + 1), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// the exact gapped X-drop of the reference's CUDA build (logan.hpp): one wavefront per extension, LDS rings; the rare extension
// whose band outgrows them is redone on rings in HBM
static int run_logan(bella_ctx* c, const bella_params* p, const bella_seed* d_seeds, const bella_pair* d_pairs, uint64_t n, bella_aln* d_out) {
    if (2 * n >= 0xFFFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "too many pairs for one batch (2^31; the redo list indexes extensions with 32 bits)");
    LoganArgs a;
    a.seeds = d_seeds; a.pairs = d_pairs; a.n = n;
    a.packed = ptr<uint32_t>(c->packed); a.roff = ptr<uint64_t>(c->roff);
    a.k = p->kmer_size; a.xdrop = p->xdrop;
    const double p_mat = pow(1 - p->error_rate, 2), p_mis = 1 - p_mat;
    a.ratiophi = 1.0 * p_mat - 1.0 * p_mis;
    a.delta = p->delta_chernoff;
    a.out = d_out;
    ENSURE(c, c->lg_res, 16 * (2 * n + 1));
    ENSURE(c, c->lg_redo, 4 * (2 * n + 2));
    a.res = ptr<int4>(c->lg_res);
    a.redo = ptr<uint32_t>(c->lg_redo) + 1;
    a.nredo = ptr<uint32_t>(c->lg_redo);
    a.scratch = nullptr; a.scratch_cap = 0;
    HIPCHK(c, hipEventRecord(c->ev[8], c->stream));
    if (n) {
        HIPCHK(c, hipMemsetAsync(a.nredo, 0, 4, c->stream));
        // one 64-thread workgroup per extension; grid x block must stay below 2^32 threads: chunks of 2^24 extensions
        HIPCHK(c, hipMemsetAsync(ptr<uint32_t>(c->status) + 14, 0, 4, c->stream));
        a.status = ptr<uint32_t>(c->status) + 14;
        const uint64_t kChunk = (c->debug & 256u) ? 1000ull : (1ull << 24);   // debug bit 8: tests, tiny chunks
        for (uint64_t eb = 0; eb < 2 * n; eb += kChunk) {
            a.ebase = eb;
            const uint64_t cnt = 2 * n - eb < kChunk ? 2 * n - eb : kChunk;
            k_logan_lds<<<(unsigned)cnt, 64, 0, c->stream>>>(a);
            KCHK(c);
        }
        uint32_t nredo = 0;
        HIPCHK(c, hipMemcpyAsync(&nredo, a.nredo, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nredo) {
            uint32_t longest = 0;
            for (uint32_t l : c->host_lens) longest = l > longest ? l : longest;
            const uint32_t cap = longest + 8;                     // a band is never wider than the shorter sequence (+ the rings' slack)
            const unsigned grid = nredo < 256u ? nredo : 256u;
            ENSURE(c, c->lg_scratch, (size_t)grid * 3 * cap * 2);
            a.scratch = ptr<int16_t>(c->lg_scratch);
            a.scratch_cap = cap;
            k_logan_hbm<<<grid, 64, 0, c->stream>>>(a);
            KCHK(c);
        }
        k_logan_finish<<<nblk(n), 256, 0, c->stream>>>(a);
        KCHK(c);
        uint32_t lst = 0;
        HIPCHK(c, hipMemcpyAsync(&lst, a.status, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (lst & 512u) return fail(c, BELLA_ERR_STATE, "internal: an extension's band outgrew the rings in HBM");
    }
    HIPCHK(c, hipEventRecord(c->ev[9], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[9]));
    c->tm.xdrop_ms = ev_ms(c->ev[8], c->ev[9]);
    return 0;
}

static int run_xdrop(bella_ctx* c, const bella_params* p, const bella_seed* d_seeds, const bella_pair* d_pairs, uint64_t n,
                     bella_aln* d_out) {
    XdropArgs a;
    a.seeds = d_seeds;
    a.pairs = d_pairs;
    a.n = n;
    a.packed = ptr<uint32_t>(c->packed);
    a.roff = ptr<uint64_t>(c->roff);
    a.k = p->kmer_size;
    a.xdrop = p->xdrop;
    a.out = d_out;
    // ratiophi = slope(e) (align.hpp:72-80), computed in double on the host exactly as main.cpp:323 does
    const double p_mat = pow(1 - p->error_rate, 2), p_mis = 1 - p_mat;
    a.ratiophi = 1.0 * p_mat - 1.0 * p_mis;
    a.delta = p->delta_chernoff;
    HIPCHK(c, hipEventRecord(c->ev[8], c->stream));
    if (n) {
        if (c->xdrop_variant == 3) {
            k_xdrop<<<nblk(n, kXdropPairsPerBlock), kXdropBlock, 0, c->stream>>>(a);
            KCHK(c);
        } else if (c->xdrop_variant == 2) {
            k_xdrop_packed<<<nblk(n, kXdropPairsPerBlock), kXdropBlock, 0, c->stream>>>(a);
            KCHK(c);
        } else {
            // plan -> sort extensions by their step bound (longest first) -> run -> combine
            const uint64_t ne = 2 * n;
            ENSURE(c, c->xest, 4 * ne);
            ENSURE(c, c->xest2, 4 * ne);
            ENSURE(c, c->xids, 4 * ne);
            ENSURE(c, c->xorder, 4 * ne);
            ENSURE(c, c->xres, 16 * ne);
            XdropSortedArgs sa;
            sa.a = a;
            sa.est = ptr<uint32_t>(c->xest);
            sa.ids = ptr<uint32_t>(c->xids);
            sa.order = ptr<uint32_t>(c->xorder);
            sa.res = ptr<int4>(c->xres);
            HIPCHK(c, hipMemsetAsync(c->xres.p, 0xFF, 16 * ne, c->stream));   // (a result nobody wrote is not a result of an earlier call)
            k_xdrop_plan<<<nblk(ne), 256, 0, c->stream>>>(sa);
            KCHK(c);
            CUB(c, hipcub::DeviceRadixSort::SortPairsDescending, ptr<uint32_t>(c->xest), ptr<uint32_t>(c->xest2), ptr<uint32_t>(c->xids), ptr<uint32_t>(c->xorder),
                (int)ne, 0, 18, c->stream);
            // In one launch a wavefront runs until its longest lane ends; chance pairs (one shared k-mer: 92 % of the pairs of the 100k-read
            // set) end long before the step bound they are scheduled by, and their wavefronts idle behind the few lanes that run on: 5.2 s
            // against 3.1 s in slices on the 100k set, 75.3 against 71.4 ms on the 10k set.
            const bool one_launch = c->xdrop_variant == 0;
            if (one_launch) {                                      // a wavefront runs until its longest lane ends
                k_xdrop_sorted<<<nblk(ne, kXdropBlock), kXdropBlock, 0, c->stream>>>(sa);
                KCHK(c);
            } else {
                // slices (xdrop_packed.hpp): the state of the live extensions lives in HBM between launches of at most kXdropSlice steps;
                // every launch runs full wavefronts of survivors.  Batches bound the state memory (288 B per extension).
                // (at most 16 M extensions = 4.8 GB, at most a quarter of the free device memory, at least 64 k; an allocation that
                // fails all the same halves the batch, and below 64 k extensions the one-launch kernel, which needs no state, takes over)
                // (BELLA_TUNE_XDROP_BATCH: the capacity as given -- tests run several batches on small inputs)
                uint64_t capB = ne < (16ull << 20) ? ne : (16ull << 20);
                if (c->tune_xdrop_batch) capB = ne < c->tune_xdrop_batch ? ne : c->tune_xdrop_batch;
                else {
                    size_t mfree = 0, mtotal = 0;
                    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) {
                        const uint64_t held = c->xstate.cap + c->xlive.cap + c->pool.bytes + c->pool.arena.largest_hole();   // (one buffer: the slab's largest hole, not the sum of its holes)
                        const uint64_t fit = ((uint64_t)mfree + held) / 4 / (4 * (uint64_t)kXStateWords + 8);
                        if (capB > fit) capB = fit;
                    }
                    if (capB < (64ull << 10)) capB = ne < (64ull << 10) ? ne : (64ull << 10);
                }
                bool have_state = false;
                for (;;) {
                    if (!ensure_bytes(c, c->xstate, 4 * (size_t)kXStateWords * capB) && !ensure_bytes(c, c->xlive, 2 * 4 * capB + 64)) { have_state = true; break; }
                    if (capB <= (64ull << 10)) break;
                    capB >>= 1;
                }
                if (!have_state) {
                    c->err.clear();
                    release(c->xstate); release(c->xlive);
                    k_xdrop_sorted<<<nblk(ne, kXdropBlock), kXdropBlock, 0, c->stream>>>(sa);
                    KCHK(c);
                } else {
                // Classes: the extensions are sorted by their step estimate, longest first.  Advanced together -- one slice per ROUND of
                // the whole batch -- the longest ones would finish alone, one wavefront per SIMD, long after everybody else (a quarter of the
                // stage at 10k reads: 41 rounds, the last 25 of them on a fifth of the machine).  So a big batch is cut, in sorted order, into
                // four classes -- 1/16, 2/16, 4/16 of the extensions and the rest -- and the three classes of long extensions run their own
                // slices back to back on side streams, at a higher wave priority (s_setprio) and queue priority, while the bulk fills the
                // machine: every class ends within lenH + lenV steps, so it gets that many launches and the empty ones return at once.
                XdropSliceArgs xa;
                xa.s = sa;
                xa.cap = capB;
                xa.steps = kXdropSlice;                              // (64 / 128 steps for the first two slices: 3.41 s against 3.35 s on the 100k set)
                uint32_t* const L = ptr<uint32_t>(c->xlive);         // per class: two lists of its slots, back to back; then two counters per class
                uint32_t* const counters = L + 2 * capB;
                uint32_t longest = 0;
                for (uint32_t l : c->host_lens) longest = l > longest ? l : longest;
                const int nsl_bound = (int)((2u * longest) / (uint32_t)kXdropSlice) + 3;
                for (uint64_t first = 0; first < ne; first += capB) {
                    const uint64_t count = ne - first < capB ? ne - first : capB;
                    xa.state = ptr<uint32_t>(c->xstate);
                    xa.first = first;
                    xa.count = count;
                    xa.live_in = nullptr; xa.nlive_in = nullptr; xa.live_out = nullptr; xa.nlive_out = nullptr; xa.prio = 0;
                    k_xdrop_begin<<<nblk(count, kXdropBlock), kXdropBlock, 0, c->stream>>>(xa);
                    KCHK(c);
                    // class boundaries (slots of the batch, sorted order): only a batch several times the machine's 4,096 resident wavefronts
                    // is worth cutting
                    uint64_t cb[5] = {0, 0, 0, 0, count};
                    const bool classes = count >= c->xdrop_class_min && count >= 1024 && c->xdrop_variant == 1;
                    if (classes) { cb[1] = (count / 16) & ~63ull; cb[2] = (3 * count / 16) & ~63ull; cb[3] = (7 * count / 16) & ~63ull; }
                    if (classes) HIPCHK(c, hipEventRecord(c->fork, c->stream));
                    int nside = 0;
                    for (int k2 = 0; k2 < 3 && classes; ++k2) {      // the long classes: fixed number of launches, no host round trip
                        const uint64_t c0 = cb[k2], cn = cb[k2 + 1] - cb[k2];
                        if (!cn) continue;
                        hipStream_t sst = c->side[k2];
                        HIPCHK(c, hipStreamWaitEvent(sst, c->fork, 0));
                        XdropSliceArgs ya = xa;
                        ya.state = ptr<uint32_t>(c->xstate) + c0;     // (word w of slot t at state[w * cap + t]: the class's slots start at c0)
                        ya.count = cn;
                        ya.prio = 3 - k2;
                        uint32_t* const lists[2] = {L + 2 * c0, L + 2 * c0 + cn};
                        uint32_t* const cnts = counters + 2 * (k2 + 1);
                        ya.live_in = nullptr; ya.nlive_in = nullptr;
                        for (int s2 = 0; s2 < nsl_bound; ++s2) {
                            ya.live_out = lists[s2 & 1]; ya.nlive_out = cnts + (s2 & 1);
                            HIPCHK(c, hipMemsetAsync(ya.nlive_out, 0, 4, sst));
                            k_xdrop_slice<<<nblk(cn, kXdropBlock), kXdropBlock, 0, sst>>>(ya);
                            KCHK(c);
                            ya.live_in = ya.live_out; ya.nlive_in = ya.nlive_out;
                        }
                        HIPCHK(c, hipEventRecord(c->join[k2], sst));
                        nside = k2 + 1;
                    }
                    {   // the bulk (or the whole batch): as many launches as it takes, the survivor count read back every fourth slice
                        const uint64_t c0 = cb[3], cn = cb[4] - cb[3];
                        XdropSliceArgs za = xa;
                        za.state = ptr<uint32_t>(c->xstate) + c0;
                        za.count = cn;
                        uint32_t* const lists[2] = {L + 2 * c0, L + 2 * c0 + cn};
                        uint64_t live = cn;
                        za.live_in = nullptr; za.nlive_in = nullptr;
                        for (int it = 0; live; ++it) {
                            const int o = it & 1;
                            za.live_out = lists[o]; za.nlive_out = counters + o;
                            HIPCHK(c, hipMemsetAsync(za.nlive_out, 0, 4, c->stream));
                            k_xdrop_slice<<<nblk(live, kXdropBlock), kXdropBlock, 0, c->stream>>>(za);   // (live: an upper bound; the kernel reads the count)
                            KCHK(c);
                            if ((it & 3) == 3 || live <= 4096) {          // the survivor count comes back every fourth slice: it only ever shrinks
                                HIPCHK(c, hipMemcpyAsync(c->pinned + 100, za.nlive_out, 4, hipMemcpyDeviceToHost, c->stream));
                                HIPCHK(c, hipStreamSynchronize(c->stream));
                                live = c->pinned[100];
                            }
                            za.live_in = za.live_out; za.nlive_in = za.nlive_out;
                            if (it > 4096) return fail(c, BELLA_ERR_STATE, "internal: X-drop slices do not terminate");
                        }
                    }
                    for (int k2 = 0; k2 < nside; ++k2)              // (the next batch reuses the state slots and the lists; k_xdrop_finish reads every result)
                        HIPCHK(c, hipStreamWaitEvent(c->stream, c->join[k2], 0));
                    if (nside) {
                        // the long classes ran a FIXED number of slices (the bound lenH + lenV of an extension's steps): their final survivor
                        // counts are checked, and a class that the bound did not finish -- it never happened; a change of the slice size or of
                        // Phase 4's length could make it happen -- goes on slicing here, like the bulk, until nobody is left
                        const int fin = (nsl_bound - 1) & 1;
                        HIPCHK(c, hipMemcpyAsync(c->pinned + 101, counters + 2, 4 * 6, hipMemcpyDeviceToHost, c->stream));
                        HIPCHK(c, hipStreamSynchronize(c->stream));
                        for (int k2 = 0; k2 < nside; ++k2) {
                            uint64_t live = c->pinned[101 + 2 * k2 + fin];
                            if (!live) continue;
                            const uint64_t c0 = cb[k2], cn = cb[k2 + 1] - cb[k2];
                            XdropSliceArgs ya = xa;
                            ya.state = ptr<uint32_t>(c->xstate) + c0;
                            ya.count = cn;
                            uint32_t* const lists[2] = {L + 2 * c0, L + 2 * c0 + cn};
                            uint32_t* const cnts = counters + 2 * (k2 + 1);
                            ya.live_in = lists[fin]; ya.nlive_in = cnts + fin;
                            for (int it = 0, o = fin ^ 1; live; ++it, o ^= 1) {
                                ya.live_out = lists[o]; ya.nlive_out = cnts + o;
                                HIPCHK(c, hipMemsetAsync(ya.nlive_out, 0, 4, c->stream));
                                k_xdrop_slice<<<nblk(live, kXdropBlock), kXdropBlock, 0, c->stream>>>(ya);
                                KCHK(c);
                                HIPCHK(c, hipMemcpyAsync(c->pinned + 100, ya.nlive_out, 4, hipMemcpyDeviceToHost, c->stream));
                                HIPCHK(c, hipStreamSynchronize(c->stream));
                                live = c->pinned[100];
                                ya.live_in = ya.live_out; ya.nlive_in = ya.nlive_out;
                                if (it > 4096) return fail(c, BELLA_ERR_STATE, "internal: X-drop slices do not terminate");
                            }
                        }
                    }
                }
                }   // have_state
            }
            k_xdrop_finish<<<nblk(n), 256, 0, c->stream>>>(sa);
            KCHK(c);
        }
    }
    HIPCHK(c, hipEventRecord(c->ev[9], c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev[9]));
    c->tm.xdrop_ms = ev_ms(c->ev[8], c->ev[9]);
    return 0;
}

static int align_pairs_impl(bella_ctx* c, const bella_params* p, uint64_t* npassed, bool exact);
int bella_hip_align_pairs(bella_ctx* c, const bella_params* p, uint64_t* npassed) { return align_pairs_impl(c, p, npassed, false); }
int bella_hip_align_pairs_exact(bella_ctx* c, const bella_params* p, uint64_t* npassed) { return align_pairs_impl(c, p, npassed, true); }

static int align_pairs_impl(bella_ctx* c, const bella_params* p, uint64_t* npassed, bool exact) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, PAIRS)) return r;
    int rc = check_params(c, p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, ALNS);
    ENSURE(c, c->alns, sizeof(bella_aln) * c->npairs);
    rc = exact ? run_logan(c, p, nullptr, ptr<bella_pair>(c->pairs), c->npairs, ptr<bella_aln>(c->alns))
               : run_xdrop(c, p, nullptr, ptr<bella_pair>(c->pairs), c->npairs, ptr<bella_aln>(c->alns));
    if (rc) { (void)hipDeviceSynchronize(); return rc; }      // (an error may leave class slices in flight on the side streams)
    c->nalns = c->npairs;
    made(c, ALNS);
    if (npassed) {
        // small reduction on the host side of the ABI would need a copy; count on device instead
        ENSURE(c, c->cubtmp, 64);
        HIPCHK(c, hipMemsetAsync(c->status.p, 0, 16, c->stream));
        if (c->nalns) {
            k_count_passed<<<nblk(c->nalns), 256, 0, c->stream>>>(ptr<bella_aln>(c->alns), c->nalns,
                                                                  (unsigned long long*)(ptr<uint32_t>(c->status) + 2));
            KCHK(c);
        }
        unsigned long long cnt = 0;
        HIPCHK(c, hipMemcpyAsync(&cnt, ptr<uint32_t>(c->status) + 2, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *npassed = cnt;
    }
    return 0;
}

int bella_hip_get_alignments(bella_ctx* c, bella_aln* out) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, ALNS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->nalns) HIPCHK(c, c->stager.d2h(out, c->alns.p, sizeof(bella_aln) * c->nalns, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

static int xdrop_batch_impl(bella_ctx* c, const bella_seed* seeds, uint64_t n, const bella_params* p, bella_aln* out, bool exact);
int bella_hip_xdrop_batch(bella_ctx* c, const bella_seed* seeds, uint64_t n, const bella_params* p, bella_aln* out) {
    return xdrop_batch_impl(c, seeds, n, p, out, false);
}
int bella_hip_xdrop_batch_exact(bella_ctx* c, const bella_seed* seeds, uint64_t n, const bella_params* p, bella_aln* out) {
    return xdrop_batch_impl(c, seeds, n, p, out, true);
}

static int xdrop_batch_impl(bella_ctx* c, const bella_seed* seeds, uint64_t n, const bella_params* p, bella_aln* out, bool exact) {
    if (!c || !p || (n && (!seeds || !out))) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (p->kmer_size < 1 || p->kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    if (!exact) if (int r = check_xavier_xdrop(c, p)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    // validate on the host: the kernel trusts seeds
    std::vector<uint64_t> off((size_t)c->nreads + 1);
    HIPCHK(c, hipMemcpy(off.data(), c->roff.p, 8 * ((size_t)c->nreads + 1), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; ++i) {
        const bella_seed& s = seeds[i];
        if (s.rid >= c->nreads || s.cid >= c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "seed %llu: read id out of range", (unsigned long long)i);
        const uint64_t lh = off[s.rid + 1] - off[s.rid], lv = off[s.cid + 1] - off[s.cid];
        if ((uint64_t)s.seedH + p->kmer_size > lh || (uint64_t)s.seedV + p->kmer_size > lv)
            return fail(c, BELLA_ERR_BAD_ARG, "seed %llu: k-mer past the end of a read", (unsigned long long)i);
    }
    TmpBuf dalns;
    ENSURE(c, c->seeds, sizeof(bella_seed) * n);
    ENSURE(c, dalns, sizeof(bella_aln) * n);
    if (n) HIPCHK(c, hipMemcpyAsync(c->seeds.p, seeds, sizeof(bella_seed) * n, hipMemcpyHostToDevice, c->stream));
    const int rc = exact ? run_logan(c, p, ptr<bella_seed>(c->seeds), nullptr, n, ptr<bella_aln>(dalns))
                         : run_xdrop(c, p, ptr<bella_seed>(c->seeds), nullptr, n, ptr<bella_aln>(dalns));
    if (rc) return rc;
    if (n) HIPCHK(c, hipMemcpyAsync(out, dalns.p, sizeof(bella_aln) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bella_hip_write_output(const char* path, const bella_params* p, int paf, uint32_t nreads, const char* const* names, const uint32_t* lens,
                           const bella_pair* pairs, const bella_aln* alns, uint64_t npairs, int nthreads, bella_write_stats* stats) {
    std::string err;
    const int rc = write_output_impl(path, p, paf, nreads, names, lens, pairs, alns, npairs, nthreads, stats, err);
    if (rc) fprintf(stderr, "bella_hip_write_output: %s\n", err.c_str());
    return rc;
}

int bella_hip_get_timings(bella_ctx* c, bella_timings* t) {
    if (!c || !t) return BELLA_ERR_BAD_ARG;
    *t = c->tm;
    return 0;
}

}  // extern "C"

// ---- traced alignments (trace.hpp) ---------------------------------------------------------------------------
namespace {
struct TraceJob { uint32_t rid, cid, seedH, seedV; bella_aln a; };

// One pair's clip into its record and into the call's sums (section 24).  An emptied pair keeps op_off, band and widened.
void clip_count(uint32_t nops, uint64_t cols, int64_t spanV, int64_t spanH, const bella_clip& r, bella_clip_stats& cs) {
    cs.pairs++;
    if (!r.nruns) cs.emptied++;
    else if (r.nruns < nops) cs.clipped++;
    cs.runs_before += nops; cs.runs_after += r.nruns;
    cs.columns_before += cols; cs.columns_after += (uint64_t)r.n_eq + r.n_x + r.n_ins + r.n_del;
    cs.bases_v_removed += (uint64_t)(spanV - ((int64_t)r.endV - r.begV));
    cs.bases_h_removed += (uint64_t)(spanH - ((int64_t)r.endH - r.begH));
}
void clip_apply(bella_trace& t, const bella_clip& r, bella_clip_stats& cs) {
    clip_count(t.nops, (uint64_t)t.n_eq + t.n_x + t.n_ins + t.n_del, (int64_t)t.tendV - t.tbegV, (int64_t)t.tendH - t.tbegH, r, cs);
    t.op_off += r.first_run;
    t.nops = r.nruns;
    t.tbegV = r.begV; t.tendV = r.endV; t.tbegH = r.begH; t.tendH = r.endH;
    t.n_eq = r.n_eq; t.n_x = r.n_x; t.n_ins = r.n_ins; t.n_del = r.n_del;
    t.score = r.score;
}

// The vote kernel on n pairs whose runs are in `ops` (device): section 10's, or with normalize section 21's.  The counters go to
// c->pile_cnt, a zeroed PileNormCnt of which k_pile_vote writes the first field only.
void launch_pile_vote(bella_ctx* c, bool normalize, const PilePair* pp, size_t n, const uint32_t* ops) {
    const unsigned blocks = nblk(n, kPileBlock / 64);
    if (normalize)
        k_pile_vote_norm<<<blocks, kPileBlock, 0, c->stream>>>(pp, (uint32_t)n, ops, ptr<uint32_t>(c->packed), ptr<uint32_t>(c->pile), ptr<PileNormCnt>(c->pile_cnt));
    else
        k_pile_vote<<<blocks, kPileBlock, 0, c->stream>>>(pp, (uint32_t)n, ops, ptr<uint32_t>(c->packed), ptr<uint32_t>(c->pile), ptr<unsigned long long>(c->pile_cnt));
}
// c->pile_cnt into the counters of `vs`; waits for the device
int read_vote_counts(bella_ctx* c, bella_vote_stats& vs) {
    static_assert(offsetof(PileNormCnt, votes) == 0, "k_pile_vote adds its votes to the first field");
    PileNormCnt nc{};
    HIPCHK(c, hipMemcpyAsync(&nc, c->pile_cnt.p, sizeof(nc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    vs.votes = nc.votes; vs.gap_runs = nc.gap_runs; vs.shifted_runs = nc.shifted_runs; vs.shifted_columns = nc.shifted_columns;
    return 0;
}

// The band -> kernel mapping of the banded sweeps (band.hpp), once: f(C, cls) with C = 4, 8, 16 for the register kernels of 256, 512 and
// 1,024 cells, C = 0 for the wide kernel above them; cls = 0 .. 3 numbers the classes.
template <int C> using BandC = std::integral_constant<int, C>;
template <class F> void for_band(uint32_t B, F&& f) {
    B == 256 ? f(BandC<4>{}, 0u) : B == 512 ? f(BandC<8>{}, 1u) : B == 1024 ? f(BandC<16>{}, 2u) : f(BandC<0>{}, 3u);
}

// Traces jobs[0 .. n): out[n] records, ops appended to `ops` (op_off counts from the vector's start).  Pairs run in batches sized by
// the free device memory (the direction bytes dominate); a pair whose path touched its band's edge on a side goes back into the queue
// with that side's band doubled, until no side touches or the band holds the side's whole rectangle.
// vote: every finished pair's runs also vote into the context's pileup table (pileup.hpp), from the batch's op array on the device;
// keep_ops == false: the runs are not copied to the host (`ops` stays as it is; the records' op_off count as if they had been).
// normalize (with vote): the votes are k_pile_vote_norm's (section 21); what the votes did goes to c->vote_stats either way.
// clip_t != 0 (section 24): every finished pair is clipped at that identity on the device, from the batch's op array, before it votes;
// the writing walk then always runs; out[] and the voting pairs carry the clipped records, c->clip_stats what the clips did.
int run_trace(bella_ctx* c, const bella_params* p, const std::vector<TraceJob>& jobs, uint32_t band0, bella_trace* out, std::vector<uint32_t>& ops,
              bella_trace_stats& st, bool vote = false, bool keep_ops = true, bool normalize = false, uint32_t clip_t = 0) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    st = bella_trace_stats{};
    bella_clip_stats cs{};
    cs.identity = clip_t;
    if (clip_t) c->clip_stats = cs;
    bella_vote_stats vs{};
    vs.normalized = normalize ? 1u : 0u;
    if (vote) c->vote_stats = vs;
    if (band0 == 0) band0 = BELLA_TRACE_DEFAULT_BAND;
    uint32_t b0 = kTrMinBand;
    while (b0 < band0 && b0 < kTrMaxBand) b0 <<= 1;
    st.band0 = b0;
    const uint32_t k = p->kmer_size;
    const size_t n = jobs.size();
    if (!n) return 0;
    std::vector<uint64_t> off((size_t)c->nreads + 1);
    HIPCHK(c, hipMemcpy(off.data(), c->roff.p, 8 * ((size_t)c->nreads + 1), hipMemcpyDeviceToHost));
    struct Side { int64_t gH, gV; uint32_t n, m, band, cover; int32_t dH, dV; };
    struct Work { Side s[2]; uint32_t comp, widened; int32_t seedHo; };
    std::vector<Work> W(n);
    for (size_t q = 0; q < n; ++q) {
        const TraceJob& j = jobs[q];
        if (j.rid >= c->nreads || j.cid >= c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "trace %zu: read id out of range", q);
        const int64_t lh = (int64_t)(off[j.rid + 1] - off[j.rid]), lv = (int64_t)(off[j.cid + 1] - off[j.cid]);
        if ((int64_t)j.seedH + k > lh || (int64_t)j.seedV + k > lv) return fail(c, BELLA_ERR_BAD_ARG, "trace %zu: k-mer past the end of a read", q);
        if (j.a.strand > 1) return fail(c, BELLA_ERR_BAD_ARG, "trace %zu: strand must be 0 or 1", q);
        const int64_t sH = j.a.strand ? lh - (int64_t)j.seedH - k : (int64_t)j.seedH, sV = j.seedV;     // the seed on the oriented H (align.hpp:181-182)
        auto clampi = [](int64_t x, int64_t hi) { return (uint32_t)(x < 0 ? 0 : (x > hi ? hi : x)); };
        Work& w = W[q];
        w.comp = j.a.strand ? 3u : 0u;
        w.widened = 0;
        w.seedHo = (int32_t)sH;
        const int64_t gH = (int64_t)off[j.rid], gV = (int64_t)off[j.cid];
        Side& L = w.s[0];
        Side& R = w.s[1];
        L.m = clampi(sH - j.a.begH, sH); L.n = clampi(sV - j.a.begV, sV);
        // (xavier.h:356-360: when the right extension does not run the reference overwrites the BEGIN points with the reads' lengths; a
        // begin point behind the seed says nothing about the left side, whose rectangle then reaches to the reads' starts)
        if (j.a.begH > sH || j.a.begV > sV) { L.m = (uint32_t)sH; L.n = (uint32_t)sV; }
        R.m = clampi((int64_t)j.a.endH - (sH + k), lh - sH - k); R.n = clampi((int64_t)j.a.endV - (sV + k), lv - sV - k);
        // element t of the left sequences: oriented H at sH - 1 - t, V at sV - 1 - t; of the right ones: sH + k + t, sV + k + t
        if (!j.a.strand) { L.gH = gH + sH - 1; L.dH = -1; R.gH = gH + sH + k; R.dH = 1; }
        else { L.gH = gH + lh - sH; L.dH = 1; R.gH = gH + lh - 1 - sH - k; R.dH = -1; }                  // oriented H[x] = complement of H[len - 1 - x]
        L.gV = gV + sV - 1; L.dV = -1; R.gV = gV + sV + k; R.dV = 1;
        for (Side& s : w.s) { s.cover = trace_cover_band(s.n, s.m); s.band = b0 < s.cover ? b0 : s.cover; }
    }
    // memory of a batch: directions + (wide) scratch; a quarter of what is free, at most 16 GB, at least what the largest pair needs
    size_t mfree = 0, mtotal = 0;
    HIPCHK(c, hipMemGetInfo(&mfree, &mtotal));
    mfree += c->pool.bytes + c->pool.arena.largest_hole() + c->tr_dirs.cap;
    uint64_t budget = std::min<uint64_t>((uint64_t)mfree / 4, 16ull << 30);
    if (budget < (64ull << 20)) budget = 64ull << 20;
    auto side_dir_bytes = [](const Side& s) { return ((uint64_t)trace_rows(s.n, s.m, s.band) * (s.band / 4) + 15) & ~15ull; };
    auto side_scr_ints = [](const Side& s) { return s.band > kTrRegBand ? 2ull * s.band : 0ull; };
    constexpr uint32_t kMaxBatchPairs = 1u << 20;
    std::vector<uint32_t> queue(n), next;
    for (size_t q = 0; q < n; ++q) queue[q] = (uint32_t)q;
    EventSet ev, evc;
    if (int r = ev.create(c, 4)) return r;
    if (clip_t) if (int r = evc.create(c, 2)) return r;
    TmpBuf clip_in, clip_out;
    std::vector<ClipPair> clipp;
    std::vector<uint32_t> clipid;                                     // the job each of them is
    std::vector<bella_clip> clipr;
    std::vector<TraceExt> exts;
    std::vector<uint32_t> lists[4];
    std::vector<TracePairRes> pres;
    std::vector<TraceExtRes> eres;
    std::vector<uint64_t> opoff;
    std::vector<PilePair> votep;
    uint64_t ops_seen = ops.size();                                   // runs written so far (= ops.size() while the runs are kept)
    if (vote) {
        ENSURE(c, c->pile_cnt, sizeof(PileNormCnt));
        HIPCHK(c, hipMemsetAsync(c->pile_cnt.p, 0, sizeof(PileNormCnt), c->stream));
    }
    const uint32_t* const packed = ptr<uint32_t>(c->packed);
    while (!queue.empty()) {
        next.clear();
        size_t at = 0;
        while (at < queue.size()) {
            // ---- cut a batch
            uint64_t dbytes = 0, sints = 0;
            exts.clear();
            for (auto& l : lists) l.clear();
            size_t end = at;
            while (end < queue.size() && end - at < kMaxBatchPairs) {
                const Work& w = W[queue[end]];
                const uint64_t need = side_dir_bytes(w.s[0]) + side_dir_bytes(w.s[1]) + 4 * (side_scr_ints(w.s[0]) + side_scr_ints(w.s[1]));
                if (end > at && dbytes + 4 * sints + need > budget) break;
                for (int sd = 0; sd < 2; ++sd) {
                    const Side& s = w.s[sd];
                    TraceExt e{};
                    e.gH = s.gH; e.gV = s.gV; e.dir_off = dbytes; e.scr_off = sints; e.n = s.n; e.m = s.m; e.band = s.band; e.dH = s.dH; e.dV = s.dV;
                    e.comp = w.comp;
                    for_band(s.band, [&](auto, uint32_t cls) { lists[cls].push_back((uint32_t)exts.size()); });
                    exts.push_back(e);
                    dbytes += side_dir_bytes(s);
                    sints += side_scr_ints(s);
                    st.dp_cells += (uint64_t)trace_rows(s.n, s.m, s.band) * s.band;
                    st.dir_bytes += side_dir_bytes(s);
                }
                ++end;
            }
            const uint32_t nb = (uint32_t)(end - at);
            st.batches++;
            st.extensions += 2ull * nb;
            if (dbytes > st.dir_bytes_peak) st.dir_bytes_peak = dbytes;
            // ---- upload, DP
            ENSURE(c, c->tr_exts, sizeof(TraceExt) * exts.size());
            ENSURE(c, c->tr_lists, 4 * exts.size());
            ENSURE(c, c->tr_res, sizeof(TraceExtRes) * exts.size());
            ENSURE(c, c->tr_pres, sizeof(TracePairRes) * nb);
            ENSURE(c, c->tr_opoff, 8 * (size_t)nb);
            ENSURE(c, c->tr_dirs, (size_t)dbytes + 64);
            if (sints) ENSURE(c, c->tr_scr, 4 * (size_t)sints + 64);
            HIPCHK(c, hipMemcpyAsync(c->tr_exts.p, exts.data(), sizeof(TraceExt) * exts.size(), hipMemcpyHostToDevice, c->stream));
            uint32_t lo[5] = {0, 0, 0, 0, 0};
            {
                std::vector<uint32_t> all;
                all.reserve(exts.size());
                for (int q = 0; q < 4; ++q) { lo[q] = (uint32_t)all.size(); all.insert(all.end(), lists[q].begin(), lists[q].end()); }
                lo[4] = (uint32_t)all.size();
                HIPCHK(c, hipMemcpyAsync(c->tr_lists.p, all.data(), 4 * all.size(), hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));             // (the host vectors are reused by the next batch)
            }
            const TraceExt* const dex = ptr<TraceExt>(c->tr_exts);
            const uint32_t* const dl = ptr<uint32_t>(c->tr_lists);
            uint8_t* const ddirs = ptr<uint8_t>(c->tr_dirs);
            TraceExtRes* const dres = ptr<TraceExtRes>(c->tr_res);
            HIPCHK(c, hipEventRecord(ev.a, c->stream));
            const uint32_t wpb = kTraceBlock / 64;
            for (int q = 0; q < 4; ++q) {
                const uint32_t nl = lo[q + 1] - lo[q];
                if (nl) for_band(exts[lists[q][0]].band, [&](auto C, uint32_t) {
                    if constexpr (decltype(C)::value != 0) k_trace_dp<decltype(C)::value><<<nblk(nl, wpb), kTraceBlock, 0, c->stream>>>(dex, dl + lo[q], nl, packed, ddirs, dres);
                    else k_trace_dp_wide<<<nl, 64, 0, c->stream>>>(dex, dl + lo[q], nl, packed, ddirs, ptr<int>(c->tr_scr), dres);
                });
                KCHK(c);
            }
            HIPCHK(c, hipEventRecord(ev.b, c->stream));
            k_trace_count<<<nblk(nb, 64), 64, 0, c->stream>>>(dex, dres, nb, packed, ddirs, (int)k, ptr<TracePairRes>(c->tr_pres));
            KCHK(c);
            HIPCHK(c, hipEventRecord(ev.d, c->stream));
            pres.resize(nb);
            eres.resize(exts.size());
            HIPCHK(c, hipMemcpyAsync(pres.data(), c->tr_pres.p, sizeof(TracePairRes) * nb, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(eres.data(), c->tr_res.p, sizeof(TraceExtRes) * exts.size(), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            st.dp_ms += ev_ms(ev.a, ev.b);
            st.walk_ms += ev_ms(ev.b, ev.d);
            // ---- who is done, who goes again
            opoff.assign(nb, ~0ull);
            votep.clear();
            clipp.clear();
            clipid.clear();
            uint64_t bops = 0;
            for (uint32_t q = 0; q < nb; ++q) {
                const uint32_t id = queue[at + q];
                Work& w = W[id];
                // (a pair goes again as a whole: the writing walk needs the directions of both sides in one batch, so the side that did not
                // touch is computed again with its band unchanged -- same result; at ~0.1 % of the pairs this costs nothing measurable)
                bool again = false;
                for (int sd = 0; sd < 2; ++sd)
                    if ((pres[q].touch >> sd & 1u) && w.s[sd].band < w.s[sd].cover) { w.s[sd].band *= 2; w.widened++; st.widened_extensions++; again = true; }
                if (again) { next.push_back(id); st.repeated_pairs++; continue; }
                const TraceJob& j = jobs[id];
                const TraceExtRes &rl = eres[2 * q], &rr = eres[2 * q + 1];
                bella_trace& t = out[id];
                t.op_off = ops_seen + bops;
                t.nops = pres[q].nops;
                t.band = std::max(w.s[0].band, w.s[1].band);
                t.score = rl.score + pres[q].seed_score + rr.score;
                t.tbegH = w.seedHo - (int32_t)rl.bj; t.tbegV = (int32_t)j.seedV - (int32_t)rl.bi;
                t.tendH = w.seedHo + (int32_t)k + (int32_t)rr.bj; t.tendV = (int32_t)j.seedV + (int32_t)k + (int32_t)rr.bi;
                t.n_eq = pres[q].n_eq; t.n_x = pres[q].n_x; t.n_ins = pres[q].n_ins; t.n_del = pres[q].n_del;
                t.widened = w.widened;
                if (clip_t && t.nops) { clipp.push_back(ClipPair{bops, t.nops, t.tbegV, t.tbegH, 0u}); clipid.push_back(id); }
                if (vote && t.nops)
                    votep.push_back(PilePair{off[j.cid], off[j.rid], bops, t.nops, (uint32_t)(off[j.cid + 1] - off[j.cid]), (uint32_t)(off[j.rid + 1] - off[j.rid]),
                                             j.a.strand ? 1u : 0u, t.tbegV, t.tbegH});
                opoff[q] = bops;
                bops += pres[q].nops;
                st.pairs++;
            }
            if (bops && !keep_ops && !vote && !clip_t) {               // nobody reads the runs: the records are complete without the writing walk
                ops_seen += bops;
                st.ops += bops;
            } else if (bops) {
                ENSURE(c, c->tr_ops, 4 * (size_t)bops);
                HIPCHK(c, hipMemcpyAsync(c->tr_opoff.p, opoff.data(), 8 * (size_t)nb, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipEventRecord(ev.a, c->stream));
                k_trace_write<<<nblk(nb, 64), 64, 0, c->stream>>>(dex, dres, nb, packed, ddirs, (int)k, ptr<uint64_t>(c->tr_opoff), ptr<TracePairRes>(c->tr_pres),
                                                                  ptr<uint32_t>(c->tr_ops));
                KCHK(c);
                HIPCHK(c, hipEventRecord(ev.b, c->stream));
                if (clip_t && !clipp.empty()) {                         // the batch's pairs are clipped before anybody reads their records
                    clipr.resize(clipp.size());
                    ENSURE(c, clip_in, sizeof(ClipPair) * clipp.size());
                    ENSURE(c, clip_out, sizeof(bella_clip) * clipp.size());
                    HIPCHK(c, hipMemcpyAsync(clip_in.p, clipp.data(), sizeof(ClipPair) * clipp.size(), hipMemcpyHostToDevice, c->stream));
                    HIPCHK(c, hipEventRecord(evc.a, c->stream));
                    k_clip<<<nblk(clipp.size(), kClipBlock / 64), kClipBlock, 0, c->stream>>>(ptr<ClipPair>(clip_in), (uint32_t)clipp.size(), ptr<uint32_t>(c->tr_ops), clip_t,
                                                                                            ptr<bella_clip>(clip_out));
                    KCHK(c);
                    HIPCHK(c, hipEventRecord(evc.b, c->stream));
                    HIPCHK(c, hipMemcpyAsync(clipr.data(), clip_out.p, sizeof(bella_clip) * clipp.size(), hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    cs.clip_ms += ev_ms(evc.a, evc.b);
                    size_t vq = 0, vkeep = 0;                           // votep lists the same pairs in the same order
                    for (size_t x = 0; x < clipp.size(); ++x) {
                        clip_apply(out[clipid[x]], clipr[x], cs);
                        if (!vote) continue;
                        PilePair vp = votep[vq++];
                        if (!clipr[x].nruns) continue;                  // an emptied pair casts no vote
                        vp.op_off += clipr[x].first_run; vp.nops = clipr[x].nruns; vp.i0 = clipr[x].begV; vp.j0 = clipr[x].begH;
                        votep[vkeep++] = vp;
                    }
                    if (vote) votep.resize(vkeep);
                }
                if (vote && !votep.empty()) {                           // the batch's runs vote while they are in device memory
                    ENSURE(c, c->pile_pairs, sizeof(PilePair) * votep.size());
                    HIPCHK(c, hipMemcpyAsync(c->pile_pairs.p, votep.data(), sizeof(PilePair) * votep.size(), hipMemcpyHostToDevice, c->stream));
                    HIPCHK(c, hipEventRecord(ev.d, c->stream));
                    launch_pile_vote(c, normalize, ptr<PilePair>(c->pile_pairs), votep.size(), ptr<uint32_t>(c->tr_ops));
                    KCHK(c);
                    vs.pairs += votep.size();
                    for (const PilePair& vp : votep) vs.runs += vp.nops;
                    HIPCHK(c, hipEventRecord(ev.e, c->stream));
                }
                if (keep_ops) {
                    const size_t base = ops.size();
                    ops.resize(base + bops);
                    HIPCHK(c, c->stager.d2h(ops.data() + base, c->tr_ops.p, 4 * (size_t)bops, c->stream));
                    st.ops_host_bytes += 4 * bops;
                }
                HIPCHK(c, hipStreamSynchronize(c->stream));              // (votep and opoff are reused by the next batch)
                st.walk_ms += ev_ms(ev.a, ev.b);
                if (vote && !votep.empty()) st.vote_ms += ev_ms(ev.d, ev.e);
                ops_seen += bops;
                st.ops += bops;
            }
            at = end;
        }
        queue.swap(next);
    }
    if (vote) {
        if (int r = read_vote_counts(c, vs)) return r;
        st.votes = vs.votes;
        vs.vote_ms = st.vote_ms;
        c->vote_stats = vs;
    }
    if (clip_t) c->clip_stats = cs;
    st.total_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    return 0;
}

void trace_release(bella_ctx* c) {      // the batch buffers go back (directions: gigabytes) once a call is over
    for (Buf* b : {&c->tr_exts, &c->tr_lists, &c->tr_res, &c->tr_pres, &c->tr_opoff, &c->tr_dirs, &c->tr_scr, &c->tr_ops}) release(*b);
}
}  // namespace

static int trace_pairs_impl(bella_ctx* c, const bella_params* p, uint32_t band0, int passed_only, bool vote, bool keep_ops, uint64_t* ntraced, uint64_t* nops,
                            bool normalize = false, uint32_t clip_t = 0) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, ALNS)) return r;
    if (vote) if (int r = need(c, PILE)) return r;
    int rc = check_params(c, p);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, TRACES);
    const size_t n = (size_t)c->nalns;
    std::vector<bella_pair> pairs(n);
    std::vector<bella_aln> alns(n);
    if (n) {
        HIPCHK(c, c->stager.d2h(pairs.data(), c->pairs.p, sizeof(bella_pair) * n, c->stream));
        HIPCHK(c, c->stager.d2h(alns.data(), c->alns.p, sizeof(bella_aln) * n, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    std::vector<TraceJob> jobs;
    std::vector<size_t> which;
    for (size_t i = 0; i < n; ++i)
        if (!passed_only || alns[i].passed) { jobs.push_back(TraceJob{pairs[i].rid, pairs[i].cid, pairs[i].seedH, pairs[i].seedV, alns[i]}); which.push_back(i); }
    std::vector<bella_trace> tr(jobs.size());
    c->trace_ops.clear();
    if (!keep_ops) std::vector<uint32_t>().swap(c->trace_ops);
    if (vote) changed(c, PILE);
    rc = run_trace(c, p, jobs, band0, tr.data(), c->trace_ops, c->trace_stats, vote, keep_ops, normalize, clip_t);
    trace_release(c);
    if (vote) release(c->pile_pairs);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    c->traces.assign(n, bella_trace{});
    for (size_t i = 0; i < which.size(); ++i) c->traces[which[i]] = tr[i];
    made(c, TRACES);
    c->trace_ops_kept = keep_ops;
    if (ntraced) *ntraced = jobs.size() - (clip_t ? c->clip_stats.emptied : 0);
    if (nops) *nops = c->trace_stats.ops;
    return 0;
}

extern "C" {

int bella_hip_trace_pairs(bella_ctx* c, const bella_params* p, uint32_t band0, int passed_only, uint64_t* ntraced, uint64_t* nops) {
    return trace_pairs_impl(c, p, band0, passed_only, false, true, ntraced, nops);
}

int bella_hip_trace_pairs_pileup(bella_ctx* c, const bella_params* p, uint32_t band0, int keep_ops, uint64_t* ntraced, uint64_t* nops) {
    return trace_pairs_impl(c, p, band0, 1, true, keep_ops != 0, ntraced, nops);
}

// section 24's parameter: the identity a call uses, or 0 with the error set
static uint32_t clip_identity(bella_ctx* c, const bella_clip_params* given, const char* who) {
    bella_clip_params cp{(uint32_t)sizeof(bella_clip_params), 0};
    if (take_params(c, cp, given, who)) return 0;
    if (cp.identity == 0) cp.identity = BELLA_CLIP_DEFAULT_IDENTITY;
    if (cp.identity > 999) { fail(c, BELLA_ERR_BAD_ARG, "%s: identity %u is not in 1 .. 999 permille (0: the default %d)", who, cp.identity, BELLA_CLIP_DEFAULT_IDENTITY); return 0; }
    return cp.identity;
}

static int trace_pairs_flags_impl(bella_ctx* c, const bella_params* p, uint32_t band0, uint32_t flags, uint64_t* ntraced, uint64_t* nops, uint32_t clip_t) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (flags & ~(BELLA_TRACE_PASSED_ONLY | BELLA_TRACE_DROP_OPS | BELLA_TRACE_PILEUP | BELLA_TRACE_NORMALIZE)) return fail(c, BELLA_ERR_BAD_ARG, "trace_pairs_flags: unknown flag");
    const bool vote = (flags & BELLA_TRACE_PILEUP) != 0;
    if ((flags & BELLA_TRACE_NORMALIZE) && !vote) return fail(c, BELLA_ERR_BAD_ARG, "trace_pairs_flags: BELLA_TRACE_NORMALIZE normalises the votes: it needs BELLA_TRACE_PILEUP");
    if (vote && !(flags & BELLA_TRACE_PASSED_ONLY)) return fail(c, BELLA_ERR_BAD_ARG, "trace_pairs_flags: the pileup takes the passed pairs only");
    return trace_pairs_impl(c, p, band0, (flags & BELLA_TRACE_PASSED_ONLY) ? 1 : 0, vote, !(flags & BELLA_TRACE_DROP_OPS), ntraced, nops, (flags & BELLA_TRACE_NORMALIZE) != 0, clip_t);
}

int bella_hip_trace_pairs_flags(bella_ctx* c, const bella_params* p, uint32_t band0, uint32_t flags, uint64_t* ntraced, uint64_t* nops) {
    return trace_pairs_flags_impl(c, p, band0, flags, ntraced, nops, 0);
}

int bella_hip_trace_pairs_clip(bella_ctx* c, const bella_params* p, uint32_t band0, uint32_t flags, const bella_clip_params* clip, uint64_t* ntraced, uint64_t* nops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    const uint32_t t = clip_identity(c, clip, "trace_pairs_clip");
    if (!t) return BELLA_ERR_BAD_ARG;
    return trace_pairs_flags_impl(c, p, band0, flags, ntraced, nops, t);
}

int bella_hip_get_clip_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    return put_sized(out, struct_size, c->clip_stats);
}

int bella_hip_clip_ops(bella_ctx* c, const bella_vote_pair* pairs, uint64_t npairs, const uint32_t* ops, uint64_t nops_total, const bella_clip_params* clip, bella_clip* out) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if ((npairs && (!pairs || !out)) || (nops_total && !ops)) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: null argument");
    if (npairs > 0xffffffffull) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: at most 2^32 - 1 pairs a call");
    const uint32_t t = clip_identity(c, clip, "clip_ops");
    if (!t) return BELLA_ERR_BAD_ARG;
    // ---- everything is checked before anything is launched
    struct Before { uint64_t cols; int64_t spanV, spanH; };
    std::vector<ClipPair> cp((size_t)npairs);
    std::vector<Before> before((size_t)npairs);
    for (uint64_t q = 0; q < npairs; ++q) {
        const bella_vote_pair& a = pairs[q];
        if (a.op_off > nops_total || a.nops > nops_total - a.op_off) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: pair %llu: its runs lie outside ops", (unsigned long long)q);
        if (a.tbegV < 0 || a.tbegH < 0) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: pair %llu: negative start", (unsigned long long)q);
        uint64_t i = (uint64_t)a.tbegV, j = (uint64_t)a.tbegH, cols = 0;
        for (uint32_t k = 0; k < a.nops; ++k) {
            const uint32_t w = ops[a.op_off + k], op = w & 15u, len = w >> 4;
            if (op > kOpDel) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: pair %llu run %u: op %u is none of = X I D", (unsigned long long)q, k, op);
            if (!len) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: pair %llu run %u: length 0", (unsigned long long)q, k);
            if (op != kOpDel) i += len;
            if (op != kOpIns) j += len;
            cols += len;
            if (i >= (1ull << 31) || j >= (1ull << 31)) return fail(c, BELLA_ERR_BAD_ARG, "clip_ops: pair %llu: its runs reach base 2^31 of a read", (unsigned long long)q);
        }
        cp[(size_t)q] = ClipPair{a.op_off, a.nops, a.tbegV, a.tbegH, 0u};
        before[(size_t)q] = Before{cols, (int64_t)i - a.tbegV, (int64_t)j - a.tbegH};
    }
    bella_clip_stats cs{};
    cs.identity = t;
    if (npairs) {
        HIPCHK(c, hipSetDevice(c->device));
        TmpBuf dp, dops, dout;
        EventSet ev;
        if (int r = ev.create(c, 2)) return r;
        std::vector<bella_clip> res((size_t)npairs);
        ENSURE(c, dp, sizeof(ClipPair) * cp.size());
        ENSURE(c, dops, 4 * (size_t)nops_total + 4);
        ENSURE(c, dout, sizeof(bella_clip) * cp.size());
        HIPCHK(c, hipMemcpyAsync(dp.p, cp.data(), sizeof(ClipPair) * cp.size(), hipMemcpyHostToDevice, c->stream));
        if (nops_total) HIPCHK(c, hipMemcpyAsync(dops.p, ops, 4 * (size_t)nops_total, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        k_clip<<<nblk(cp.size(), kClipBlock / 64), kClipBlock, 0, c->stream>>>(ptr<ClipPair>(dp), (uint32_t)cp.size(), ptr<uint32_t>(dops), t, ptr<bella_clip>(dout));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipMemcpyAsync(res.data(), dout.p, sizeof(bella_clip) * cp.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        cs.clip_ms = ev_ms(ev.a, ev.b);
        for (size_t q = 0; q < cp.size(); ++q)
            if (cp[q].nops) clip_count(cp[q].nops, before[q].cols, before[q].spanV, before[q].spanH, res[q], cs);
        std::memcpy(out, res.data(), sizeof(bella_clip) * res.size());
    }
    c->clip_stats = cs;
    return 0;
}

int bella_hip_get_traces(bella_ctx* c, bella_trace* out, uint32_t* ops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TRACES)) return r;
    if (ops && !c->trace_ops_kept) return fail(c, BELLA_ERR_STATE, "the last trace ran with keep_ops = 0 / BELLA_TRACE_DROP_OPS: the runs were not kept (pass ops = NULL)");
    if (out && !c->traces.empty()) std::memcpy(out, c->traces.data(), sizeof(bella_trace) * c->traces.size());
    if (ops && !c->trace_ops.empty()) std::memcpy(ops, c->trace_ops.data(), 4 * c->trace_ops.size());
    return 0;
}

int bella_hip_trace_batch(bella_ctx* c, const bella_seed* seeds, const bella_aln* alns, uint64_t n, const bella_params* p, uint32_t band0, bella_trace* out,
                          uint32_t* ops, uint64_t ops_cap, uint64_t* nops) {
    if (!c || !p || (n && (!seeds || !alns || !out))) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (p->kmer_size < 1 || p->kmer_size > 32) return fail(c, BELLA_ERR_BAD_ARG, "k must be in [1,32]");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<TraceJob> jobs((size_t)n);
    for (uint64_t i = 0; i < n; ++i) jobs[(size_t)i] = TraceJob{seeds[i].rid, seeds[i].cid, seeds[i].seedH, seeds[i].seedV, alns[i]};
    std::vector<uint32_t>& v = c->batch_ops;       // the runs stay with the context: a caller that could not know their number fetches them
    v.clear();
    drop(c, BATCH_OPS);
    bella_trace_stats st;
    const int rc = run_trace(c, p, jobs, band0, out, v, st);
    trace_release(c);
    if (rc) { (void)hipDeviceSynchronize(); return rc; }
    c->trace_stats = st;
    made(c, BATCH_OPS);
    if (nops) *nops = v.size();
    if (!ops) return 0;
    if (v.size() > ops_cap) return fail(c, BELLA_ERR_NOMEM, "trace_batch: %zu ops, room for %llu (bella_hip_get_batch_ops hands them out)", v.size(), (unsigned long long)ops_cap);
    if (!v.empty()) std::memcpy(ops, v.data(), 4 * v.size());
    return 0;
}

int bella_hip_get_batch_ops(bella_ctx* c, uint32_t* ops, uint64_t ops_cap) {
    if (!c || (!ops && ops_cap)) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, BATCH_OPS)) return r;
    if (c->batch_ops.size() > ops_cap) return fail(c, BELLA_ERR_BAD_ARG, "get_batch_ops: %zu ops, room for %llu", c->batch_ops.size(), (unsigned long long)ops_cap);
    if (!c->batch_ops.empty()) std::memcpy(ops, c->batch_ops.data(), 4 * c->batch_ops.size());
    return 0;
}

int bella_hip_get_trace_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    return put_sized(out, struct_size, c->trace_stats);
}

}  // extern "C"

// ---- read correction (pileup.hpp) ----------------------------------------------------------------------------
namespace {
struct EmitCount {
    __host__ __device__ uint64_t operator()(const uint8_t& v) const { return (uint64_t)(v & 3u); }
};

// A vote table into the sequence it emits, for the consensus and for the rounds of sections 18 and 20: `table` is about the `nseq`
// sequences of `packed` that begin at `offs` (`total` bases); the emitted bases go to `out` (*nout of them), their offsets to `noffs`,
// the per-sequence statistics to `stats`.  Waits for the device once, to size `out`.  `scan` stays alive: where every old base went,
// which the callers' own kernels read afterwards.
int consensus_tail(bella_ctx* c, const Buf& table, const uint32_t* packed, const Buf& offs, uint32_t nseq, uint64_t total, uint32_t min_depth, Buf& emit, Buf& scan,
                   Buf& stats, Buf& noffs, Buf& out, uint64_t* nout) {
    const size_t nst = sizeof(bella_consensus_read) * std::max<size_t>(nseq, 1);
    ENSURE(c, emit, (size_t)total + 1); ENSURE(c, scan, 8 * ((size_t)total + 1));
    ENSURE(c, noffs, 8 * ((size_t)nseq + 1)); ENSURE(c, stats, nst);
    HIPCHK(c, hipMemsetAsync(stats.p, 0, nst, c->stream));
    HIPCHK(c, hipMemsetAsync(ptr<uint8_t>(emit) + total, 0, 1, c->stream));
    if (total) {
        k_cons_decide<<<nblk(total), 256, 0, c->stream>>>(ptr<uint32_t>(table), packed, ptr<uint64_t>(offs), nseq, total, min_depth, ptr<uint8_t>(emit),
                                                          ptr<bella_consensus_read>(stats));
        KCHK(c);
    }
    {
        hipcub::TransformInputIterator<uint64_t, EmitCount, const uint8_t*> it(ptr<uint8_t>(emit), EmitCount());
        CUB(c, hipcub::DeviceScan::ExclusiveSum, it, ptr<uint64_t>(scan), (int)(total + 1), c->stream);
    }
    HIPCHK(c, hipMemcpyAsync(nout, ptr<uint64_t>(scan) + total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ENSURE(c, out, (size_t)*nout);
    if (total) {
        k_cons_write<<<nblk(total), 256, 0, c->stream>>>(ptr<uint8_t>(emit), ptr<uint64_t>(scan), total, ptr<uint8_t>(out));
        KCHK(c);
    }
    k_cons_reads<<<nblk((uint64_t)nseq + 1), 256, 0, c->stream>>>(ptr<uint64_t>(offs), ptr<uint64_t>(scan), nseq, ptr<uint64_t>(noffs), ptr<bella_consensus_read>(stats));
    KCHK(c);
    return 0;
}

// ---- what the realignment rounds (section 18) and the correction rounds (section 20) share -----------------------------------------------
int check_round_params(bella_ctx* c, const char* who, uint32_t band0, uint32_t band_max, uint32_t min_depth, uint32_t min_identity) {
    auto pow2 = [](uint32_t x) { return x && !(x & (x - 1)); };
    if (!pow2(band0) || !pow2(band_max) || band0 < kTrMinBand || band_max > kTrMaxBand || band0 > band_max)
        return fail(c, BELLA_ERR_BAD_ARG, "%s: band0 and band_max must be powers of two with 256 <= band0 <= band_max <= 262144", who);
    if (min_depth < 1) return fail(c, BELLA_ERR_BAD_ARG, "min_depth must be >= 1");
    if (min_identity > 1000) return fail(c, BELLA_ERR_BAD_ARG, "min_identity is in permille: at most 1000");
    return 0;
}

// direction bytes of a batch: BELLA_TUNE_ROUND_BUDGET as given, else half of what is free, 64 MB .. 8 GB
int round_budget(bella_ctx* c, uint64_t* budget) {
    size_t mfree = 0, mtotal = 0;
    if (!c->tune_round_budget) HIPCHK(c, hipMemGetInfo(&mfree, &mtotal));
    *budget = c->tune_round_budget ? c->tune_round_budget : std::max<uint64_t>(64ull << 20, std::min<uint64_t>((uint64_t)mfree / 2, 8ull << 30));
    return 0;
}

// What a family's sweep stores and keeps: direction bits per cell, scratch ints of the wide kernel per job and band cell, the two walks.
// The linear families (ReaFamily, LnkFamily, PalGlobal, PalSemi): 2 bits, two rows of B ints, k_rea_count / k_rea_write; an affine family
// (pairalign.hpp; section 29) states its own, and its DP kernels take the scores.
template <class Family, class = void>
struct BandTraits {
    static constexpr bool affine = false;
    static constexpr uint32_t dir_bits = 2, scr_ints = 2;
    static constexpr auto count() { return k_rea_count<typename Family::Res>; }
    static constexpr auto write() { return k_rea_write<typename Family::Res>; }
};
template <class Family>
struct BandTraits<Family, std::enable_if_t<Family::affine>> {
    static constexpr bool affine = true;
    static constexpr uint32_t dir_bits = Family::dir_bits, scr_ints = Family::scr_ints;
    static constexpr auto count() { return Family::count(); }
    static constexpr auto write() { return Family::write(); }
};

// jobs of a batch at most: the wide kernel keeps scr_ints rows of B ints per job in scratch (two: the linear sweep), and a batch's scratch
// stays within the budget too
uint32_t round_max_jobs(uint32_t B, uint64_t budget, uint32_t scr_ints = 2) {
    return B > kTrRegBand ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kRecMaxBatch, budget / (4ull * scr_ints * B))) : kRecMaxBatch;
}

// A round's batches on the device.  The round cuts a batch -- `nj` jobs of band `B` in `jobs`, `dbytes` direction bytes -- and owns what
// happens between the two steps: the read-backs, what becomes of every job, the jobs' op_off.  Family: ReaFamily (realign.hpp),
// LnkFamily (links.hpp) or one of pairalign.hpp's -- what the DP leaves per job, the DP kernels, whether the runs vote.
template <class Family>
struct RoundBatches {
    using Res = typename Family::Res;
    using Traits = BandTraits<Family>;
    bella_ctx* c;
    const char *who, *unit;                                           // for the messages: "realign" and its "reads", "recorrect" and its "jobs"
    EventSet& ev;
    const uint32_t *rpacked, *upacked;
    uint32_t* table;
    unsigned long long* votes;
    bool keep_ops;
    std::vector<uint32_t>& kept;                                      // ... where the ops of every batch are appended
    double &dp_ms, &walk_ms, &vote_ms;
    TmpBuf jobs, res, cnt, dirs, scr, ops;
    AfnScore score{1, 1, 0, 1};                                       // an affine family's scores (section 29); the linear kernels take none

    // DP and the counting walk.  The caller launches what is its own behind them, records ev.d, reads back, waits, and calls counted().
    int dp_count(uint32_t nj, uint32_t B, uint64_t dbytes) {
        ENSURE(c, res, sizeof(Res) * (size_t)nj); ENSURE(c, cnt, sizeof(ReaCnt) * (size_t)nj);
        if (ensure_bytes(c, dirs, (size_t)dbytes))
            return fail(c, BELLA_ERR_NOMEM, "%s: %llu direction bytes for a batch of %u %s do not fit", who, (unsigned long long)dbytes, nj, unit);
        if (B > kTrRegBand) ENSURE(c, scr, 4 * (size_t)Traits::scr_ints * nj * B);
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        auto launch = [&](auto kernel, uint32_t grid, uint32_t block, auto... args) {      // an affine family's kernels take the scores last
            if constexpr (Traits::affine) kernel<<<grid, block, 0, c->stream>>>(args..., score);
            else kernel<<<grid, block, 0, c->stream>>>(args...);
        };
        for_band(B, [&](auto C, uint32_t) {
            if constexpr (decltype(C)::value != 0)
                launch(Family::template dp<decltype(C)::value>(), nblk((uint64_t)nj * 64, kTraceBlock), kTraceBlock, ptr<ReaJob>(jobs), nj, rpacked, upacked, ptr<uint8_t>(dirs), ptr<Res>(res));
            else launch(Family::dp_wide(), nj, 64u, ptr<ReaJob>(jobs), nj, rpacked, upacked, ptr<uint8_t>(dirs), ptr<int>(scr), ptr<Res>(res));
        });
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        Traits::count()<<<nblk(nj), 256, 0, c->stream>>>(ptr<ReaJob>(jobs), ptr<Res>(res), nj, rpacked, upacked, ptr<uint8_t>(dirs), ptr<ReaCnt>(cnt));
        KCHK(c);
        return 0;
    }
    void counted() { dp_ms += ev_ms(ev.a, ev.b); walk_ms += ev_ms(ev.b, ev.d); }

    // the writing walk and the votes of a batch with ops (the jobs' op_off set); waits for the device
    int write_vote(uint32_t nj, uint64_t nops) {
        ENSURE(c, ops, 4 * (size_t)nops);
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        Traits::write()<<<nblk(nj), 256, 0, c->stream>>>(ptr<ReaJob>(jobs), ptr<Res>(res), ptr<ReaCnt>(cnt), nj, rpacked, upacked, ptr<uint8_t>(dirs), ptr<uint32_t>(ops));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        if constexpr (Family::votes) {
            k_rea_vote<<<nblk((uint64_t)nj * 64, kPileBlock), kPileBlock, 0, c->stream>>>(ptr<ReaJob>(jobs), ptr<ReaCnt>(cnt), nj, ptr<uint32_t>(ops), rpacked, table, votes);
            KCHK(c);
        }
        HIPCHK(c, hipEventRecord(ev.d, c->stream));
        if (keep_ops) {
            const size_t at = kept.size();
            kept.resize(at + (size_t)nops);
            HIPCHK(c, c->stager.d2h(kept.data() + at, ops.p, 4 * (size_t)nops, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        walk_ms += ev_ms(ev.a, ev.b);
        vote_ms += ev_ms(ev.b, ev.d);
        return 0;
    }
};
}  // namespace

extern "C" {

int bella_hip_pileup_reset(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, READS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->total_bases * kPileCounters * 4;
    drop(c, PILE);
    if (ensure_bytes(c, c->pile, bytes))
        return fail(c, BELLA_ERR_NOMEM, "the pileup table needs %zu bytes of device memory (36 per base of %llu bases) and they do not fit", bytes,
                    (unsigned long long)c->total_bases);
    HIPCHK(c, hipMemsetAsync(c->pile.p, 0, bytes ? bytes : 16, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    made(c, PILE);
    return 0;
}

int bella_hip_get_pileup_bytes(bella_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return BELLA_ERR_BAD_ARG;
    *bytes = has(c, PILE) ? (uint64_t)c->total_bases * kPileCounters * 4 : 0;
    return 0;
}

int bella_hip_get_vote_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    return put_sized(out, struct_size, c->vote_stats);
}

int bella_hip_pileup_vote(bella_ctx* c, const bella_vote_pair* pairs, uint64_t npairs, const uint32_t* ops, uint64_t nops_total, uint32_t flags) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if ((npairs && !pairs) || (nops_total && !ops)) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: null argument");
    if (flags & ~BELLA_TRACE_NORMALIZE) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: flags is 0 or BELLA_TRACE_NORMALIZE");
    if (npairs > 0xffffffffull) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: at most 2^32 - 1 pairs a call");
    if (int r = need(c, PILE)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint64_t> off((size_t)c->nreads + 1);
    HIPCHK(c, hipMemcpy(off.data(), c->roff.p, 8 * ((size_t)c->nreads + 1), hipMemcpyDeviceToHost));
    // ---- everything is checked before anything is launched
    std::vector<PilePair> vp;
    vp.reserve((size_t)npairs);
    bella_vote_stats vs{};
    vs.normalized = flags ? 1u : 0u;
    for (uint64_t q = 0; q < npairs; ++q) {
        const bella_vote_pair& a = pairs[q];
        if (a.rid >= c->nreads || a.cid >= c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu: read id out of range", (unsigned long long)q);
        if (a.strand > 1) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu: strand must be 0 or 1", (unsigned long long)q);
        if (a.op_off > nops_total || a.nops > nops_total - a.op_off) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu: its runs lie outside ops", (unsigned long long)q);
        if (a.tbegV < 0 || a.tbegH < 0) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu: negative start", (unsigned long long)q);
        const uint64_t lenV = off[a.cid + 1] - off[a.cid], lenH = off[a.rid + 1] - off[a.rid];
        uint64_t i = (uint64_t)a.tbegV, j = (uint64_t)a.tbegH;
        for (uint32_t k = 0; k < a.nops; ++k) {
            const uint32_t w = ops[a.op_off + k], op = w & 15u, len = w >> 4;
            if (op > kOpDel) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu run %u: op %u is none of = X I D", (unsigned long long)q, k, op);
            if (!len) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu run %u: length 0", (unsigned long long)q, k);
            if (op != kOpDel) i += len;
            if (op != kOpIns) j += len;
        }
        if (i > lenV || j > lenH) return fail(c, BELLA_ERR_BAD_ARG, "pileup_vote: pair %llu: its runs leave a read", (unsigned long long)q);
        if (!a.nops) continue;
        vp.push_back(PilePair{off[a.cid], off[a.rid], a.op_off, a.nops, (uint32_t)lenV, (uint32_t)lenH, (uint32_t)a.strand, a.tbegV, a.tbegH});
        vs.pairs++;
        vs.runs += a.nops;
    }
    changed(c, PILE);
    if (!vp.empty()) {
        TmpBuf dp, dops;
        EventSet ev;
        if (int r = ev.create(c, 2)) return r;
        ENSURE(c, dp, sizeof(PilePair) * vp.size());
        ENSURE(c, dops, 4 * (size_t)nops_total);
        ENSURE(c, c->pile_cnt, sizeof(PileNormCnt));
        HIPCHK(c, hipMemsetAsync(c->pile_cnt.p, 0, sizeof(PileNormCnt), c->stream));
        HIPCHK(c, hipMemcpyAsync(dp.p, vp.data(), sizeof(PilePair) * vp.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dops.p, ops, 4 * (size_t)nops_total, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        launch_pile_vote(c, flags != 0, ptr<PilePair>(dp), vp.size(), ptr<uint32_t>(dops));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        if (int r = read_vote_counts(c, vs)) return r;                // (waits: vp and the caller's ops are free again)
        vs.vote_ms = ev_ms(ev.a, ev.b);
    }
    c->vote_stats = vs;
    return 0;
}

// counters [*first, *first + *count) of the table = the reads [first_read, first_read + nreads)
static int pileup_range(bella_ctx* c, uint32_t first_read, uint32_t nreads, uint64_t* first, uint64_t* count) {
    if (int r = need(c, PILE)) return r;
    if ((uint64_t)first_read + nreads > c->nreads) return fail(c, BELLA_ERR_BAD_ARG, "reads [%u, %u + %u) out of range", first_read, first_read, nreads);
    uint64_t a = 0, b = 0;
    for (uint32_t r = 0; r < first_read + nreads; ++r) { if (r < first_read) a += c->host_lens[r]; b += c->host_lens[r]; }
    *first = a * kPileCounters;
    *count = (b - a) * kPileCounters;
    return 0;
}

int bella_hip_get_pileup(bella_ctx* c, uint32_t first_read, uint32_t nreads, uint32_t* out) {
    if (!c) return BELLA_ERR_BAD_ARG;
    uint64_t first = 0, count = 0;
    const int rc = pileup_range(c, first_read, nreads, &first, &count);
    if (rc) return rc;
    if (!count) return 0;
    if (!out) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->stager.d2h(out, ptr<uint32_t>(c->pile) + first, 4 * (size_t)count, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bella_hip_add_pileup(bella_ctx* c, uint32_t first_read, uint32_t nreads, const uint32_t* in) {
    if (!c) return BELLA_ERR_BAD_ARG;
    uint64_t first = 0, count = 0;
    const int rc = pileup_range(c, first_read, nreads, &first, &count);
    if (rc) return rc;
    if (!count) return 0;
    if (!in) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    changed(c, PILE);
    constexpr uint64_t kChunk = 16ull << 20;                          // counters per step: 64 MB of device scratch whatever the range
    ENSURE(c, c->pile_tmp, 4 * (size_t)std::min(kChunk, count));
    for (uint64_t o = 0; o < count; o += kChunk) {
        const uint64_t n = std::min(kChunk, count - o);
        HIPCHK(c, c->stager.h2d(c->pile_tmp.p, in + o, 4 * (size_t)n, c->stream));
        k_pile_add<<<nblk(n), 256, 0, c->stream>>>(ptr<uint32_t>(c->pile) + first + o, ptr<uint32_t>(c->pile_tmp), n);
        KCHK(c);
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    release(c->pile_tmp);
    return 0;
}

int bella_hip_consensus(bella_ctx* c, const bella_consensus_params* params, uint64_t* total_bases) {
    if (!c || !params) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    bella_consensus_params cp{};                                      // (no defaults: NULL was refused)
    if (int r = take_params(c, cp, params, "bella_consensus_params")) return r;
    if (cp.min_depth < 1) return fail(c, BELLA_ERR_BAD_ARG, "min_depth must be >= 1");
    if (int r = need(c, PILE)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, CONS);
    const uint64_t total = c->total_bases;
    const uint32_t nr = c->nreads;
    if (total >= 0x7FFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "consensus: the read set must have fewer than 2^31 bases");
    uint64_t nout = 0;
    if (int r = consensus_tail(c, c->pile, ptr<uint32_t>(c->packed), c->roff, nr, total, cp.min_depth, c->cons_emit, c->cons_scan, c->cons_stats, c->cons_offs, c->cons_out, &nout))
        return r;
    std::vector<uint64_t> aoff((size_t)nr + 1, 0);
    {   // the anchors of the correction rounds (section 20): where every 256th raw base went, from the scan before it is released
        for (uint32_t r = 0; r < nr; ++r) aoff[r + 1] = aoff[r] + rec_nanchors(c->host_lens[r]);
        c->rc_nanch = aoff[nr];
        ENSURE(c, c->rc_aoff, 8 * ((size_t)nr + 1));
        ENSURE(c, c->cons_anch, 8 * (size_t)c->rc_nanch);
        HIPCHK(c, c->stager.h2d(c->rc_aoff.p, aoff.data(), 8 * ((size_t)nr + 1), c->stream));
        if (nr) {
            k_rec_anchors<<<nblk(c->rc_nanch), 256, 0, c->stream>>>(ptr<uint64_t>(c->roff), ptr<uint64_t>(c->cons_scan), ptr<uint64_t>(c->rc_aoff), nullptr, nr, c->rc_nanch,
                                                                  ptr<uint64_t>(c->cons_anch));
            KCHK(c);
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release(c->cons_emit);
    release(c->cons_scan);
    c->cons_total = nout;
    made(c, CONS);
    if (total_bases) *total_bases = nout;
    return 0;
}

int bella_hip_get_consensus(bella_ctx* c, uint64_t* offsets, uint8_t* bases, bella_consensus_read* stats) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, CONS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (offsets) HIPCHK(c, c->stager.d2h(offsets, c->cons_offs.p, 8 * ((size_t)c->nreads + 1), c->stream));
    if (bases && c->cons_total) HIPCHK(c, c->stager.d2h(bases, c->cons_out.p, (size_t)c->cons_total, c->stream));
    if (stats && c->nreads) HIPCHK(c, c->stager.d2h(stats, c->cons_stats.p, sizeof(bella_consensus_read) * (size_t)c->nreads, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bella_hip_write_fasta(const char* path, uint32_t nreads, const char* const* names, const uint64_t* offsets, const uint8_t* bases, int append) {
    if (!path || (nreads && (!names || !offsets)) || (nreads && offsets[nreads] && !bases)) {
        fprintf(stderr, "bella_hip_write_fasta: null argument\n");
        return BELLA_ERR_BAD_ARG;
    }
    TextFile file("bella_hip_write_fasta", path, append ? "ab" : "wb");
    FILE* const f = file.f;
    if (!f) return BELLA_ERR_BAD_ARG;
    bool ok = true;
    for (uint32_t r = 0; r < nreads && ok; ++r) {
        if (!names[r] || offsets[r + 1] < offsets[r]) { ok = false; break; }
        const size_t n = (size_t)(offsets[r + 1] - offsets[r]);
        ok = std::fputc('>', f) != EOF && std::fputs(names[r], f) != EOF && std::fputc('\n', f) != EOF && (n == 0 || std::fwrite(bases + offsets[r], 1, n, f) == n) &&
             std::fputc('\n', f) != EOF;
    }
    return file.close(ok);
}

// ---- string graph (graph.hpp) ----------------------------------------------------------------------------------
int bella_hip_graph_reset(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    std::vector<bella_overlap>().swap(c->as.records);
    changed(c, RECORDS);
    return 0;
}

int bella_hip_graph_add_overlaps(bella_ctx* c, const bella_overlap* recs, uint64_t n) {
    if (!c || (n && !recs)) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    if (int r = need(c, READS)) return r;
    if (c->as.records.size() + n >= (1ull << 30)) return fail(c, BELLA_ERR_BAD_ARG, "graph: fewer than 2^30 overlap records");
    for (uint64_t i = 0; i < n; ++i) {
        const bella_overlap& r = recs[i];
        if (r.cid == r.rid || r.cid >= c->nreads || r.rid >= c->nreads || r.strand > 1)
            return fail(c, BELLA_ERR_BAD_ARG, "overlap record %llu: reads %u and %u (of %u), strand %u", (unsigned long long)i, r.cid, r.rid, c->nreads, (unsigned)r.strand);
        const int64_t l1 = c->host_lens[r.cid], l2 = c->host_lens[r.rid];
        if (r.begV < 0 || r.begV >= r.endV || r.endV > l1 || r.begH < 0 || r.begH >= r.endH || r.endH > l2)
            return fail(c, BELLA_ERR_BAD_ARG, "overlap record %llu: [%d, %d) of %lld bases and [%d, %d) of %lld", (unsigned long long)i, r.begV, r.endV, (long long)l1, r.begH,
                        r.endH, (long long)l2);
    }
    c->as.records.insert(c->as.records.end(), recs, recs + n);
    changed(c, RECORDS);                                              // (the clips were those of the records before)
    return 0;
}

int bella_hip_graph_add_traced(bella_ctx* c, uint64_t* added) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TRACES)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->nalns;
    if (c->traces.size() != n) return fail(c, BELLA_ERR_STATE, "the traces are not those of the last alignment");
    std::vector<bella_pair> pairs(n);
    std::vector<bella_aln> alns(n);
    if (n) {
        HIPCHK(c, c->stager.d2h(pairs.data(), c->pairs.p, sizeof(bella_pair) * n, c->stream));
        HIPCHK(c, c->stager.d2h(alns.data(), c->alns.p, sizeof(bella_aln) * n, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    std::vector<bella_overlap> recs;
    for (size_t i = 0; i < n; ++i) {
        const bella_trace& t = c->traces[i];
        if (!alns[i].passed || !t.nops) continue;
        bella_overlap r{};
        r.cid = pairs[i].cid; r.rid = pairs[i].rid;
        r.begV = t.tbegV; r.endV = t.tendV; r.begH = t.tbegH; r.endH = t.tendH;
        r.score = alns[i].score;
        r.strand = alns[i].strand ? 1 : 0;
        recs.push_back(r);
    }
    const int rc = bella_hip_graph_add_overlaps(c, recs.data(), recs.size());
    if (rc) return rc;
    if (added) *added = recs.size();
    return 0;
}

int bella_hip_graph_get_overlaps(bella_ctx* c, bella_overlap* out, uint64_t* n) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (n) *n = c->as.records.size();
    copy_out(out, c->as.records);
    return 0;
}

int bella_hip_graph_build(bella_ctx* c, const bella_graph_params* params) {
    using clk = std::chrono::steady_clock;
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_graph_params gp{(uint32_t)sizeof(bella_graph_params), 1000, 1000, 800, 1000};
    if (int r = take_params(c, gp, params, "bella_graph_params")) return r;
    if (int r = need(c, READS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const auto t_begin = clk::now();
    drop(c, GRAPH);
    StageState::Graph& g = c->as.graph;
    const uint32_t nr = c->nreads, nv = 2 * nr;
    const uint32_t n = (uint32_t)c->as.records.size(), nc = 2 * n;
    if (nr >= (1u << 30)) return fail(c, BELLA_ERR_BAD_ARG, "graph: fewer than 2^30 reads");
    bella_graph_stats st{};
    st.records = n;
    TmpBuf recs, cand, cont, cnt, ok, deg, off, key1, key1b, idx, idxb, key2, key2b, edges, pos, bykey, bykeyb, gmark, red, keep, scan, fin, foff;
    ENSURE(c, cand, sizeof(bella_graph_edge) * (size_t)nc);
    ENSURE(c, cont, 4 * (size_t)nr);
    ENSURE(c, cnt, 4 * kGcCount);
    ENSURE(c, ok, nc);
    ENSURE(c, deg, 4 * ((size_t)nv + 1));
    ENSURE(c, off, 4 * ((size_t)nv + 1));
    ENSURE(c, key1, 4 * (size_t)nc); ENSURE(c, key1b, 4 * (size_t)nc);
    ENSURE(c, idx, 4 * (size_t)nc); ENSURE(c, idxb, 4 * (size_t)nc);
    ENSURE(c, key2, 8 * (size_t)nc); ENSURE(c, key2b, 8 * (size_t)nc);
    ENSURE(c, pos, 4 * (size_t)nc);
    uint32_t* const d_cnt = ptr<uint32_t>(cnt);
    EventSet ev;
    if (int r = ev.create(c, 4)) return r;
    if (int r = upload_records(c, recs)) return r;
    HIPCHK(c, hipMemsetAsync(cont.p, 0, std::max<size_t>(4 * (size_t)nr, 16), c->stream));
    TmpBuf clipb;
    const bella_read_clip* d_clip = nullptr;                              // the clips of bella_hip_graph_trim, while they exist
    if (has(c, TRIM) && nr) {
        if (int r = upload_clips(c, clipb)) return r;
        d_clip = ptr<bella_read_clip>(clipb);
        k_trim_flags<<<nblk(nr), 256, 0, c->stream>>>(d_clip, nr, ptr<uint32_t>(cont));
        KCHK(c);
    }
    HIPCHK(c, hipMemsetAsync(cnt.p, 0, 4 * kGcCount, c->stream));
    HIPCHK(c, hipMemsetAsync(deg.p, 0, 4 * ((size_t)nv + 1), c->stream));
    // ---- classes
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (n) {
        k_graph_classify<<<nblk(n), 256, 0, c->stream>>>(ptr<bella_overlap>(recs), n, ptr<uint64_t>(c->roff), d_clip, gp.min_overlap, gp.max_overhang, gp.overhang_permille,
                                                         ptr<bella_graph_edge>(cand), ptr<uint32_t>(cont), d_cnt);
        KCHK(c);
    }
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    // ---- lists: filter, degrees, scan, two stable sorts, gather
    if (nc) {
        k_graph_filter<<<nblk(nc), 256, 0, c->stream>>>(ptr<bella_graph_edge>(cand), nc, ptr<uint32_t>(cont), ptr<uint8_t>(ok), ptr<uint32_t>(deg), ptr<uint32_t>(key1),
                                                        ptr<uint32_t>(idx), d_cnt);
        KCHK(c);
    }
    int rc = scan_u32(c, ptr<uint32_t>(deg), ptr<uint32_t>(off), (uint64_t)nv + 1);
    if (rc) return rc;
    if (nc) {
        CUB(c, hipcub::DeviceRadixSort::SortPairs, ptr<uint32_t>(key1), ptr<uint32_t>(key1b), ptr<uint32_t>(idx), ptr<uint32_t>(idxb), (int)nc, 0, 32, c->stream);
        k_graph_key2<<<nblk(nc), 256, 0, c->stream>>>(ptr<bella_graph_edge>(cand), ptr<uint8_t>(ok), ptr<uint32_t>(idxb), nc, ptr<uint64_t>(key2));
        KCHK(c);
        CUB(c, hipcub::DeviceRadixSort::SortPairs, ptr<uint64_t>(key2), ptr<uint64_t>(key2b), ptr<uint32_t>(idxb), ptr<uint32_t>(idx), (int)nc, 0, 64, c->stream);
    }
    uint32_t hc[kGcCount] = {};
    HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kGcCount, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint32_t m = hc[kGcEdgesKept];
    ENSURE(c, edges, sizeof(bella_graph_edge) * (size_t)m);
    ENSURE(c, bykey, 8 * (size_t)m); ENSURE(c, bykeyb, 8 * (size_t)m);
    if (m) {
        k_graph_gather<<<nblk(m), 256, 0, c->stream>>>(ptr<bella_graph_edge>(cand), ptr<uint32_t>(idx), m, ptr<bella_graph_edge>(edges), ptr<uint32_t>(pos), ptr<uint64_t>(bykey));
        KCHK(c);
    }
    k_graph_vertex_stats<<<nblk((uint64_t)nv + 1), 256, 0, c->stream>>>(ptr<uint32_t>(off), nv, ptr<uint32_t>(cont), nr, kGraphLdsCap, d_cnt);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kGcCount, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool force_global = (c->debug & (1u << 19)) != 0;
    const bool need_global = m && (force_global || hc[kGcOvercap] != 0);
    const uint64_t* d_bykey = nullptr;
    if (need_global) {                                                    // the over-cap path's neighbour sets: every vertex's dst values, ascending
        CUB(c, hipcub::DeviceRadixSort::SortKeys, ptr<uint64_t>(bykey), ptr<uint64_t>(bykeyb), (int)m, 0, 64, c->stream);
        d_bykey = ptr<uint64_t>(bykeyb);
        ENSURE(c, gmark, m);
    }
    HIPCHK(c, hipEventRecord(ev.d, c->stream));
    // ---- reduction, twin pass, compaction
    ENSURE(c, red, (size_t)m + 1);
    ENSURE(c, keep, (size_t)m + 1);
    ENSURE(c, scan, 4 * ((size_t)m + 1));
    ENSURE(c, foff, 4 * ((size_t)nv + 1));
    HIPCHK(c, hipMemsetAsync(red.p, 0, (size_t)m + 1, c->stream));
    if (m) {
        k_graph_reduce<<<nblk(nv, kGraphBlock / 64), kGraphBlock, 0, c->stream>>>(ptr<uint32_t>(off), ptr<bella_graph_edge>(edges), nv, gp.fuzz, force_global ? 1u : 0u, d_bykey,
                                                                                 need_global ? ptr<uint8_t>(gmark) : nullptr, ptr<uint8_t>(red), d_cnt);
        KCHK(c);
    }
    k_graph_symmetric<<<nblk((uint64_t)m + 1), 256, 0, c->stream>>>(ptr<bella_graph_edge>(edges), m, ptr<uint32_t>(pos), ptr<uint8_t>(red), ptr<uint8_t>(keep));
    KCHK(c);
    rc = scan_u8_to_u32(c, ptr<uint8_t>(keep), ptr<uint32_t>(scan), (uint64_t)m + 1);
    if (rc) return rc;
    uint32_t nfinal = 0;
    HIPCHK(c, hipMemcpyAsync(&nfinal, ptr<uint32_t>(scan) + m, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kGcCount, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hc[kGcDuplicate]) return fail(c, BELLA_ERR_BAD_ARG, "graph: two overlap records for one read pair (an edge's source and target must be unique)");
    ENSURE(c, fin, sizeof(bella_graph_edge) * (size_t)nfinal);
    if (m) {
        k_graph_compact<<<nblk(m), 256, 0, c->stream>>>(ptr<bella_graph_edge>(edges), ptr<uint8_t>(keep), ptr<uint32_t>(scan), m, ptr<bella_graph_edge>(fin));
        KCHK(c);
    }
    k_graph_new_offsets<<<nblk((uint64_t)nv + 1), 256, 0, c->stream>>>(ptr<uint32_t>(off), ptr<uint32_t>(scan), nv, ptr<uint32_t>(foff));
    KCHK(c);
    HIPCHK(c, hipEventRecord(ev.e, c->stream));
    g.off.assign((size_t)nv + 1, 0);
    g.edges.assign(nfinal, bella_graph_edge{});
    std::vector<uint32_t> cont32(nr);
    HIPCHK(c, hipMemcpyAsync(g.off.data(), foff.p, 4 * ((size_t)nv + 1), hipMemcpyDeviceToHost, c->stream));
    if (nfinal) HIPCHK(c, c->stager.d2h(g.edges.data(), fin.p, sizeof(bella_graph_edge) * (size_t)nfinal, c->stream));
    if (nr) HIPCHK(c, hipMemcpyAsync(cont32.data(), cont.p, 4 * (size_t)nr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    g.contained.resize(nr);
    for (uint32_t r = 0; r < nr; ++r) g.contained[r] = (uint8_t)cont32[r];    // 1 contained; 2 uncovered (only with clips)
    if (has(c, TRIM)) c->as.trim.stats.records_outside = hc[kGcOutside];
    st.n_short = hc[kGcShort]; st.n_internal = hc[kGcInternal]; st.contained_reads = hc[kGcContained];
    st.edges_all = hc[kGcEdgesAll]; st.edges_kept = m; st.edges_reduced = hc[kGcReduced]; st.edges_final = nfinal;
    st.max_degree = hc[kGcMaxDegree]; st.overcap_vertices = hc[kGcOvercap];
    st.classify_ms = ev_ms(ev.a, ev.b); st.sort_ms = ev_ms(ev.b, ev.d); st.reduce_ms = ev_ms(ev.d, ev.e);
    st.host_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    g.stats = st;
    g.removed.assign(nr, 0);
    g.clean = bella_unitig_stats{};
    g.bubbles = bella_bubble_stats{};
    g.weak = bella_weak_stats{};
    c->as.unitigs.stats = bella_unitig_stats{};
    made(c, GRAPH);
    return 0;
}

int bella_hip_graph_get(bella_ctx* c, uint32_t* nvertices, uint64_t* nedges, uint64_t* offsets, bella_graph_edge* edges, uint8_t* contained) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, GRAPH)) return r;
    const StageState::Graph& g = c->as.graph;
    if (nvertices) *nvertices = (uint32_t)(g.off.size() - 1);
    if (nedges) *nedges = g.edges.size();
    if (offsets) std::copy(g.off.begin(), g.off.end(), offsets);      // (the ABI's offsets are 64 bits wide)
    copy_out(edges, g.edges);
    copy_out(contained, g.contained);
    return 0;
}

int bella_hip_graph_get_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, GRAPH, out, struct_size, [](const StageState& a) { return a.graph.stats; });
}

// ---- coverage trimming (trim.hpp) ------------------------------------------------------------------------------
int bella_hip_graph_trim(bella_ctx* c, const bella_graph_trim_params* params) {
    using clk = std::chrono::steady_clock;
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_graph_trim_params tp{(uint32_t)sizeof(bella_graph_trim_params), 3, 500, 1000};
    if (int r = take_params(c, tp, params, "bella_graph_trim_params")) return r;
    if (tp.min_depth < 1 || tp.min_depth > 0x7FFFFFFFu) return fail(c, BELLA_ERR_BAD_ARG, "trim: min_depth must be in [1, 2^31)");
    if (tp.end_clip >= (1u << 16)) tp.end_clip = 1u << 16;            // (no read is that long: the same result, and the sums stay small)
    if (int r = need(c, READS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const auto t_begin = clk::now();
    drop(c, TRIM);
    StageState::Trim& t = c->as.trim;
    const uint32_t nr = c->nreads, n = (uint32_t)c->as.records.size();
    if (nr >= (1u << 30)) return fail(c, BELLA_ERR_BAD_ARG, "graph: fewer than 2^30 reads");
    if (n >= (1u << 29)) return fail(c, BELLA_ERR_BAD_ARG, "trim: fewer than 2^29 overlap records (four sort keys each)");
    const uint64_t nkeys = 4 * (uint64_t)n;
    bella_trim_stats st{};
    t.clips.assign(nr, bella_read_clip{0, 0, 0, 0});
    uint32_t nint = 0;
    if (n && nr) {
        TmpBuf recs, keys, keysb, evoff, clip, cnt;
        ENSURE(c, keys, 8 * (size_t)nkeys); ENSURE(c, keysb, 8 * (size_t)nkeys);
        ENSURE(c, evoff, 4 * ((size_t)nr + 1));
        ENSURE(c, clip, sizeof(bella_read_clip) * (size_t)nr);
        ENSURE(c, cnt, 4);
        EventSet ev;
        if (int r = ev.create(c, 4)) return r;
        if (int r = upload_records(c, recs)) return r;
        HIPCHK(c, hipMemsetAsync(cnt.p, 0, 4, c->stream));
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        k_trim_events<<<nblk(n), 256, 0, c->stream>>>(ptr<bella_overlap>(recs), n, ptr<uint64_t>(c->roff), tp.end_clip, tp.min_span, ptr<uint64_t>(keys), ptr<uint32_t>(cnt));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        int read_bits = 1;                                            // all ones in the sorted bits lies behind every read id
        while (((1ull << read_bits) - 1) < nr) ++read_bits;
        CUB(c, hipcub::DeviceRadixSort::SortKeys, ptr<uint64_t>(keys), ptr<uint64_t>(keysb), (int)nkeys, 0, 32 + read_bits, c->stream);
        k_trim_offsets<<<nblk((uint64_t)nr + 1), 256, 0, c->stream>>>(ptr<uint64_t>(keysb), nkeys, nr, ptr<uint32_t>(evoff));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.d, c->stream));
        k_trim_sweep<<<nblk(nr, kTrimBlock / 64), kTrimBlock, 0, c->stream>>>(ptr<uint64_t>(keysb), ptr<uint32_t>(evoff), nr, tp.min_depth, tp.min_span,
                                                                             ptr<bella_read_clip>(clip));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.e, c->stream));
        HIPCHK(c, c->stager.d2h(t.clips.data(), clip.p, sizeof(bella_read_clip) * (size_t)nr, c->stream));
        HIPCHK(c, hipMemcpyAsync(&nint, cnt.p, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.events_ms = ev_ms(ev.a, ev.b); st.sort_ms = ev_ms(ev.b, ev.d); st.sweep_ms = ev_ms(ev.d, ev.e);
    }
    st.intervals = nint;
    for (uint32_t r = 0; r < nr; ++r) {
        const bella_read_clip& k = t.clips[r];
        st.bases_before += c->host_lens[r];
        st.bases_after += k.end - k.beg;
        if (k.end == k.beg) ++st.reads_uncovered;
        else if (k.beg != 0 || k.end != c->host_lens[r]) ++st.reads_clipped;
        if (k.nregions >= 2) ++st.reads_multi;
    }
    st.host_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    t.stats = st;
    made(c, TRIM);
    return 0;
}

int bella_hip_graph_get_trim(bella_ctx* c, bella_read_clip* out) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, TRIM)) return r;
    copy_out(out, c->as.trim.clips);
    return 0;
}

int bella_hip_graph_get_trim_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, TRIM, out, struct_size, [](const StageState& a) { return a.trim.stats; });
}

int bella_hip_graph_untrim(bella_ctx* c) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (has(c, TRIM)) drop(c, TRIM);                                  // (no trim: the graph was built without one and stays)
    return 0;
}

}  // extern "C"

// ---- unitigs (unitig.hpp) -----------------------------------------------------------------------------------------
namespace {
// the context's current graph on the device: 32-bit offsets, the edges
int graph_upload(bella_ctx* c, Buf& off, Buf& edges) {
    const StageState::Graph& g = c->as.graph;
    const size_t nv1 = g.off.size(), m = g.edges.size();
    ENSURE(c, off, 4 * nv1);
    ENSURE(c, edges, sizeof(bella_graph_edge) * m);
    HIPCHK(c, c->stager.h2d(off.p, g.off.data(), 4 * nv1, c->stream));
    if (m) HIPCHK(c, c->stager.h2d(edges.p, g.edges.data(), sizeof(bella_graph_edge) * m, c->stream));
    return 0;
}

// Where every read's span begins and ends among all bases, for the kernels that read bases along the unitigs: roff and roff + 1 (whole
// reads), or the clipped spans while the context holds clips (trim.hpp).
struct ReadSpans {
    TmpBuf clipb, begs, ends;
    const uint64_t *beg = nullptr, *end = nullptr;
    int make(bella_ctx* c) {
        const uint32_t nr = c->nreads;
        beg = ptr<uint64_t>(c->roff); end = ptr<uint64_t>(c->roff) + 1;
        if (!has(c, TRIM) || !nr) return 0;
        if (int r = upload_clips(c, clipb)) return r;
        ENSURE(c, begs, 8 * (size_t)nr); ENSURE(c, ends, 8 * (size_t)nr);
        k_trim_spans<<<nblk(nr), 256, 0, c->stream>>>(ptr<bella_read_clip>(clipb), ptr<uint64_t>(c->roff), nr, ptr<uint64_t>(begs), ptr<uint64_t>(ends));
        KCHK(c);
        beg = ptr<uint64_t>(begs); end = ptr<uint64_t>(ends);
        return 0;
    }
};

// The context's unitigs on the device, for the kernels that go along their vertices (polish, realignment): the vertices, the unitig of
// every vertex slot, where a vertex's bases begin in its unitig, and the unitigs' offsets among the slots and among the bases.
struct UnitigLayout {
    TmpBuf verts, slot_utg, pos, uvoff, uboff;
    std::vector<uint32_t> slot;
    int upload(bella_ctx* c) {
        const StageState::Unitigs& u = c->as.unitigs;
        const size_t nutg = u.len.size(), nseg = u.verts.size();
        slot.resize(nseg);
        for (size_t j = 0; j < nutg; ++j)
            for (uint64_t i = u.voff[j]; i < u.voff[j + 1]; ++i) slot[(size_t)i] = (uint32_t)j;
        ENSURE(c, verts, 4 * nseg); ENSURE(c, slot_utg, 4 * nseg); ENSURE(c, pos, 8 * nseg);
        ENSURE(c, uvoff, 8 * (nutg + 1)); ENSURE(c, uboff, 8 * (nutg + 1));
        HIPCHK(c, c->stager.h2d(verts.p, u.verts.data(), 4 * nseg, c->stream));
        HIPCHK(c, c->stager.h2d(slot_utg.p, slot.data(), 4 * nseg, c->stream));
        HIPCHK(c, c->stager.h2d(pos.p, u.pos.data(), 8 * nseg, c->stream));
        HIPCHK(c, c->stager.h2d(uvoff.p, u.voff.data(), 8 * (nutg + 1), c->stream));
        HIPCHK(c, c->stager.h2d(uboff.p, u.boff.data(), 8 * (nutg + 1), c->stream));
        return 0;
    }
};

// What tip clipping and bubble popping share: the graph and the removed-read marks on the device, the buffers a round filters and
// compacts with, the stage's two events.  A stage marks the reads of a round in `hit` and owns everything else: its kernels, its
// counters, its read-backs and synchronisations.  Nothing here waits for the device but finish().
struct GraphRound {
    TmpBuf off, off2, E, E2, rem, hit, keep, scan;
    EventSet ev;
    uint32_t nr = 0, nv = 0, m = 0, m0 = 0;
    // upload, allocate, start the clock
    int begin(bella_ctx* c) {
        nr = c->nreads; nv = 2 * nr;
        m = m0 = (uint32_t)c->as.graph.edges.size();
        int rc = graph_upload(c, off, E);
        if (rc) return rc;
        ENSURE(c, off2, 4 * ((size_t)nv + 1));
        ENSURE(c, E2, sizeof(bella_graph_edge) * (size_t)m);
        ENSURE(c, hit, nr); ENSURE(c, rem, nr);
        ENSURE(c, keep, (size_t)m + 1);
        ENSURE(c, scan, 4 * ((size_t)m + 1));
        HIPCHK(c, hipMemcpyAsync(rem.p, c->as.graph.removed.data(), nr, hipMemcpyHostToDevice, c->stream));
        if ((rc = ev.create(c, 2))) return rc;
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        return 0;
    }
    // the edges that stay (no end of theirs in `hit`, not named by `ekill` when there is one) into `keep`, its scan, and how many they
    // are on the way into *kept
    int filter(bella_ctx* c, const uint8_t* ekill, uint32_t* kept) {
        k_graph_keep_filter<<<nblk((uint64_t)m + 1), 256, 0, c->stream>>>(ptr<bella_graph_edge>(E), m, ptr<uint8_t>(hit), ekill, ptr<uint8_t>(keep));
        KCHK(c);
        if (int rc = scan_u8_to_u32(c, ptr<uint8_t>(keep), ptr<uint32_t>(scan), (uint64_t)m + 1)) return rc;
        HIPCHK(c, hipMemcpyAsync(kept, ptr<uint32_t>(scan) + m, 4, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    // the kept edges become the graph; the caller sets m to the count it read back
    int apply_keep(bella_ctx* c) {
        k_graph_compact<<<nblk(m), 256, 0, c->stream>>>(ptr<bella_graph_edge>(E), ptr<uint8_t>(keep), ptr<uint32_t>(scan), m, ptr<bella_graph_edge>(E2));
        KCHK(c);
        k_graph_new_offsets<<<nblk((uint64_t)nv + 1), 256, 0, c->stream>>>(ptr<uint32_t>(off), ptr<uint32_t>(scan), nv, ptr<uint32_t>(off2));
        KCHK(c);
        E.swap(E2);
        off.swap(off2);
        return 0;
    }
    // stop the clock; the graph and the marks back into the context
    int finish(bella_ctx* c, uint64_t* edges_removed, double* ms) {
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        std::vector<uint32_t> offs((size_t)nv + 1);
        std::vector<bella_graph_edge> edges(m);
        std::vector<uint8_t> removed(nr);
        HIPCHK(c, hipMemcpyAsync(offs.data(), off.p, 4 * ((size_t)nv + 1), hipMemcpyDeviceToHost, c->stream));
        if (m) HIPCHK(c, c->stager.d2h(edges.data(), E.p, sizeof(bella_graph_edge) * (size_t)m, c->stream));
        HIPCHK(c, hipMemcpyAsync(removed.data(), rem.p, nr, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->as.graph.off.swap(offs);
        c->as.graph.edges.swap(edges);
        c->as.graph.removed.swap(removed);
        *edges_removed = m0 - m;
        *ms = ev_ms(ev.a, ev.b);
        return 0;
    }
};
}  // namespace

extern "C" {

int bella_hip_graph_clean(bella_ctx* c, const bella_graph_clean_params* params) {
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_graph_clean_params cp{(uint32_t)sizeof(bella_graph_clean_params), 4, 3};
    if (int r = take_params(c, cp, params, "bella_graph_clean_params")) return r;
    if (cp.tip_rounds > BELLA_MAX_TIP_ROUNDS) return fail(c, BELLA_ERR_BAD_ARG, "tip_rounds %u: at most %d", cp.tip_rounds, BELLA_MAX_TIP_ROUNDS);
    if (int r = need(c, GRAPH)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    changed(c, GRAPH);
    c->as.unitigs.stats = bella_unitig_stats{};
    bella_unitig_stats& st = c->as.graph.clean;
    st = bella_unitig_stats{};
    const uint32_t nr = c->nreads, nv = 2 * nr;
    if (!cp.max_tip_reads || !cp.tip_rounds) return 0;
    if (c->as.graph.edges.empty()) { st.rounds = 1; return 0; }       // (a round over no edges finds nothing)
    TmpBuf cnt;
    ENSURE(c, cnt, 4 * kUcCount);
    GraphRound g;
    int rc = g.begin(c);
    if (rc) return rc;
    for (uint32_t round = 0; round < cp.tip_rounds; ++round) {
        uint32_t hc[kUcCount] = {};
        HIPCHK(c, hipMemsetAsync(g.hit.p, 0, nr, c->stream));
        HIPCHK(c, hipMemsetAsync(cnt.p, 0, 4 * kUcCount, c->stream));
        k_tip_walk<<<nblk(nv), 256, 0, c->stream>>>(ptr<uint32_t>(g.off), ptr<bella_graph_edge>(g.E), nv, cp.max_tip_reads, ptr<uint8_t>(g.hit), ptr<uint32_t>(cnt));
        KCHK(c);
        k_graph_mark_reads<<<nblk(nr), 256, 0, c->stream>>>(ptr<uint8_t>(g.hit), nr, ptr<uint8_t>(g.rem), ptr<uint32_t>(cnt) + kUcReads);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kUcCount, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.tips_per_round[round] = hc[kUcTips];
        st.reads_per_round[round] = hc[kUcReads];
        st.rounds = round + 1;
        st.reads_removed += hc[kUcReads];
        if (!hc[kUcReads]) break;
        uint32_t nm = 0;
        if ((rc = g.filter(c, nullptr, &nm))) return rc;
        if ((rc = g.apply_keep(c))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        g.m = nm;
    }
    return g.finish(c, &st.edges_removed, &st.clean_ms);
}

int bella_hip_graph_get_removed(bella_ctx* c, uint8_t* removed) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, GRAPH)) return r;
    copy_out(removed, c->as.graph.removed);
    return 0;
}

// ---- bubble popping (bubble.hpp) ----
int bella_hip_graph_pop_bubbles(bella_ctx* c, const bella_graph_bubble_params* params) {
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_graph_bubble_params bp{(uint32_t)sizeof(bella_graph_bubble_params), 64, 50000, 3};
    if (int r = take_params(c, bp, params, "bella_graph_bubble_params")) return r;
    if (bp.bubble_rounds > BELLA_MAX_BUBBLE_ROUNDS) return fail(c, BELLA_ERR_BAD_ARG, "bubble_rounds %u: at most %d", bp.bubble_rounds, BELLA_MAX_BUBBLE_ROUNDS);
    if (bp.max_bubble_reads > BELLA_MAX_BUBBLE_READS) return fail(c, BELLA_ERR_BAD_ARG, "max_bubble_reads %u: at most %d", bp.max_bubble_reads, BELLA_MAX_BUBBLE_READS);
    if (int r = need(c, GRAPH)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    changed(c, GRAPH);
    bella_bubble_stats& st = c->as.graph.bubbles;
    st = bella_bubble_stats{};
    const uint32_t nr = c->nreads, nv = 2 * nr;
    const uint32_t m = (uint32_t)c->as.graph.edges.size();
    if (!bp.max_bubble_reads || !bp.bubble_rounds) return 0;
    if (!m) { st.rounds = 1; return 0; }                              // (a round over no edges finds nothing)
    TmpBuf list, claim, ekill, cnt;
    ENSURE(c, list, 4 * (size_t)nv);
    ENSURE(c, claim, 4 * (size_t)nr);
    ENSURE(c, ekill, (size_t)m + 1);
    ENSURE(c, cnt, 4 * kBcCount);
    GraphRound g;
    int rc = g.begin(c);
    if (rc) return rc;
    for (uint32_t round = 0; round < bp.bubble_rounds; ++round) {
        uint32_t hc[kBcCount] = {}, nm = 0;
        HIPCHK(c, hipMemsetAsync(g.hit.p, 0, nr, c->stream));
        HIPCHK(c, hipMemsetAsync(ekill.p, 0, (size_t)g.m + 1, c->stream));
        HIPCHK(c, hipMemsetAsync(claim.p, 0xFF, 4 * (size_t)nr, c->stream));
        HIPCHK(c, hipMemsetAsync(cnt.p, 0, 4 * kBcCount, c->stream));
        k_bub_sources<<<nblk(nv), 256, 0, c->stream>>>(ptr<uint32_t>(g.off), nv, ptr<uint32_t>(list), ptr<uint32_t>(cnt));
        KCHK(c);
        // one wavefront per listed source; the grid covers every vertex and the wavefronts past the list leave at once
        k_bub_detect<<<nblk(nv, kBubBlock / 64), kBubBlock, 0, c->stream>>>(ptr<uint32_t>(g.off), ptr<bella_graph_edge>(g.E), ptr<uint32_t>(list), bp.max_bubble_reads,
                                                                            bp.max_bubble_dist, ptr<uint32_t>(claim), ptr<uint32_t>(cnt));
        KCHK(c);
        k_bub_apply<<<nblk(nv, kBubBlock / 64), kBubBlock, 0, c->stream>>>(ptr<uint32_t>(g.off), ptr<bella_graph_edge>(g.E), ptr<uint32_t>(list), bp.max_bubble_reads,
                                                                           bp.max_bubble_dist, ptr<uint32_t>(claim), ptr<uint8_t>(g.hit), ptr<uint8_t>(ekill), ptr<uint32_t>(cnt));
        KCHK(c);
        k_graph_mark_reads<<<nblk(nr), 256, 0, c->stream>>>(ptr<uint8_t>(g.hit), nr, ptr<uint8_t>(g.rem), ptr<uint32_t>(cnt) + kBcReads);
        KCHK(c);
        if ((rc = g.filter(c, ptr<uint8_t>(ekill), &nm))) return rc;
        HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kBcCount, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));                   // the round's one read-back
        st.sources[round] = hc[kBcSources]; st.found[round] = hc[kBcFound]; st.popped[round] = hc[kBcPopped];
        st.reads_per_round[round] = hc[kBcReads]; st.edges_per_round[round] = g.m - nm;
        st.rounds = round + 1;
        st.reads_removed += hc[kBcReads];
        if (!hc[kBcPopped]) break;
        if ((rc = g.apply_keep(c))) return rc;
        g.m = nm;
    }
    return g.finish(c, &st.edges_removed, &st.pop_ms);
}

int bella_hip_graph_get_bubble_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, GRAPH, out, struct_size, [](const StageState& a) { return a.graph.bubbles; });
}

// ---- weak-overlap removal (graph.hpp) ----
int bella_hip_graph_cut_weak(bella_ctx* c, const bella_graph_weak_params* params) {
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_graph_weak_params wp{(uint32_t)sizeof(bella_graph_weak_params), 500};
    if (int r = take_params(c, wp, params, "bella_graph_weak_params")) return r;
    if (wp.ratio_permille > 1000) return fail(c, BELLA_ERR_BAD_ARG, "ratio_permille %u: at most 1000", wp.ratio_permille);
    if (int r = need(c, GRAPH)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    changed(c, GRAPH);
    bella_weak_stats& st = c->as.graph.weak;
    st = bella_weak_stats{};
    st.ratio_permille = wp.ratio_permille;
    const uint32_t nr = c->nreads, nv = 2 * nr;
    const uint32_t m = (uint32_t)c->as.graph.edges.size();
    if (!wp.ratio_permille || !m) return 0;
    TmpBuf ekill, cnt;
    ENSURE(c, ekill, m);
    ENSURE(c, cnt, 4 * kWcCount);
    GraphRound g;
    int rc = g.begin(c);
    if (rc) return rc;
    uint32_t hc[kWcCount] = {}, nm = 0;
    HIPCHK(c, hipMemsetAsync(g.hit.p, 0, nr, c->stream));             // (no read is removed: the filter sees the killed edges alone)
    HIPCHK(c, hipMemsetAsync(cnt.p, 0, 4 * kWcCount, c->stream));
    k_graph_weak<<<nblk(std::max(m, nv)), 256, 0, c->stream>>>(ptr<uint32_t>(g.off), ptr<bella_graph_edge>(g.E), m, nv, wp.ratio_permille, ptr<uint8_t>(ekill), ptr<uint32_t>(cnt));
    KCHK(c);
    if ((rc = g.filter(c, ptr<uint8_t>(ekill), &nm))) return rc;
    HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kWcCount, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                       // the call's one read-back
    st.forks = hc[kWcForks]; st.weak = hc[kWcWeak];
    if (hc[kWcRemoved]) {                                             // (kept = m - removed)
        if ((rc = g.apply_keep(c))) return rc;
        g.m = nm;
    }
    return g.finish(c, &st.edges_removed, &st.cut_ms);
}

int bella_hip_graph_get_weak_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, GRAPH, out, struct_size, [](const StageState& a) { return a.graph.weak; });
}

int bella_hip_graph_unitigs(bella_ctx* c, uint64_t* nunitigs, uint64_t* nvertices, uint64_t* nlinks, uint64_t* total_bases) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, GRAPH)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, UNITIGS);
    const StageState::Graph& g = c->as.graph;
    StageState::Unitigs& u = c->as.unitigs;
    const uint32_t nr = c->nreads, nv = 2 * nr, m = (uint32_t)g.edges.size();
    bella_unitig_stats& st = u.stats;                                 // (the clean's figures are the graph's)
    st = bella_unitig_stats{};
    std::vector<uint8_t> dead(nr);
    uint32_t nlive = 0;
    for (uint32_t r = 0; r < nr; ++r) { dead[r] = (g.contained[r] | g.removed[r]) ? 1 : 0; nlive += dead[r] ? 0u : 1u; }
    u.voff.assign(1, 0); u.boff.assign(1, 0);
    u.pos.clear(); u.len.clear(); u.verts.clear(); u.nb.clear(); u.circ.clear(); u.bases.clear(); u.links.clear();
    uint32_t nutg = 0, nverts = 0, nlk = 0;
    uint64_t total = 0;
    if (nlive) {
        TmpBuf off, E, dd, succ, pred, outlen, inlen, ra, rb, ma, mb, cut, cmin2, tail_of, cnt_of, emit, nvert, uid, voff, cnt, verts, pos, nb, slot_utg, uvoff, ulen, uboff,
            ucirc, gseg, lflag, lscan, links, out;
        int rc = graph_upload(c, off, E);
        if (rc) return rc;
        ReadSpans spans;
        if ((rc = spans.make(c))) return rc;
        ENSURE(c, dd, nr);
        for (Buf* b : {&succ, &pred, &outlen, &inlen, &tail_of, &cnt_of}) ENSURE(c, *b, 4 * (size_t)nv);
        for (Buf* b : {&emit, &nvert, &uid, &voff}) ENSURE(c, *b, 4 * ((size_t)nv + 1));
        ENSURE(c, ra, sizeof(UtgRank) * (size_t)nv); ENSURE(c, rb, sizeof(UtgRank) * (size_t)nv);
        ENSURE(c, cnt, 4 * kUcCount);
        ENSURE(c, lflag, (size_t)m + 1);
        ENSURE(c, lscan, 4 * ((size_t)m + 1));
        HIPCHK(c, hipMemcpyAsync(dd.p, dead.data(), nr, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(pred.p, 0xFF, 4 * (size_t)nv, c->stream));
        HIPCHK(c, hipMemsetAsync(inlen.p, 0, 4 * (size_t)nv, c->stream));
        HIPCHK(c, hipMemsetAsync(tail_of.p, 0, 4 * (size_t)nv, c->stream));
        HIPCHK(c, hipMemsetAsync(cnt_of.p, 0, 4 * (size_t)nv, c->stream));
        HIPCHK(c, hipMemsetAsync(cnt.p, 0, 4 * kUcCount, c->stream));
        EventSet ev;
        if ((rc = ev.create(c, 4))) return rc;
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        const uint32_t* const d_off = ptr<uint32_t>(off);
        const bella_graph_edge* const d_E = ptr<bella_graph_edge>(E);
        k_utg_succ<<<nblk(nv), 256, 0, c->stream>>>(d_off, d_E, nv, ptr<uint32_t>(succ), ptr<uint32_t>(pred), ptr<uint32_t>(outlen), ptr<uint32_t>(inlen));
        KCHK(c);
        uint32_t rounds = 1;
        while ((1ull << rounds) < nv) ++rounds;
        st.rank_rounds = rounds;
        const uint8_t* d_cut = nullptr;
        UtgRank* rank = nullptr;                                      // the ranking's result
        auto do_rank = [&]() -> int {
            UtgRank *a = ptr<UtgRank>(ra), *b = ptr<UtgRank>(rb);
            k_utg_rank_init<<<nblk(nv), 256, 0, c->stream>>>(ptr<uint32_t>(pred), ptr<uint32_t>(inlen), d_cut, nv, a);
            KCHK(c);
            for (uint32_t i = 0; i < rounds; ++i) {
                k_utg_rank_jump<<<nblk(nv), 256, 0, c->stream>>>(a, b, nv);
                KCHK(c);
                std::swap(a, b);
            }
            rank = a;
            return 0;
        };
        if ((rc = do_rank())) return rc;
        uint32_t hc[kUcCount] = {};
        k_utg_cycle_count<<<nblk(nv), 256, 0, c->stream>>>(rank, ptr<uint32_t>(pred), nv, ptr<uint32_t>(cnt));
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(hc, cnt.p, 4 * kUcCount, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.cycle_vertices = hc[kUcCycle];
        if (hc[kUcCycle]) {                                           // all-mergeable cycles: their smallest vertex becomes the head
            ENSURE(c, ma, sizeof(UtgMin) * (size_t)nv); ENSURE(c, mb, sizeof(UtgMin) * (size_t)nv);
            ENSURE(c, cut, nv); ENSURE(c, cmin2, 4 * (size_t)nv);
            UtgMin *a = ptr<UtgMin>(ma), *b = ptr<UtgMin>(mb);
            k_utg_min_init<<<nblk(nv), 256, 0, c->stream>>>(ptr<uint32_t>(pred), nv, a);
            KCHK(c);
            for (uint32_t i = 0; i < rounds; ++i) {
                k_utg_min_jump<<<nblk(nv), 256, 0, c->stream>>>(a, b, nv);
                KCHK(c);
                std::swap(a, b);
            }
            k_utg_cut<<<nblk(nv), 256, 0, c->stream>>>(rank, a, ptr<uint32_t>(pred), nv, ptr<uint8_t>(cut), ptr<uint32_t>(cmin2));
            KCHK(c);
            d_cut = ptr<uint8_t>(cut);
            if ((rc = do_rank())) return rc;
        }
        const uint32_t* const d_cmin2 = d_cut ? ptr<uint32_t>(cmin2) : nullptr;
        k_utg_tail<<<nblk(nv), 256, 0, c->stream>>>(rank, ptr<uint32_t>(succ), d_cut, ptr<uint8_t>(dd), nv, ptr<uint32_t>(tail_of), ptr<uint32_t>(cnt_of));
        KCHK(c);
        k_utg_select<<<nblk((uint64_t)nv + 1), 256, 0, c->stream>>>(ptr<uint32_t>(pred), d_cut, d_cmin2, ptr<uint8_t>(dd), ptr<uint32_t>(tail_of), ptr<uint32_t>(cnt_of), nv,
                                                                   ptr<uint32_t>(emit), ptr<uint32_t>(nvert));
        KCHK(c);
        if ((rc = scan_u32(c, ptr<uint32_t>(emit), ptr<uint32_t>(uid), (size_t)nv + 1))) return rc;
        if ((rc = scan_u32(c, ptr<uint32_t>(nvert), ptr<uint32_t>(voff), (size_t)nv + 1))) return rc;
        k_utg_linkflag<<<nblk((uint64_t)m + 1), 256, 0, c->stream>>>(d_E, m, ptr<uint32_t>(succ), ptr<uint8_t>(lflag));
        KCHK(c);
        if ((rc = scan_u8_to_u32(c, ptr<uint8_t>(lflag), ptr<uint32_t>(lscan), (size_t)m + 1))) return rc;
        HIPCHK(c, hipMemcpyAsync(&nutg, ptr<uint32_t>(uid) + nv, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&nverts, ptr<uint32_t>(voff) + nv, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&nlk, ptr<uint32_t>(lscan) + m, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nverts != nlive) return fail(c, BELLA_ERR_BAD_ARG, "unitigs: %u vertices for %u live reads (the graph is not twin-symmetric)", nverts, nlive);
        ENSURE(c, verts, 4 * (size_t)nverts); ENSURE(c, nb, 4 * (size_t)nverts); ENSURE(c, slot_utg, 4 * (size_t)nverts);
        ENSURE(c, pos, 8 * (size_t)nverts);
        ENSURE(c, gseg, 8 * ((size_t)nverts + 1));
        ENSURE(c, uvoff, 8 * ((size_t)nutg + 1)); ENSURE(c, ulen, 8 * ((size_t)nutg + 1)); ENSURE(c, uboff, 8 * ((size_t)nutg + 1));
        ENSURE(c, ucirc, nutg);
        ENSURE(c, links, sizeof(bella_unitig_link) * (size_t)nlk);
        HIPCHK(c, hipMemsetAsync(ulen.p, 0, 8 * ((size_t)nutg + 1), c->stream));
        k_utg_scatter<<<nblk(nv), 256, 0, c->stream>>>(rank, ptr<uint32_t>(succ), ptr<uint32_t>(outlen), ptr<uint32_t>(inlen), d_cut, ptr<uint8_t>(dd), spans.beg, spans.end,
                                                       ptr<uint32_t>(emit), ptr<uint32_t>(uid), ptr<uint32_t>(voff), nv, ptr<uint32_t>(verts), ptr<uint64_t>(pos),
                                                       ptr<uint32_t>(nb), ptr<uint32_t>(slot_utg), ptr<uint64_t>(uvoff), ptr<uint64_t>(ulen), ptr<uint8_t>(ucirc));
        KCHK(c);
        CUB(c, hipcub::DeviceScan::ExclusiveSum, ptr<uint64_t>(ulen), ptr<uint64_t>(uboff), (int)(nutg + 1), c->stream);
        k_utg_segoff<<<nblk((uint64_t)nverts + 1), 256, 0, c->stream>>>(ptr<uint32_t>(slot_utg), ptr<uint64_t>(pos), ptr<uint64_t>(uboff), nverts, nutg, ptr<uint64_t>(gseg));
        KCHK(c);
        if (nlk) {
            k_utg_links<<<nblk(m), 256, 0, c->stream>>>(d_E, ptr<uint8_t>(lflag), ptr<uint32_t>(lscan), m, rank, ptr<uint32_t>(uid), ptr<uint32_t>(tail_of),
                                                        ptr<bella_unitig_link>(links));
            KCHK(c);
        }
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipMemcpyAsync(&total, ptr<uint64_t>(uboff) + nutg, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const uint64_t nlanes = (total + kUtgBasesPerLane - 1) / kUtgBasesPerLane;
        ENSURE(c, out, (size_t)(nlanes * kUtgBasesPerLane));
        HIPCHK(c, hipEventRecord(ev.d, c->stream));
        if (total) {
            k_utg_gather<<<nblk(nlanes), 256, 0, c->stream>>>(ptr<uint64_t>(gseg), ptr<uint32_t>(verts), ptr<uint32_t>(nb), nverts, total, spans.beg, spans.end,
                                                              ptr<uint32_t>(c->packed), ptr<uint4>(out));
            KCHK(c);
        }
        HIPCHK(c, hipEventRecord(ev.e, c->stream));
        u.voff.assign((size_t)nutg + 1, 0); u.boff.assign((size_t)nutg + 1, 0);
        u.len.assign(nutg, 0); u.circ.assign(nutg, 0);
        u.verts.assign(nverts, 0); u.nb.assign(nverts, 0); u.pos.assign(nverts, 0);
        u.links.assign(nlk, bella_unitig_link{});
        u.bases.assign((size_t)total, 0);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.rank_ms = ev_ms(ev.a, ev.b);
        st.gather_ms = ev_ms(ev.d, ev.e);
        if (nutg) {
            HIPCHK(c, hipMemcpy(u.voff.data(), uvoff.p, 8 * (size_t)nutg, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(u.boff.data(), uboff.p, 8 * ((size_t)nutg + 1), hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(u.len.data(), ulen.p, 8 * (size_t)nutg, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(u.circ.data(), ucirc.p, nutg, hipMemcpyDeviceToHost));
        }
        u.voff[nutg] = nverts;
        if (nverts) {
            HIPCHK(c, c->stager.d2h(u.verts.data(), verts.p, 4 * (size_t)nverts, c->stream));
            HIPCHK(c, c->stager.d2h(u.nb.data(), nb.p, 4 * (size_t)nverts, c->stream));
            HIPCHK(c, c->stager.d2h(u.pos.data(), pos.p, 8 * (size_t)nverts, c->stream));
        }
        if (nlk) HIPCHK(c, c->stager.d2h(u.links.data(), links.p, sizeof(bella_unitig_link) * (size_t)nlk, c->stream));
        if (total) HIPCHK(c, c->stager.d2h(u.bases.data(), out.p, (size_t)total, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    st.unitigs = nutg; st.vertices = nverts; st.links = nlk; st.total_bases = total; st.gather_bytes = total;
    {
        std::vector<uint64_t> sorted(u.len);
        std::sort(sorted.begin(), sorted.end(), std::greater<uint64_t>());
        uint64_t acc = 0;
        for (uint64_t l : sorted) { acc += l; if (2 * acc >= total) { st.n50 = l; break; } }
        st.largest = sorted.empty() ? 0 : sorted[0];
        for (uint8_t f : u.circ) st.circular += f;
    }
    made(c, UNITIGS);
    if (nunitigs) *nunitigs = nutg;
    if (nvertices) *nvertices = nverts;
    if (nlinks) *nlinks = nlk;
    if (total_bases) *total_bases = total;
    return 0;
}

int bella_hip_graph_get_unitigs(bella_ctx* c, uint64_t* vertex_offsets, uint32_t* vertices, uint64_t* pos, uint32_t* nbases, uint64_t* len, uint8_t* circular,
                                bella_unitig_link* links) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, UNITIGS)) return r;
    const StageState::Unitigs& u = c->as.unitigs;
    copy_out(vertex_offsets, u.voff);
    copy_out(vertices, u.verts);
    copy_out(pos, u.pos);
    copy_out(nbases, u.nb);
    copy_out(len, u.len);
    copy_out(circular, u.circ);
    copy_out(links, u.links);
    return 0;
}

int bella_hip_graph_get_unitig_bases(bella_ctx* c, uint64_t* offsets, uint8_t* bases) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, UNITIGS)) return r;
    copy_out(offsets, c->as.unitigs.boff);
    copy_out(bases, c->as.unitigs.bases);
    return 0;
}

// the unitigs' figures (zero while there are none) with the clean's, which belong to the graph
int bella_hip_graph_get_unitig_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, GRAPH, out, struct_size, [](const StageState& a) {
        bella_unitig_stats s = a.unitigs.stats;
        const bella_unitig_stats& k = a.graph.clean;
        s.reads_removed = k.reads_removed; s.edges_removed = k.edges_removed; s.rounds = k.rounds; s.clean_ms = k.clean_ms;
        std::memcpy(s.tips_per_round, k.tips_per_round, sizeof(s.tips_per_round));
        std::memcpy(s.reads_per_round, k.reads_per_round, sizeof(s.reads_per_round));
        return s;
    });
}

// ---- unitig consensus (polish.hpp) ---------------------------------------------------------------------------------
int bella_hip_graph_polish_unitigs(bella_ctx* c, const bella_polish_params* params, uint64_t* total_bases) {
    if (!c || !params) return fail(c, BELLA_ERR_BAD_ARG, "null argument");
    bella_polish_params pp{};                                         // (no defaults: NULL was refused)
    if (int r = take_params(c, pp, params, "bella_polish_params")) return r;
    if (pp.min_depth < 1) return fail(c, BELLA_ERR_BAD_ARG, "min_depth must be >= 1");
    if (int r = need(c, UNITIGS)) return r;
    if (int r = need(c, PILE)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, POLISH);
    const StageState::Unitigs& u = c->as.unitigs;
    StageState::Polish& p = c->as.polish;
    const uint32_t nutg = (uint32_t)u.len.size(), nseg = (uint32_t)u.verts.size();
    const uint64_t total = u.boff[nutg];
    bella_polish_stats st{};
    st.unitigs = nutg; st.vertices = nseg; st.bases_before = total; st.min_depth = pp.min_depth;
    p.offs.assign((size_t)nutg + 1, 0);
    p.pos.assign(nseg, 0); p.nb.assign(nseg, 0);
    p.recs.assign(nutg, bella_polish_unitig{});
    p.bases.clear();
    uint64_t nout = 0;
    if (total) {                                                      // (no unitig position: nothing is launched)
        const uint64_t ntiles = (total + kPolTile - 1) / kPolTile;
        if (ntiles >= 0x7FFFFFFFull) return fail(c, BELLA_ERR_BAD_ARG, "polish: fewer than 2^31 tiles of unitig positions");
        st.tiles = (uint32_t)ntiles;
        st.table_bytes = total * kPileCounters * 4;
        UnitigLayout ul;
        int rc = ul.upload(c);
        if (rc) return rc;
        TmpBuf gseg, emit, tcnt, tpref, gp, ppos, pnb, poffs, recs, out;
        ENSURE(c, pnb, 4 * (size_t)nseg); ENSURE(c, ppos, 8 * (size_t)nseg);
        ENSURE(c, gseg, 8 * ((size_t)nseg + 1)); ENSURE(c, gp, 8 * ((size_t)nseg + 1));
        ENSURE(c, poffs, 8 * ((size_t)nutg + 1));
        ENSURE(c, recs, sizeof(bella_polish_unitig) * (size_t)nutg);
        ENSURE(c, emit, (size_t)(ntiles * kPolTile));
        ENSURE(c, tcnt, 4 * ((size_t)ntiles + 1)); ENSURE(c, tpref, 8 * ((size_t)ntiles + 1));
        HIPCHK(c, hipMemsetAsync(recs.p, 0, sizeof(bella_polish_unitig) * (size_t)nutg, c->stream));
        HIPCHK(c, hipMemsetAsync(ptr<uint32_t>(tcnt) + ntiles, 0, 4, c->stream));
        k_utg_segoff<<<nblk((uint64_t)nseg + 1), 256, 0, c->stream>>>(ptr<uint32_t>(ul.slot_utg), ptr<uint64_t>(ul.pos), ptr<uint64_t>(ul.uboff), nseg, nutg, ptr<uint64_t>(gseg));
        KCHK(c);
        EventSet ev;
        if ((rc = ev.create(c, 4))) return rc;
        ReadSpans spans;
        if ((rc = spans.make(c))) return rc;
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        k_pol_decide<<<(uint32_t)ntiles, kPolBlock, 0, c->stream>>>(ptr<uint64_t>(gseg), ptr<uint32_t>(ul.verts), ptr<uint32_t>(ul.slot_utg), nseg, total, ptr<uint64_t>(c->roff),
                                                                    spans.beg, spans.end, ptr<uint32_t>(c->packed), ptr<uint32_t>(c->pile), pp.min_depth, ptr<uint8_t>(emit),
                                                                    ptr<bella_polish_unitig>(recs), ptr<uint32_t>(tcnt));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        if ((rc = scan_u32_to_u64(c, ptr<uint32_t>(tcnt), ptr<uint64_t>(tpref), (uint64_t)ntiles + 1))) return rc;
        k_pol_segoff<<<nblk(((uint64_t)nseg + 1) * 64, kPolBlock), kPolBlock, 0, c->stream>>>(ptr<uint64_t>(gseg), nseg, ptr<uint8_t>(emit), ptr<uint64_t>(tpref),
                                                                                              ptr<uint64_t>(gp));
        KCHK(c);
        k_pol_finish<<<nblk((uint64_t)std::max(nseg, nutg) + 1), 256, 0, c->stream>>>(ptr<uint64_t>(gp), ptr<uint32_t>(ul.slot_utg), ptr<uint64_t>(ul.uvoff), ptr<uint64_t>(ul.uboff), nseg,
                                                                                       nutg, ptr<uint64_t>(ppos), ptr<uint32_t>(pnb), ptr<uint64_t>(poffs),
                                                                                       ptr<bella_polish_unitig>(recs));
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(&nout, ptr<uint64_t>(tpref) + ntiles, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        ENSURE(c, out, (size_t)((nout + 15) / 16 * 16 + 16));
        HIPCHK(c, hipEventRecord(ev.d, c->stream));
        k_pol_write<<<(uint32_t)ntiles, kPolBlock, 0, c->stream>>>(ptr<uint8_t>(emit), ptr<uint64_t>(tpref), ptr<uint8_t>(out));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.e, c->stream));
        p.bases.assign((size_t)nout, 0);
        HIPCHK(c, c->stager.d2h(p.offs.data(), poffs.p, 8 * ((size_t)nutg + 1), c->stream));
        HIPCHK(c, c->stager.d2h(p.recs.data(), recs.p, sizeof(bella_polish_unitig) * (size_t)nutg, c->stream));
        HIPCHK(c, c->stager.d2h(p.pos.data(), ppos.p, 8 * (size_t)nseg, c->stream));
        HIPCHK(c, c->stager.d2h(p.nb.data(), pnb.p, 4 * (size_t)nseg, c->stream));
        if (nout) HIPCHK(c, c->stager.d2h(p.bases.data(), out.p, (size_t)nout, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.decide_ms = ev_ms(ev.a, ev.b);
        st.write_ms = ev_ms(ev.d, ev.e);
    }
    st.bases_after = nout;
    for (const bella_polish_unitig& r : p.recs) {
        st.substituted += r.substituted; st.deleted += r.deleted; st.inserted += r.inserted; st.covered += r.covered; st.depth_sum += r.depth_sum;
    }
    p.stats = st;
    made(c, POLISH);
    if (total_bases) *total_bases = nout;
    return 0;
}

int bella_hip_graph_get_polished(bella_ctx* c, uint64_t* offsets, uint8_t* bases, uint64_t* ppos, uint32_t* pnbases, bella_polish_unitig* per_unitig) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, POLISH)) return r;
    const StageState::Polish& p = c->as.polish;
    copy_out(offsets, p.offs);
    copy_out(bases, p.bases);
    copy_out(ppos, p.pos);
    copy_out(pnbases, p.nb);
    copy_out(per_unitig, p.recs);
    return 0;
}

int bella_hip_graph_get_polish_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, POLISH, out, struct_size, [](const StageState& a) { return a.polish.stats; });
}

// ---- realignment (realign.hpp; DESIGN.md sections 18 and 19) -----------------------------------------------------------------------------
// unroll: the round places the reads of circular unitigs on the unrolled circle (section 19)
static int realign_round(bella_ctx* c, const bella_realign_params* params, uint64_t* total_bases, bool unroll) {
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_realign_params rp{};
    rp.band0 = BELLA_REALIGN_DEFAULT_BAND; rp.band_max = BELLA_REALIGN_DEFAULT_BAND_MAX; rp.min_identity = BELLA_REALIGN_DEFAULT_MIN_IDENTITY; rp.min_depth = 3;
    if (int r = take_params(c, rp, params, "bella_realign_params")) return r;
    if (int r = check_round_params(c, "realign", rp.band0, rp.band_max, rp.min_depth, rp.min_identity)) return r;
    if (int r = need(c, POLISH)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const StageState::Unitigs& u = c->as.unitigs;
    const StageState::Graph& g = c->as.graph;
    const bool again = has(c, REALIGN);                               // the sequence to align against: the last round's, or the polish's
    const std::vector<uint64_t>& coffs = again ? c->as.realign.offs : c->as.polish.offs;
    const std::vector<uint64_t>& cpos = again ? c->as.realign.pos : c->as.polish.pos;
    const std::vector<uint32_t>& cnb = again ? c->as.realign.nb : c->as.polish.nb;
    const std::vector<uint8_t>& cbases = again ? c->as.realign.bases : c->as.polish.bases;
    const uint32_t nutg = (uint32_t)u.len.size(), nseg = (uint32_t)u.verts.size(), nr = c->nreads;
    const uint64_t total = coffs[nutg];
    StageState::Realign out;
    bella_realign_stats st{};
    st.round = again ? c->as.realign.stats.round + 1 : 1;
    st.bases_before = total;
    out.offs.assign((size_t)nutg + 1, 0);
    out.pos.assign(nseg, 0); out.nb.assign(nseg, 0);
    out.recs.assign(nutg, bella_polish_unitig{});
    bella_realign_placement none{};
    none.unitig = kReaNone; none.anchor = kReaNone;
    out.placements.assign(nr, none);
    uint64_t nout = 0;
    if (nutg) {                                                       // (no unitig: nothing is launched)
        if (total >= 0x7FFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "realign: the unitigs must have fewer than 2^31 bases");
        for (uint32_t j = 0; j < nutg; ++j)
            if (coffs[j + 1] - coffs[j] >= kReaMaxUnitig) return fail(c, BELLA_ERR_BAD_ARG, "realign: unitig %u has 2^30 bases or more", j);
        const size_t nrec = c->as.records.size();
        const size_t npw = (size_t)(total / 16 + 1);
        // the pack the DP reads: the unitigs as they are, or (section 19) every circular unitig of fewer than 2^29 bases twice in a row
        std::vector<uint64_t> poffs(coffs.begin(), coffs.begin() + nutg + 1);
        bool any_unrolled = false;
        if (unroll) {
            uint64_t at = 0;
            for (uint32_t j = 0; j < nutg; ++j) {
                const uint64_t plen = coffs[j + 1] - coffs[j];
                const bool twice = u.circ[j] && plen && plen < kReaMaxUnrolled;
                poffs[j] = at;
                at += twice ? 2 * plen : plen;
                any_unrolled |= twice;
            }
            poffs[nutg] = at;
        }
        const uint64_t ptotal = poffs[nutg];
        const size_t nppw = (size_t)(ptotal / 16 + 1);
        TmpBuf recs, nb, dcpos, dcnb, dcoffs, cont, rem, bvert, key, place, ascii, upk, table, votes, dcirc, dpoffs, upk2;
        UnitigLayout ul;
        int rc = upload_records(c, recs);
        if (rc || (rc = ul.upload(c))) return rc;
        ENSURE(c, nb, 4 * (size_t)nseg); ENSURE(c, dcnb, 4 * (size_t)nseg); ENSURE(c, dcpos, 8 * (size_t)nseg);
        ENSURE(c, dcoffs, 8 * ((size_t)nutg + 1));
        ENSURE(c, cont, nr); ENSURE(c, rem, nr);
        ENSURE(c, bvert, 4 * (size_t)nr); ENSURE(c, key, 8 * (size_t)nr);
        ENSURE(c, place, sizeof(bella_realign_placement) * (size_t)nr);
        ENSURE(c, ascii, (size_t)total); ENSURE(c, upk, 4 * npw);
        ENSURE(c, votes, 8);
        ENSURE(c, dcirc, nutg);
        if (any_unrolled) { ENSURE(c, dpoffs, 8 * ((size_t)nutg + 1)); ENSURE(c, upk2, 4 * nppw); }
        const size_t tbytes = (size_t)total * kPileCounters * 4;
        if (ensure_bytes(c, table, tbytes))
            return fail(c, BELLA_ERR_NOMEM, "the realignment table needs %zu bytes of device memory (36 per base of %llu unitig bases) and they do not fit", tbytes,
                        (unsigned long long)total);
        HIPCHK(c, c->stager.h2d(nb.p, u.nb.data(), 4 * (size_t)nseg, c->stream));
        HIPCHK(c, c->stager.h2d(dcnb.p, cnb.data(), 4 * (size_t)nseg, c->stream));
        HIPCHK(c, c->stager.h2d(dcpos.p, cpos.data(), 8 * (size_t)nseg, c->stream));
        HIPCHK(c, c->stager.h2d(dcoffs.p, coffs.data(), 8 * ((size_t)nutg + 1), c->stream));
        HIPCHK(c, c->stager.h2d(cont.p, g.contained.data(), nr, c->stream));
        HIPCHK(c, c->stager.h2d(rem.p, g.removed.data(), nr, c->stream));
        HIPCHK(c, c->stager.h2d(dcirc.p, u.circ.data(), nutg, c->stream));
        if (any_unrolled) HIPCHK(c, c->stager.h2d(dpoffs.p, poffs.data(), 8 * ((size_t)nutg + 1), c->stream));
        if (total) HIPCHK(c, c->stager.h2d(ascii.p, cbases.data(), (size_t)total, c->stream));
        HIPCHK(c, hipMemsetAsync(bvert.p, 0xFF, 4 * (size_t)nr, c->stream));
        HIPCHK(c, hipMemsetAsync(key.p, 0, 8 * (size_t)nr, c->stream));
        HIPCHK(c, hipMemsetAsync(table.p, 0, tbytes ? tbytes : 16, c->stream));
        HIPCHK(c, hipMemsetAsync(votes.p, 0, 8, c->stream));
        ReadSpans spans;
        if ((rc = spans.make(c))) return rc;
        EventSet ev;
        if ((rc = ev.create(c, 3))) return rc;
        const uint32_t* const rpacked = ptr<uint32_t>(c->packed);
        const uint32_t* const cpacked = ptr<uint32_t>(upk);             // the consensus reads the unitigs as they are
        const uint32_t* const upacked = any_unrolled ? ptr<uint32_t>(upk2) : cpacked;
        // ---- placement
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        k_rea_backbone<<<nblk(nseg), 256, 0, c->stream>>>(ptr<uint32_t>(ul.verts), nseg, ptr<uint32_t>(bvert));
        KCHK(c);
        if (nrec) {
            k_rea_anchor<<<nblk(nrec), 256, 0, c->stream>>>(ptr<bella_overlap>(recs), (uint32_t)nrec, ptr<uint32_t>(bvert), ptr<uint8_t>(cont), ptr<uint8_t>(rem),
                                                            ptr<unsigned long long>(key));
            KCHK(c);
        }
        k_rea_place<<<nblk(nr), 256, 0, c->stream>>>(nr, ptr<uint64_t>(c->roff), spans.beg, spans.end, ptr<uint32_t>(bvert), ptr<unsigned long long>(key), ptr<bella_overlap>(recs),
                                                     ptr<uint8_t>(cont), ptr<uint8_t>(rem), ptr<uint32_t>(ul.verts), ptr<uint32_t>(ul.slot_utg), ptr<uint64_t>(ul.pos), ptr<uint32_t>(nb),
                                                     ptr<uint64_t>(dcpos), ptr<uint32_t>(dcnb), ptr<uint64_t>(ul.uvoff), ptr<uint64_t>(ul.uboff), ptr<uint64_t>(dcoffs), rp.band0,
                                                     ptr<uint8_t>(dcirc), rp.band_max, unroll ? 1u : 0u, ptr<bella_realign_placement>(place));
        KCHK(c);
        if (total) {
            k_rea_pack<<<nblk(npw), 256, 0, c->stream>>>(ptr<uint8_t>(ascii), total, ptr<uint32_t>(upk));
            KCHK(c);
        }
        if (any_unrolled) {
            k_rea_pack_unrolled<<<nblk(nppw), 256, 0, c->stream>>>(ptr<uint8_t>(ascii), ptr<uint64_t>(dcoffs), ptr<uint64_t>(dpoffs), nutg, ptotal, ptr<uint32_t>(upk2));
            KCHK(c);
        }
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, c->stager.d2h(out.placements.data(), place.p, sizeof(bella_realign_placement) * (size_t)nr, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.place_ms = ev_ms(ev.a, ev.b);
        ascii.reset();
        // the reads' clips, as the kernels see them
        std::vector<uint64_t> hroff((size_t)nr + 1, 0);
        for (uint32_t r = 0; r < nr; ++r) hroff[r + 1] = hroff[r] + c->host_lens[r];
        const bool clipped = has(c, TRIM);
        std::vector<uint32_t> pending;
        uint64_t nvert_reads = 0;
        for (uint32_t r = 0; r < nr; ++r) {
            bella_realign_placement& P = out.placements[r];
            if (P.status == BELLA_REALIGN_NONE) continue;
            if (P.anchor == kReaNone && P.status != BELLA_REALIGN_UNPLACED) { ++st.backbone; ++nvert_reads; }
            else if (P.status != BELLA_REALIGN_UNPLACED) ++st.contained;
            if (P.status == BELLA_REALIGN_UNPLACED) ++st.unplaced;
            else if (P.status == BELLA_REALIGN_OUTSIDE) ++st.outside;
            else pending.push_back(r);
        }
        st.repeated = nseg - nvert_reads;
        // ---- DP, walks and votes: band by band, batch by batch
        uint64_t budget = 0;
        if ((rc = round_budget(c, &budget))) return rc;
        RoundBatches<ReaFamily> rb{c, "realign", "reads", ev, rpacked, upacked, ptr<uint32_t>(table), ptr<unsigned long long>(votes), rp.keep_ops != 0, out.ops, st.dp_ms, st.walk_ms, st.vote_ms};
        std::vector<ReaJob> hj;
        std::vector<ReaRes> hres;
        std::vector<ReaCnt> hcnt;
        for (uint32_t B = rp.band0; !pending.empty(); B *= 2) {
            std::vector<uint32_t> next;
            const uint32_t maxjobs = round_max_jobs(B, budget);
            for (size_t b0 = 0; b0 < pending.size();) {
                hj.clear();
                uint64_t dbytes = 0;
                size_t b1 = b0;
                for (; b1 < pending.size(); ++b1) {
                    const uint32_t r = pending[b1];
                    const bella_realign_placement& P = out.placements[r];
                    const uint64_t beg = clipped ? c->as.trim.clips[r].beg : 0, end = clipped ? c->as.trim.clips[r].end : c->host_lens[r];
                    const uint64_t n = end - beg, need_bytes = n * (B / 4);
                    if (!hj.empty() && (dbytes + need_bytes > budget || hj.size() >= maxjobs)) break;
                    ReaJob j{};
                    const int32_t plen = (int32_t)(coffs[P.unitig + 1] - coffs[P.unitig]);
                    j.gH = (int64_t)poffs[P.unitig]; j.gT = (int64_t)coffs[P.unitig];
                    j.gV = (int64_t)(hroff[r] + (P.orient ? end - 1 : beg));
                    j.dir_off = dbytes; j.scr_off = 2ull * B * hj.size(); j.op_off = ~0ull;
                    j.n = (uint32_t)n; j.m = P.pad ? 2 * plen : plen; j.mt = P.pad ? plen : j.m;       // (pad: placed on the unrolled circle)
                    const int64_t slack = (P.e - P.s) - (int64_t)n;
                    j.c = (int32_t)(P.s + (slack >= 0 ? slack / 2 : -((-slack + 1) / 2)));      // floor
                    j.band = B; j.dV = P.orient ? -1 : 1; j.comp = P.orient ? 3u : 0u;
                    hj.push_back(j);
                    dbytes += need_bytes;
                    st.dp_cells += n * B;
                }
                const uint32_t nj = (uint32_t)hj.size();
                ENSURE(c, rb.jobs, sizeof(ReaJob) * (size_t)nj);
                st.dir_bytes_peak = std::max<uint64_t>(st.dir_bytes_peak, dbytes);
                ++st.batches;
                HIPCHK(c, c->stager.h2d(rb.jobs.p, hj.data(), sizeof(ReaJob) * (size_t)nj, c->stream));
                if ((rc = rb.dp_count(nj, B, dbytes))) return rc;
                HIPCHK(c, hipEventRecord(ev.d, c->stream));
                hres.resize(nj); hcnt.resize(nj);
                HIPCHK(c, c->stager.d2h(hres.data(), rb.res.p, sizeof(ReaRes) * (size_t)nj, c->stream));
                HIPCHK(c, c->stager.d2h(hcnt.data(), rb.cnt.p, sizeof(ReaCnt) * (size_t)nj, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                rb.counted();
                uint64_t nops = 0;
                for (uint32_t x = 0; x < nj; ++x) {
                    const uint32_t r = pending[b0 + x];
                    bella_realign_placement& P = out.placements[r];
                    const ReaCnt& k = hcnt[x];
                    P.band = B;
                    P.n_eq = k.n_eq; P.n_x = k.n_x; P.n_ins = k.n_ins; P.n_del = k.n_del;
                    const bool ended = k.nops > 0;
                    P.score = ended ? hres[x].score : 0;
                    P.q_begin = ended ? k.q_begin : 0; P.q_end = ended ? hres[x].q_end : 0;
                    if (k.touch) {
                        if (B < rp.band_max) next.push_back(r);
                        else { P.status = BELLA_REALIGN_BAND_CAPPED; ++st.band_capped; }
                    } else if (1000ull * k.n_eq < (uint64_t)rp.min_identity * ((uint64_t)k.n_eq + k.n_x + k.n_ins + k.n_del)) {
                        P.status = BELLA_REALIGN_LOW_IDENTITY; ++st.low_identity;
                    } else {
                        P.status = BELLA_REALIGN_VOTED; ++st.voted;
                        if (P.pad && (P.e > hj[x].mt || P.q_end > hj[x].mt)) ++out.wrapped;
                        hj[x].op_off = nops;
                        P.nops = k.nops;
                        if (rp.keep_ops) P.op_off = out.ops.size() + nops;
                        nops += k.nops;
                    }
                }
                if (nops) {
                    HIPCHK(c, c->stager.h2d(rb.jobs.p, hj.data(), sizeof(ReaJob) * (size_t)nj, c->stream));
                    if ((rc = rb.write_vote(nj, nops))) return rc;
                }
                b0 = b1;
            }
            pending.swap(next);
            if (B >= rp.band_max) break;
        }
        rb.dirs.reset(); rb.scr.reset(); rb.ops.reset();
        HIPCHK(c, hipMemcpyAsync(&st.votes, votes.p, 8, hipMemcpyDeviceToHost, c->stream));
        if (rp.keep_ops && total) {
            out.table.resize((size_t)total * kPileCounters);
            HIPCHK(c, c->stager.d2h(out.table.data(), table.p, tbytes, c->stream));
        }
        // ---- consensus: every unitig a read whose own bases are the sequence it was aligned against
        TmpBuf emit, scan, outb, noffs, cstats, npos, nnb;
        ENSURE(c, npos, 8 * (size_t)nseg); ENSURE(c, nnb, 4 * (size_t)nseg);
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        if ((rc = consensus_tail(c, table, cpacked, dcoffs, nutg, total, rp.min_depth, emit, scan, cstats, noffs, outb, &nout))) return rc;
        if (nseg) {
            k_rea_segpos<<<nblk(nseg), 256, 0, c->stream>>>(ptr<uint64_t>(scan), ptr<uint64_t>(dcpos), ptr<uint32_t>(ul.slot_utg), ptr<uint64_t>(ul.uvoff), ptr<uint64_t>(dcoffs), nseg,
                                                            ptr<uint64_t>(npos), ptr<uint32_t>(nnb));
            KCHK(c);
        }
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        std::vector<bella_consensus_read> hs(nutg);
        out.bases.assign((size_t)nout, 0);
        HIPCHK(c, c->stager.d2h(out.offs.data(), noffs.p, 8 * ((size_t)nutg + 1), c->stream));
        HIPCHK(c, c->stager.d2h(hs.data(), cstats.p, sizeof(bella_consensus_read) * (size_t)nutg, c->stream));
        if (nseg) {
            HIPCHK(c, c->stager.d2h(out.pos.data(), npos.p, 8 * (size_t)nseg, c->stream));
            HIPCHK(c, c->stager.d2h(out.nb.data(), nnb.p, 4 * (size_t)nseg, c->stream));
        }
        if (nout) HIPCHK(c, c->stager.d2h(out.bases.data(), outb.p, (size_t)nout, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.decide_ms = ev_ms(ev.a, ev.b);
        for (uint32_t j = 0; j < nutg; ++j) {
            bella_polish_unitig& q = out.recs[j];
            q.len_before = hs[j].len_before; q.len_after = hs[j].len_after;
            q.substituted = hs[j].substituted; q.deleted = hs[j].deleted; q.inserted = hs[j].inserted; q.covered = hs[j].covered; q.depth_sum = hs[j].depth_sum;
            st.substituted += q.substituted; st.deleted += q.deleted; st.inserted += q.inserted;
        }
    }
    st.bases_after = nout;
    out.stats = st;
    c->as.realign = std::move(out);
    changed(c, REALIGN);                                              // (the links were aligned on the sequence this round replaces)
    made(c, REALIGN);
    if (total_bases) *total_bases = nout;
    return 0;
}

int bella_hip_graph_realign_unitigs(bella_ctx* c, const bella_realign_params* params, uint64_t* total_bases) { return realign_round(c, params, total_bases, false); }

int bella_hip_graph_realign_unitigs_circular(bella_ctx* c, const bella_realign_params* params, uint64_t* total_bases) { return realign_round(c, params, total_bases, true); }

int bella_hip_graph_get_realigned(bella_ctx* c, uint64_t* offsets, uint8_t* bases, uint64_t* pos, uint32_t* nbases, bella_polish_unitig* per_unitig) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, REALIGN)) return r;
    const StageState::Realign& p = c->as.realign;
    copy_out(offsets, p.offs);
    copy_out(bases, p.bases);
    copy_out(pos, p.pos);
    copy_out(nbases, p.nb);
    copy_out(per_unitig, p.recs);
    return 0;
}

int bella_hip_graph_get_realign_placements(bella_ctx* c, bella_realign_placement* out) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, REALIGN)) return r;
    copy_out(out, c->as.realign.placements);
    return 0;
}

int bella_hip_graph_get_realign_ops(bella_ctx* c, uint64_t* nops, uint32_t* ops, uint32_t* table) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, REALIGN)) return r;
    if (nops) *nops = c->as.realign.ops.size();
    copy_out(ops, c->as.realign.ops);
    copy_out(table, c->as.realign.table);
    return 0;
}

int bella_hip_graph_get_realign_wrapped(bella_ctx* c, uint64_t* wrapped) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, REALIGN)) return r;
    if (wrapped) *wrapped = c->as.realign.wrapped;
    return 0;
}

int bella_hip_graph_get_realign_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, REALIGN, out, struct_size, [](const StageState& a) { return a.realign.stats; });
}

// ---- link alignment (links.hpp) -------------------------------------------------------------------------------------
// The links live on the host, so the pairing of twins, the windows and the derivation of a twin's record are host code; the pack, the DP and
// the walks run on the device, batched and band-doubled by RoundBatches as a realignment round's reads are.
int bella_hip_graph_align_links(bella_ctx* c, const bella_link_params* params, uint64_t* naligned) {
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_link_params lp{};
    lp.band0 = BELLA_LINK_DEFAULT_BAND; lp.band_max = BELLA_LINK_DEFAULT_BAND_MAX; lp.min_identity = BELLA_LINK_DEFAULT_MIN_IDENTITY;
    if (int r = take_params(c, lp, params, "bella_link_params")) return r;
    auto pow2 = [](uint32_t x) { return x && !(x & (x - 1)); };
    if (!pow2(lp.band0) || !pow2(lp.band_max) || lp.band0 < kTrMinBand || lp.band_max > kLnkMaxBand || lp.band0 > lp.band_max)
        return fail(c, BELLA_ERR_BAD_ARG, "align_links: band0 and band_max must be powers of two with 256 <= band0 <= band_max <= 4096");
    if (lp.min_identity > 1000) return fail(c, BELLA_ERR_BAD_ARG, "min_identity is in permille: at most 1000");
    if (int r = need(c, UNITIGS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    drop(c, LINKS);
    const StageState::Unitigs& u = c->as.unitigs;
    // the newest sequence of every unitig: the last round's, else the polish's, else the raw bases (whose map is the identity)
    const bool rea = has(c, REALIGN), pol = has(c, POLISH);
    const std::vector<uint64_t>& coffs = rea ? c->as.realign.offs : pol ? c->as.polish.offs : u.boff;
    const std::vector<uint64_t>& cpos = rea ? c->as.realign.pos : pol ? c->as.polish.pos : u.pos;
    const std::vector<uint32_t>& cnb = rea ? c->as.realign.nb : pol ? c->as.polish.nb : u.nb;
    const std::vector<uint8_t>& cbases = rea ? c->as.realign.bases : pol ? c->as.polish.bases : u.bases;
    const uint32_t nl = (uint32_t)u.links.size();
    const int64_t S = (int64_t)lp.band_max / 2;
    StageState::Links out;
    bella_link_aln none{};
    none.mate = kLnkNone;
    out.alns.assign(nl, none);
    bella_link_stats st{};
    st.links = nl;
    // ---- twins: link k, not SELF and not yet paired, takes the smallest later unpaired link that is its twin
    using Key = std::array<uint32_t, 5>;                              // a, its sign, b, its sign, rec
    auto key_of = [&](uint32_t k, bool twin) {
        const bella_unitig_link& l = u.links[k];
        const uint32_t sa = l.flags & BELLA_UNITIG_LINK_A_MINUS ? 1u : 0u, sb = l.flags & BELLA_UNITIG_LINK_B_MINUS ? 1u : 0u;
        return twin ? Key{l.b, sb ^ 1u, l.a, sa ^ 1u, l.rec} : Key{l.a, sa, l.b, sb, l.rec};
    };
    std::map<Key, std::vector<uint32_t>> by_key;
    for (uint32_t k = 0; k < nl; ++k)
        if (u.links[k].a != u.links[k].b) by_key[key_of(k, false)].push_back(k);
    std::map<Key, size_t> cursor;
    for (uint32_t k = 0; k < nl; ++k) {
        bella_link_aln& A = out.alns[k];
        if (u.links[k].a == u.links[k].b) { A.status = BELLA_LINK_SELF; continue; }
        if (A.mate != kLnkNone) continue;
        const Key tk = key_of(k, true);
        auto it = by_key.find(tk);
        if (it == by_key.end()) continue;
        size_t& at = cursor[tk];                                      // (every index of the list below k is paired: it was asked for k's own key)
        while (at < it->second.size() && (it->second[at] <= k || out.alns[it->second[at]].mate != kLnkNone)) ++at;
        if (at == it->second.size()) continue;
        const uint32_t t = it->second[at];
        A.mate = t;
        out.alns[t].mate = k; out.alns[t].derived = 1;
    }
    // ---- expected overlaps, windows and centre diagonals
    struct Want { int64_t oa, m, n, c; };
    std::vector<Want> want(nl, Want{});
    std::vector<uint32_t> pending;                                    // the links that are aligned, in index order
    std::vector<LnkWin> wins;
    std::vector<uint64_t> woff(1, 0);
    for (uint32_t k = 0; k < nl; ++k) {
        const bella_unitig_link& l = u.links[k];
        if (l.a == l.b) continue;
        auto map = [&](uint32_t j, int64_t x) {
            return rea_map(x, u.pos.data(), u.nb.data(), cpos.data(), cnb.data(), u.voff[j], u.voff[j + 1], (int64_t)u.len[j], (int64_t)(coffs[j + 1] - coffs[j]));
        };
        const int64_t Pa = (int64_t)(coffs[l.a + 1] - coffs[l.a]), Pb = (int64_t)(coffs[l.b + 1] - coffs[l.b]);
        if ((uint64_t)Pa >= kReaMaxUnitig || (uint64_t)Pb >= kReaMaxUnitig) return fail(c, BELLA_ERR_BAD_ARG, "align_links: a unitig has 2^30 bases or more");
        const int64_t la = (int64_t)u.len[l.a], lb = (int64_t)u.len[l.b];
        const int64_t xa = std::min<int64_t>(l.ovl, la), xb = std::min<int64_t>(l.ovl, lb);
        const bool am = (l.flags & BELLA_UNITIG_LINK_A_MINUS) != 0, bm = (l.flags & BELLA_UNITIG_LINK_B_MINUS) != 0;
        Want& w = want[k];
        w.oa = am ? map(l.a, xa) : Pa - map(l.a, la - xa);
        const int64_t ob = bm ? Pb - map(l.b, lb - xb) : map(l.b, xb);
        w.m = std::min(Pa, w.oa + S);
        w.n = std::min(Pb, ob + S);
        const int64_t sum = w.oa + ob;
        w.c = w.m - (sum >= 0 ? sum / 2 : -((-sum + 1) / 2));         // floor
        if (out.alns[k].derived) continue;
        // X: the last m bases of A^ (minus: the first m of cur(a), reversed and complemented); Y: the first n bases of B^
        wins.push_back(LnkWin{coffs[l.a] + (uint64_t)(am ? 0 : Pa - w.m), (uint32_t)w.m, am ? 1u : 0u});
        woff.push_back(woff.back() + (uint64_t)(w.m + 15) / 16);
        wins.push_back(LnkWin{coffs[l.b] + (uint64_t)(bm ? Pb - w.n : 0), (uint32_t)w.n, bm ? 1u : 0u});
        woff.push_back(woff.back() + (uint64_t)(w.n + 15) / 16);
        pending.push_back(k);
    }
    st.jobs = pending.size();
    if (!pending.empty()) {                                           // (no link, or SELF links only: nothing is launched)
        std::vector<uint32_t> job_of(nl, 0);                          // link -> its pair of windows
        for (size_t x = 0; x < pending.size(); ++x) job_of[pending[x]] = (uint32_t)x;
        const uint64_t total = coffs.back(), nwords = woff.back();
        TmpBuf ascii, dwins, dwoff, pack;
        ENSURE(c, ascii, (size_t)total);
        ENSURE(c, dwins, sizeof(LnkWin) * wins.size());
        ENSURE(c, dwoff, 8 * woff.size());
        ENSURE(c, pack, 4 * (size_t)(nwords + 1));
        if (total) HIPCHK(c, c->stager.h2d(ascii.p, cbases.data(), (size_t)total, c->stream));
        HIPCHK(c, c->stager.h2d(dwins.p, wins.data(), sizeof(LnkWin) * wins.size(), c->stream));
        HIPCHK(c, c->stager.h2d(dwoff.p, woff.data(), 8 * woff.size(), c->stream));
        EventSet ev;
        int rc = ev.create(c, 3);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        if (nwords) {
            k_lnk_pack<<<nblk(nwords), 256, 0, c->stream>>>(ptr<uint8_t>(ascii), ptr<LnkWin>(dwins), ptr<uint64_t>(dwoff), (uint32_t)wins.size(), nwords, ptr<uint32_t>(pack));
            KCHK(c);
        }
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.pack_ms = ev_ms(ev.a, ev.b);
        ascii.reset();
        // ---- DP and walks: band by band, batch by batch
        uint64_t budget = 0;
        if ((rc = round_budget(c, &budget))) return rc;
        double no_votes = 0;
        RoundBatches<LnkFamily> rb{c, "align_links", "links", ev, ptr<uint32_t>(pack), ptr<uint32_t>(pack), nullptr, nullptr, true, out.ops, st.dp_ms, st.walk_ms, no_votes};
        std::vector<ReaJob> hj;
        std::vector<LnkRes> hres;
        std::vector<ReaCnt> hcnt;
        for (uint32_t B = lp.band0; !pending.empty(); B *= 2) {
            std::vector<uint32_t> next;
            const uint32_t maxjobs = round_max_jobs(B, budget);
            for (size_t b0 = 0; b0 < pending.size();) {
                hj.clear();
                uint64_t dbytes = 0;
                size_t b1 = b0;
                for (; b1 < pending.size(); ++b1) {
                    const uint32_t k = pending[b1];
                    const Want& w = want[k];
                    const uint64_t need_bytes = (uint64_t)w.n * (B / 4);
                    if (!hj.empty() && (dbytes + need_bytes > budget || hj.size() >= maxjobs)) break;
                    ReaJob j{};
                    j.gH = (int64_t)(16 * woff[2 * (size_t)job_of[k]]); j.gV = (int64_t)(16 * woff[2 * (size_t)job_of[k] + 1]);
                    j.dir_off = dbytes; j.scr_off = 2ull * B * hj.size(); j.op_off = ~0ull;
                    j.n = (uint32_t)w.n; j.m = (int32_t)w.m; j.mt = j.m; j.c = (int32_t)w.c;
                    j.band = B; j.dV = 1; j.comp = 0;
                    hj.push_back(j);
                    dbytes += need_bytes;
                    st.dp_cells += (uint64_t)w.n * B;
                }
                const uint32_t nj = (uint32_t)hj.size();
                ENSURE(c, rb.jobs, sizeof(ReaJob) * (size_t)nj);
                ++st.batches;
                HIPCHK(c, c->stager.h2d(rb.jobs.p, hj.data(), sizeof(ReaJob) * (size_t)nj, c->stream));
                if ((rc = rb.dp_count(nj, B, dbytes))) return rc;
                HIPCHK(c, hipEventRecord(ev.d, c->stream));
                hres.resize(nj); hcnt.resize(nj);
                HIPCHK(c, c->stager.d2h(hres.data(), rb.res.p, sizeof(LnkRes) * (size_t)nj, c->stream));
                HIPCHK(c, c->stager.d2h(hcnt.data(), rb.cnt.p, sizeof(ReaCnt) * (size_t)nj, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                rb.counted();
                uint64_t nops = 0;
                for (uint32_t x = 0; x < nj; ++x) {
                    const uint32_t k = pending[b0 + x];
                    bella_link_aln& A = out.alns[k];
                    const ReaCnt& q = hcnt[x];
                    const bool reached = hres[x].score > kReaNoEnd;
                    A.band = B;
                    A.score = reached ? hres[x].score : 0;
                    A.ovl_a = reached ? (uint32_t)(hj[x].m - q.q_begin) : 0; A.ovl_b = reached ? (uint32_t)hres[x].i_end : 0;
                    A.n_eq = q.n_eq; A.n_x = q.n_x; A.n_ins = q.n_ins; A.n_del = q.n_del;
                    if (q.touch) {
                        if (B < lp.band_max) next.push_back(k);
                        else A.status = BELLA_LINK_BAND_CAPPED;
                    } else if (A.score <= 0) {
                        A.status = BELLA_LINK_EMPTY;
                    } else if (1000ull * q.n_eq < (uint64_t)lp.min_identity * ((uint64_t)q.n_eq + q.n_x + q.n_ins + q.n_del)) {
                        A.status = BELLA_LINK_LOW_IDENTITY;
                    } else {
                        A.status = BELLA_LINK_ALIGNED;
                        hj[x].op_off = nops;
                        A.nops = q.nops;
                        A.op_off = out.ops.size() + nops;
                        nops += q.nops;
                    }
                }
                if (nops) {
                    HIPCHK(c, c->stager.h2d(rb.jobs.p, hj.data(), sizeof(ReaJob) * (size_t)nj, c->stream));
                    if ((rc = rb.write_vote(nj, nops))) return rc;
                }
                b0 = b1;
            }
            pending.swap(next);
            if (B >= lp.band_max) break;
        }
    }
    // ---- the twins' records, from their mates'; the counts
    for (uint32_t k = 0; k < nl; ++k) {
        bella_link_aln& A = out.alns[k];
        if (A.derived) {
            const bella_link_aln M = out.alns[A.mate];
            A.status = M.status; A.band = M.band; A.score = M.score;
            A.ovl_a = M.ovl_b; A.ovl_b = M.ovl_a;
            A.n_eq = M.n_eq; A.n_x = M.n_x; A.n_ins = M.n_del; A.n_del = M.n_ins;
            A.nops = M.nops; A.op_off = out.ops.size();
            for (uint32_t x = 0; x < M.nops; ++x) {                   // reversed, 'I' and 'D' swapped
                const uint32_t w = out.ops[(size_t)M.op_off + M.nops - 1 - x], op = w & 15u;
                out.ops.push_back((w & ~15u) | (op == kOpIns ? (uint32_t)kOpDel : op == kOpDel ? (uint32_t)kOpIns : op));
            }
            if (!A.nops) A.op_off = 0;
            ++st.derived;
        }
        switch (A.status) {
            case BELLA_LINK_ALIGNED: ++st.aligned; st.overlap_before += (uint64_t)want[k].oa; st.overlap_after += A.ovl_a; break;
            case BELLA_LINK_EMPTY: ++st.empty; break;
            case BELLA_LINK_BAND_CAPPED: ++st.band_capped; break;
            case BELLA_LINK_LOW_IDENTITY: ++st.low_identity; break;
            default: ++st.self; break;
        }
    }
    st.ops = out.ops.size();
    out.stats = st;
    c->as.links = std::move(out);
    made(c, LINKS);
    if (naligned) *naligned = st.aligned;
    return 0;
}

int bella_hip_graph_get_link_alignments(bella_ctx* c, bella_link_aln* alns, uint64_t* nops, uint32_t* ops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, LINKS)) return r;
    copy_out(alns, c->as.links.alns);
    if (nops) *nops = c->as.links.ops.size();
    copy_out(ops, c->as.links.ops);
    return 0;
}

int bella_hip_graph_get_link_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, LINKS, out, struct_size, [](const StageState& a) { return a.links.stats; });
}

}  // extern "C"

// ---- pair alignment (pairalign.hpp) ---------------------------------------------------------------------------------
// The caller's sequences are uploaded and packed once per (sequence, orientation); the DP and the walks run batched and band-doubled by
// RoundBatches, as the links' do, one family per mode.  Nothing of the context's stages is read or written.
namespace {
struct PalPair { uint32_t n, m; int32_t c; uint32_t wq, wt; };       // a checked pair: rows, columns, centre, its two windows of the pack

// whether a band of B can hold what the mode needs: global, the start (0, 0) and the end (n, m); else, any cell of the rectangle
bool pal_feasible(uint32_t mode, const PalPair& p, uint32_t B) {
    const int64_t half = B / 2, c = p.c;
    auto in = [&](int64_t d) { return d - c >= -half && d - c < half; };      // the diagonal d = q - i
    if (mode == BELLA_ALIGN_GLOBAL) return in(0) && in((int64_t)p.m - (int64_t)p.n);
    return c + half > -(int64_t)p.n && c - half <= (int64_t)p.m;              // one of the diagonals -n .. m
}

// what a mode's DP result and the counting walk say about an ALIGNED pair
void pal_fill(bella_align_result& R, const ReaJob& j, const GlbRes& r, const ReaCnt& q) {
    R.score = r.score; R.q_begin = 0; R.q_end = j.n; R.t_begin = (uint32_t)q.q_begin; R.t_end = (uint32_t)j.m;
}
void pal_fill(bella_align_result& R, const ReaJob& j, const ReaRes& r, const ReaCnt& q) {
    R.score = r.score; R.q_begin = 0; R.q_end = j.n; R.t_begin = (uint32_t)q.q_begin; R.t_end = (uint32_t)r.q_end;
}
void pal_fill(bella_align_result& R, const ReaJob& j, const LnkRes& r, const ReaCnt& q) {
    R.score = r.score; R.q_begin = 0; R.q_end = (uint32_t)r.i_end; R.t_begin = (uint32_t)q.q_begin; R.t_end = (uint32_t)j.m;
}

template <class Family>
int pal_run(bella_ctx* c, uint32_t mode, uint32_t band0, uint32_t band_max, const std::vector<PalPair>& pp, const std::vector<uint64_t>& woff, const uint32_t* pack, EventSet& ev,
            std::vector<bella_align_result>& res, std::vector<uint32_t>& ops, bella_align_stats& st, const AfnScore& score = AfnScore{1, 1, 0, 1}) {
    using Res = typename Family::Res;
    using Traits = BandTraits<Family>;
    constexpr uint32_t per_byte = 8 / Traits::dir_bits;               // cells of a direction byte: a row is B / per_byte bytes
    // every reachable score stays above kTrNeg / 2: section 28's n + m >= 2^27 under +1 / -1 / -1
    const uint64_t worst = Traits::affine ? (uint64_t)std::max(std::max(score.a, score.b), score.o + score.e) : 1;
    uint64_t budget = 0;
    if (int rc = round_budget(c, &budget)) return rc;
    // ---- the first band of every pair: doubled without a DP while it cannot hold what the mode needs
    std::map<uint32_t, std::vector<uint32_t>> starters;              // band -> the pairs that begin with it, in index order
    for (uint32_t k = 0; k < (uint32_t)pp.size(); ++k) {
        bella_align_result& R = res[k];
        R.band = band0;
        if (((uint64_t)pp[k].n + pp[k].m) * worst >= kPalMaxCells) { R.status = BELLA_ALIGN_STATUS_TOO_LARGE; continue; }
        while (!pal_feasible(mode, pp[k], R.band) && R.band < band_max) { R.band *= 2; ++R.widened; }
        if (!pal_feasible(mode, pp[k], R.band)) { R.status = BELLA_ALIGN_STATUS_BAND_CAPPED; continue; }
        starters[R.band].push_back(k);
    }
    double no_votes = 0;
    RoundBatches<Family> rb{c, "align_sequences", "pairs", ev, pack, pack, nullptr, nullptr, true, ops, st.dp_ms, st.walk_ms, no_votes};
    rb.score = score;
    std::vector<ReaJob> hj;
    std::vector<Res> hres;
    std::vector<ReaCnt> hcnt;
    std::vector<uint32_t> next, pending;
    for (uint32_t B = band0;; B *= 2) {
        pending.clear();
        const std::vector<uint32_t>& fresh = starters[B];
        std::merge(next.begin(), next.end(), fresh.begin(), fresh.end(), std::back_inserter(pending));
        next.clear();
        size_t keep = 0;                                              // a pair whose direction bytes exceed a batch at this band goes no further
        for (uint32_t k : pending) {
            if ((uint64_t)pp[k].n * (B / per_byte) > budget) { res[k].status = BELLA_ALIGN_STATUS_TOO_LARGE; res[k].band = B; }
            else pending[keep++] = k;
        }
        pending.resize(keep);
        const uint32_t maxjobs = round_max_jobs(B, budget, Traits::scr_ints);
        for (size_t b0 = 0; b0 < pending.size();) {
            hj.clear();
            uint64_t dbytes = 0;
            size_t b1 = b0;
            for (; b1 < pending.size(); ++b1) {
                const PalPair& p = pp[pending[b1]];
                const uint64_t need_bytes = (uint64_t)p.n * (B / per_byte);
                if (!hj.empty() && (dbytes + need_bytes > budget || hj.size() >= maxjobs)) break;
                ReaJob j{};
                j.gH = (int64_t)(16 * woff[p.wt]); j.gV = (int64_t)(16 * woff[p.wq]);
                j.dir_off = dbytes; j.scr_off = (uint64_t)Traits::scr_ints * B * hj.size(); j.op_off = ~0ull;
                j.n = p.n; j.m = (int32_t)p.m; j.mt = j.m; j.c = p.c;
                j.band = B; j.dV = 1; j.comp = 0;
                hj.push_back(j);
                dbytes += need_bytes;
                st.dp_cells += (uint64_t)p.n * B;
            }
            const uint32_t nj = (uint32_t)hj.size();
            ENSURE(c, rb.jobs, sizeof(ReaJob) * (size_t)nj);
            ++st.batches;
            HIPCHK(c, c->stager.h2d(rb.jobs.p, hj.data(), sizeof(ReaJob) * (size_t)nj, c->stream));
            if (int rc = rb.dp_count(nj, B, dbytes)) return rc;
            HIPCHK(c, hipEventRecord(ev.d, c->stream));
            hres.resize(nj); hcnt.resize(nj);
            HIPCHK(c, c->stager.d2h(hres.data(), rb.res.p, sizeof(Res) * (size_t)nj, c->stream));
            HIPCHK(c, c->stager.d2h(hcnt.data(), rb.cnt.p, sizeof(ReaCnt) * (size_t)nj, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            rb.counted();
            uint64_t nops = 0;
            for (uint32_t x = 0; x < nj; ++x) {
                const uint32_t k = pending[b0 + x];
                bella_align_result& R = res[k];
                const ReaCnt& q = hcnt[x];
                R.band = B;
                if (q.touch) {
                    if (B < band_max) { next.push_back(k); ++R.widened; ++st.repeated; }
                    else R.status = BELLA_ALIGN_STATUS_BAND_CAPPED;
                    continue;
                }
                R.status = BELLA_ALIGN_STATUS_ALIGNED;
                pal_fill(R, hj[x], hres[x], q);
                R.n_eq = q.n_eq; R.n_x = q.n_x; R.n_ins = q.n_ins; R.n_del = q.n_del;
                hj[x].op_off = nops;
                R.nops = q.nops;
                R.op_off = ops.size() + nops;
                nops += q.nops;
            }
            if (nops) {
                HIPCHK(c, c->stager.h2d(rb.jobs.p, hj.data(), sizeof(ReaJob) * (size_t)nj, c->stream));
                if (int rc = rb.write_vote(nj, nops)) return rc;
            }
            b0 = b1;
        }
        if (B >= band_max) break;
    }
    return 0;
}
// the two public calls: afn == nullptr runs the linear families (section 28), else the affine ones under *afn (section 29)
int pal_align(bella_ctx* c, const uint8_t* bases, uint64_t nbases, const bella_align_pair* pairs, uint64_t npairs, const bella_align_params* params, const AfnScore* afn,
              bella_align_result* out, uint64_t* nops) {
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();
    // ---- everything is checked before anything is launched
    bella_align_params ap{};
    ap.mode = BELLA_ALIGN_GLOBAL;
    if (int r = take_params(c, ap, params, "bella_align_params")) return r;
    if (!ap.band0) ap.band0 = BELLA_ALIGN_DEFAULT_BAND;
    if (!ap.band_max) ap.band_max = BELLA_ALIGN_DEFAULT_BAND_MAX;
    auto pow2 = [](uint32_t x) { return x && !(x & (x - 1)); };
    if (ap.mode > BELLA_ALIGN_DOVETAIL) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: mode %u is none of global, semi-global, dovetail", ap.mode);
    if (!pow2(ap.band0) || !pow2(ap.band_max) || ap.band0 < kTrMinBand || ap.band_max > kPalMaxBand || ap.band0 > ap.band_max)
        return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: band0 and band_max must be powers of two with 256 <= band0 <= band_max <= 16384");
    if (npairs && (!pairs || !out || !bases)) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: null argument");
    if (npairs >= (1ull << 31)) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: at most 2^31 - 1 pairs a call");
    std::vector<PalPair> pp((size_t)npairs);
    std::vector<LnkWin> wins;                                         // one window per (sequence, orientation) in use
    std::vector<uint64_t> woff(1, 0);
    std::map<std::array<uint64_t, 3>, uint32_t> win_of;
    uint64_t lo = nbases, hi = 0;                                     // the bases in use lie in [lo, hi)
    bool is_base[256] = {};
    is_base['A'] = is_base['C'] = is_base['G'] = is_base['T'] = true;
    for (uint64_t k = 0; k < npairs; ++k) {
        const bella_align_pair& a = pairs[k];
        if (a.flags & ~BELLA_ALIGN_PAIR_RC) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: pair %llu: flags is 0 or BELLA_ALIGN_PAIR_RC", (unsigned long long)k);
        auto window = [&](uint64_t off, uint32_t len, uint32_t rc, uint32_t* w) {
            if (!len) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: pair %llu: a sequence of length 0", (unsigned long long)k);
            if (len >= kPalMaxSeq) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: pair %llu: a sequence of 2^30 bases or more", (unsigned long long)k);
            if (off > nbases || len > nbases - off) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: pair %llu: a sequence lies outside bases", (unsigned long long)k);
            auto ins = win_of.emplace(std::array<uint64_t, 3>{off, len, rc}, (uint32_t)wins.size());
            *w = ins.first->second;
            if (!ins.second) return 0;
            for (uint64_t t = off; t < off + len; ++t)
                if (!is_base[bases[t]]) return fail(c, BELLA_ERR_BAD_ARG, "align_sequences: pair %llu: base %llu of bases is not one of ACGT", (unsigned long long)k, (unsigned long long)t);
            wins.push_back(LnkWin{off, len, rc});
            woff.push_back(woff.back() + ((uint64_t)len + 15) / 16);
            lo = std::min(lo, off); hi = std::max(hi, off + len);
            return 0;
        };
        PalPair& p = pp[(size_t)k];
        p.n = a.q_len; p.m = a.t_len; p.c = a.centre;
        if (int r = window(a.q_off, a.q_len, a.flags & BELLA_ALIGN_PAIR_RC, &p.wq)) return r;
        if (int r = window(a.t_off, a.t_len, 0u, &p.wt)) return r;
    }
    std::vector<bella_align_result> res((size_t)npairs, bella_align_result{});
    std::vector<uint32_t> ops;
    bella_align_stats st{};
    st.pairs = npairs; st.mode = ap.mode;
    if (npairs) {
        HIPCHK(c, hipSetDevice(c->device));
        for (LnkWin& w : wins) w.src -= lo;
        const uint64_t nwords = woff.back();
        TmpBuf ascii, dwins, dwoff, pack;
        ENSURE(c, ascii, (size_t)(hi - lo));
        ENSURE(c, dwins, sizeof(LnkWin) * wins.size());
        ENSURE(c, dwoff, 8 * woff.size());
        ENSURE(c, pack, 4 * (size_t)(nwords + 1));
        HIPCHK(c, c->stager.h2d(ascii.p, bases + lo, (size_t)(hi - lo), c->stream));
        HIPCHK(c, c->stager.h2d(dwins.p, wins.data(), sizeof(LnkWin) * wins.size(), c->stream));
        HIPCHK(c, c->stager.h2d(dwoff.p, woff.data(), 8 * woff.size(), c->stream));
        EventSet ev;
        int rc = ev.create(c, 3);
        if (rc) return rc;
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        k_lnk_pack<<<nblk(nwords), 256, 0, c->stream>>>(ptr<uint8_t>(ascii), ptr<LnkWin>(dwins), ptr<uint64_t>(dwoff), (uint32_t)wins.size(), nwords, ptr<uint32_t>(pack));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.pack_ms = ev_ms(ev.a, ev.b);
        ascii.reset();
        if (afn)
            rc = ap.mode == BELLA_ALIGN_GLOBAL       ? pal_run<PalAfnGlobal>(c, ap.mode, ap.band0, ap.band_max, pp, woff, ptr<uint32_t>(pack), ev, res, ops, st, *afn)
                 : ap.mode == BELLA_ALIGN_SEMIGLOBAL ? pal_run<PalAfnSemi>(c, ap.mode, ap.band0, ap.band_max, pp, woff, ptr<uint32_t>(pack), ev, res, ops, st, *afn)
                                                     : pal_run<PalAfnDovetail>(c, ap.mode, ap.band0, ap.band_max, pp, woff, ptr<uint32_t>(pack), ev, res, ops, st, *afn);
        else
            rc = ap.mode == BELLA_ALIGN_GLOBAL       ? pal_run<PalGlobal>(c, ap.mode, ap.band0, ap.band_max, pp, woff, ptr<uint32_t>(pack), ev, res, ops, st)
                 : ap.mode == BELLA_ALIGN_SEMIGLOBAL ? pal_run<PalSemi>(c, ap.mode, ap.band0, ap.band_max, pp, woff, ptr<uint32_t>(pack), ev, res, ops, st)
                                                     : pal_run<PalDovetail>(c, ap.mode, ap.band0, ap.band_max, pp, woff, ptr<uint32_t>(pack), ev, res, ops, st);
        if (rc) { (void)hipDeviceSynchronize(); return rc; }
    }
    for (const bella_align_result& R : res)
        ++(R.status == BELLA_ALIGN_STATUS_ALIGNED ? st.aligned : R.status == BELLA_ALIGN_STATUS_BAND_CAPPED ? st.band_capped : st.too_large);
    st.ops = ops.size();
    st.total_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    copy_out(out, res);
    c->pal_ops = std::move(ops);
    c->pal_stats = st;
    if (nops) *nops = st.ops;
    return 0;
}
}  // namespace

extern "C" {

int bella_hip_align_sequences(bella_ctx* c, const uint8_t* bases, uint64_t nbases, const bella_align_pair* pairs, uint64_t npairs, const bella_align_params* params,
                              bella_align_result* out, uint64_t* nops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    return pal_align(c, bases, nbases, pairs, npairs, params, nullptr, out, nops);
}

int bella_hip_align_sequences_affine(bella_ctx* c, const uint8_t* bases, uint64_t nbases, const bella_align_pair* pairs, uint64_t npairs, const bella_align_params* params,
                                     const bella_align_scoring* scoring, bella_align_result* out, uint64_t* nops) {
    if (!c) return BELLA_ERR_BAD_ARG;
    AfnScore sc{1, 1, 0, 1};
    if (scoring) {
        if (scoring->struct_size < sizeof(bella_align_scoring))
            return fail(c, BELLA_ERR_BAD_ARG, "bella_align_scoring: struct_size %u is smaller than the %zu bytes this library knows", scoring->struct_size, sizeof(bella_align_scoring));
        if (scoring->reserved) return fail(c, BELLA_ERR_BAD_ARG, "bella_align_scoring: reserved must be 0");
        if (scoring->match < 1 || scoring->match > 255 || scoring->mismatch > 255 || scoring->gap_open > 255 || scoring->gap_extend < 1 || scoring->gap_extend > 255)
            return fail(c, BELLA_ERR_BAD_ARG, "bella_align_scoring: 1 <= match <= 255, mismatch <= 255, gap_open <= 255, 1 <= gap_extend <= 255");
        sc = AfnScore{(int)scoring->match, (int)scoring->mismatch, (int)scoring->gap_open, (int)scoring->gap_extend};
    }
    return pal_align(c, bases, nbases, pairs, npairs, params, &sc, out, nops);
}

int bella_hip_get_align_ops(bella_ctx* c, uint32_t* ops, uint64_t cap) {
    if (!c || (!ops && cap)) return BELLA_ERR_BAD_ARG;
    if (c->pal_ops.size() > cap) return fail(c, BELLA_ERR_BAD_ARG, "get_align_ops: %zu ops, room for %llu", c->pal_ops.size(), (unsigned long long)cap);
    copy_out(ops, c->pal_ops);
    return 0;
}

int bella_hip_get_align_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    if (!c || !out) return BELLA_ERR_BAD_ARG;
    return put_sized(out, struct_size, c->pal_stats);
}

// ---- read correction rounds (recorrect.hpp) -------------------------------------------------------------------------
// Section 18's round with the jobs placed, batched and sorted into bands on the device: per band the host reads the pending count, per
// batch its end, its direction bytes and its runs -- nothing per job.  The new sequences, statistics, anchors and job records are built in
// buffers of the call and handed to the context when everything has succeeded: a failed round leaves the round before.
int bella_hip_recorrect(bella_ctx* c, const bella_recorrect_params* params, uint64_t* total_bases) {
    if (!c) return BELLA_ERR_BAD_ARG;
    bella_recorrect_params rp{};
    rp.band0 = BELLA_RECORRECT_DEFAULT_BAND; rp.band_max = BELLA_RECORRECT_DEFAULT_BAND_MAX; rp.min_identity = BELLA_RECORRECT_DEFAULT_MIN_IDENTITY; rp.min_depth = 3;
    if (int r = take_params(c, rp, params, "bella_recorrect_params")) return r;
    if (int r = check_round_params(c, "recorrect", rp.band0, rp.band_max, rp.min_depth, rp.min_identity)) return r;
    if (int r = need(c, CONS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const bool again = has(c, RECORRECT);                             // the sequences to align against: the last round's, or the consensus's
    const Buf& coffs = again ? c->rc_offs : c->cons_offs;
    const Buf& cbases = again ? c->rc_out : c->cons_out;
    const Buf& canch = again ? c->rc_anch : c->cons_anch;
    const uint64_t total = again ? c->as.recorrect.total : c->cons_total;
    const uint32_t nr = c->nreads;
    const size_t nrec = c->as.records.size();
    const uint64_t njobs = 2 * (uint64_t)nrec;
    if (total >= 0x7FFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "recorrect: the corrected reads must have fewer than 2^31 bases");
    StageState::Recorrect out;
    bella_recorrect_stats st{};
    st.round = again ? c->as.recorrect.stats.round + 1 : 2;
    st.bases_before = total;
    st.jobs = njobs;
    const size_t nst = sizeof(bella_consensus_read) * std::max<size_t>(nr, 1);
    TmpBuf nbases, noffs, nstats, nanch, jrec;                        // the round's result
    uint64_t nout = total;
    ENSURE(c, noffs, 8 * ((size_t)nr + 1)); ENSURE(c, nstats, nst); ENSURE(c, nanch, 8 * (size_t)c->rc_nanch);
    std::vector<bella_consensus_read> hs(nr);
    if (!nrec) {                                                      // (no record: nothing is launched, the input is the result)
        st.none = njobs;
        std::vector<uint64_t> ho((size_t)nr + 1, 0);
        HIPCHK(c, hipMemcpyAsync(ho.data(), coffs.p, 8 * ((size_t)nr + 1), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t r = 0; r < nr; ++r) hs[r].len_before = hs[r].len_after = (uint32_t)(ho[r + 1] - ho[r]);
        ENSURE(c, nbases, (size_t)total);
        ENSURE(c, jrec, sizeof(bella_recorrect_job) * (size_t)njobs);
        HIPCHK(c, hipMemsetAsync(jrec.p, 0, sizeof(bella_recorrect_job) * (size_t)njobs, c->stream));
        HIPCHK(c, hipMemcpyAsync(noffs.p, coffs.p, 8 * ((size_t)nr + 1), hipMemcpyDeviceToDevice, c->stream));
        if (total) HIPCHK(c, hipMemcpyAsync(nbases.p, cbases.p, (size_t)total, hipMemcpyDeviceToDevice, c->stream));
        if (c->rc_nanch) HIPCHK(c, hipMemcpyAsync(nanch.p, canch.p, 8 * (size_t)c->rc_nanch, hipMemcpyDeviceToDevice, c->stream));
        if (nr) HIPCHK(c, c->stager.h2d(nstats.p, hs.data(), sizeof(bella_consensus_read) * (size_t)nr, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        if (njobs >= 0x7FFFFFF0ull) return fail(c, BELLA_ERR_BAD_ARG, "recorrect: fewer than 2^30 overlap records");
        const uint32_t nj_all = (uint32_t)njobs;
        const size_t npw = (size_t)(total / 16 + 1);
        TmpBuf recs, upk, table, votes, counts, jbase, live, pend, next, bytes, pre, ctl, touch;
        int rc = upload_records(c, recs);
        if (rc) return rc;
        ENSURE(c, upk, 4 * npw);
        const size_t tbytes = (size_t)total * kPileCounters * 4;
        if (ensure_bytes(c, table, tbytes))
            return fail(c, BELLA_ERR_NOMEM, "the correction round's table needs %zu bytes of device memory (36 per base of %llu corrected bases) and they do not fit", tbytes,
                        (unsigned long long)total);
        ENSURE(c, jrec, sizeof(bella_recorrect_job) * (size_t)njobs); ENSURE(c, jbase, sizeof(ReaJob) * (size_t)njobs);
        ENSURE(c, live, (size_t)njobs); ENSURE(c, touch, (size_t)njobs);
        ENSURE(c, pend, 4 * (size_t)njobs); ENSURE(c, next, 4 * (size_t)njobs);
        ENSURE(c, bytes, 8 * ((size_t)njobs + 1)); ENSURE(c, pre, 8 * ((size_t)njobs + 1));
        ENSURE(c, ctl, 32); ENSURE(c, votes, 8); ENSURE(c, counts, sizeof(RecCounts));
        uint64_t* const dctl = ptr<uint64_t>(ctl);
        uint32_t* const dcount = (uint32_t*)(dctl + 2);
        HIPCHK(c, hipMemsetAsync(table.p, 0, tbytes ? tbytes : 16, c->stream));
        HIPCHK(c, hipMemsetAsync(votes.p, 0, 8, c->stream));
        HIPCHK(c, hipMemsetAsync(counts.p, 0, sizeof(RecCounts), c->stream));
        EventSet ev;
        if ((rc = ev.create(c, 3))) return rc;
        const uint32_t* const rpacked = ptr<uint32_t>(c->packed);
        const uint32_t* const upacked = ptr<uint32_t>(upk);
        bella_recorrect_job* const djrec = ptr<bella_recorrect_job>(jrec);
        // ---- placement, and the list of the jobs that take part
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        k_rec_place<<<nblk(njobs), 256, 0, c->stream>>>(ptr<bella_overlap>(recs), (uint32_t)nrec, ptr<uint64_t>(c->roff), ptr<uint64_t>(coffs), ptr<uint64_t>(c->rc_aoff),
                                                        ptr<uint64_t>(canch), djrec, ptr<ReaJob>(jbase), ptr<uint8_t>(live));
        KCHK(c);
        k_rea_pack<<<nblk(npw), 256, 0, c->stream>>>(ptr<uint8_t>(cbases), total, ptr<uint32_t>(upk));
        KCHK(c);
        CUB(c, hipcub::DeviceSelect::Flagged, hipcub::CountingInputIterator<uint32_t>(0u), ptr<uint8_t>(live), ptr<uint32_t>(pend), dcount, (int)nj_all, c->stream);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        uint32_t np = 0;
        HIPCHK(c, hipMemcpyAsync(&np, dcount, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.place_ms = ev_ms(ev.a, ev.b);
        st.none = njobs - np;
        live.reset();
        // ---- DP, walks and votes: band by band, batch by batch
        uint64_t budget = 0;
        if ((rc = round_budget(c, &budget))) return rc;
        RoundBatches<ReaFamily> rb{c, "recorrect", "jobs", ev, rpacked, upacked, ptr<uint32_t>(table), ptr<unsigned long long>(votes), rp.keep_ops != 0, out.ops, st.dp_ms, st.walk_ms, st.vote_ms};
        TmpBuf vnops, opscan;
        for (uint32_t B = rp.band0; np; B *= 2) {
            k_rec_bytes<<<nblk((uint64_t)np + 1), 256, 0, c->stream>>>(ptr<uint32_t>(pend), np, ptr<ReaJob>(jbase), B, ptr<uint64_t>(bytes));
            KCHK(c);
            CUB(c, hipcub::DeviceScan::ExclusiveSum, ptr<uint64_t>(bytes), ptr<uint64_t>(pre), (int)(np + 1), c->stream);
            uint64_t band_bytes = 0;
            HIPCHK(c, hipMemcpyAsync(&band_bytes, ptr<uint64_t>(pre) + np, 8, hipMemcpyDeviceToHost, c->stream));
            const uint32_t maxjobs = round_max_jobs(B, budget);
            for (uint32_t b0 = 0; b0 < np;) {
                k_rec_cut<<<1, 64, 0, c->stream>>>(ptr<uint64_t>(pre), np, b0, budget, maxjobs, dctl);
                KCHK(c);
                uint64_t cut[2] = {0, 0};
                HIPCHK(c, hipMemcpyAsync(cut, dctl, 16, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                const uint32_t b1 = (uint32_t)cut[0], nj = b1 - b0;
                const uint64_t dbytes = cut[1];
                if (b1 <= b0 || b1 > np) return fail(c, BELLA_ERR_STATE, "recorrect: a batch [%u, %u) of %u pending jobs", b0, b1, np);
                ENSURE(c, rb.jobs, sizeof(ReaJob) * (size_t)nj);
                ENSURE(c, vnops, 4 * ((size_t)nj + 1)); ENSURE(c, opscan, 8 * ((size_t)nj + 1));
                st.dir_bytes_peak = std::max<uint64_t>(st.dir_bytes_peak, dbytes);
                ++st.batches;
                k_rec_gather<<<nblk(nj), 256, 0, c->stream>>>(ptr<uint32_t>(pend), b0, nj, ptr<ReaJob>(jbase), ptr<uint64_t>(pre), B, ptr<ReaJob>(rb.jobs));
                KCHK(c);
                if ((rc = rb.dp_count(nj, B, dbytes))) return rc;
                k_rec_settle<<<nblk((uint64_t)nj + 1), 256, 0, c->stream>>>(ptr<uint32_t>(pend), b0, nj, ptr<ReaRes>(rb.res), ptr<ReaCnt>(rb.cnt), B, rp.band_max, rp.min_identity, djrec,
                                                                           ptr<uint8_t>(touch), ptr<uint32_t>(vnops), ptr<RecCounts>(counts));
                KCHK(c);
                HIPCHK(c, hipEventRecord(ev.d, c->stream));
                if ((rc = scan_u32_to_u64(c, ptr<uint32_t>(vnops), ptr<uint64_t>(opscan), (uint64_t)nj + 1))) return rc;
                uint64_t nops = 0;
                HIPCHK(c, hipMemcpyAsync(&nops, ptr<uint64_t>(opscan) + nj, 8, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                rb.counted();
                if (nops) {
                    k_rec_opoff<<<nblk(nj), 256, 0, c->stream>>>(ptr<uint32_t>(pend), b0, nj, ptr<uint32_t>(vnops), ptr<uint64_t>(opscan),
                                                                 rp.keep_ops ? (uint64_t)out.ops.size() : ~0ull, ptr<ReaJob>(rb.jobs), djrec);
                    KCHK(c);
                    if ((rc = rb.write_vote(nj, nops))) return rc;
                }
                b0 = b1;
            }
            st.dp_cells += 4 * band_bytes;                            // (n B / 4 bytes per job)
            if (B >= rp.band_max) break;
            CUB(c, hipcub::DeviceSelect::Flagged, ptr<uint32_t>(pend), ptr<uint8_t>(touch), ptr<uint32_t>(next), dcount, (int)np, c->stream);
            HIPCHK(c, hipMemcpyAsync(&np, dcount, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            pend.swap(next);
        }
        rb.dirs.reset(); rb.scr.reset(); rb.ops.reset(); jbase.reset(); pend.reset(); next.reset(); bytes.reset(); pre.reset(); touch.reset();
        RecCounts hc{};
        HIPCHK(c, hipMemcpyAsync(&st.votes, votes.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&hc, counts.p, sizeof(RecCounts), hipMemcpyDeviceToHost, c->stream));
        if (rp.keep_ops) {
            out.table.resize((size_t)total * kPileCounters);
            HIPCHK(c, c->stager.d2h(out.table.data(), table.p, tbytes, c->stream));
        }
        // ---- consensus: every current sequence a read whose own bases are the sequence that was aligned against; the new anchors
        TmpBuf emit, scan;
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        if ((rc = consensus_tail(c, table, upacked, coffs, nr, total, rp.min_depth, emit, scan, nstats, noffs, nbases, &nout))) return rc;
        st.band_capped = hc.band_capped; st.low_identity = hc.low_identity; st.voted = hc.voted;      // (the tail has waited for the device)
        k_rec_anchors<<<nblk(c->rc_nanch), 256, 0, c->stream>>>(ptr<uint64_t>(coffs), ptr<uint64_t>(scan), ptr<uint64_t>(c->rc_aoff), ptr<uint64_t>(canch), nr, c->rc_nanch,
                                                              ptr<uint64_t>(nanch));
        KCHK(c);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, c->stager.d2h(hs.data(), nstats.p, sizeof(bella_consensus_read) * (size_t)nr, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        st.decide_ms = ev_ms(ev.a, ev.b);
        for (uint32_t r = 0; r < nr; ++r) { st.substituted += hs[r].substituted; st.deleted += hs[r].deleted; st.inserted += hs[r].inserted; }
    }
    st.bases_after = nout;
    out.stats = st;
    out.total = nout;
    out.njobs = njobs;
    nbases.give_to(c->rc_out); noffs.give_to(c->rc_offs); nstats.give_to(c->rc_stats); nanch.give_to(c->rc_anch); jrec.give_to(c->rc_jobs);
    c->as.recorrect = std::move(out);
    made(c, RECORRECT);
    if (total_bases) *total_bases = nout;
    return 0;
}

int bella_hip_get_recorrected(bella_ctx* c, uint64_t* offsets, uint8_t* bases, bella_consensus_read* stats) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, RECORRECT)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (offsets) HIPCHK(c, c->stager.d2h(offsets, c->rc_offs.p, 8 * ((size_t)c->nreads + 1), c->stream));
    if (bases && c->as.recorrect.total) HIPCHK(c, c->stager.d2h(bases, c->rc_out.p, (size_t)c->as.recorrect.total, c->stream));
    if (stats && c->nreads) HIPCHK(c, c->stager.d2h(stats, c->rc_stats.p, sizeof(bella_consensus_read) * (size_t)c->nreads, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bella_hip_get_recorrect_jobs(bella_ctx* c, uint64_t* njobs, bella_recorrect_job* out) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, RECORRECT)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n = c->as.recorrect.njobs;
    if (njobs) *njobs = n;
    if (out && n) {
        HIPCHK(c, c->stager.d2h(out, c->rc_jobs.p, sizeof(bella_recorrect_job) * (size_t)n, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

int bella_hip_get_recorrect_ops(bella_ctx* c, uint64_t* nops, uint32_t* ops, uint32_t* table) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, RECORRECT)) return r;
    if (nops) *nops = c->as.recorrect.ops.size();
    copy_out(ops, c->as.recorrect.ops);
    copy_out(table, c->as.recorrect.table);
    return 0;
}

int bella_hip_get_recorrect_stats(bella_ctx* c, void* out, uint64_t struct_size) {
    return get_stats(c, RECORRECT, out, struct_size, [](const StageState& a) { return a.recorrect.stats; });
}

int bella_hip_get_recorrect_anchors(bella_ctx* c, uint64_t* offsets, uint64_t* anchors) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, CONS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const Buf& a = has(c, RECORRECT) ? c->rc_anch : c->cons_anch;
    if (offsets) HIPCHK(c, c->stager.d2h(offsets, c->rc_aoff.p, 8 * ((size_t)c->nreads + 1), c->stream));
    if (anchors && c->rc_nanch) HIPCHK(c, c->stager.d2h(anchors, a.p, 8 * (size_t)c->rc_nanch, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// both writers of the unitig GFA: `who` is the one that was called; alns == NULL: every L line carries <ovl>M
static int write_unitig_gfa_impl(const char* who, const char* path, uint32_t nreads, const char* const* names, uint64_t nunitigs, const uint64_t* vertex_offsets,
                                 const uint32_t* vertices, const uint64_t* pos, const uint32_t* nbases, const uint64_t* len, const uint8_t* circular,
                                 const uint64_t* base_offsets, const uint8_t* bases, uint64_t nlinks, const bella_unitig_link* links, const bella_link_aln* alns,
                                 const uint32_t* ops) {
    if (!path || (nreads && !names) || (nunitigs && (!vertex_offsets || !vertices || !pos || !nbases || !len || !circular)) || (bases && !base_offsets) || (nlinks && !links) || (nlinks && alns && !ops)) {
        fprintf(stderr, "%s: null argument\n", who);
        return BELLA_ERR_BAD_ARG;
    }
    const uint64_t nvert = nunitigs ? vertex_offsets[nunitigs] : 0;
    for (uint64_t i = 0; i < nvert; ++i)
        if (vertices[i] >= 2 * (uint64_t)nreads || !names[vertices[i] >> 1]) { fprintf(stderr, "%s: vertex %llu out of range\n", who, (unsigned long long)i); return BELLA_ERR_BAD_ARG; }
    for (uint64_t i = 0; i < nlinks; ++i)
        if (links[i].a >= nunitigs || links[i].b >= nunitigs) { fprintf(stderr, "%s: link %llu out of range\n", who, (unsigned long long)i); return BELLA_ERR_BAD_ARG; }
    TextFile file(who, path, "wb");
    FILE* const f = file.f;
    if (!f) return BELLA_ERR_BAD_ARG;
    bool ok = std::fputs("H\tVN:Z:1.0\n", f) != EOF;
    char name[32], other[32];
    std::string cigar;
    auto mk = [&](char* dst, uint64_t u) { std::snprintf(dst, 32, "utg%06llu%c", (unsigned long long)(u + 1), circular[u] ? 'c' : 'l'); };
    for (uint64_t u = 0; u < nunitigs && ok; ++u) {
        mk(name, u);
        ok = std::fprintf(f, "S\t%s\t", name) > 0;
        if (ok && bases) { const size_t n = (size_t)(base_offsets[u + 1] - base_offsets[u]); ok = n == 0 || std::fwrite(bases + base_offsets[u], 1, n, f) == n; }
        else if (ok) ok = std::fputc('*', f) != EOF;
        ok = ok && std::fprintf(f, "\tLN:i:%llu\tRC:i:%llu\n", (unsigned long long)len[u], (unsigned long long)(vertex_offsets[u + 1] - vertex_offsets[u])) > 0;
        for (uint64_t i = vertex_offsets[u]; i < vertex_offsets[u + 1] && ok; ++i)
            ok = std::fprintf(f, "a\t%s\t%llu\t%s\t%c\t%u\n", name, (unsigned long long)pos[i], names[vertices[i] >> 1], (vertices[i] & 1) ? '-' : '+', nbases[i]) > 0;
    }
    for (uint64_t i = 0; i < nlinks && ok; ++i) {
        const bella_unitig_link& l = links[i];
        mk(name, l.a); mk(other, l.b);
        if (alns && alns[i].status == BELLA_LINK_ALIGNED) {           // the CIGAR in M / I / D: '=' and 'X' are one M
            const bella_link_aln& a = alns[i];
            cigar.clear();
            uint64_t run = 0;
            char last = 0;
            for (uint32_t x = 0; x <= a.nops; ++x) {
                const uint32_t w = x < a.nops ? ops[a.op_off + x] : 0u;
                const char ch = x == a.nops ? 0 : (w & 15u) <= kOpX ? 'M' : (w & 15u) == kOpIns ? 'I' : 'D';
                if (ch != last && run) { cigar += std::to_string(run); cigar += last; run = 0; }
                last = ch;
                run += w >> 4;
            }
            ok = std::fprintf(f, "L\t%s\t%c\t%s\t%c\t%s\trc:i:%u\tNM:i:%u\tol:i:%u\n", name, (l.flags & BELLA_UNITIG_LINK_A_MINUS) ? '-' : '+', other,
                              (l.flags & BELLA_UNITIG_LINK_B_MINUS) ? '-' : '+', cigar.c_str(), l.rec, a.n_x + a.n_ins + a.n_del, l.ovl) > 0;
            continue;
        }
        ok = std::fprintf(f, "L\t%s\t%c\t%s\t%c\t%uM\trc:i:%u\n", name, (l.flags & BELLA_UNITIG_LINK_A_MINUS) ? '-' : '+', other, (l.flags & BELLA_UNITIG_LINK_B_MINUS) ? '-' : '+', l.ovl,
                         l.rec) > 0;
    }
    return file.close(ok);
}

int bella_hip_write_unitig_gfa(const char* path, uint32_t nreads, const char* const* names, uint64_t nunitigs, const uint64_t* vertex_offsets, const uint32_t* vertices,
                               const uint64_t* pos, const uint32_t* nbases, const uint64_t* len, const uint8_t* circular, const uint64_t* base_offsets,
                               const uint8_t* bases, uint64_t nlinks, const bella_unitig_link* links) {
    return write_unitig_gfa_impl("bella_hip_write_unitig_gfa", path, nreads, names, nunitigs, vertex_offsets, vertices, pos, nbases, len, circular, base_offsets, bases, nlinks,
                                 links, nullptr, nullptr);
}

int bella_hip_write_unitig_gfa_links(const char* path, uint32_t nreads, const char* const* names, uint64_t nunitigs, const uint64_t* vertex_offsets, const uint32_t* vertices,
                                     const uint64_t* pos, const uint32_t* nbases, const uint64_t* len, const uint8_t* circular, const uint64_t* base_offsets,
                                     const uint8_t* bases, uint64_t nlinks, const bella_unitig_link* links, const bella_link_aln* alns, const uint32_t* ops) {
    return write_unitig_gfa_impl("bella_hip_write_unitig_gfa_links", path, nreads, names, nunitigs, vertex_offsets, vertices, pos, nbases, len, circular, base_offsets, bases,
                                 nlinks, links, alns, ops);
}

int bella_hip_get_read_bases(bella_ctx* c, uint64_t* offsets, uint8_t* bases) {
    if (!c) return BELLA_ERR_BAD_ARG;
    if (int r = need(c, READS)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    if (offsets) {
        offsets[0] = 0;
        for (uint32_t r = 0; r < c->nreads; ++r) offsets[r + 1] = offsets[r] + c->host_lens[r];
    }
    if (bases && c->total_bases) {
        const size_t nw = (size_t)((c->total_bases + 15) / 16);
        std::vector<uint32_t> w(nw);
        HIPCHK(c, c->stager.d2h(w.data(), c->packed.p, 4 * nw, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint64_t g = 0; g < c->total_bases; ++g) bases[g] = (uint8_t)"ACGT"[(w[(size_t)(g >> 4)] >> ((uint32_t)(g & 15) * 2)) & 3u];
    }
    return 0;
}

int bella_hip_write_gfa(const char* path, uint32_t nreads, const char* const* names, const uint32_t* lens, const uint64_t* base_offsets, const uint8_t* bases,
                        const uint64_t* offsets, const bella_graph_edge* edges, const uint8_t* contained) {
    if (!path || !offsets || (nreads && (!names || !lens || !contained)) || (bases && !base_offsets) || (offsets[2 * (size_t)nreads] && !edges)) {
        fprintf(stderr, "bella_hip_write_gfa: null argument\n");
        return BELLA_ERR_BAD_ARG;
    }
    const uint64_t ne = offsets[2 * (size_t)nreads];
    for (uint64_t i = 0; i < ne; ++i)
        if (edges[i].src >= 2 * (uint64_t)nreads || edges[i].dst >= 2 * (uint64_t)nreads) { fprintf(stderr, "bella_hip_write_gfa: edge %llu: vertex out of range\n", (unsigned long long)i); return BELLA_ERR_BAD_ARG; }
    TextFile file("bella_hip_write_gfa", path, "wb");
    FILE* const f = file.f;
    if (!f) return BELLA_ERR_BAD_ARG;
    bool ok = std::fputs("H\tVN:Z:1.0\n", f) != EOF;
    for (uint32_t r = 0; r < nreads && ok; ++r) {
        if (contained[r]) continue;
        if (!names[r]) { ok = false; break; }
        ok = std::fprintf(f, "S\t%s\t", names[r]) > 0;
        if (ok && bases) { const size_t nb = (size_t)(base_offsets[r + 1] - base_offsets[r]); ok = nb == 0 || std::fwrite(bases + base_offsets[r], 1, nb, f) == nb; }
        else if (ok) ok = std::fputc('*', f) != EOF;
        ok = ok && std::fprintf(f, "\tLN:i:%u\n", lens[r]) > 0;
    }
    for (uint64_t i = 0; i < ne && ok; ++i) {
        const bella_graph_edge& e = edges[i];
        ok = std::fprintf(f, "L\t%s\t%c\t%s\t%c\t%uM\tel:i:%u\trc:i:%u\n", names[e.src >> 1], (e.src & 1) ? '-' : '+', names[e.dst >> 1], (e.dst & 1) ? '-' : '+', e.ovl, e.len, e.rec) > 0;
    }
    return file.close(ok);
}

int bella_hip_write_output_traced(const char* path, const bella_params* p, uint32_t nreads, const char* const* names, const uint32_t* lens, const bella_pair* pairs,
                                  const bella_aln* alns, const bella_trace* traces, const uint32_t* ops, uint64_t nops_total, uint64_t npairs, int nthreads,
                                  bella_write_stats* stats) {
    std::string err;
    if ((npairs && (!traces || !alns)) || (nops_total && !ops) || (p && p->skip_alignment)) {     // (no pairs: nothing is required, as in bella_hip_write_output)
        fprintf(stderr, "bella_hip_write_output_traced: traces and alignments are required\n");
        return BELLA_ERR_BAD_ARG;
    }
    static const bella_trace none{};
    const int rc = write_output_impl(path, p, 1, nreads, names, lens, pairs, alns, npairs, nthreads, stats, err, traces ? traces : &none, ops, nops_total);
    if (rc) fprintf(stderr, "bella_hip_write_output_traced: %s\n", err.c_str());
    return rc;
}

}  // extern "C"
