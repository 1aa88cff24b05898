// bella_hip_driver.hpp -- what a host program does AROUND the C ABI once the operands are on the device: the reference's stage plan,
// the passes, the alignment, the output file and the stdout protocol of HashSpGEMM (include/overlap.hpp:650-789).  Shared by the two
// host programs of this repository: the reference-side shim (bella_hip_shim.hpp: BELLA's own main.cpp, its k-mer counter and CSC
// constructor on the host) and the native command line (bella_hip_main.cpp: FASTQ to output file on the device).  No reference types,
// no reference code: plain C++ over include/bella_hip.h.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "bella_hip.h"

namespace bella_hip_detail {

inline void check(bella_ctx* c, int rc, const char* what) {
    if (rc == 0) return;
    std::cerr << "bella_hip: " << what << " failed: " << (c ? bella_hip_last_error(c) : bella_hip_strerror(rc)) << " (" << rc << ")"
              << std::endl;
    std::abort();                                    // (the reference returns void and prints; CSC.cpp:269 aborts the same way)
}

// a host array the library fills: no value-initialisation (std::vector::resize writes 2.4 GB of zeros in front of the copy that
// overwrites them: 0.25 s of a 100k-read run with alignment)
template <class T>
struct RawBuf {
    T* p = nullptr;
    size_t n = 0, cap = 0;
    RawBuf() = default;
    RawBuf(const RawBuf&) = delete;
    RawBuf& operator=(const RawBuf&) = delete;
    RawBuf(RawBuf&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    ~RawBuf() { std::free(p); }
    void resize(size_t m) {
        if (m > cap) { std::free(p); p = (T*)std::malloc(m * sizeof(T) + 64); if (!p) { std::cerr << "bella_hip: out of host memory" << std::endl; std::abort(); } cap = m; }
        n = m;
    }
    T* data() { return p; }
    const T* data() const { return p; }
    const T* begin() const { return p; }
    size_t size() const { return n; }
};

// one context = one GPU: operands in, then per stage [lo, hi): overlap (+ alignment) and the records of ITS columns
struct Worker {
    bella_ctx* ctx = nullptr;
    std::vector<uint64_t> colptr;            // colptrC of the last pass (nreads + 1)
    RawBuf<bella_pair> pairs;
    RawBuf<bella_aln> alns;
    RawBuf<bella_trace> traces;              // --cigar: the stage's traced alignments and their runs
    RawBuf<uint32_t> ops;
    uint64_t nnzc = 0;
    uint64_t gap_runs = 0, shifted_runs = 0, shifted_columns = 0;      // normalize_gaps: summed over the stages (bella_vote_stats)
    bella_clip_stats clip{};                 // clip_ends: summed over the stages (bella_clip_stats)
};
// what the last call of this process did (tests, logs): every column must be computed by the numeric phase exactly once
struct CallStats {
    uint64_t numeric_columns = 0;    // sum over the contexts of the columns their numeric passes computed
    uint64_t numeric_passes = 0, symbolic_passes = 0;
    uint64_t nreads = 0;
    int stages = 0, contexts = 0;
    uint64_t layout_B_bytes_max = 0, layout_B_bytes_sum = 0;   // B' per context: follows the partition
    uint64_t host_upload_bytes = 0;  // matrix bytes that went host -> device, all contexts together
    uint64_t nnzc = 0, lines = 0;    // nnz(C); lines written
    double overlap_seconds = 0, align_seconds = 0, write_seconds = 0;   // wall clock, summed over the stages
};
inline CallStats& last_call_stats() { static CallStats s; return s; }   // single caller, like HashSpGEMM itself (not re-entrant: overlap.hpp:92)

// the reference's printLog (include/common/common.h:40-44): "INFO:\tfile(line)\tname = value" on stderr
#define BELLA_HIP_LOGT(tag, var) do { std::cerr << "INFO:\t" << (tag) << "(" << __LINE__ << ")\t" << #var << " = " << (var) << std::endl; } while (0)

inline void on_all(int N, const std::function<void(int)>& fn) {             // one host thread per context
    if (N == 1) { fn(0); return; }
    std::vector<std::thread> th;
    for (int g = 0; g < N; ++g) th.emplace_back(fn, g);
    for (auto& t : th) t.join();
}

// One slab of device memory up front (bella_hip_reserve): every stage then cuts its buffers from it instead of going to the driver --
// the first hipMalloc of a multi-GB buffer costs tens of ms per GB on ROCm 7.2.  Sized like bench.py sizes it: 44 bytes per base of the
// read set (what counting + assembly + one pass hold at their peak), at least 1 GB; a failed reservation is not an error (the stages
// allocate for themselves).  BELLA_HIP_NO_RESERVE=1 leaves it out.
inline void reserve_for(bella_ctx* ctx, uint64_t total_bases, int contexts_per_device) {
    if (std::getenv("BELLA_HIP_NO_RESERVE")) return;
    uint64_t per_base = 44;
    if (const char* e = std::getenv("BELLA_HIP_RESERVE_BYTES_PER_BASE")) per_base = (uint64_t)std::strtoull(e, nullptr, 10);
    uint64_t want = per_base * total_bases;
    if (want < (1ull << 30)) want = 1ull << 30;
    if (contexts_per_device > 1) want /= (uint64_t)contexts_per_device;
    double ms = 0.0;
    while (want >= (1ull << 29) && bella_hip_reserve(ctx, want, &ms) != 0) want /= 2;   // (a slab the device cannot give: try half)
}

struct StageOpts {
    int N = 1;                       // contexts
    uint32_t nreads = 0;
    bella_params p{};
    int paf = 0;
    double total_memory_mb = 0;      // BELLApars::totalMemory (-m); <= 0: one stage
    double per_nnz = 20.0;           // sizeof(spmatPtr_) + sizeof(uint32_t) = 16 + 4 (overlap.hpp:365-404)
    const char* filename = nullptr;  // the output file: lines are APPENDED
    const char* tag = "bella_hip_driver.hpp";   // the log lines' file name
    int exact = 0;                   // alignments by the exact (growing band) X-drop of the reference's CUDA build
    int cigar = 0;                   // true PAF: every stage traces its passed pairs before it writes them (needs paf, no skip_alignment)
    uint32_t trace_band = 0;         // first band of the traces; 0 = the library's default
    const char* correct = nullptr;   // read correction: every stage piles its traced pairs up on the device, the consensus
                                     // of every read is written to this FASTA file after the last stage (needs alignment)
    uint32_t min_depth = 3;          // ... positions with fewer votes keep the read's own base
    const char* gfa = nullptr;       // string graph: every stage adds its traced passed pairs as overlap records, the graph is
                                     // built on the device after the last stage and written to this GFA 1 file (needs alignment)
    uint32_t gfa_min_overlap = 1000, gfa_max_overhang = 1000, gfa_fuzz = 1000;
    int gfa_no_seq = 0;              // S lines carry '*' instead of the reads' bases
    const char* unitigs = nullptr;   // unitigs: tips are clipped off the graph, the unitigs of the cleaned graph are written as GFA 1 ...
    const char* unitigs_fasta = nullptr;   // ... and / or as FASTA; either one builds the graph, with or without gfa
    uint32_t tip_reads = 4, tip_rounds = 3;
    int gfa_clean = 0;               // the gfa file shows the cleaned graph (removed reads' S lines dropped like contained ones)
    int pop_bubbles = 0;             // bubble popping after the tip clipping, before the unitigs and the cleaned gfa file
    uint32_t bubble_reads = 64, bubble_dist = 50000, bubble_rounds = 3;
    int polish = 0;                  // unitig consensus: every stage's traced pairs vote as with correct; the unitigs files carry the
    uint32_t polish_min_depth = 3;   // polished sequences and coordinates
    uint32_t polish_rounds = 1;      // consensus rounds: polish_rounds - 1 realignment rounds follow the polish, each aligning the reads
    uint32_t realign_band = 512, realign_min_identity = 700;    // against the round before; the files carry the last round's sequences and coordinates
    bool realign_circular = false;   // those rounds place the reads of circular unitigs on the unrolled circle
    int align_links = 0;             // link alignment: the ends of the unitigs every link joins are aligned on the device, on the sequences
    uint32_t link_band = 512, link_min_identity = 700;          // the unitigs file carries; its ALIGNED L lines take a true CIGAR, NM:i: and ol:i:
    int trim = 0;                    // coverage trimming: the reads are clipped to their longest well-covered stretch before the graph
    uint32_t trim_depth = 3, trim_end_clip = 500;     // is built (min_span = gfa_min_overlap); every graph file is in clipped coordinates
    const char* trimmed_reads = nullptr;              // the clipped reads as FASTA, in input order, without the uncovered ones
    int cut_weak = 0;                // weak-overlap removal after the tip clipping and the bubble popping: weak_steps + 1 cuts with the
    uint32_t weak_min = 500, weak_max = 700, weak_steps = 2;   // ratio rising from weak_min to weak_max permille, tips and bubbles again after each that cut
    uint32_t correct_rounds = 1;     // correction rounds: correct_rounds - 1 rounds follow the consensus, each aligning the partners'
    uint32_t correct_band = 512, correct_min_identity = 700;    // raw clips against the corrected reads of the round before; the file carries the last round
    int normalize_gaps = 0;          // gap normalisation of every stage's votes
    int clip_ends = 0;               // every stage's traced alignments are clipped at clip_identity permille
    uint32_t clip_identity = BELLA_CLIP_DEFAULT_IDENTITY;
    bool graph() const { return gfa || unitigs || unitigs_fasta; }
    bool pileup() const { return correct || polish; }
    bool records() const { return graph() || (correct && correct_rounds > 1); }      // every stage adds its traced passed pairs as overlap records
};

// After the last stage: the records of the contexts 1 .. N-1 (each added its own columns' pairs) are gathered into context 0 in the
// single-context order -- column ascending; a column's pairs all come from one context, in its order.  Once, before the correction rounds
// and the graph.
inline void gather_records(std::vector<Worker>& W, const StageOpts& o) {
    bella_ctx* const c0 = W[0].ctx;
    if (o.N > 1) {
        std::vector<bella_overlap> all;
        for (int g = 0; g < o.N; ++g) {
            bella_ctx* const cg = W[(size_t)g].ctx;
            uint64_t n = 0;
            check(cg, bella_hip_graph_get_overlaps(cg, nullptr, &n), "bella_hip_graph_get_overlaps");
            const size_t at = all.size();
            all.resize(at + (size_t)n);
            if (n) check(cg, bella_hip_graph_get_overlaps(cg, all.data() + at, &n), "bella_hip_graph_get_overlaps");
        }
        std::stable_sort(all.begin(), all.end(), [](const bella_overlap& a, const bella_overlap& b) { return a.cid < b.cid; });
        check(c0, bella_hip_graph_reset(c0), "bella_hip_graph_reset");
        check(c0, bella_hip_graph_add_overlaps(c0, all.data(), all.size()), "bella_hip_graph_add_overlaps");
    }
}

// The string graph from context 0's (gathered) records: the build on the device and the GFA file.
inline void write_graph(std::vector<Worker>& W, const StageOpts& o, const char* const* names, const uint32_t* lens) {
    bella_ctx* const c0 = W[0].ctx;
    std::vector<bella_read_clip> clips;                              // --trim: on context 0, after the records are gathered: -m and -g change nothing
    if (o.trim) {
        bella_graph_trim_params tp;
        tp.struct_size = (uint32_t)sizeof(tp);
        tp.min_depth = o.trim_depth; tp.end_clip = o.trim_end_clip; tp.min_span = o.gfa_min_overlap;
        check(c0, bella_hip_graph_trim(c0, &tp), "bella_hip_graph_trim");
        clips.resize(o.nreads);
        check(c0, bella_hip_graph_get_trim(c0, clips.data()), "bella_hip_graph_get_trim");
    }
    bella_graph_params gp;
    gp.struct_size = (uint32_t)sizeof(gp);
    gp.min_overlap = o.gfa_min_overlap; gp.max_overhang = o.gfa_max_overhang; gp.overhang_permille = 800; gp.fuzz = o.gfa_fuzz;
    check(c0, bella_hip_graph_build(c0, &gp), "bella_hip_graph_build");
    std::vector<uint64_t> boffs;
    RawBuf<uint8_t> bases;
    std::vector<uint32_t> clens;                                      // --trim: the clipped lengths; the reads' bases are cut to the clips in place
    auto read_bases = [&]() {
        if (!boffs.empty()) return;
        boffs.assign((size_t)o.nreads + 1, 0);
        check(c0, bella_hip_get_read_bases(c0, boffs.data(), nullptr), "bella_hip_get_read_bases");
        bases.resize((size_t)boffs[o.nreads] + 1);
        check(c0, bella_hip_get_read_bases(c0, nullptr, bases.data()), "bella_hip_get_read_bases");
        if (!o.trim) return;
        uint64_t at = 0;
        for (uint32_t r = 0; r < o.nreads; ++r) {
            const uint64_t from = boffs[r] + clips[r].beg, n = clips[r].end - clips[r].beg;
            std::memmove(bases.data() + at, bases.data() + from, (size_t)n);
            boffs[r] = at;
            at += n;
        }
        boffs[o.nreads] = at;
    };
    if (o.trim) {
        clens.resize(o.nreads);
        for (uint32_t r = 0; r < o.nreads; ++r) clens[r] = clips[r].end - clips[r].beg;
        lens = clens.data();
        bella_trim_stats ts;
        check(c0, bella_hip_graph_get_trim_stats(c0, &ts, sizeof(ts)), "bella_hip_graph_get_trim_stats");
        const std::string Trim = std::to_string(ts.intervals) + " intervals, " + std::to_string(ts.reads_clipped) + " reads clipped, " + std::to_string(ts.reads_uncovered) +
                                 " uncovered, " + std::to_string(ts.reads_multi) + " with two or more regions, " + std::to_string(ts.bases_before) + " -> " +
                                 std::to_string(ts.bases_after) + " bases, " + std::to_string(ts.records_outside) + " records outside";
        BELLA_HIP_LOGT(o.tag, Trim);
        if (o.trimmed_reads) {
            read_bases();
            std::vector<const char*> tnames;
            std::vector<uint64_t> toffs(1, 0);
            for (uint32_t r = 0; r < o.nreads; ++r)
                if (clens[r]) { tnames.push_back(names[r]); toffs.push_back(boffs[r + 1]); }      // (an uncovered read is empty: the offsets stay consecutive)
            toffs[0] = boffs[0];
            const int wrc = bella_hip_write_fasta(o.trimmed_reads, (uint32_t)tnames.size(), tnames.data(), toffs.data(), bases.data(), 0);
            if (wrc) check(nullptr, wrc, "bella_hip_write_fasta");
        }
    }
    auto write_gfa = [&]() {                                          // the context's current graph
        uint32_t nv = 0;
        uint64_t ne = 0;
        check(c0, bella_hip_graph_get(c0, &nv, &ne, nullptr, nullptr, nullptr), "bella_hip_graph_get");
        std::vector<uint64_t> offs((size_t)nv + 1, 0);
        std::vector<bella_graph_edge> edges((size_t)ne);
        std::vector<uint8_t> contained(o.nreads, 0), removed(o.nreads, 0);
        check(c0, bella_hip_graph_get(c0, nullptr, nullptr, offs.data(), edges.data(), contained.data()), "bella_hip_graph_get");
        check(c0, bella_hip_graph_get_removed(c0, removed.data()), "bella_hip_graph_get_removed");
        for (uint32_t r = 0; r < o.nreads; ++r) contained[r] |= removed[r];
        if (!o.gfa_no_seq) read_bases();
        const int wrc = bella_hip_write_gfa(o.gfa, o.nreads, names, lens, o.gfa_no_seq ? nullptr : boffs.data(), o.gfa_no_seq ? nullptr : bases.data(), offs.data(), edges.data(),
                                            contained.data());
        if (wrc) check(nullptr, wrc, "bella_hip_write_gfa");
    };
    if (o.gfa && !o.gfa_clean) write_gfa();
    bella_graph_stats st;
    check(c0, bella_hip_graph_get_stats(c0, &st, sizeof(st)), "bella_hip_graph_get_stats");
    const std::string StringGraph = std::to_string(st.records) + " records (" + std::to_string(st.n_short) + " short, " + std::to_string(st.n_internal) + " internal), " +
                                    std::to_string(st.contained_reads) + " contained reads, " + std::to_string(st.edges_kept) + " edges, " + std::to_string(st.edges_reduced) +
                                    " reduced, " + std::to_string(st.edges_final) + " final";
    BELLA_HIP_LOGT(o.tag, StringGraph);
    if (!o.unitigs && !o.unitigs_fasta && !o.gfa_clean) return;
    bella_graph_clean_params cp;
    cp.struct_size = (uint32_t)sizeof(cp);
    cp.max_tip_reads = o.tip_reads; cp.tip_rounds = o.tip_rounds;
    check(c0, bella_hip_graph_clean(c0, &cp), "bella_hip_graph_clean");
    bella_bubble_stats bs{};
    bella_graph_bubble_params bp;
    bp.struct_size = (uint32_t)sizeof(bp);
    bp.max_bubble_reads = o.bubble_reads; bp.max_bubble_dist = o.bubble_dist; bp.bubble_rounds = o.bubble_rounds;
    if (o.pop_bubbles) {                                              // (popping cannot create a tip: a bubble is closed)
        check(c0, bella_hip_graph_pop_bubbles(c0, &bp), "bella_hip_graph_pop_bubbles");
        check(c0, bella_hip_graph_get_bubble_stats(c0, &bs, sizeof(bs)), "bella_hip_graph_get_bubble_stats");
    }
    // --cut-weak: miniasm's order -- del_short with a rising ratio, and after every cut that took an edge cut_tip and pop_bubble again.  The
    // stats calls report their last invocation, so the sums of the log line are kept here, and so are the first clean's figures for the
    // Unitigs line.
    bella_unitig_stats first_clean{};
    if (o.cut_weak) {
        check(c0, bella_hip_graph_get_unitig_stats(c0, &first_clean, sizeof(first_clean)), "bella_hip_graph_get_unitig_stats");
        uint64_t cut_edges = 0, clipped_after = 0, popped_after = 0;
        uint32_t r_first = 0, r_last = 0;
        for (uint32_t i = 0; i <= o.weak_steps; ++i) {
            bella_graph_weak_params wp;
            wp.struct_size = (uint32_t)sizeof(wp);
            wp.ratio_permille = o.weak_steps ? o.weak_min + (o.weak_max - o.weak_min) * i / o.weak_steps : o.weak_min;
            if (!i) r_first = wp.ratio_permille;
            r_last = wp.ratio_permille;
            check(c0, bella_hip_graph_cut_weak(c0, &wp), "bella_hip_graph_cut_weak");
            bella_weak_stats ws;
            check(c0, bella_hip_graph_get_weak_stats(c0, &ws, sizeof(ws)), "bella_hip_graph_get_weak_stats");
            cut_edges += ws.edges_removed;
            if (!ws.edges_removed) continue;
            check(c0, bella_hip_graph_clean(c0, &cp), "bella_hip_graph_clean");
            bella_unitig_stats cs;
            check(c0, bella_hip_graph_get_unitig_stats(c0, &cs, sizeof(cs)), "bella_hip_graph_get_unitig_stats");
            clipped_after += cs.reads_removed;
            if (!o.pop_bubbles) continue;
            check(c0, bella_hip_graph_pop_bubbles(c0, &bp), "bella_hip_graph_pop_bubbles");
            bella_bubble_stats ps;
            check(c0, bella_hip_graph_get_bubble_stats(c0, &ps, sizeof(ps)), "bella_hip_graph_get_bubble_stats");
            for (uint32_t r = 0; r < ps.rounds; ++r) popped_after += ps.popped[r];
        }
        const std::string WeakOverlaps = std::to_string(cut_edges) + " edges cut in " + std::to_string(o.weak_steps + 1) + " rounds at " + std::to_string(r_first) + ".." +
                                         std::to_string(r_last) + " permille, " + std::to_string(clipped_after) + " reads clipped after, " + std::to_string(popped_after) +
                                         " bubbles popped after";
        BELLA_HIP_LOGT(o.tag, WeakOverlaps);
    }
    if (o.gfa && o.gfa_clean) write_gfa();
    if (!o.unitigs && !o.unitigs_fasta) return;
    uint64_t nu = 0, nuv = 0, nl = 0, tb = 0;
    check(c0, bella_hip_graph_unitigs(c0, &nu, &nuv, &nl, &tb), "bella_hip_graph_unitigs");
    std::vector<uint64_t> voff((size_t)nu + 1, 0), pos((size_t)nuv), ulen((size_t)nu), uboff((size_t)nu + 1, 0);
    std::vector<uint32_t> verts((size_t)nuv), nb((size_t)nuv);
    std::vector<uint8_t> circ((size_t)nu);
    std::vector<bella_unitig_link> links((size_t)nl);
    RawBuf<uint8_t> ubases;
    ubases.resize((size_t)tb + 1);
    check(c0, bella_hip_graph_get_unitigs(c0, voff.data(), verts.data(), pos.data(), nb.data(), ulen.data(), circ.data(), links.data()), "bella_hip_graph_get_unitigs");
    check(c0, bella_hip_graph_get_unitig_bases(c0, uboff.data(), ubases.data()), "bella_hip_graph_get_unitig_bases");
    bella_polish_stats ps{};
    if (o.polish) {                                                   // the files take the polished coordinates and bases in place of the raw ones
        bella_polish_params pp;
        pp.struct_size = (uint32_t)sizeof(pp);
        pp.min_depth = o.polish_min_depth;
        uint64_t ptotal = 0;
        check(c0, bella_hip_graph_polish_unitigs(c0, &pp, &ptotal), "bella_hip_graph_polish_unitigs");
        std::vector<bella_polish_unitig> pu((size_t)nu);
        ubases.resize((size_t)ptotal + 1);
        check(c0, bella_hip_graph_get_polished(c0, uboff.data(), ubases.data(), pos.data(), nb.data(), pu.data()), "bella_hip_graph_get_polished");
        for (uint64_t u = 0; u < nu; ++u) ulen[(size_t)u] = pu[(size_t)u].len_after;
        check(c0, bella_hip_graph_get_polish_stats(c0, &ps, sizeof(ps)), "bella_hip_graph_get_polish_stats");
        for (uint32_t round = 2; round <= o.polish_rounds; ++round) {
            bella_realign_params rp{};
            rp.struct_size = (uint32_t)sizeof(rp);
            rp.band0 = o.realign_band; rp.band_max = o.realign_band > BELLA_REALIGN_DEFAULT_BAND_MAX ? o.realign_band : BELLA_REALIGN_DEFAULT_BAND_MAX;
            rp.min_identity = o.realign_min_identity; rp.min_depth = o.polish_min_depth;
            if (o.realign_circular) check(c0, bella_hip_graph_realign_unitigs_circular(c0, &rp, &ptotal), "bella_hip_graph_realign_unitigs_circular");
            else check(c0, bella_hip_graph_realign_unitigs(c0, &rp, &ptotal), "bella_hip_graph_realign_unitigs");
            ubases.resize((size_t)ptotal + 1);
            check(c0, bella_hip_graph_get_realigned(c0, uboff.data(), ubases.data(), pos.data(), nb.data(), pu.data()), "bella_hip_graph_get_realigned");
            for (uint64_t u = 0; u < nu; ++u) ulen[(size_t)u] = pu[(size_t)u].len_after;
            bella_realign_stats rs{};
            check(c0, bella_hip_graph_get_realign_stats(c0, &rs, sizeof(rs)), "bella_hip_graph_get_realign_stats");
            uint64_t wrapped = 0;
            check(c0, bella_hip_graph_get_realign_wrapped(c0, &wrapped), "bella_hip_graph_get_realign_wrapped");
            const std::string Realigned = "round " + std::to_string(round) + ": " + std::to_string(rs.voted) + " of " + std::to_string(rs.backbone + rs.contained + rs.unplaced) +
                                      " reads realigned (" + std::to_string(rs.unplaced) + " unplaced, " + std::to_string(rs.outside) + " outside, " +
                                      std::to_string(rs.band_capped) + " band-capped, " + std::to_string(rs.low_identity) + " of low identity), " +
                                      (o.realign_circular ? std::to_string(wrapped) + " across an origin, " : std::string()) +
                                      std::to_string(rs.bases_before) + " -> " + std::to_string(rs.bases_after) + " bases";
            BELLA_HIP_LOGT(o.tag, Realigned);
        }
    }
    std::vector<bella_link_aln> lalns;
    std::vector<uint32_t> lops;
    if (o.align_links) {                                              // on the newest sequences: the ones the files carry
        bella_link_params lp{};
        lp.struct_size = (uint32_t)sizeof(lp);
        lp.band0 = o.link_band; lp.band_max = o.link_band > BELLA_LINK_DEFAULT_BAND_MAX ? o.link_band : BELLA_LINK_DEFAULT_BAND_MAX;
        lp.min_identity = o.link_min_identity;
        check(c0, bella_hip_graph_align_links(c0, &lp, nullptr), "bella_hip_graph_align_links");
        bella_link_stats ls{};
        check(c0, bella_hip_graph_get_link_stats(c0, &ls, sizeof(ls)), "bella_hip_graph_get_link_stats");
        lalns.resize((size_t)nl);
        lops.resize((size_t)ls.ops + 1);
        check(c0, bella_hip_graph_get_link_alignments(c0, lalns.data(), nullptr, lops.data()), "bella_hip_graph_get_link_alignments");
        const std::string AlignedLinks = std::to_string(ls.aligned) + " of " + std::to_string(ls.links) + " links aligned (" + std::to_string(ls.empty) + " empty, " +
                                         std::to_string(ls.band_capped) + " band-capped, " + std::to_string(ls.low_identity) + " of low identity, " + std::to_string(ls.self) +
                                         " self), " + std::to_string(ls.derived) + " derived from their twins, " + std::to_string(ls.overlap_before) + " -> " +
                                         std::to_string(ls.overlap_after) + " overlap bases";
        BELLA_HIP_LOGT(o.tag, AlignedLinks);
    }
    if (o.unitigs) {
        const uint64_t* const so = o.gfa_no_seq ? nullptr : uboff.data();
        const uint8_t* const sb = o.gfa_no_seq ? nullptr : ubases.data();
        const int wrc = o.align_links ? bella_hip_write_unitig_gfa_links(o.unitigs, o.nreads, names, nu, voff.data(), verts.data(), pos.data(), nb.data(), ulen.data(), circ.data(), so,
                                                                         sb, nl, links.data(), lalns.data(), lops.data())
                                      : bella_hip_write_unitig_gfa(o.unitigs, o.nreads, names, nu, voff.data(), verts.data(), pos.data(), nb.data(), ulen.data(), circ.data(), so, sb,
                                                                   nl, links.data());
        if (wrc) check(nullptr, wrc, o.align_links ? "bella_hip_write_unitig_gfa_links" : "bella_hip_write_unitig_gfa");
    }
    if (o.unitigs_fasta) {
        std::vector<std::string> unames((size_t)nu);
        std::vector<const char*> uptr((size_t)nu);
        for (uint64_t u = 0; u < nu; ++u) {
            char buf[32];
            std::snprintf(buf, sizeof(buf), "utg%06llu%c", (unsigned long long)(u + 1), circ[(size_t)u] ? 'c' : 'l');
            unames[(size_t)u] = buf;
            uptr[(size_t)u] = unames[(size_t)u].c_str();
        }
        const int wrc = bella_hip_write_fasta(o.unitigs_fasta, (uint32_t)nu, uptr.data(), uboff.data(), ubases.data(), 0);
        if (wrc) check(nullptr, wrc, "bella_hip_write_fasta");
    }
    bella_unitig_stats us;
    check(c0, bella_hip_graph_get_unitig_stats(c0, &us, sizeof(us)), "bella_hip_graph_get_unitig_stats");
    if (o.cut_weak) { us.reads_removed = first_clean.reads_removed; us.rounds = first_clean.rounds; }   // (the schedule's cleans are in its own line)
    uint64_t npopped = 0;
    for (uint32_t r = 0; r < bs.rounds; ++r) npopped += bs.popped[r];
    const std::string Popped = o.pop_bubbles ? std::to_string(npopped) + " bubbles popped, " + std::to_string(bs.reads_removed) + " reads, " : std::string();
    const std::string Unitigs = std::to_string(us.reads_removed) + " reads clipped in " + std::to_string(us.rounds) + " rounds, " + Popped + std::to_string(us.unitigs) + " unitigs (" +
                                std::to_string(us.circular) + " circular) of " + std::to_string(us.vertices) + " reads, " + std::to_string(us.links) + " links, " +
                                std::to_string(us.total_bases) + " bases, largest " + std::to_string(us.largest) + ", N50 " + std::to_string(us.n50) +
                                (o.polish ? ", polished " + std::to_string(ps.bases_before) + " -> " + std::to_string(ps.bases_after) + " bases" : std::string());
    BELLA_HIP_LOGT(o.tag, Unitigs);
}

// The pileup after the last stage: the tables of the contexts 1 .. N-1 (each piled up its own columns) are added into context 0 in
// chunks of whole reads of at most ~4 M bases (144 MB on the host, whatever the read set).  Once, before the consensus and the polish.
inline void merge_pileups(std::vector<Worker>& W, const StageOpts& o, const uint32_t* lens) {
    const uint32_t nreads = o.nreads;
    bella_ctx* const c0 = W[0].ctx;
    if (o.N > 1) {
        constexpr uint64_t kChunkBases = 4ull << 20;
        std::vector<uint32_t> buf;
        for (uint32_t lo = 0; lo < nreads;) {
            uint32_t hi = lo;
            uint64_t nb = 0;
            while (hi < nreads && (hi == lo || nb + lens[hi] <= kChunkBases)) nb += lens[hi++];
            buf.resize((size_t)nb * BELLA_PILEUP_COUNTERS);
            for (int g = 1; g < o.N; ++g) {
                check(W[(size_t)g].ctx, bella_hip_get_pileup(W[(size_t)g].ctx, lo, hi - lo, buf.data()), "bella_hip_get_pileup");
                check(c0, bella_hip_add_pileup(c0, lo, hi - lo, buf.data()), "bella_hip_add_pileup");
            }
            lo = hi;
        }
    }
}

// Read correction: the consensus of every read from context 0's (merged) table, and the FASTA file.
inline void write_corrected(std::vector<Worker>& W, const StageOpts& o, const char* const* names) {
    const uint32_t nreads = o.nreads;
    bella_ctx* const c0 = W[0].ctx;
    bella_consensus_params cp;
    cp.struct_size = (uint32_t)sizeof(cp);
    cp.min_depth = o.min_depth;
    uint64_t total = 0;
    check(c0, bella_hip_consensus(c0, &cp, &total), "bella_hip_consensus");
    std::vector<uint64_t> offs((size_t)nreads + 1, 0);
    RawBuf<uint8_t> bases;
    bases.resize((size_t)total);
    std::vector<bella_consensus_read> st(nreads);
    check(c0, bella_hip_get_consensus(c0, offs.data(), o.correct_rounds > 1 ? nullptr : bases.data(), st.data()), "bella_hip_get_consensus");
    if (o.correct_rounds <= 1) {
        const int wrc = bella_hip_write_fasta(o.correct, nreads, names, offs.data(), bases.data(), 0);
        if (wrc) check(nullptr, wrc, "bella_hip_write_fasta");
    }
    uint64_t sub = 0, del = 0, ins = 0, cov = 0, all = 0;
    for (const auto& s : st) { sub += s.substituted; del += s.deleted; ins += s.inserted; cov += s.covered; all += s.len_before; }
    const std::string CorrectedReads = std::to_string(nreads) + " reads, " + std::to_string(all) + " -> " + std::to_string(total) + " bases, " + std::to_string(cov) +
                                       " positions covered, " + std::to_string(sub) + " substituted, " + std::to_string(del) + " deleted, " + std::to_string(ins) + " inserted";
    BELLA_HIP_LOGT(o.tag, CorrectedReads);
    if (o.correct_rounds <= 1) return;
    // correction rounds on context 0's gathered records; the file carries the last round
    for (uint32_t round = 2; round <= o.correct_rounds; ++round) {
        bella_recorrect_params rp{};
        rp.struct_size = (uint32_t)sizeof(rp);
        rp.band0 = o.correct_band; rp.band_max = o.correct_band > BELLA_RECORRECT_DEFAULT_BAND_MAX ? o.correct_band : BELLA_RECORRECT_DEFAULT_BAND_MAX;
        rp.min_identity = o.correct_min_identity; rp.min_depth = o.min_depth;
        check(c0, bella_hip_recorrect(c0, &rp, &total), "bella_hip_recorrect");
        bella_recorrect_stats rs{};
        check(c0, bella_hip_get_recorrect_stats(c0, &rs, sizeof(rs)), "bella_hip_get_recorrect_stats");
        const std::string Recorrected = "round " + std::to_string(round) + ": " + std::to_string(rs.voted) + " of " + std::to_string(rs.jobs) + " alignments voted (" +
                                        std::to_string(rs.none) + " without a target, " + std::to_string(rs.band_capped) + " band-capped, " + std::to_string(rs.low_identity) +
                                        " of low identity), " + std::to_string(rs.bases_before) + " -> " + std::to_string(rs.bases_after) + " bases, " +
                                        std::to_string(rs.substituted) + " substituted, " + std::to_string(rs.deleted) + " deleted, " + std::to_string(rs.inserted) + " inserted";
        BELLA_HIP_LOGT(o.tag, Recorrected);
    }
    bases.resize((size_t)total);
    check(c0, bella_hip_get_recorrected(c0, offs.data(), bases.data(), nullptr), "bella_hip_get_recorrected");
    const int wrc = bella_hip_write_fasta(o.correct, nreads, names, offs.data(), bases.data(), 0);
    if (wrc) check(nullptr, wrc, "bella_hip_write_fasta");
}

// Stage plan (overlap.hpp:365-404,682-710), passes, alignment, output.  W[g].ctx holds the operands, laid out for the output columns
// i % N == g.  The products (estimateFLOP, a sum over a count stream) bound nnz(C) from above: if even they fit one stage the numeric phase
// runs at once over all columns; otherwise the symbolic phase (bella_hip_count_pairs = the reference's estimateNNZ_Hash + prefixsum,
// :674-679) gives the exact colptrC the boundaries are taken from -- every column is computed by the numeric phase exactly once.  With
// more than one stage the output is formed stage by stage (each pass holds its own columns only) and APPENDED -- the reference overwrites
// the file from offset 0 in every stage (overlap.hpp:613-636, a defect); the file written here is the single-stage one.
// stdout: nnz(C) (overlap.hpp:686) and, when aligning, the number of lines written per stage (:771).
inline void run_stages(std::vector<Worker>& W, const StageOpts& o, const char* const* names, const uint32_t* lens) {
    const int N = o.N;
    const uint32_t nreads = o.nreads;
    const bella_params& p = o.p;
    const char* const tag = o.tag;
    auto do_overlap = [&](uint32_t lo, uint32_t hi) {                        // the numeric phase on the columns [lo, hi) of every context
        on_all(N, [&](int g) {
            Worker& w = W[(size_t)g];
            check(w.ctx, bella_hip_set_column_range(w.ctx, lo, hi - lo), "bella_hip_set_column_range");
            uint64_t flops = 0;
            check(w.ctx, bella_hip_overlap(w.ctx, &p, &w.nnzc, &flops), "bella_hip_overlap");
            w.colptr.assign((size_t)nreads + 1, 0);
            check(w.ctx, bella_hip_get_pairs(w.ctx, nullptr, nullptr, w.colptr.data()), "bella_hip_get_pairs");
        });
    };
    auto fetch = [&]() {                                                     // the records of the last pass (+ their alignments)
        on_all(N, [&](int g) {
            Worker& w = W[(size_t)g];
            w.pairs.resize(w.nnzc);
            check(w.ctx, bella_hip_get_pairs(w.ctx, w.pairs.data(), nullptr, nullptr), "bella_hip_get_pairs");
            if (!p.skip_alignment) {
                uint64_t npass = 0;
                if (o.exact) check(w.ctx, bella_hip_align_pairs_exact(w.ctx, &p, &npass), "bella_hip_align_pairs_exact");
                else check(w.ctx, bella_hip_align_pairs(w.ctx, &p, &npass), "bella_hip_align_pairs");
                w.alns.resize(w.nnzc);
                if (w.nnzc) check(w.ctx, bella_hip_get_alignments(w.ctx, w.alns.data()), "bella_hip_get_alignments");
                uint64_t ntr = 0, nops = 0;
                // (--correct / --polish: the stage's runs vote on the device; they come to the host only when the true PAF wants them too)
                if (o.clip_ends && (o.pileup() || o.cigar || o.records())) {      // the calls below, flag for flag, through the clip
                    const bool nz = o.pileup() && o.normalize_gaps;
                    const uint32_t fl = BELLA_TRACE_PASSED_ONLY | (o.pileup() ? BELLA_TRACE_PILEUP : 0u) | (nz ? BELLA_TRACE_NORMALIZE : 0u) | (o.cigar ? 0u : BELLA_TRACE_DROP_OPS);
                    const bella_clip_params kp{(uint32_t)sizeof(bella_clip_params), o.clip_identity};
                    check(w.ctx, bella_hip_trace_pairs_clip(w.ctx, &p, o.trace_band, fl, &kp, &ntr, &nops), "bella_hip_trace_pairs_clip");
                    bella_clip_stats ks{};
                    check(w.ctx, bella_hip_get_clip_stats(w.ctx, &ks, sizeof(ks)), "bella_hip_get_clip_stats");
                    w.clip.pairs += ks.pairs; w.clip.clipped += ks.clipped; w.clip.emptied += ks.emptied;
                    w.clip.columns_before += ks.columns_before; w.clip.columns_after += ks.columns_after;
                    w.clip.bases_v_removed += ks.bases_v_removed; w.clip.bases_h_removed += ks.bases_h_removed; w.clip.clip_ms += ks.clip_ms;
                    if (nz) {
                        bella_vote_stats vs{};
                        check(w.ctx, bella_hip_get_vote_stats(w.ctx, &vs, sizeof(vs)), "bella_hip_get_vote_stats");
                        w.gap_runs += vs.gap_runs; w.shifted_runs += vs.shifted_runs; w.shifted_columns += vs.shifted_columns;
                    }
                } else if (o.pileup() && o.normalize_gaps) {
                    const uint32_t fl = BELLA_TRACE_PASSED_ONLY | BELLA_TRACE_PILEUP | BELLA_TRACE_NORMALIZE | (o.cigar ? 0u : BELLA_TRACE_DROP_OPS);
                    check(w.ctx, bella_hip_trace_pairs_flags(w.ctx, &p, o.trace_band, fl, &ntr, &nops), "bella_hip_trace_pairs_flags");
                    bella_vote_stats vs{};
                    check(w.ctx, bella_hip_get_vote_stats(w.ctx, &vs, sizeof(vs)), "bella_hip_get_vote_stats");
                    w.gap_runs += vs.gap_runs; w.shifted_runs += vs.shifted_runs; w.shifted_columns += vs.shifted_columns;
                } else if (o.pileup()) check(w.ctx, bella_hip_trace_pairs_pileup(w.ctx, &p, o.trace_band, o.cigar ? 1 : 0, &ntr, &nops), "bella_hip_trace_pairs_pileup");
                else if (o.cigar) check(w.ctx, bella_hip_trace_pairs(w.ctx, &p, o.trace_band, 1, &ntr, &nops), "bella_hip_trace_pairs");
                // (--gfa alone: the records are all the graph reads; no run is written or staged)
                else if (o.records()) check(w.ctx, bella_hip_trace_pairs_flags(w.ctx, &p, o.trace_band, BELLA_TRACE_PASSED_ONLY | BELLA_TRACE_DROP_OPS, &ntr, &nops), "bella_hip_trace_pairs_flags");
                if (o.records()) check(w.ctx, bella_hip_graph_add_traced(w.ctx, nullptr), "bella_hip_graph_add_traced");
                if (o.cigar) {
                    w.traces.resize(w.nnzc);
                    w.ops.resize(nops);                                       // (host memory: 4 bytes per run; -m stages bound it as they bound the records)
                    check(w.ctx, bella_hip_get_traces(w.ctx, w.traces.data(), w.ops.data()), "bella_hip_get_traces");
                }
            }
        });
    };
    auto merged_colptr = [&](std::vector<uint64_t>& colptrC) {               // column i lives on context i % N
        colptrC.assign((size_t)nreads + 1, 0);
        for (uint32_t i = 0; i < nreads; ++i) {
            const Worker& w = W[(size_t)(i % (uint32_t)N)];
            colptrC[i + 1] = colptrC[i] + (w.colptr[i + 1] - w.colptr[i]);
        }
    };
    if (o.pileup()) on_all(N, [&](int g) { check(W[(size_t)g].ctx, bella_hip_pileup_reset(W[(size_t)g].ctx), "bella_hip_pileup_reset"); });
    if (o.records()) on_all(N, [&](int g) { check(W[(size_t)g].ctx, bella_hip_graph_reset(W[(size_t)g].ctx), "bella_hip_graph_reset"); });
    CallStats& cs = last_call_stats();
    cs = CallStats();
    const double free_memory = o.total_memory_mb * 1024 * 1024;               // estimateMemory, overlap.hpp:365-404 (no LINUX/OSX define)
    const double safety_net = 1.5;                                            // overlap.hpp:92
    const double per_nnz = o.per_nnz;
    std::vector<uint64_t> colptrC;
    uint64_t nnzc = 0;
    std::vector<uint64_t> wflops((size_t)N, 0);
    on_all(N, [&](int g) { check(W[(size_t)g].ctx, bella_hip_count_pairs(W[(size_t)g].ctx, &p, nullptr, nullptr, &wflops[(size_t)g]), "bella_hip_count_pairs (flops)"); });
    uint64_t flops_all = 0;
    for (uint64_t f : wflops) flops_all += f;
    bool computed = false;                                                    // the numeric phase already ran over all columns
    const bool no_budget = !(free_memory > 0.0);                              // -m 0 or unset: one stage (the formula would divide by it)
    const auto t_first = std::chrono::steady_clock::now();
    if (no_budget || safety_net * (double)flops_all * per_nnz <= free_memory) {
        do_overlap(0, nreads);
        computed = true;
    } else {
        on_all(N, [&](int g) {
            Worker& w = W[(size_t)g];
            w.colptr.assign((size_t)nreads + 1, 0);
            uint64_t fl = 0;
            check(w.ctx, bella_hip_count_pairs(w.ctx, &p, w.colptr.data(), &w.nnzc, &fl), "bella_hip_count_pairs");
        });
    }
    cs.overlap_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_first).count();
    merged_colptr(colptrC);
    nnzc = colptrC[nreads];
    std::cout << nnzc << std::endl;                                           // overlap.hpp:686
    const uint64_t required_memory = (uint64_t)(safety_net * nnzc * per_nnz);
    int stages = no_budget ? 1 : (int)std::ceil((double)required_memory / free_memory);       // overlap.hpp:683
    if (stages < 1) stages = 1;
    const uint64_t nnzcperstage = no_budget ? nnzc + 1 : (uint64_t)(free_memory / (safety_net * per_nnz));
    std::vector<uint32_t> colStart((size_t)stages + 1, 0);
    for (int i = 1; i < stages; ++i) {                                        // overlap.hpp:704-710
        auto upper = std::upper_bound(colptrC.begin(), colptrC.end(), (uint64_t)i * nnzcperstage);
        colStart[(size_t)i] = (uint32_t)(upper - colptrC.begin() - 1);
    }
    colStart[(size_t)stages] = nreads;

    for (int b = 0; b < stages; ++b) {
        const uint32_t lo = colStart[(size_t)b], hi = colStart[(size_t)b + 1];
        const auto t_stage = std::chrono::steady_clock::now();
        if (!computed) {
            do_overlap(lo, hi);                                               // (computed: one stage was certain, the pass over all columns ran above)
            cs.overlap_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_stage).count();
        }
        const auto t_align = std::chrono::steady_clock::now();
        fetch();
        const double aligntime = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_stage).count();
        cs.align_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_align).count();
        // the stage's records in the reference's column order (N contexts: column i lives on context i % N)
        const bella_pair* pp = W[0].pairs.data();
        const bella_aln* aa = W[0].alns.data();
        uint64_t np = W[0].nnzc;
        std::vector<bella_pair> mp;
        std::vector<bella_aln> ma;
        std::vector<bella_trace> mt;
        std::vector<uint32_t> mo;
        const bella_trace* tt = W[0].traces.data();
        const uint32_t* oo = W[0].ops.data();
        uint64_t no = W[0].ops.size();
        if (N > 1) {
            for (uint32_t i = lo; i < hi; ++i) {
                const Worker& w = W[(size_t)(i % (uint32_t)N)];
                mp.insert(mp.end(), w.pairs.begin() + (std::ptrdiff_t)w.colptr[i], w.pairs.begin() + (std::ptrdiff_t)w.colptr[i + 1]);
                if (!p.skip_alignment) ma.insert(ma.end(), w.alns.begin() + (std::ptrdiff_t)w.colptr[i], w.alns.begin() + (std::ptrdiff_t)w.colptr[i + 1]);
                if (o.cigar)
                    for (uint64_t q = w.colptr[i]; q < w.colptr[i + 1]; ++q) {       // the runs move into one array, the records' offsets with them
                        bella_trace t = w.traces.data()[q];
                        const uint32_t* src = w.ops.data() + t.op_off;
                        t.op_off = mo.size();
                        mo.insert(mo.end(), src, src + t.nops);
                        mt.push_back(t);
                    }
            }
            pp = mp.data(); aa = ma.data(); np = mp.size(); tt = mt.data(); oo = mo.data(); no = mo.size();
        }
        bella_write_stats ws;
        const int wrc = o.cigar ? bella_hip_write_output_traced(o.filename, &p, nreads, names, lens, pp, aa, tt, oo, no, np, 0, &ws)
                                : bella_hip_write_output(o.filename, &p, o.paf ? 1 : 0, nreads, names, lens, pp, p.skip_alignment ? nullptr : aa, np, 0, &ws);
        if (wrc) check(nullptr, wrc, "bella_hip_write_output");
        cs.write_seconds += ws.seconds;
        cs.lines += ws.lines;
        const std::string ColumnsRange = "[" + std::to_string(lo) + " - " + std::to_string(hi) + "]";
        BELLA_HIP_LOGT(tag, ColumnsRange);
        if (!p.skip_alignment) {                                              // the per-stage statistics of overlap.hpp:750-777
            const std::string AlignmentTime = std::to_string(aligntime) + " seconds";
            BELLA_HIP_LOGT(tag, AlignmentTime);
            const std::string AlignmentRate = std::to_string((long long)((double)ws.aligned_bases / aligntime)) + " bases/second";
            BELLA_HIP_LOGT(tag, AlignmentRate);
            const std::string AverageReadLength = std::to_string(ws.aligned_pairs ? (long long)((double)ws.total_read_len / (2.0 * (double)ws.aligned_pairs)) : 0LL);
            BELLA_HIP_LOGT(tag, AverageReadLength);
            const std::string PairsAligned = std::to_string(ws.aligned_pairs);
            BELLA_HIP_LOGT(tag, PairsAligned);
            std::cout << ws.lines << std::endl;                               // overlap.hpp:771 (per stage)
            const std::string AverageLengthSuccessfulAlignment = std::to_string(ws.lines ? (long long)((double)ws.bases_passed / (double)ws.lines) : 0LL) + " bps";
            BELLA_HIP_LOGT(tag, AverageLengthSuccessfulAlignment);
            const uint64_t nfail = ws.aligned_pairs - ws.lines;
            const std::string AverageLengthFailedAlignment = std::to_string(nfail ? (long long)((double)ws.bases_failed / (double)nfail) : 0LL) + " bps";
            BELLA_HIP_LOGT(tag, AverageLengthFailedAlignment);
        }
        const uint64_t LinesOutputted = ws.lines;
        BELLA_HIP_LOGT(tag, LinesOutputted);
        const std::string OutputtingTime = std::to_string(ws.seconds) + " seconds";
        BELLA_HIP_LOGT(tag, OutputtingTime);
    }
    if (o.pileup()) merge_pileups(W, o, lens);
    if (o.pileup() && o.normalize_gaps) {                                     // the run's sums over stages and contexts
        uint64_t gaps = 0, runs = 0, cols = 0;
        for (const Worker& w : W) { gaps += w.gap_runs; runs += w.shifted_runs; cols += w.shifted_columns; }
        const std::string NormalizedGaps = std::to_string(runs) + " shifted_runs, " + std::to_string(cols) + " shifted_columns (of " + std::to_string(gaps) + " gap runs, two voted reads each)";
        BELLA_HIP_LOGT(tag, NormalizedGaps);
    }
    if (o.clip_ends) {                                                        // the run's sums over stages and contexts
        bella_clip_stats k{};
        for (const Worker& w : W) {
            k.pairs += w.clip.pairs; k.clipped += w.clip.clipped; k.emptied += w.clip.emptied; k.columns_before += w.clip.columns_before;
            k.columns_after += w.clip.columns_after; k.bases_v_removed += w.clip.bases_v_removed; k.bases_h_removed += w.clip.bases_h_removed;
        }
        const std::string ClippedEnds = std::to_string(k.clipped) + " clipped, " + std::to_string(k.emptied) + " emptied (of " + std::to_string(k.pairs) + " traced pairs at identity " +
                                        std::to_string(o.clip_identity) + "), " + std::to_string(k.columns_before - k.columns_after) + " of " + std::to_string(k.columns_before) +
                                        " columns removed, " + std::to_string(k.bases_v_removed + k.bases_h_removed) + " bases";
        BELLA_HIP_LOGT(tag, ClippedEnds);
    }
    if (o.records()) gather_records(W, o);
    if (o.correct) write_corrected(W, o, names);
    if (o.graph()) write_graph(W, o, names, lens);
    cs.nreads = nreads; cs.stages = stages; cs.contexts = N; cs.nnzc = nnzc;
    for (auto& w : W) {
        bella_timings tm;
        bella_memory mm;
        if (bella_hip_get_timings(w.ctx, &tm) == 0) { cs.numeric_columns += tm.numeric_columns; cs.numeric_passes += tm.numeric_passes; cs.symbolic_passes += tm.symbolic_passes; }
        if (bella_hip_get_memory(w.ctx, &mm) == 0) { cs.layout_B_bytes_sum += mm.layout_B_bytes; cs.layout_B_bytes_max = std::max<uint64_t>(cs.layout_B_bytes_max, mm.layout_B_bytes); }
    }
    const uint64_t NumericColumns = cs.numeric_columns, NumericPasses = cs.numeric_passes, SymbolicPasses = cs.symbolic_passes;
    BELLA_HIP_LOGT(tag, NumericColumns);
    BELLA_HIP_LOGT(tag, NumericPasses);
    BELLA_HIP_LOGT(tag, SymbolicPasses);
}

}  // namespace bella_hip_detail
