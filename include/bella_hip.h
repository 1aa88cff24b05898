/*
 * bella_hip.h -- C ABI of the MI355X-native BELLA overlap engine (libbella_hip.so).
 *
 * The reference (PASSIONLab/BELLA) has no FFI layer: its boundary for this path is two header-level
 * C++ call sites.  Each entry point below names the reference interface it replaces (paths relative
 * to the reference tree).  INTEGRATION.md shows the shim a BELLA maintainer adds so that
 * src/main.cpp:498-525 calls these instead of include/overlap.hpp's HashSpGEMM.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 or a negative BELLA_ERR_*;
 * no exceptions or exit() cross the ABI; inputs are borrowed for the duration of the call; results
 * live in the context (device memory) until overwritten or destroyed and are copied out by the
 * bella_hip_get_* calls into caller-owned buffers.  One host thread per context.
 * The library never falls back to a CPU implementation: without a gfx950 device
 * bella_hip_init returns BELLA_ERR_NO_DEVICE.
 */
#ifndef BELLA_HIP_H
#define BELLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BELLA_HIP_ABI_VERSION 6

enum {
    BELLA_OK = 0,
    BELLA_ERR_NO_DEVICE = -1,     /* no HIP device / not gfx950                                         */
    BELLA_ERR_HIP = -2,           /* a HIP runtime call failed (bella_hip_last_error has the text)       */
    BELLA_ERR_BAD_ARG = -3,       /* incl. a k-mer present in more than 16,383 reads                     */
    BELLA_ERR_BAD_BASE = -4,      /* read contains a character other than ACGT (align.hpp:40-55 asserts) */
    BELLA_ERR_READ_TOO_LONG = -5, /* read >= 65,536 bases: u16 positions (common.h:122-126)             */
    BELLA_ERR_TUPLE_ORDER = -6,   /* tuples not grouped by non-decreasing read id                       */
    BELLA_ERR_STATE = -7,         /* call order: reads -> matrix -> overlap -> align                    */
    BELLA_ERR_ROW_TOO_LARGE = -8, /* one output column has >= 2^31 products                             */
    BELLA_ERR_BINS = -9,          /* a pair ended with > 16 overlap bins: std::sort tie order path      */
    BELLA_ERR_NOMEM = -10
};

typedef struct bella_ctx bella_ctx;

/* BELLApars (include/common/common.h:46-74), the fields the hot path reads. */
typedef struct {
    uint16_t kmer_size;       /* -k, kmerSize      (<= 32)                       */
    uint16_t bin_size;        /* -b, binSize       (chain.hpp:114)               */
    uint16_t xdrop;           /* -x, xDrop         (align.hpp:152)               */
    uint16_t skip_alignment;  /* --skip-alignment  (overlap.hpp:542,577)         */
    double error_rate;        /* -e : ratiophi = slope(e) (align.hpp:72-80)      */
    double delta_chernoff;    /* --score-deviation (overlap.hpp:456)             */
} bella_params;

/* One nonzero of C = A*A^T after the semiring fold, i.e. what RunPairWiseAlignments
 * (overlap.hpp:531-585) reads from a spmatType_ (common.h:119-183): count, and choose()'s seed.
 * Order of the array = the reference's 1-thread output order: column (cid) ascending, hash-slot
 * order inside a column (overlap.hpp:343-361). */
typedef struct {
    uint32_t rid;     /* row of C: the larger read id; "read1"/H in chain.hpp            */
    uint32_t cid;     /* column of C: read i; "read2"/V                                   */
    uint16_t count;   /* spmatType_::count (u16 wrap kept)                                */
    uint16_t seedH;   /* choose().first  : seed k-mer position on read rid               */
    uint16_t seedV;   /* choose().second : seed k-mer position on read cid               */
    uint16_t flags;   /* bit0: seed k-mers identical (checkstrand true, chain.hpp:35-44)
                         bit1: revcomp(seedH)==seedV (strand "c", align.hpp:171)          */
} bella_pair;

/* Diagnostics of the final semiring value (tests compare them with the oracle). */
typedef struct {
    uint16_t nbins;    /* pos.size() at the end                                           */
    uint16_t support;  /* chain(): support of the winning bin (common.h:142-150)          */
    uint16_t binov;    /* overlap[] of the winning bin                                    */
    uint16_t pad;
} bella_pair_ext;

/* xavierResult (common.h:83-87) + what PostAlignDecision (overlap.hpp:413-497) derives from it. */
typedef struct {
    int32_t score;            /* best1 + best2 (simdutils.h:333-337)                      */
    int32_t begH, endH;       /* SeedX positions on (possibly reverse-complemented) read rid */
    int32_t begV, endV;       /* on read cid                                              */
    uint16_t ov;              /* overlap estimate `ov` (overlap.hpp:449)                   */
    uint8_t strand;           /* 0 = "n", 1 = "c"                                          */
    uint8_t passed;           /* (float)score >= (1-delta)*phi*ov (overlap.hpp:456-460)    */
    uint32_t steps;           /* anti-diagonal steps taken (both directions): GCUPS = 31*steps */
    uint32_t flagged;         /* 1 if an extension began with no positive lane: the reference reads an
                                 uninitialised `maxpos` there (xavier.h:165); we use 0 */
} bella_aln;

/* Explicit seed for the batched xavierAlign (the alignLogan-shaped entry, align.hpp:210-211). */
typedef struct {
    uint32_t rid, cid;        /* reads previously given to bella_hip_set_reads             */
    uint16_t seedH, seedV;
} bella_seed;

typedef struct {
    float assemble_ms;        /* tuples/B -> device CSR layout (all assembly kernels)      */
    float symbolic_ms;        /* per-row flops + tiering (estimateFLOP, overlap.hpp:157)   */
    float spgemm_ms;          /* row kernels: symbolic + expansion + slot order (overlap.hpp:205,281) */
    float fold_ms;            /* semiring fold kernels (chain.hpp:74-150)                    */
    float compact_ms;         /* pair compaction to the dense output                        */
    float xdrop_ms;           /* X-drop kernel                                              */
    float overlap_total_ms;   /* bella_hip_overlap, stream time start to end                */
    uint32_t spgemm_launches; /* row-kernel launches (one per non-empty LDS tier)            */
    float kcount_ms;          /* bella_hip_count_kmers: counting + dictionary + tuples      */
    uint32_t retry_columns;   /* last pass: columns an LDS tier handed to the global-workspace path (key table too small for
                                 the column's pairs, or a product list out of order -- see DESIGN 4.1, phase S).  Normally 0 or a
                                 handful; a large value is a performance cliff worth reporting                              */
    uint32_t overflow_pairs;  /* last pass: pairs that ended with > 16 bins (serial fold with libstdc++'s sort order)       */
    float layout_ms;          /* part of assemble_ms: CSR of B -> device layout B' / A' (sort + segmented passes)           */
    float rows_ms;            /* part of assemble_ms: tuples -> rows of B in MergeDuplicates slot order (CSC.cpp:301-420)    */
    uint32_t lane_order;      /* init-time self-test of the LDS-atomic lane order the LDS tiers rely on (phase S):
                                 1 = holds; 2 = does not hold on this device/driver: every column takes the repairing
                                 global-workspace path (correct, slower)                                                 */
    float expand_ms;          /* part of layout_ms: the product expansion done at assembly time (the row lists of
                                 BELLA_TUNE_ROW_LISTS; 0 in the default layout, where every pass expands B' x A' itself)   */
    uint32_t numeric_passes;  /* since bella_hip_init: calls of bella_hip_overlap that ran the numeric phase ...          */
    uint32_t symbolic_passes; /* ... and calls of bella_hip_count_pairs (symbolic phase only)                            */
    uint32_t wide_batches;    /* last pass, the path of the columns above the LDS tiers: low 16 bits = batches whose
                                 products were grouped by partner in LDS, high 16 bits = batches that took the sort-based path
                                 (debug bit 12, a failed lane-order self-test, no room for the batch's lists, or a column with
                                 more partners than the grouping table holds); both halves saturate at 65,535             */
    uint64_t numeric_columns; /* since bella_hip_init: output columns the numeric phase computed (a staged run that computes
                                 every column once ends at nreads)                                                        */
} bella_timings;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
int bella_hip_abi_version(void);
int bella_hip_device_count(void);
int bella_hip_init(int device, bella_ctx** out);
void bella_hip_destroy(bella_ctx* ctx);
const char* bella_hip_strerror(int code);
const char* bella_hip_last_error(const bella_ctx* ctx);

/* ---- reads: readVector_ (common.h:98-109) -------------------------------------------------------- */
/* `bases` = all reads concatenated, upper-case ASCII ACGT; offsets has nreads+1 entries. */
int bella_hip_set_reads(bella_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads);
/* FASTQ ingest: replaces ParallelFASTQ::fill_block / get_next_fq_record (kmercode/fq_reader.c:540-610) and the
 * name handling of get_fq_name (fq_reader.c:88-130) + src/main.cpp:352-360 for one plain (not compressed, as in the
 * reference's NO_GZIP build) 4-line FASTQ file: the file is mapped and indexed on all host cores (records are found by line
 * number, not by looking for '@'), the bases stream mapping -> pinned buffer -> device in 64 MB chunks (gather of chunk i+1 under
 * the transfer of chunk i) and are packed to 2 bit/base on the device.  Same effect as bella_hip_set_reads; the names (without
 * '@', cut at the comment as the reference does) stay in the context. */
int bella_hip_load_fastq(bella_ctx* ctx, const char* path, uint32_t* nreads, uint64_t* nbases);
/* the same for the reference's LIST of FASTQ files (-f: include/kmercount.hpp:82-105 GetFiles reads one path per line; src/main.cpp:339-423
 * numbers the reads through the files in list order): read ids continue from file to file, every file is mapped and indexed for itself. */
int bella_hip_load_fastq_list(bella_ctx* ctx, const char* const* paths, uint32_t nfiles, uint32_t* nreads, uint64_t* nbases);
/* what the last bella_hip_load_fastq / _list did (file_bytes, threads: over all files) */
typedef struct bella_ingest_stats {
    uint64_t file_bytes;
    uint64_t bases;
    uint32_t reads;
    uint32_t threads;     /* host threads of the index and of the gather */
    double index_ms;      /* map + both passes over the file */
    double upload_ms;     /* gather + host->device + pack, until the packed reads are on the device */
} bella_ingest_stats;
int bella_hip_get_ingest_stats(bella_ctx* ctx, bella_ingest_stats* out);
/* names back to back, NUL-terminated; offsets[nreads+1] into buf; *needed = bytes required (call with buf = NULL first) */
int bella_hip_get_read_names(bella_ctx* ctx, char* buf, uint64_t buflen, uint64_t* offsets, uint64_t* needed);
int bella_hip_get_read_lengths(bella_ctx* ctx, uint32_t* lens);

/* ---- k-mer counting, reliable dictionary, tuple generation ---------------------------- */
/* Replaces SplitCount (include/kmercount.hpp:467-677) and the tuple loop of src/main.cpp:393-416 on the reads given to
 * bella_hip_set_reads: every position j <= len-k contributes Kmer::rep() (kmercode/Kmer.cpp:314-317); a k-mer is reliable
 * when lower <= (occurrences mod 65536) <= upper (the reference counts in an unsigned short, kmercount.hpp:632-655;
 * lower >= 2 as in the reference's defaults: its table only holds k-mers seen twice).  K-mer ids are labels: the reference
 * numbers in libcuckoo's iteration order, this library in ascending order of the canonical word (first base most
 * significant, A<C<G<T, the order of Kmer::operator<).  The tuples (id, read, position) are generated in the reference's
 * order -- read by read, positions ascending -- and stay on the device for bella_hip_assemble_counted.
 * Out: *nkmers = dictionary size, *ntuples, *ndistinct = distinct canonical k-mers seen (the reference's HyperLogLog
 * estimates this number, kmercount.hpp:585-590; here it is exact).  Any of them may be NULL. */
int bella_hip_count_kmers(bella_ctx* ctx, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t* nkmers,
                          uint64_t* ntuples, uint64_t* ndistinct);
/* The same for the reference's syncmer mode (-s): SyncmerCount (include/kmercount.hpp:845-985) with isSyncmer
 * (include/syncmer.hpp:47-79, s = 5, Kmer::hash = MurmurHash3_x64_64 seed 313) + the tuple loop of src/main.cpp:393-416.
 * Counted: the strand-specific word of every syncmer position, saturating at 65535; the dictionary holds those words; tuples:
 * every position whose CANONICAL k-mer is a dictionary key (the reference's tuple loop has no syncmer branch).  k > 5. */
int bella_hip_count_syncmers(bella_ctx* ctx, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t* nkmers,
                             uint64_t* ntuples, uint64_t* ndistinct);
/* The reference's minimizer mode (-w window): MinimizerCount (include/kmercount.hpp:691-835) with getMinimizers
 * (include/minimizer.hpp:49-79: monotone deque on rep().hash(), robust winnowing, the first `window` k-mers of a read are
 * never sampled -- the reference's size_t range test) + the minimizer branch of the tuple loop (src/main.cpp:363-388).
 * Counted: rep() of the minimizer positions, saturating at 65535; tuples: the minimizer positions whose rep() is reliable. */
int bella_hip_count_minimizers(bella_ctx* ctx, uint16_t kmer_size, uint32_t window, uint32_t lower, uint32_t upper,
                               uint32_t* nkmers, uint64_t* ntuples, uint64_t* ndistinct);
/* codes[nkmers]: the dictionary's words (canonical for count_kmers, strand-specific for count_syncmers), ascending (id = index),
 * right-aligned in 2k bits; counts[nkmers].  Either may be NULL. */
int bella_hip_get_dictionary(bella_ctx* ctx, uint64_t* codes, uint16_t* counts);
/* the tuple list of the last bella_hip_count_kmers (what the reference's alltranstuples holds, main.cpp:339-423) */
int bella_hip_get_tuples(bella_ctx* ctx, uint32_t* t_kmer, uint32_t* t_read, uint16_t* t_pos);
/* what the host decided for the last count (host values only, no device work): values[0..7] = uses the sort-with-positions path
 * (0 / 1), position bits in the sort keys, low word bits the sort leaves out, passes, slots of the look-up table (0: none built),
 * selector (0 all, 1 syncmers, 2 minimizers), positions of the read set, k-mers per pass allowed; then per pass {first bin, end bin,
 * words, tiles of the run kernels}.  Writes at most `capacity` values; *nvalues = how many there are. */
int bella_hip_get_count_stats(bella_ctx* ctx, uint64_t* values, uint32_t capacity, uint32_t* nvalues);
/* which path the last assembly took (host values only, no device work): values[0..4] = the reads per table class of the row
 * assembly (tables of <= 1024, 2048, 4096, 8192 slots in LDS, larger ones in global memory; of the last panel where rows were
 * assembled in panels, stale after bella_hip_set_B*), then: B' entries in the inline form (0 / 1), one B' entry per product (0 / 1),
 * lists of A' in first-appearance order (0 / 1), the place pass went through its radix pass (0 / 1).  Writes at most `capacity`
 * values; *nvalues = how many there are. */
int bella_hip_get_assemble_stats(bella_ctx* ctx, uint64_t* values, uint32_t capacity, uint32_t* nvalues);
/* bella_hip_assemble_tuples on the device-resident tuples of bella_hip_count_kmers (no host copy) */
int bella_hip_assemble_counted(bella_ctx* ctx);
/* bella_hip_assemble_panel on the device-resident tuples of the reads [first_read, first_read + nreads_panel) (multi-GPU:
 * every rank counts, each assembles the rows of its own read block; then the all-gather of bella_hip_panel_device_ptrs) */
int bella_hip_assemble_counted_panel(bella_ctx* ctx, uint32_t first_read, uint32_t nreads_panel);

/* ---- operands ------------------------------------------------------------------------------------ */
/* From the (kmer, read, pos) tuple list: replaces the CSC tuple constructor + MergeDuplicates +
 * Transpose of src/main.cpp:476-489 (src/CSC.cpp:422-479,301-420; include/common/transpose.h:13).
 * Tuples must be grouped by non-decreasing read id, in generation order inside a read.
 * kmer_size = Kmer::set_k (main.cpp:183): needed here because the strand test of multiop
 * (chain.hpp:35-44) is precomputed as one orientation bit per nonzero. */
int bella_hip_assemble_tuples(bella_ctx* ctx, uint16_t kmer_size, uint32_t nkmers, uint64_t ntuples,
                              const uint32_t* t_kmer, const uint32_t* t_read, const uint16_t* t_pos);
/* From the reference's own B = transpmat CSC arrays (the HashSpGEMM boundary, overlap.hpp:650):
 * colptr[nreads+1], rowids = k-mer ids in MergeDuplicates slot order, values = positions.
 * A = spmat is derived on device (ascending read ids per k-mer = the reference's 1-thread Transpose).
 * Every call that installs operands (this one, the assemble_* calls, bella_hip_allgather_panels) also lays them out for the passes:
 * A' (whole) and B' (the columns of the context's partition, bella_hip_set_partition); every pass expands B' x A' itself.  With
 * BELLA_TUNE_ROW_LISTS (callers that run several passes over the same columns) also the row lists -- the two operand entries of every
 * product side by side in product order, 10 bytes per product -- when they fit.  Same results either way. */
int bella_hip_set_B(bella_ctx* ctx, uint16_t kmer_size, uint32_t nkmers, const uint32_t* colptr,
                    const uint32_t* rowids, const uint16_t* values);
/* Multi-GPU assembly: rank r builds only the rows of B of ITS reads (a row-block panel) from their tuples (global read ids,
 * same rules as above); the panels' device arrays are exchanged with one all-gather (RCCL over xGMI, done by the caller:
 * bella_amd/dist.py) and the full matrix comes back through bella_hip_set_B_device.  Rows = per-read entry counts (u32),
 * rowids = k-mer ids in MergeDuplicates slot order (u32), values = positions (u16). */
int bella_hip_assemble_panel(bella_ctx* ctx, uint16_t kmer_size, uint32_t nkmers, uint32_t first_read, uint32_t nreads_panel,
                             uint64_t ntuples, const uint32_t* t_kmer, const uint32_t* t_read, const uint16_t* t_pos);
/* The same panel from the reference's CSC arrays of B (colptr[nreads + 1], rowids, values: the WHOLE matrix on the host; only the
 * block's slice is uploaded).  A host program that holds B and drives several GPUs gives every context its block this way and lets
 * bella_hip_allgather_panels move the blocks device to device, instead of uploading the whole matrix once per GPU. */
int bella_hip_set_B_panel(bella_ctx* ctx, uint16_t kmer_size, uint32_t nkmers, uint32_t first_read, uint32_t nreads_panel,
                          const uint32_t* colptr, const uint32_t* rowids, const uint16_t* values);
int bella_hip_panel_device_ptrs(bella_ctx* ctx, uint32_t* first_read, uint32_t* nreads_panel, uint64_t* nnz,
                                const void** d_rowcnt, const void** d_rowids, const void** d_values);
/* As bella_hip_set_B, from DEVICE pointers (colptr[nreads+1], rowids[nnz], values[nnz]); copied, the caller keeps ownership. */
int bella_hip_set_B_device(bella_ctx* ctx, uint16_t kmer_size, uint32_t nkmers, const uint32_t* d_colptr, const uint32_t* d_rowids,
                           const uint16_t* d_values, uint64_t nnz);
/* Copies B back in the reference's layout (tests: compare with CSC.cpp's result). Any pointer may be NULL. */
int bella_hip_get_B(bella_ctx* ctx, uint64_t* nnz, uint32_t* colptr, uint32_t* rowids, uint16_t* values);

/* Multi-GPU (one context per GPU/process): this context computes output columns i with
 * i % stride == first.  Default (0,1) = all columns.  The device layout follows the partition: operands installed AFTER this call
 * get B' entries (and row lists) for the OWNED columns only -- per-column layout work and memory are 1/stride of the whole; A' (the
 * k-mer -> reads lists every column gathers from) and the exchanged reference-layout B stay whole.  Changing the partition of a
 * context whose layout was built for another one rebuilds the layout from the resident B at the next pass. */
int bella_hip_set_partition(bella_ctx* ctx, uint32_t first, uint32_t stride);
/* Stages (the reference forms the output in stages of consecutive columns when it does not fit the -m budget:
 * estimateMemory, overlap.hpp:365-404, stage loop :682-789): the next passes compute only the output columns
 * [first, first + count) (intersected with the partition above); default = all.  Running the ranges in ascending order and
 * appending their outputs reproduces the single-stage output, and every pass only holds its own columns' records. */
int bella_hip_set_column_range(bella_ctx* ctx, uint32_t first, uint32_t count);

/* ---- HashSpGEMM (overlap.hpp:650-789): estimateFLOP + estimateNNZ_Hash + LocalSpGEMM ---------------- */
int bella_hip_overlap(bella_ctx* ctx, const bella_params* p, uint64_t* npairs, uint64_t* flops);
/* The symbolic phase alone: estimateFLOP (overlap.hpp:157-202) + estimateNNZ_Hash (:205-276) + prefixsum (:110-146) over the
 * columns of the current partition and column range -- distinct row ids per output column, no product lists, no fold, no records,
 * and no product-sized buffers (a bitmap over the reads per workgroup).  colptrC[nreads + 1] (host, nullable): exclusive prefix sums
 * of the per-column pair counts (columns outside the partition / range count 0); *npairs = nnz(C), *flops = products.  This is what
 * the reference knows BEFORE its numeric phase and sizes its stages from (overlap.hpp:674-710); the shim's stage planner uses it
 * so that no column is computed twice.  With colptrC == NULL and npairs == NULL only estimateFLOP runs (*flops; sums over the
 * count stream, no gather): an upper bound of nnz(C) that lets a planner skip the symbolic phase when one stage is certain. */
int bella_hip_count_pairs(bella_ctx* ctx, const bella_params* p, uint64_t* colptrC, uint64_t* npairs, uint64_t* flops);
/* pairs[npairs]; ext (nullable) [npairs]; colptrC (nullable) [nreads+1] */
int bella_hip_get_pairs(bella_ctx* ctx, bella_pair* pairs, bella_pair_ext* ext, uint64_t* colptrC);

/* ---- RunPairWiseAlignments (overlap.hpp:499-645): xavierAlign + PostAlignDecision on every pair ----- */
int bella_hip_align_pairs(bella_ctx* ctx, const bella_params* p, uint64_t* npassed);
int bella_hip_get_alignments(bella_ctx* ctx, bella_aln* out);
/* xavierAlign (align.hpp:152) on explicit seeds; out[n] index-aligned with seeds[n]. */
int bella_hip_xdrop_batch(bella_ctx* ctx, const bella_seed* seeds, uint64_t n, const bella_params* p,
                          bella_aln* out);

/* ---- output writer (overlap.hpp:531-590 formatting, :603-642 per-thread buffers + offset writes) -------------------------
 * Formats pairs[npairs] (in the reference's order, as bella_hip_get_pairs delivers them) -- 6-column lines when
 * p->skip_alignment (overlap.hpp:577-588), else the passed alignments as BELLA's 12 columns (:472-473) or PAF (paf != 0,
 * :476-489) -- and APPENDS the text to `path` (the reference opens its file in append mode, :613).  names[nreads]: NUL-terminated
 * read names (readType_::nametag); lens[nreads]: read lengths; alns may be NULL when p->skip_alignment.  nthreads host threads
 * (0 = min(hardware threads, 16): more threads into ONE file are slower, the writes serialise on the inode) first measure contiguous
 * shares (exact bytes, no formatting), then format pieces of about 1 MB into private buffers and pwrite() each at its offset behind
 * the file's size at entry (fstat, not O_APPEND: ONE writer per file at a time is assumed; mapping the file was measured and
 * rejected, page faults).  Plain host code: no context, usable from any thread.  stats (nullable): what RunPairWiseAlignments
 * returns (:644) + timings. */
typedef struct {
    uint64_t lines;            /* outputted                                                       */
    uint64_t bytes;
    uint64_t aligned_pairs;    /* numAlignmentsThread (overlap.hpp:544)                           */
    uint64_t aligned_bases;    /* sum of endV - begV (:569)                                       */
    uint64_t total_read_len;   /* sum of both read lengths (:545)                                 */
    uint64_t bases_passed;     /* numBasesAlignedTrue (:491)                                      */
    uint64_t bases_failed;     /* numBasesAlignedFalse (:495)                                     */
    double seconds;            /* whole call                                                       */
    double format_seconds;     /* of which: validation + measuring pass (before the file is touched) */
    uint32_t threads;
    uint32_t pad;
} bella_write_stats;
int bella_hip_write_output(const char* path, const bella_params* p, int paf, uint32_t nreads, const char* const* names, const uint32_t* lens,
                           const bella_pair* pairs, const bella_aln* alns, uint64_t npairs, int nthreads, bella_write_stats* stats);

/* The exact (growing band) gapped X-drop of the reference's CUDA build instead of Xavier's 32-cell adaptive band: the scores and
 * seed positions of loganGPU/functions.cuh:223-408,505-547,680-682 (= SeqAn's extendSeed(GappedXDrop), include/align.hpp:93-139)
 * and the pass test of PostAlignDecisionGPU (include/overlap.hpp:797-871).  Same inputs and outputs as the two calls above;
 * bella_aln::steps = anti-diagonals computed, flagged = 0.  Extension scores live in int16 rings as in the CUDA kernel (`short`
 * anti-diagonals, loganGPU/functions.cuh:236-240): a one-direction score above 32,767 wraps there and here. */
int bella_hip_align_pairs_exact(bella_ctx* ctx, const bella_params* p, uint64_t* npassed);
int bella_hip_xdrop_batch_exact(bella_ctx* ctx, const bella_seed* seeds, uint64_t n, const bella_params* p, bella_aln* out);

/* ---- traced alignments: base-level alignment of a pair, as run-length ops (no counterpart in the reference) ----
 * Scoring is the X-drop's (match +1, mismatch -1, gap -1, linear).  For a pair with alignment a, V = read cid, H = read rid reverse-
 * complemented when a.strand == 1, the seed at (seedH', seedV) where xavierAlign places it, the traced alignment is: an extension from
 * the seed's start leftwards inside [a.begH, seedH') x [a.begV, seedV), the seed's k columns, an extension from the seed's end inside
 * [seedH' + k, a.endH) x [seedV + k, a.endV).  An extension is anchored at the seed and FREE at its far end: it ends at the cell with
 * the best score (ties: smallest i + j, then smallest i; i counts bases of V, j of H, from the seed).  So a trace has its own end
 * points, inside the X-drop's.  The DP runs in a band of `band0` diagonals (a power of two >= 256; 0 = BELLA_TRACE_DEFAULT_BAND)
 * centred on the seed's diagonal; a side whose path touches the band's first or last diagonal is redone with the band doubled until it
 * does not, or the band holds the side's whole rectangle (then the score is the exact optimum of the definition).
 * ops: one uint32 per run, len << 4 | op, op 0 '=' match, 1 'X' mismatch, 2 'I' (a base of V only), 3 'D' (a base of H only);
 * adjacent runs differ; in V order (left part, seed, right part). */
#define BELLA_TRACE_DEFAULT_BAND 256
typedef struct {
    uint64_t op_off;          /* first run of this pair in the ops array                                    */
    uint32_t nops;            /* runs; 0 = the pair was not traced                                          */
    uint32_t band;            /* band finally used (the larger of the two sides)                            */
    int32_t score;            /* left + seed + right under the scoring above                                */
    int32_t tbegH, tendH;     /* same coordinate convention as bella_aln                                    */
    int32_t tbegV, tendV;
    uint32_t n_eq, n_x, n_ins, n_del;   /* bases, not runs                                                 */
    uint32_t widened;         /* band doublings this pair took (both sides)                                 */
} bella_trace;
/* What the last bella_hip_trace_pairs / _batch did.  A sized struct (it will grow): bella_hip_get_trace_stats writes at most
 * struct_size bytes. */
typedef struct {
    double dp_ms;                 /* DP kernels (device time, all batches and widening rounds)               */
    double walk_ms;               /* backtrace kernels: counting walk + writing walk                         */
    double total_ms;              /* the whole call on the host clock, copies of the ops to the host included */
    uint64_t pairs;               /* pairs traced                                                            */
    uint64_t extensions;          /* extension DPs run: 2 per pair and 2 more every time a pair is repeated    */
    uint64_t widened_extensions;  /* sides whose band was doubled (a side can count more than once)           */
    uint64_t repeated_pairs;      /* times a pair went again because a side touched its band: the pair is repeated as a whole,
                                     also the side that did not touch (same band, same result)                */
    uint64_t dp_cells;            /* band cells computed                                                     */
    uint64_t dir_bytes;           /* direction bytes written (dp_cells / 4), summed over the batches          */
    uint64_t dir_bytes_peak;      /* the largest batch's direction buffer                                    */
    uint64_t ops;                 /* runs written                                                            */
    uint32_t batches;
    uint32_t band0;               /* the band the first round used                                           */
    double vote_ms;               /* bella_hip_trace_pairs_pileup: the vote kernel (device time, all batches) */
    uint64_t votes;               /* ... counter increments it issued                                        */
    uint64_t ops_host_bytes;      /* bytes of runs the call staged on the host (0 with keep_ops == 0)         */
} bella_trace_stats;
/* Traces the pairs of the last bella_hip_align_pairs / _exact (passed_only != 0: those with bella_aln::passed).  *ntraced pairs,
 * *nops runs in all.  BELLA_ERR_STATE without alignments.  Pairs run in batches sized from the free device memory (direction bytes:
 * rows x band / 4 per extension); the ops are staged on the HOST batch by batch and stay there until the next call: 4 bytes per run,
 * about 2,400 runs = 9.5 KB per pair of 10 kb reads at 15 % error, and bella_hip_get_traces copies them once more into the caller's
 * array.  A caller with more passed pairs than its host memory holds runs traces stage by stage (bella_hip_set_column_range). */
int bella_hip_trace_pairs(bella_ctx* ctx, const bella_params* p, uint32_t band0, int passed_only, uint64_t* ntraced, uint64_t* nops);
/* out[npairs] index-aligned with bella_hip_get_pairs (untraced pairs: nops = 0); ops[*nops of trace_pairs].  Either may be NULL. */
int bella_hip_get_traces(bella_ctx* ctx, bella_trace* out, uint32_t* ops);
/* The same on explicit seeds and alignments (the twin of bella_hip_xdrop_batch: alns[i] is what it returned for seeds[i], or any
 * rectangle the caller wants traced; end points are clamped to the reads).  Seed columns that do not match become 'X'.
 * out[n]; *nops = runs in all.  The runs stay with the context until the next call: with ops == NULL the call only reports *nops and
 * bella_hip_get_batch_ops copies them out (nobody can know their number beforehand; the trace is not run twice); with ops != NULL
 * they are copied into ops[ops_cap], BELLA_ERR_NOMEM when they do not fit (they can still be fetched). */
int bella_hip_trace_batch(bella_ctx* ctx, const bella_seed* seeds, const bella_aln* alns, uint64_t n, const bella_params* p, uint32_t band0,
                          bella_trace* out, uint32_t* ops, uint64_t ops_cap, uint64_t* nops);
int bella_hip_get_batch_ops(bella_ctx* ctx, uint32_t* ops, uint64_t ops_cap);
int bella_hip_get_trace_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* bella_hip_write_output for true PAF: one line per passed pair THAT HAS A TRACE (nops > 0), columns 1-9 as the PAF of
 * bella_hip_write_output but with the trace's end points, column 10 = n_eq, 11 = n_eq + n_x + n_ins + n_del, 12 = 255, then
 * AS:i:<X-drop score> ov:i:<ov> NM:i:<n_x + n_ins + n_del> cg:Z:<runs as = X I D>.  Strand '-': H coordinates on the original
 * strand and the runs in reverse order (the CIGAR reads along the target's forward strand).  traces[npairs], ops[nops_total] = the
 * array their op_off point into: a record whose runs lie outside it is BELLA_ERR_BAD_ARG.  npairs == 0 needs no arrays (an empty
 * stage appends nothing, as with bella_hip_write_output). */
int bella_hip_write_output_traced(const char* path, const bella_params* p, uint32_t nreads, const char* const* names, const uint32_t* lens,
                                  const bella_pair* pairs, const bella_aln* alns, const bella_trace* traces, const uint32_t* ops, uint64_t nops_total,
                                  uint64_t npairs, int nthreads, bella_write_stats* stats);

/* ---- read correction: pileup of the traced alignments and consensus (no counterpart in the reference) --------
 * The table: for every base position of every read nine uint32 counters, BELLA_PILEUP_COUNTERS * 4 = 36 bytes per base, in read order:
 * [0..3] votes for A, C, G, T at the position, [4] votes that the base is not there, [5..8] votes for ONE base (A, C, G, T) inserted in
 * the junction just before the position.  A traced pair votes on both of its reads (V = read cid, H = read rid; on strand 1 every vote on H
 * lands at the mirrored position with the complemented base); a run of inserted bases casts one vote, with the base that comes first in
 * the voted read's own direction; the junction behind a read's last base has no counters.  Counters are plain sums (a counter above
 * 2^32 - 1 is out of scope), so the table does not depend on the order of the pairs, batches, stages or contexts. */
#define BELLA_PILEUP_COUNTERS 9
/* Allocates (first use) and zeroes the table for the loaded reads: 36 bytes x total bases of device memory, BELLA_ERR_NOMEM when it does not
 * fit.  Loading other reads drops the table. */
int bella_hip_pileup_reset(bella_ctx* ctx);
/* What bella_hip_trace_pairs(passed_only = 1) does, and every traced pair's votes added to the table, batch by batch, from the batch's runs
 * while they are in device memory.  keep_ops == 0: the runs are not staged on the host (host memory of the call does not grow with the
 * pairs); bella_hip_get_traces then hands out the records only (ops must be NULL) -- op_off / nops are what they would be with the runs
 * kept.  keep_ops != 0: the context is left exactly as bella_hip_trace_pairs leaves it.  The table accumulates over calls until the next
 * bella_hip_pileup_reset; a pair repeated with a wider band votes once, with its final trace.  BELLA_ERR_STATE without a table. */
int bella_hip_trace_pairs_pileup(bella_ctx* ctx, const bella_params* p, uint32_t band0, int keep_ops, uint64_t* ntraced, uint64_t* nops);
/* ---- gap normalisation of the votes --------------------------------------------------------------------------
 * BELLA_TRACE_NORMALIZE (bella_hip_trace_pairs_flags; needs BELLA_TRACE_PILEUP) and the same flag of bella_hip_pileup_vote make every
 * gap run vote at a canonical position: moved towards the START of the read being voted on, in that read's own forward direction.
 * For a gap run k of length L that starts at (i_k, j_k), S = V, x = i_k for 'I' and S = H', x = j_k for 'D':
 *   sL_k = 0 unless run k - 1 is an '=' run (length d); else the largest s in [0, d] with S[x-1-t] == S[x+L-1-t] for all t < s;
 *   sR_k = 0 unless run k + 1 is an '=' run (length d'); else the largest s in [0, d'] with S[x+t] == S[x+L+t] for all t < s.
 * Every gap run shifts independently and only inside its ORIGINAL neighbouring '=' run.  The votes on V, and on H when strand == 0,
 * are those of the alignment with every gap moved left by sL (the '=' columns it jumped over follow it, still matches); the votes on H
 * when strand == 1 are those of the alignment with every gap moved right by sR (right in V order is left in H's own direction).  A gap
 * run still casts ONE ins vote, also where it now abuts another gap run; the junction behind a read's last base still has no counters.
 * Only the votes change: the records and runs a call hands out are what they are without the flag. */
#define BELLA_TRACE_NORMALIZE 8u
/* What the last voting call (bella_hip_trace_pairs_pileup, bella_hip_trace_pairs_flags with BELLA_TRACE_PILEUP, bella_hip_pileup_vote)
 * did.  A sized struct: bella_hip_get_vote_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t pairs;               /* pairs that voted                                                          */
    uint64_t runs;                /* their runs                                                                */
    uint64_t gap_runs;            /* 'I' and 'D' runs among them (0 without BELLA_TRACE_NORMALIZE: nobody counts them) */
    uint64_t shifted_runs;        /* (gap run, voted read) combinations with a non-zero shift: sL for V; sL (strand 0) or sR (strand 1) for H */
    uint64_t shifted_columns;     /* the sum of those shifts                                                   */
    uint64_t votes;               /* counter increments issued                                                 */
    double vote_ms;               /* the vote kernel (device time, all batches)                                */
    uint32_t normalized;          /* 1: the call ran with BELLA_TRACE_NORMALIZE                                */
    uint32_t pad;
} bella_vote_stats;
int bella_hip_get_vote_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* One traced pair of a caller: V = read cid, H = read rid (H' = its reverse complement when strand == 1), nops runs (len << 4 | op, as
 * bella_trace's) from ops[op_off] in V order, the first at (tbegV, tbegH) of V and H'. */
typedef struct {
    uint32_t rid, cid;
    int32_t tbegV, tbegH;
    uint64_t op_off;
    uint32_t nops;
    uint8_t strand;
    uint8_t pad[3];
} bella_vote_pair;
/* Votes caller-supplied traced pairs into the table: the pileup counterpart of bella_hip_trace_batch, for alignments made elsewhere.
 * flags: 0 (the votes of bella_hip_trace_pairs_pileup) or BELLA_TRACE_NORMALIZE.  The host checks everything BEFORE anything is
 * launched -- read ids in range, strand 0 or 1, every run's op in 0..3 and its length at least 1, every pair's runs inside both
 * reads from (tbegV, tbegH) >= 0, op_off + nops inside ops[nops_total] -- and returns BELLA_ERR_BAD_ARG with nothing voted otherwise.
 * '=' columns are TRUSTED to be matches: they vote the other read's base like any aligned column, and the normalisation relies on
 * them when it moves a gap across them.  BELLA_ERR_STATE without a table. */
int bella_hip_pileup_vote(bella_ctx* ctx, const bella_vote_pair* pairs, uint64_t npairs, const uint32_t* ops, uint64_t nops_total, uint32_t flags);
/* Copies the counters of the reads [first_read, first_read + nreads) out (out: 9 uint32 per base of those reads), or adds a caller's
 * counters into the table (how several contexts merge: each piles up its own columns, one of them adds the others' tables). */
int bella_hip_get_pileup(bella_ctx* ctx, uint32_t first_read, uint32_t nreads, uint32_t* out);
int bella_hip_add_pileup(bella_ctx* ctx, uint32_t first_read, uint32_t nreads, const uint32_t* in);
/* device bytes of the table (0 without one) */
int bella_hip_get_pileup_bytes(bella_ctx* ctx, uint64_t* bytes);
/* Consensus of every read from the table.  With depth(p) = sum of base[p] + del[p], own base b[p], for p = 0 .. len - 1:
 * (1) junction before p (p >= 1): c = min(depth(p - 1), depth(p)), I = sum of ins[p]; if c >= min_depth and 2 I > c + 1 emit the base with
 * the most ins votes (ties: A < C < G < T); (2) position p: depth(p) < min_depth emits b[p]; else 2 del[p] > depth(p) + 1 emits nothing;
 * else emits the base of largest base[p][x] + (x == b[p]) (ties: b[p] if it is one of them, else A < C < G < T).  A read nobody voted on
 * comes out unchanged.  The result stays with the context for bella_hip_get_consensus. */
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_consensus_params) of the caller's header (the struct may grow) */
    uint32_t min_depth;           /* >= 1; the documented default is 3                                          */
} bella_consensus_params;
typedef struct {
    uint32_t len_before, len_after;
    uint32_t substituted;         /* positions whose emitted base differs from the read's                       */
    uint32_t deleted;             /* positions that emitted nothing                                             */
    uint32_t inserted;            /* junctions that emitted a base                                              */
    uint32_t covered;             /* positions with depth >= min_depth                                          */
    uint64_t depth_sum;           /* sum of depth over the read's positions                                     */
} bella_consensus_read;
int bella_hip_consensus(bella_ctx* ctx, const bella_consensus_params* params, uint64_t* total_bases);
/* offsets[nreads + 1] into bases[total_bases] (upper-case ASCII), stats[nreads].  Any pointer may be NULL. */
int bella_hip_get_consensus(bella_ctx* ctx, uint64_t* offsets, uint8_t* bases, bella_consensus_read* stats);
/* ">name\n" + one sequence line per read, in input order.  append == 0 truncates the file.  Plain host code, no context. */
int bella_hip_write_fasta(const char* path, uint32_t nreads, const char* const* names, const uint64_t* offsets, const uint8_t* bases, int append);

/* ---- string graph: overlap classes, containment, transitive reduction, GFA (no counterpart in the reference) ----
 * Vertices: two per read, 2 r + o, o = 0 the read as given, o = 1 its reverse complement; twin(v -> w) = (w ^ 1 -> v ^ 1).  An overlap
 * record is a pair's end points on V = read cid and on H' = read rid oriented by the strand (the convention of bella_aln / bella_trace).
 * Class of a record with b1, e1 on V (length l1) and b2, e2 on H' (length l2), tested in this order:
 *   1. e1 - b1 < min_overlap or e2 - b2 < min_overlap: SHORT, dropped;
 *   2. overhang = min(b1, b2) + min(l1 - e1, l2 - e2), maplen = max(e1 - b1, e2 - b2); overhang > max_overhang or
 *      1000 overhang > overhang_permille maplen: INTERNAL, dropped;
 *   3. b1 <= b2 and l1 - e1 <= l2 - e2: V CONTAINED;          4. b1 >= b2 and l1 - e1 >= l2 - e2: H CONTAINED;
 *   5. b1 > b2: edge (V,0) -> (H,strand), len = b1 - b2, and its twin (H,strand^1) -> (V,1), len = (l2 - e2) - (l1 - e1);
 *   6. else:    edge (H,strand) -> (V,0), len = b2 - b1, and its twin (V,1) -> (H,strand^1), len = (l1 - e1) - (l2 - e2).
 * A read that any record puts in class 3 or 4 on its side is contained; every edge with a contained end is removed.  The out-edges of a
 * vertex are ordered by (len, dst) ascending; two edges with the same (src, dst) -- two records of one read pair -- fail the build.
 * Reduction (Myers 2005 as miniasm states it), for every vertex v with out-edges: (1) its out-neighbours are INPLAY, L = the largest len
 * of v's list + fuzz; (2) for v -> w in list order, skipped unless w is INPLAY at that moment: for w -> x in list order, stopping at the
 * first with len(v -> w) + len(w -> x) > L: an INPLAY x becomes ELIMINATED; (3) for every v -> w, whatever its mark, and w -> x at index
 * j of w's list with j == 0 or len(w -> x) < fuzz: an INPLAY x becomes ELIMINATED; (4) the edges v -> x with x ELIMINATED are reduced.
 * An edge leaves the graph when it OR ITS TWIN is reduced.  Tip clipping, unitig compaction (the next section) and bubble popping (the
 * one after it) work on this graph. */
typedef struct {
    uint32_t cid, rid;            /* V, H                                                                       */
    int32_t begV, endV;           /* on V                                                                       */
    int32_t begH, endH;           /* on H' (H reverse-complemented when strand == 1)                             */
    int32_t score;                /* carried, not read                                                          */
    uint8_t strand;               /* 0 or 1                                                                     */
    uint8_t pad[3];
} bella_overlap;
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_graph_params) of the caller's header (the struct may grow)     */
    uint32_t min_overlap;         /* documented default 1000                                                    */
    uint32_t max_overhang;        /* 1000                                                                       */
    uint32_t overhang_permille;   /* 800                                                                        */
    uint32_t fuzz;                /* 1000                                                                       */
} bella_graph_params;
#define BELLA_GRAPH_EDGE_TWIN 1u  /* bella_graph_edge::flags bit0: the edge is the second ("its twin") of its record's class 5 / 6 line */
typedef struct {
    uint32_t src, dst;            /* vertices                                                                   */
    uint32_t len;                 /* bases of src's read before dst's read begins                               */
    uint32_t ovl;                 /* length of src's read - len                                                 */
    uint32_t rec;                 /* index of the edge's record among the accumulated records                   */
    uint32_t flags;
} bella_graph_edge;
/* What the last bella_hip_graph_build did.  A sized struct: bella_hip_graph_get_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t records, n_short, n_internal;
    uint64_t contained_reads;
    uint64_t edges_all;           /* directed edges of classes 5 and 6 (two per record)                          */
    uint64_t edges_kept;          /* ... without a contained end: what the reduction runs on                     */
    uint64_t edges_reduced;       /* edges step (4) marked                                                      */
    uint64_t edges_final;         /* edges_kept minus the edges that were reduced or whose twin was              */
    uint32_t max_degree;          /* largest out-degree among the kept edges                                    */
    uint32_t overcap_vertices;    /* vertices whose neighbour set did not fit the wavefront's LDS table (global-memory path) */
    double classify_ms, sort_ms, reduce_ms;   /* device time: classes + flags; filter, degrees, scan, sorts, lists; reduction, twin pass, compaction */
    double host_ms;               /* the whole call on the host clock                                           */
} bella_graph_stats;
/* Drops the accumulated records and the last graph.  Loading other reads does the same. */
int bella_hip_graph_reset(bella_ctx* ctx);
/* Appends explicit records.  BELLA_ERR_BAD_ARG (nothing is appended) when a record has cid == rid, an id >= nreads, beg >= end, beg < 0,
 * end > the read's length or strand > 1.  Records accumulate over calls (stages, column ranges) until the next reset. */
int bella_hip_graph_add_overlaps(bella_ctx* ctx, const bella_overlap* recs, uint64_t n);
/* Appends one record per passed pair with a trace (nops > 0) of the context's last alignment + trace, in pair order, from the trace's end
 * points (tbegV .. tendH), score = the X-drop's.  *added (nullable) = how many.  BELLA_ERR_STATE without traces. */
int bella_hip_graph_add_traced(bella_ctx* ctx, uint64_t* added);
/* The accumulated records: *n = their number; out (nullable) receives them.  How several contexts merge: one of them adds the others'. */
int bella_hip_graph_get_overlaps(bella_ctx* ctx, bella_overlap* out, uint64_t* n);
/* Classifies, builds the lists, reduces (all on the device).  params == NULL: the documented defaults.  An empty record set gives an empty graph.
 * While the clips of bella_hip_graph_trim exist (the coverage trimming section below) every record is cut to them first. */
int bella_hip_graph_build(bella_ctx* ctx, const bella_graph_params* params);
/* *nvertices = 2 nreads, *nedges = final edges (size query: every other pointer NULL); offsets[2 nreads + 1] (CSR over the vertices),
 * edges[nedges] in list order, contained[nreads] (0 / 1; 2 for an uncovered read, only while the clips of bella_hip_graph_trim exist: such a
 * read is dead downstream like a contained one).  Any pointer may be NULL.  BELLA_ERR_STATE without a built graph. */
int bella_hip_graph_get(bella_ctx* ctx, uint32_t* nvertices, uint64_t* nedges, uint64_t* offsets, bella_graph_edge* edges, uint8_t* contained);
int bella_hip_graph_get_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* What bella_hip_trace_pairs does, steered by flags: bit0 = passed pairs only; bit1 = the runs are DROPPED: not staged on the host, and
 * when nothing else reads them (no bit2) not written at all -- the records (end points, counts, nops, op_off as they would be) are all a
 * caller such as bella_hip_graph_add_traced needs; bella_hip_get_traces then takes ops == NULL only; bit2 = the runs vote into the pileup
 * table (needs bit0 and a table); bit3 = BELLA_TRACE_NORMALIZE (the read-correction section above; needs bit2, BELLA_ERR_BAD_ARG without
 * it): those votes are cast with every gap run at its canonical position.  flags = 1 is bella_hip_trace_pairs(passed_only = 1), 5 / 7
 * are bella_hip_trace_pairs_pileup with keep_ops 1 / 0. */
#define BELLA_TRACE_PASSED_ONLY 1u
#define BELLA_TRACE_DROP_OPS 2u
#define BELLA_TRACE_PILEUP 4u
int bella_hip_trace_pairs_flags(bella_ctx* ctx, const bella_params* p, uint32_t band0, uint32_t flags, uint64_t* ntraced, uint64_t* nops);

/* ---- clipped ends: a traced alignment cut to where the similarity ends (no counterpart in the reference) --------
 * The extension of a trace is free at its far end and scores +1 / -1 / -1, under which random DNA drifts upwards: a trace runs through
 * junk ends, chimeric junctions and the far side of a repeat copy to the end of the read.  The clip keeps the maximum-scoring segment
 * of the path under an identity threshold.  For a pair with runs r = 0 .. n - 1 and identity = t permille (1 <= t <= 999):
 *   w_r = len_r (1000 - t) for an '=' run, w_r = -len_r t for 'X', 'I', 'D';  P_0 = 0, P_{r+1} = P_r + w_r (64 bits).
 * The clip is the (a, b), 0 <= a < b <= n, that maximises P_b - P_a; ties: the smallest b, for that b the largest a.  A maximum that
 * is not positive EMPTIES the pair.  A clipped alignment begins and ends with an '=' run.  The segment need not contain the seed: of
 * a chimera the better half stays.  The runs themselves are never rewritten: a clip moves op_off and nops. */
#define BELLA_CLIP_DEFAULT_IDENTITY 650
typedef struct {
    uint32_t struct_size;     /* sizeof(bella_clip_params)                                                   */
    uint32_t identity;        /* t, permille; 0 = BELLA_CLIP_DEFAULT_IDENTITY; otherwise 1 .. 999             */
} bella_clip_params;
/* One pair's clip.  An emptied pair (also a pair without runs): nruns = 0, first_run = 0, begV = endV = the pair's tbegV, begH = endH =
 * its tbegH, counts, score and clip_score 0. */
typedef struct {
    uint32_t first_run;       /* a: runs of the pair in front of the segment                                 */
    uint32_t nruns;           /* b - a                                                                       */
    int32_t begV, endV;       /* the segment on V and on H', in the pair's coordinates                       */
    int32_t begH, endH;
    uint32_t n_eq, n_x, n_ins, n_del;   /* bases of the segment                                              */
    int32_t score;            /* n_eq - n_x - n_ins - n_del                                                  */
    uint32_t pad;
    int64_t clip_score;       /* P_b - P_a                                                                   */
} bella_clip;
/* What the last bella_hip_trace_pairs_clip / bella_hip_clip_ops did (pairs without runs are not counted).  A sized struct:
 * bella_hip_get_clip_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t pairs;               /* pairs with runs                                                          */
    uint64_t clipped;             /* ... whose segment is shorter than the path (and not empty)               */
    uint64_t emptied;             /* ... that have no positive segment                                        */
    uint64_t runs_before, runs_after;
    uint64_t columns_before, columns_after;
    uint64_t bases_v_removed;     /* bases of V / of H' the alignments no longer cover (emptied pairs: all)   */
    uint64_t bases_h_removed;
    uint32_t identity;            /* the t the call used                                                      */
    uint32_t pad;
    double clip_ms;               /* the clip kernel (device time, all batches)                               */
} bella_clip_stats;
/* bella_hip_trace_pairs_flags with every traced alignment clipped on the device, batch by batch, while its runs are in device memory.
 * flags: the four of bella_hip_trace_pairs_flags, with their rules.  clip == NULL: the default identity; an identity outside 1 .. 999
 * (0: the default) or a struct_size too small is BELLA_ERR_BAD_ARG.  Everything downstream sees the clipped record: op_off += a,
 * nops = b - a, the end points, the counts and score = n_eq - n_x - n_ins - n_del recounted over the segment; band and widened stay.
 * An emptied pair keeps op_off, band and widened and has nops = 0 (not traced), tend = tbeg, counts and score 0; it casts no vote and
 * is not counted in *ntraced.  The ops array and *nops are those of the call without the clip (runs outside a segment stay in it,
 * unreferenced).  With BELLA_TRACE_DROP_OPS the runs are still written on the device (the clip reads them) but not staged. */
int bella_hip_trace_pairs_clip(bella_ctx* ctx, const bella_params* p, uint32_t band0, uint32_t flags, const bella_clip_params* clip,
                               uint64_t* ntraced, uint64_t* nops);
/* The same kernel on a caller's runs: of every pair only op_off, nops, tbegV and tbegH are read; no reads need to be loaded.  out[npairs].
 * The host checks everything BEFORE anything is launched -- every run's op in 0..3 and its length at least 1, op_off + nops inside
 * ops[nops_total], tbegV, tbegH >= 0 and a pair's last base on either read below 2^31 -- and returns BELLA_ERR_BAD_ARG with `out`
 * untouched otherwise. */
int bella_hip_clip_ops(bella_ctx* ctx, const bella_vote_pair* pairs, uint64_t npairs, const uint32_t* ops, uint64_t nops_total,
                       const bella_clip_params* clip, bella_clip* out);
int bella_hip_get_clip_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* The loaded reads as upper-case ASCII: offsets[nreads + 1] into bases[total bases].  Either may be NULL. */
int bella_hip_get_read_bases(bella_ctx* ctx, uint64_t* offsets, uint8_t* bases);
/* GFA 1: "H\tVN:Z:1.0"; one "S\tname\tsequence\tLN:i:len" per non-contained read in input order (sequence = base_offsets / bases, or "*"
 * when bases == NULL); one "L\tsrc\t+/-\tdst\t+/-\t<ovl>M\tel:i:<len>\trc:i:<rec>" per edge in CSR order.  Truncates the file.  Plain host
 * code, no context. */
int bella_hip_write_gfa(const char* path, uint32_t nreads, const char* const* names, const uint32_t* lens, const uint64_t* base_offsets,
                        const uint8_t* bases, const uint64_t* offsets, const bella_graph_edge* edges, const uint8_t* contained);

/* ---- unitigs: tip clipping, compaction, sequences (no counterpart in the reference) -----------------------------
 * On the graph of the last bella_hip_graph_build, in its notation; in-degree(v) = out-degree(v ^ 1) because the graph is twin-symmetric.
 * Tip clipping, one round, on a snapshot of the current graph: every vertex v with in-degree 0 and out-degree >= 1 starts a walk,
 * chain = [v], cur = v; tested in this order: out-degree(cur) == 0: END; out-degree(cur) > 1: OUT; w = the single out-neighbour,
 * in-degree(w) != 1: IN; len(chain) == max_tip_reads: LONG; else w is appended and cur = w.  Chains that stop with IN or OUT are tips:
 * every read with a vertex in one is removed, in both orientations, with every edge that touches it.  END chains (a short isolated chain
 * is a contig) and LONG chains stay.  Rounds repeat until tip_rounds or until one removes nothing.  A small Y-shaped component can vanish
 * whole in one round (all three arms are tips of each other), as with miniasm's asg_cut_tip.
 * Unitigs: edge v -> w is mergeable iff out-degree(v) == 1 and in-degree(w) == 1.  The maximal mergeable paths and all-mergeable cycles
 * partition the vertices of the live reads (neither contained nor removed; a live read without edges is a one-vertex path).  Path
 * v0 .. vk has the mirror vk^1 .. v0^1 and is emitted iff v0 <= vk^1; a cycle is rotated to its smallest vertex m, is emitted iff
 * m <= min(v^1 over the cycle) and is flagged circular.  Unitigs are ordered by first vertex and named utg%06d{l|c}, counting from 1.
 * Vertex i of a unitig contributes the first nbases[i] bases of its read in the vertex's orientation (1 = reverse complement), at offset
 * pos[i]: nbases = the len of the edge to the next vertex (the closing edge for the last vertex of a cycle), the whole read for the last
 * vertex of a path; len = their sum.  Every edge that is not mergeable joins the last vertex of a path to the first of another and is a
 * link, in CSR order, a link and its twin both listed; MINUS = that end is on the emitted unitig's mirror path. */
#define BELLA_MAX_TIP_ROUNDS 16
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_graph_clean_params) of the caller's header (the struct may grow)          */
    uint32_t max_tip_reads;       /* documented default 4; 0 = no clipping                                                 */
    uint32_t tip_rounds;          /* 3; at most BELLA_MAX_TIP_ROUNDS                                                        */
} bella_graph_clean_params;
#define BELLA_UNITIG_LINK_A_MINUS 1u
#define BELLA_UNITIG_LINK_B_MINUS 2u
typedef struct {
    uint32_t a, b;                /* unitigs: the edge leaves a, enters b                                                  */
    uint32_t ovl, rec;            /* the edge's                                                                            */
    uint32_t flags;               /* BELLA_UNITIG_LINK_*                                                                   */
    uint32_t edge;                /* the edge's position in the CSR                                                        */
} bella_unitig_link;
/* What the last bella_hip_graph_clean (rounds .. edges_removed, clean_ms; zero without one) and bella_hip_graph_unitigs did.  A sized
 * struct: bella_hip_graph_get_unitig_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t unitigs, vertices, links, total_bases, circular;
    uint64_t largest, n50;        /* n50: the length at which the lengths, largest first, sum to half of total_bases or more */
    uint64_t reads_removed, edges_removed;
    uint32_t rounds;              /* tip rounds that ran (the last may have removed nothing)                               */
    uint32_t rank_rounds;         /* pointer-jumping rounds of one ranking                                                 */
    uint32_t tips_per_round[BELLA_MAX_TIP_ROUNDS], reads_per_round[BELLA_MAX_TIP_ROUNDS];
    uint64_t cycle_vertices;      /* vertices on all-mergeable cycles                                                      */
    uint64_t gather_bytes;        /* bytes the sequence gather wrote                                                       */
    double clean_ms, rank_ms, gather_ms;      /* between two events on the stream: tip rounds; succ .. links; the gather.      */
                                              /* gather_ms is one launch, so device time.  clean_ms and rank_ms span the host's */
                                              /* small read-backs (one per tip round, three per compaction) and the buffers     */
                                              /* allocated between them: time on the stream, an upper bound of device time      */
} bella_unitig_stats;
/* Clips tips off the context's current graph (on the device) and REPLACES it: bella_hip_graph_get then returns the cleaned CSR -- the same
 * order, the deleted edges compacted out.  params == NULL: the documented defaults.  BELLA_ERR_STATE without a built graph; BELLA_ERR_BAD_ARG
 * for a struct_size too small or tip_rounds > BELLA_MAX_TIP_ROUNDS.  Drops the unitigs.  A second call clips the cleaned graph further. */
int bella_hip_graph_clean(bella_ctx* ctx, const bella_graph_clean_params* params);
/* removed[nreads] (0 / 1): the reads the clean and pop calls since the last build took out (all 0 without one).  BELLA_ERR_STATE without a graph. */
int bella_hip_graph_get_removed(bella_ctx* ctx, uint8_t* removed);
/* Unitigs, links and unitig bases of the current graph (cleaned or not), on the device; the results are kept on the host until the graph
 * changes.  Every count pointer may be NULL.  An empty graph (no live read) launches nothing and gives zero unitigs; live reads without
 * edges are one-vertex unitigs with bases, and for those the kernels run. */
int bella_hip_graph_unitigs(bella_ctx* ctx, uint64_t* nunitigs, uint64_t* nvertices, uint64_t* nlinks, uint64_t* total_bases);
/* vertex_offsets[nunitigs + 1] into vertices / pos / nbases [nvertices]; len[nunitigs], circular[nunitigs] (0 / 1), links[nlinks].  Any
 * pointer may be NULL.  BELLA_ERR_STATE without bella_hip_graph_unitigs. */
int bella_hip_graph_get_unitigs(bella_ctx* ctx, uint64_t* vertex_offsets, uint32_t* vertices, uint64_t* pos, uint32_t* nbases, uint64_t* len, uint8_t* circular,
                                bella_unitig_link* links);
/* offsets[nunitigs + 1] into bases[total_bases] (upper-case ASCII).  Either may be NULL. */
int bella_hip_graph_get_unitig_bases(bella_ctx* ctx, uint64_t* offsets, uint8_t* bases);
int bella_hip_graph_get_unitig_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* GFA 1 of the unitigs: "H\tVN:Z:1.0"; per unitig "S\tutg%06d{l|c}\t<bases or *>\tLN:i:<len>\tRC:i:<reads>" (RC = the unitig's reads; '*'
 * when bases == NULL) followed by one "a\tutg...\t<pos>\t<read name>\t+/-\t<nbases>" per vertex; then one
 * "L\tutgA\t+/-\tutgB\t+/-\t<ovl>M\trc:i:<rec>" per link.  Truncates the file.  Plain host code, no context.  FASTA: bella_hip_write_fasta
 * with the same names. */
int bella_hip_write_unitig_gfa(const char* path, uint32_t nreads, const char* const* names, uint64_t nunitigs, const uint64_t* vertex_offsets, const uint32_t* vertices,
                               const uint64_t* pos, const uint32_t* nbases, const uint64_t* len, const uint8_t* circular, const uint64_t* base_offsets,
                               const uint8_t* bases, uint64_t nlinks, const bella_unitig_link* links);

/* ---- bubble popping (no counterpart in the reference; the pass is miniasm's asg_pop_bubble) -----------------------
 * One round works on a snapshot of the current graph.  Every vertex s with out-degree >= 2 runs detect(s), a Kahn traversal: each visited
 * vertex carries r (in-edges not yet seen), d (smallest distance from s) and (c, D, p), its best path: reads on it, its length, its
 * predecessor.  visited = {s: r = 0, d = 0, c = 0, D = 0}, stack = [s], pending = 0.  While the stack is not empty: v = pop; out-degree(v)
 * == 0 fails (a tip inside); for v -> w of length l in list order: w == s or w ^ 1 visited fails (a cycle; both orientations of a read);
 * d(v) + l > max_bubble_dist fails; a new w fails when visited - {s} already holds max_bubble_reads vertices, else it is visited with
 * r = in-degree(w), d = d(v) + l, (c, D, p) = (c(v) + 1, D(v) + l, v) and pending += 1; a known w takes d = min(d, d(v) + l) and the new
 * (c, D, p) when (c(v) + 1, D(v) + l) is lexicographically larger than (c(w), D(w)), or equal with v < p(w); then r(w) -= 1 and, at 0, w is
 * pushed and pending -= 1.  After v's edges: stack == [t] and pending == 0 is SUCCESS (t is not expanded).  An empty stack fails (an
 * in-edge from outside keeps a vertex waiting).  Success, t, the visited set and every (d, c, D, p) do not depend on which ready vertex
 * is popped first; the reason of a failure can, and is not reported.
 * Only the side of a bubble with s < t ^ 1 acts.  Interior I = visited - {s, t}; kept path K = t, p(t), p(p(t)), ... s.  Every acting
 * bubble claims the reads of I: claim[read] = min(claim[read], s); it is ACCEPTED iff it holds the claim on every read of I (nested
 * bubbles and bubbles that meet in opposite orientations are settled so; the smallest s always wins).  An accepted bubble removes the
 * reads of I - K, in both orientations, with every edge that touches them, and every edge v -> w with v, w in visited that is not an edge
 * of K, with its twin.  The round's result is the CSR in the old order with the deleted edges compacted out; the removed reads are OR-ed
 * into what bella_hip_graph_get_removed returns, so the unitigs treat them as dead.  Rounds repeat until bubble_rounds or until one
 * accepts nothing (that round is counted). */
#define BELLA_MAX_BUBBLE_READS 255
#define BELLA_MAX_BUBBLE_ROUNDS 16
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_graph_bubble_params) of the caller's header (the struct may grow)         */
    uint32_t max_bubble_reads;    /* documented default 64; at most BELLA_MAX_BUBBLE_READS; 0 = no popping                  */
    uint32_t max_bubble_dist;     /* 50000 bases (miniasm's default)                                                       */
    uint32_t bubble_rounds;       /* 3; at most BELLA_MAX_BUBBLE_ROUNDS                                                     */
} bella_graph_bubble_params;
/* What the last bella_hip_graph_pop_bubbles did (zero without one since the build).  A sized struct: bella_hip_graph_get_bubble_stats
 * writes at most struct_size bytes. */
typedef struct {
    uint64_t reads_removed, edges_removed;    /* over all rounds                                                               */
    uint32_t rounds;                          /* rounds that ran (the last may have accepted nothing)                          */
    uint32_t pad;
    uint32_t sources[BELLA_MAX_BUBBLE_ROUNDS];        /* per round: vertices with out-degree >= 2                              */
    uint32_t found[BELLA_MAX_BUBBLE_ROUNDS];          /* successes of detect with s < t ^ 1                                    */
    uint32_t popped[BELLA_MAX_BUBBLE_ROUNDS];         /* accepted bubbles                                                      */
    uint32_t reads_per_round[BELLA_MAX_BUBBLE_ROUNDS], edges_per_round[BELLA_MAX_BUBBLE_ROUNDS];
    double pop_ms;                            /* between two events on the stream: all rounds, their read-backs included       */
} bella_bubble_stats;
/* Pops bubbles of the context's current graph (on the device) and REPLACES it, as bella_hip_graph_clean does; the popped reads show in
 * bella_hip_graph_get_removed.  params == NULL: the defaults.  BELLA_ERR_STATE without a built graph; BELLA_ERR_BAD_ARG for a struct_size
 * too small, bubble_rounds > BELLA_MAX_BUBBLE_ROUNDS or max_bubble_reads > BELLA_MAX_BUBBLE_READS.  Drops the unitigs.  A graph without
 * edges, max_bubble_reads == 0 or bubble_rounds == 0 launch nothing.  Bubbles of more than max_bubble_reads reads are left alone. */
int bella_hip_graph_pop_bubbles(bella_ctx* ctx, const bella_graph_bubble_params* params);
int bella_hip_graph_get_bubble_stats(bella_ctx* ctx, void* out, uint64_t struct_size);

/* ---- weak-overlap removal (no counterpart in the reference; the pass is miniasm's asg_arc_del_short) -------------
 * On the context's current graph, in the notation of the string graph section; integers only.  best(v) = the largest ovl among v's
 * out-edges: they share the source read's length and the list is ordered by len, so it is the ovl of the list's first edge.  Edge
 * e = v -> w is WEAK iff 1000 ovl(e) < ratio_permille best(v); with ratio_permille <= 1000 the best edge of a vertex is never weak, and a
 * vertex with one out-edge loses nothing by its own rule.  All decisions are taken on one snapshot, and an edge leaves when it OR ITS TWIN
 * (w ^ 1 -> v ^ 1) is weak: the graph stays twin-symmetric and the result does not depend on the order the device works in.  No read is
 * removed (bella_hip_graph_get_removed is unchanged); a read left without edges becomes a one-vertex unitig.  ovl is the edge's own field,
 * in clipped coordinates while a trim exists.  The result is the CSR in the old order with the deleted edges compacted out. */
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_graph_weak_params) of the caller's header (the struct may grow)           */
    uint32_t ratio_permille;      /* documented default 500; at most 1000; 0 = off                                         */
} bella_graph_weak_params;
/* What the last bella_hip_graph_cut_weak did (zero without one since the build).  A sized struct: bella_hip_graph_get_weak_stats writes
 * at most struct_size bytes. */
typedef struct {
    uint64_t forks;               /* vertices with out-degree >= 2                                                         */
    uint64_t weak;                /* edges below their own vertex's threshold                                              */
    uint64_t edges_removed;       /* edges that are weak or whose twin is                                                  */
    uint32_t ratio_permille;      /* the call's                                                                            */
    double cut_ms;                /* between two events on the stream: the kernel, filter, scan, compaction, one read-back */
} bella_weak_stats;
/* Removes the weak edges of the context's current graph (on the device) and REPLACES it, as bella_hip_graph_clean and
 * bella_hip_graph_pop_bubbles do.  params == NULL: the defaults.  BELLA_ERR_STATE without a built graph; BELLA_ERR_BAD_ARG for a
 * struct_size too small or ratio_permille > 1000.  Drops the unitigs; keeps the clips, the contained and the removed marks.  A graph
 * without edges or ratio_permille == 0 launch nothing. */
int bella_hip_graph_cut_weak(bella_ctx* ctx, const bella_graph_weak_params* params);
int bella_hip_graph_get_weak_stats(bella_ctx* ctx, void* out, uint64_t struct_size);

/* ---- unitig consensus: the pileup's majority vote per position of the backbone reads (no counterpart in the
 * reference) -----------------------------------------------------------------------------------------------------------------------
 * Needs the unitigs of bella_hip_graph_unitigs and the pileup table of the read-correction section, both on this context.  The DECISION
 * at position p of read r is the string E_r(p) of 0, 1 or 2 bases that bella_hip_consensus's rule emits for p: the junction's base of
 * step (1) if it fires (p >= 1 only), then the position's base of step (2) unless it is deleted; E_r(0) .. E_r(len - 1) is the read's
 * bella_hip_consensus output.  Vertex i of a unitig (v = 2 r + o, n = nbases[i], L = the read's length) contributes
 *   o == 0: E(0) E(1) .. E(n - 1);      o == 1: rc(E(L - 1)) rc(E(L - 2)) .. rc(E(L - n)), rc = the reverse complement of a decision string,
 * and the polished unitig is the concatenation of its vertices' segments, circular unitigs alike.  A segment takes the decisions of its
 * own positions and nothing else (the junction in front of the first position behind a forward segment is not part of it: an edge effect
 * of at most one base per segment).  With an all-zero table the result is the raw unitigs.  Limits as in the read correction: one
 * inserted base per junction, plain majority; the segment boundaries stay where the raw unitig has them; the links keep their raw
 * overlaps (the link alignment section below aligns them); a second round, with the reads re-aligned to the unitig, is the realignment section below. */
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_polish_params) of the caller's header (the struct may grow)               */
    uint32_t min_depth;           /* >= 1; the documented default is 3                                                     */
} bella_polish_params;
typedef struct {                  /* bella_consensus_read's fields, summed over the unitig's positions                     */
    uint64_t len_before, len_after;
    uint64_t substituted, deleted, inserted, covered, depth_sum;
} bella_polish_unitig;
/* What the last bella_hip_graph_polish_unitigs did.  A sized struct: bella_hip_graph_get_polish_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t unitigs, vertices;
    uint64_t bases_before, bases_after;
    uint64_t substituted, deleted, inserted, covered, depth_sum;
    uint64_t table_bytes;         /* bytes of table rows the decision read: 36 per unitig position                          */
    uint32_t min_depth, tiles;    /* tiles of 4,096 unitig positions                                                       */
    double decide_ms, write_ms;   /* one event pair around the one launch each: device time                                */
} bella_polish_stats;
/* Polishes the unitigs of the last bella_hip_graph_unitigs with the context's pileup table, on the device; the result stays with the
 * context until the unitigs are dropped, the table changes (bella_hip_pileup_reset, bella_hip_add_pileup, a trace that votes) or reads
 * are loaded.  BELLA_ERR_STATE without unitigs or without a table; BELLA_ERR_BAD_ARG for min_depth < 1 or a struct_size too small.  Zero
 * unitigs launch nothing and give empty results.  total_bases may be NULL. */
int bella_hip_graph_polish_unitigs(bella_ctx* ctx, const bella_polish_params* params, uint64_t* total_bases);
/* offsets[nunitigs + 1] into bases[total_bases] (upper-case ASCII); ppos[nvertices] / pnbases[nvertices]: where every vertex's segment
 * starts inside its polished unitig and how long it is; per_unitig[nunitigs].  Any pointer may be NULL.  bella_hip_write_unitig_gfa takes
 * them in place of pos / nbases / len / base_offsets / bases. */
int bella_hip_graph_get_polished(bella_ctx* ctx, uint64_t* offsets, uint8_t* bases, uint64_t* ppos, uint32_t* pnbases, bella_polish_unitig* per_unitig);
int bella_hip_graph_get_polish_stats(bella_ctx* ctx, void* out, uint64_t struct_size);

/* ---- realignment: every read aligned against its polished unitig, a second consensus (no counterpart in the
 * reference) -----------------------------------------------------------------------------------------------------------------------
 * One ROUND takes the newest sequence of every unitig (the polish's, or the round before's), aligns the backbone reads and the contained
 * reads against it base by base, piles their votes up in a nine-counter table indexed by unitig position and applies
 * bella_hip_consensus's rule to every unitig as if it were one read.  Section 18 states the placement, the semi-global banded DP (read
 * global, unitig window free; the trace's scoring and direction choice), the band rule and the votes in full; the tests hold a numpy
 * statement of it, and the device result equals it.  Limits: one inserted base per junction, plain majority, a fixed
 * centre diagonal per read, reads across the origin of a circular unitig are skipped (bella_hip_graph_realign_unitigs_circular below
 * does not skip them), removed reads do not vote, the links keep their raw overlaps (the link alignment section below aligns them), a unitig has fewer than 2^31 - band_max bases.
 *
 * Circles (opt-in: bella_hip_graph_realign_unitigs_circular).  Notation of section 18; u a circular unitig, len its
 * raw and plen its current length, x the raw coordinate where the read's clip starts, n the clip's length.  A read on u is placed on the
 * UNROLLED circle iff (1) plen < 2^29; (2) with xm = x mod len (floor modulo), s0 = P(xm) and ym = xm + n: e0 = P(ym) if ym < len,
 * e0 = plen + P(ym - len) if ym - len < len, otherwise the read is not eligible (P is used inside [0, len) only); (3) e0 >= s0 and
 * max(n, e0 - s0) + band_max <= plen: the read cannot lap itself at the widest band.  Its window is s = s0, or s0 + plen if
 * s0 < band_max / 2, and e = s + (e0 - s0), so s lies in [band_max / 2, plen + band_max / 2); its status is VOTED (a candidate), never
 * OUTSIDE, and its placement's pad word is 1.  A read that is not eligible -- any read on a linear unitig, a circle shorter than
 * n + band_max -- keeps section 18's placement and status, so the option never loses a voter.  The DP is section 18's against the
 * unitig's current sequence twice in a row (2 plen columns; with the window rule no row reaches column 2 plen); s, e, q_begin and q_end
 * are in unrolled coordinates and may exceed plen.  A vote at column or junction q goes to row q mod plen of the unitig's table (an
 * alignment spans at most plen columns: one vote per position and read); an insertion votes for q < 2 plen.  Consensus and segment
 * positions are unchanged.  Limit: the junction before base 0 still takes no insertion. */
#define BELLA_REALIGN_DEFAULT_BAND 512
#define BELLA_REALIGN_DEFAULT_BAND_MAX 4096
#define BELLA_REALIGN_DEFAULT_MIN_IDENTITY 700
enum {
    BELLA_REALIGN_NONE = 0,          /* the read takes no part: removed, uncovered, or not loaded on a unitig                 */
    BELLA_REALIGN_VOTED = 1,
    BELLA_REALIGN_UNPLACED = 2,      /* contained, and no record joins it to a backbone read                                  */
    BELLA_REALIGN_OUTSIDE = 3,       /* its window leaves the unitig by more than band0 / 2                                   */
    BELLA_REALIGN_BAND_CAPPED = 4,   /* the path still touched the band's edge at band_max                                    */
    BELLA_REALIGN_LOW_IDENTITY = 5
};
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_realign_params) of the caller's header (the struct may grow)              */
    uint32_t band0;               /* a power of two in [256, band_max]; the documented default is 512                      */
    uint32_t band_max;            /* a power of two <= 262144; 4096                                                        */
    uint32_t min_identity;        /* permille of '=' among the alignment's columns below which a read does not vote; 700   */
    uint32_t min_depth;           /* >= 1; 3                                                                               */
    uint32_t keep_ops;            /* tests: != 0 keeps the voters' runs for bella_hip_graph_get_realign_ops                */
} bella_realign_params;
typedef struct {
    uint32_t unitig;              /* ~0: status NONE or UNPLACED                                                           */
    uint32_t orient;              /* 1: the read lies on the unitig reverse-complemented                                   */
    int64_t s, e;                 /* the window expected for the read's clip on the current sequence                       */
    uint32_t anchor;              /* contained reads: the record that placed it; ~0 otherwise                              */
    uint32_t status;              /* BELLA_REALIGN_*                                                                       */
    uint32_t band;                /* the last band the read was aligned with (0: never aligned)                            */
    uint32_t n_eq, n_x, n_ins, n_del;
    int32_t score;
    int64_t q_begin, q_end;       /* the unitig junctions the alignment spans                                              */
    uint64_t op_off;              /* keep_ops: first run among the kept runs                                               */
    uint32_t nops, pad;           /* pad: 1 when the read was placed on the unrolled circle (section 19), otherwise 0          */
} bella_realign_placement;
/* What the last round did.  A sized struct: bella_hip_graph_get_realign_stats writes at most struct_size bytes. */
typedef struct {
    uint32_t round;               /* 1 = the first realignment (the second consensus round)                                */
    uint32_t batches;             /* DP launches' batches                                                                  */
    uint64_t backbone, contained; /* reads that were placed as a unitig's vertex / through an anchor record                */
    uint64_t unplaced, outside, band_capped, low_identity, voted;
    uint64_t repeated;            /* reads on more than one vertex: the first vertex counts                                */
    uint64_t dp_cells;            /* rows x band summed over every DP that ran                                             */
    uint64_t dir_bytes_peak;      /* the largest batch's direction bytes                                                   */
    uint64_t votes;
    uint64_t bases_before, bases_after;
    uint64_t substituted, deleted, inserted;
    double place_ms, dp_ms, walk_ms, vote_ms, decide_ms;      /* device time between events                               */
} bella_realign_stats;
/* One round on the device.  params == NULL: the defaults.  BELLA_ERR_STATE without a polish; BELLA_ERR_BAD_ARG for a band that is no
 * power of two or out of range, min_depth < 1, min_identity > 1000, a struct_size too small; BELLA_ERR_NOMEM when the table (36 bytes per
 * unitig base) does not fit.  The result replaces the last round's and goes with the polish.  Zero unitigs launch nothing. */
int bella_hip_graph_realign_unitigs(bella_ctx* ctx, const bella_realign_params* params, uint64_t* total_bases);
/* The same round with the circle rule above: the same parameters, errors, state rules and getters.  Without a circular unitig the result
 * is bella_hip_graph_realign_unitigs' exactly; `outside` counts what is still outside. */
int bella_hip_graph_realign_unitigs_circular(bella_ctx* ctx, const bella_realign_params* params, uint64_t* total_bases);
/* *wrapped = the last round's voters on the unrolled circle with e > plen or q_end > plen: the reads that reach across an origin (0 after
 * a plain round).  A getter of its own: bella_realign_stats keeps its 176 bytes.  BELLA_ERR_STATE without a round; wrapped may be NULL. */
int bella_hip_graph_get_realign_wrapped(bella_ctx* ctx, uint64_t* wrapped);
/* As bella_hip_graph_get_polished: pos / nbases are where the polish's segments begin in the new sequence.  Any pointer may be NULL. */
int bella_hip_graph_get_realigned(bella_ctx* ctx, uint64_t* offsets, uint8_t* bases, uint64_t* pos, uint32_t* nbases, bella_polish_unitig* per_unitig);
/* out[nreads] */
int bella_hip_graph_get_realign_placements(bella_ctx* ctx, bella_realign_placement* out);
/* tests: *nops = the kept runs; ops (nullable) receives them, table (nullable) the round's counters (9 uint32 per base of the sequence the
 * round aligned against).  Both are empty unless the round ran with keep_ops. */
int bella_hip_graph_get_realign_ops(bella_ctx* ctx, uint64_t* nops, uint32_t* ops, uint32_t* table);
int bella_hip_graph_get_realign_stats(bella_ctx* ctx, void* out, uint64_t struct_size);

/* ---- link alignment: the ends of two linked unitigs aligned against each other (no counterpart in the reference) --
 * Link k = (a, b, ovl, rec, flags) of bella_hip_graph_unitigs claims that a suffix of A^ overlaps a prefix of B^.  cur(u) is the newest
 * sequence of unitig u (the last realignment round's, else the polish's, else the raw bases), P_u its length, len_u the raw length,
 * C_u the raw -> current map of the realignment section (the identity when nothing was polished); A^ = cur(a), or its reverse
 * complement when A_MINUS is set, B^ likewise from b and B_MINUS.
 *   Expected overlaps.  o_a = min(ovl, len_a), o_b = min(ovl, len_b); oa = P_a - C_a(len_a - o_a) when A is plus, C_a(o_a) when minus;
 * ob = C_b(o_b) when B is plus, P_b - C_b(len_b - o_b) when minus.
 *   Windows.  S = band_max / 2.  Columns: X, the last m = min(P_a, oa + S) bases of A^.  Rows: Y, the first n = min(P_b, ob + S) bases
 * of B^.  Centre diagonal c = m - (oa + ob) / 2 (floor).
 *   DP.  The realignment section's cell rule, scoring (+1 / -1 / -1), recurrence and direction preference; cell (i, q) exists iff
 * -B/2 <= q - i - c < B/2 and 0 <= q <= m; row 0 is 0.  The end is the best existing cell of COLUMN m over the rows 0 .. n, ties to the
 * smallest row: B^ starts at its first base, A^ ends at its last.  The walk goes from (i_end, m) back to row 0 and gives q_begin; it has
 * TOUCHED as in the realignment section, and a column m without a reachable cell counts as touched.  B starts at band0 and doubles
 * while the path touches, up to band_max.
 *   Status, tested in this order: a == b: SELF (never aligned: a sequence's tail against its own head has a trivial full-length answer);
 * touched at band_max: BAND_CAPPED; best score <= 0: EMPTY; 1000 n_eq < min_identity (n_eq + n_x + n_ins + n_del): LOW_IDENTITY; else
 * ALIGNED.  ovl_a = m - q_begin, ovl_b = i_end; 'I' is a base of B^ only, 'D' a base of A^ only (`from` is the reference); the runs are in
 * the order of B^, op | len << 4 with op 0 '=', 1 'X', 2 'I', 3 'D', and only ALIGNED links have runs.  A link whose column m no path
 * reached has all-zero results.
 *   Twins.  The twin of (a, sa, b, sb) is (b, !sb, a, !sa) with the same rec.  Links are paired in index order: link k, not SELF and not
 * yet paired, takes the smallest later unpaired link that is its twin.  Only the lower-indexed link of a pair is aligned; the other is
 * DERIVED: its runs are the mate's reversed with 'I' and 'D' swapped, ovl_a and ovl_b swapped, n_ins and n_del swapped, status, band,
 * score, n_eq and n_x the mate's, and mate = the other link's index on both (~0 on a link without a twin).  The DP's tie-breaks are not
 * reversal-symmetric, so deriving is what keeps the two L lines consistent.
 *   Limits: SELF links and links of more than one alignment segment are not aligned; band_max is at most 4096. */
#define BELLA_LINK_DEFAULT_BAND 512
#define BELLA_LINK_DEFAULT_BAND_MAX 4096
#define BELLA_LINK_DEFAULT_MIN_IDENTITY 700
enum {
    BELLA_LINK_ALIGNED = 0,
    BELLA_LINK_EMPTY = 1,            /* the best score is not positive                                                        */
    BELLA_LINK_BAND_CAPPED = 2,      /* the path still touched the band's edge at band_max                                    */
    BELLA_LINK_LOW_IDENTITY = 3,
    BELLA_LINK_SELF = 4              /* a == b                                                                                */
};
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_link_params) of the caller's header (the struct may grow)                 */
    uint32_t band0;               /* a power of two in [256, band_max]; the documented default is 512                      */
    uint32_t band_max;            /* a power of two <= 4096; 4096                                                          */
    uint32_t min_identity;        /* permille of '=' among the alignment's columns below which a link is LOW_IDENTITY; 700 */
} bella_link_params;
typedef struct {
    uint32_t status;              /* BELLA_LINK_*                                                                          */
    uint32_t band;                /* the last band the link was aligned with (0: SELF)                                     */
    int32_t score;
    uint32_t ovl_a, ovl_b;        /* bases of A^'s suffix and of B^'s prefix that the alignment spans                      */
    uint32_t n_eq, n_x, n_ins, n_del;
    uint32_t mate;                /* the twin's index; ~0: none                                                            */
    uint64_t op_off;              /* first run among all runs                                                              */
    uint32_t nops;                /* ALIGNED only                                                                          */
    uint32_t derived;             /* 1: taken from the mate's alignment                                                    */
} bella_link_aln;
/* What the last bella_hip_graph_align_links did.  A sized struct: bella_hip_graph_get_link_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t links;
    uint64_t aligned, empty, band_capped, low_identity, self;     /* links by status, the derived ones included               */
    uint64_t derived;
    uint64_t overlap_before, overlap_after;   /* over the ALIGNED links: the expected overlaps oa, and ovl_a                   */
    uint64_t jobs;                /* links that were aligned                                                               */
    uint64_t dp_cells;            /* rows x band summed over every DP that ran                                             */
    uint64_t ops;                 /* runs of all links                                                                     */
    uint32_t batches, pad;
    double pack_ms, dp_ms, walk_ms;           /* device time between events                                                    */
} bella_link_stats;
/* Aligns the links of the last bella_hip_graph_unitigs on the device.  params == NULL: the defaults; naligned (nullable): the ALIGNED
 * links.  BELLA_ERR_STATE without unitigs; BELLA_ERR_BAD_ARG for a band that is no power of two or outside [256, 4096], band0 > band_max,
 * min_identity > 1000, a struct_size too small.  The result stays with the context until the unitigs are dropped, or the sequence it was
 * made from is replaced: a polish, a realignment round.  Zero links, or SELF links only, launch nothing. */
int bella_hip_graph_align_links(bella_ctx* ctx, const bella_link_params* params, uint64_t* naligned);
/* alns[nlinks] in the order of the links; *nops = the runs of all links; ops[*nops].  Any pointer may be NULL.  BELLA_ERR_STATE without
 * an alignment of the links. */
int bella_hip_graph_get_link_alignments(bella_ctx* ctx, bella_link_aln* alns, uint64_t* nops, uint32_t* ops);
int bella_hip_graph_get_link_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* bella_hip_write_unitig_gfa with the links' alignments: an ALIGNED link's line is
 * "L\tutgA\t+/-\tutgB\t+/-\t<CIGAR>\trc:i:<rec>\tNM:i:<n_x + n_ins + n_del>\tol:i:<ovl>", the CIGAR in M / I / D with '=' and 'X' merged into
 * M; every other link's line is bella_hip_write_unitig_gfa's.  alns[nlinks] and ops as bella_hip_graph_get_link_alignments returned them;
 * alns == NULL writes what bella_hip_write_unitig_gfa writes.  The sequences passed should be the ones the links were aligned on.  Plain
 * host code, no context. */
int bella_hip_write_unitig_gfa_links(const char* path, uint32_t nreads, const char* const* names, uint64_t nunitigs, const uint64_t* vertex_offsets, const uint32_t* vertices,
                                     const uint64_t* pos, const uint32_t* nbases, const uint64_t* len, const uint8_t* circular, const uint64_t* base_offsets,
                                     const uint8_t* bases, uint64_t nlinks, const bella_unitig_link* links, const bella_link_aln* alns, const uint32_t* ops);

/* ---- pair alignment: caller-supplied pairs of sequences aligned on the device, with their runs (no counterpart
 * in the reference) -----------------------------------------------------------------------------------------------------------------
 * bases[nbases] holds every sequence, upper-case ACGT.  Pair k names a query Q = bases[q_off, q_off + q_len) and a target T =
 * bases[t_off, t_off + t_len), n = q_len >= 1 and m = t_len >= 1, and a centre diagonal c; with BELLA_ALIGN_PAIR_RC set, Q is
 * reverse-complemented before anything else.  Rows i = 0 .. n are bases of Q, columns q = 0 .. m bases of T.
 *   DP.  The realignment section's scoring (+1 / -1 / -1, linear), cell rule (cell (i, q) exists iff -B/2 <= q - i - c < B/2 and
 * 0 <= q <= m), recurrence, direction preference (the first of diagonal, up, left that attains the maximum), clamp of the walk and
 * TOUCHED rule (a visited cell with p = q - i - c + B/2 <= 0 or >= B - 1 in a row >= 1, or an end that no path reaches).  The mode
 * sets row 0, the end and where the walk stops:
 *   BELLA_ALIGN_GLOBAL      row 0 is -q; the end is the cell (n, m); the walk goes back to (0, 0), leftwards along row 0 as 'D'.  An end
 *                           or a start outside the band counts as touched.
 *   BELLA_ALIGN_SEMIGLOBAL  row 0 is 0; the end is the best cell of row n, ties to the smallest q; the walk stops in row 0: Q whole, a
 *                           window of T (the realignment section's alignment).
 *   BELLA_ALIGN_DOVETAIL    row 0 is 0; the end is the best cell of column m, ties to the smallest row; the walk stops in row 0: a
 *                           suffix of T against a prefix of Q (the link section's alignment).
 *   Bands.  B starts at band0 and doubles while the pair is touched, up to band_max.  A band that cannot hold what the mode needs is
 * doubled without a DP: global, the start (0, 0) or the end (n, m) outside it; the other two, no cell of the rectangle inside it.
 *   Status.  BELLA_ALIGN_STATUS_TOO_LARGE: n + m >= 2^27, or the pair's direction bytes n * B / 4 at the band it is to run with exceed
 * one batch (BELLA_TUNE_ROUND_BUDGET, else by the free memory); band = that band.  BELLA_ALIGN_STATUS_BAND_CAPPED: touched at
 * band_max.  Both leave every other field of the result but band and widened zero.  BELLA_ALIGN_STATUS_ALIGNED: everything else.
 *   Result.  q_begin, q_end: the rows the alignment spans (0 and n, or 0 and the end row of a dovetail); t_begin, t_end: the columns (0
 * and m for global, the window for semi-global, the start and m for a dovetail).  'I' is a base of Q only, 'D' a base of T only; the
 * runs are in the order of Q, len << 4 | op with op 0 '=', 1 'X', 2 'I', 3 'D', adjacent runs differ, and only ALIGNED pairs have runs.  A
 * dovetail whose best cell is (0, m) is ALIGNED with no runs.  The runs of all pairs lie by the pairs' last band, then by index. */
#define BELLA_ALIGN_DEFAULT_BAND 512
#define BELLA_ALIGN_DEFAULT_BAND_MAX 4096
#define BELLA_ALIGN_MAX_BAND 16384
#define BELLA_ALIGN_PAIR_RC 1u
enum { BELLA_ALIGN_GLOBAL = 0, BELLA_ALIGN_SEMIGLOBAL = 1, BELLA_ALIGN_DOVETAIL = 2 };
enum { BELLA_ALIGN_STATUS_ALIGNED = 0, BELLA_ALIGN_STATUS_BAND_CAPPED = 1, BELLA_ALIGN_STATUS_TOO_LARGE = 2 };
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_align_params) of the caller's header (the struct may grow)                */
    uint32_t mode;                /* BELLA_ALIGN_GLOBAL / _SEMIGLOBAL / _DOVETAIL                                          */
    uint32_t band0;               /* a power of two in [256, band_max]; 0: 512                                             */
    uint32_t band_max;            /* a power of two <= 16384; 0: 4096                                                      */
} bella_align_params;
typedef struct {
    uint64_t q_off, t_off;        /* first base of Q and of T in bases                                                     */
    uint32_t q_len, t_len;        /* n and m: 1 .. 2^30 - 1                                                                */
    uint32_t flags;               /* BELLA_ALIGN_PAIR_RC                                                                   */
    int32_t centre;               /* c, taken as given                                                                     */
} bella_align_pair;
typedef struct {
    uint32_t status;              /* BELLA_ALIGN_STATUS_*                                                                  */
    uint32_t band;                /* the last band of the pair                                                             */
    uint32_t widened;             /* doublings of the band                                                                 */
    int32_t score;
    uint32_t q_begin, q_end;      /* rows                                                                                  */
    uint32_t t_begin, t_end;      /* columns                                                                               */
    uint32_t n_eq, n_x, n_ins, n_del;
    uint64_t op_off;              /* first run among the runs of the call                                                  */
    uint32_t nops;                /* ALIGNED only                                                                          */
    uint32_t pad;
} bella_align_result;
/* What the last bella_hip_align_sequences did.  A sized struct: bella_hip_get_align_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t pairs;
    uint64_t aligned, band_capped, too_large;     /* pairs by status                                                       */
    uint64_t repeated;            /* DPs that ran again with the band doubled                                              */
    uint64_t dp_cells;            /* rows x band summed over every DP that ran                                             */
    uint64_t ops;                 /* runs of all pairs                                                                     */
    uint32_t batches, mode;
    double pack_ms, dp_ms, walk_ms;               /* device time between events                                            */
    double total_ms;              /* the whole call on the host clock                                                      */
} bella_align_stats;
/* Aligns pairs[npairs] over bases[nbases]: out[npairs] in the order of the pairs, *nops (nullable) = the runs of all pairs, which stay
 * with the context until the next successful call (bella_hip_get_align_ops).  params == NULL: global with the default bands.
 * Everything is checked before anything is launched: BELLA_ERR_BAD_ARG, with `out` and the runs of the call before untouched, for a byte
 * other than ACGT inside a window that a pair uses, a window outside bases, a length of zero, a sequence of 2^30 bases or more, mode > 2,
 * a band that is no power of two or outside [256, 16384], band0 > band_max, a struct_size too small.  npairs == 0 launches nothing.
 * The call needs a context but no loaded reads, and leaves every stage of the context as it found it. */
int bella_hip_align_sequences(bella_ctx* ctx, const uint8_t* bases, uint64_t nbases, const bella_align_pair* pairs, uint64_t npairs, const bella_align_params* params,
                              bella_align_result* out, uint64_t* nops);
/* the runs of the last bella_hip_align_sequences or bella_hip_align_sequences_affine, whichever succeeded last, into ops[cap];
 * BELLA_ERR_BAD_ARG when they do not fit.  The stats are that call's too. */
int bella_hip_get_align_ops(bella_ctx* ctx, uint32_t* ops, uint64_t cap);
int bella_hip_get_align_stats(bella_ctx* ctx, void* out, uint64_t struct_size);

/* ---- pair alignment with affine gaps and the caller's scores (no counterpart in the reference) -------------------
 * The pair alignment above under Gotoh's three matrices.  Everything not said here is the section above's, word for word: the pairs, the
 * rc flag, the centre diagonal, the cells that exist, the three modes' ends and tie rules, the doubling of the band, the statuses, the
 * result fields, the run encoding and the order of the runs.
 *   Scoring.  (a, b, o, e) = (match, mismatch, gap_open, gap_extend): a match +a, a mismatch -b, a gap of L bases -(o + e L);
 * 1 <= a <= 255, 0 <= b <= 255, 0 <= o <= 255, 1 <= e <= 255.
 *   Matrices.  Three per cell; a cell that does not exist is minus infinity in all three:
 *       E[i][q] = max(H[i-1][q] - o - e, E[i-1][q] - e)      a gap that consumes Q ('I')
 *       F[i][q] = max(H[i][q-1] - o - e, F[i][q-1] - e)      a gap that consumes T ('D')
 *       H[i][q] = max(H[i-1][q-1] + s(i, q), E[i][q], F[i][q])
 *   Row 0.  Global: H[0][0] = 0, H[0][q] = F[0][q] = -(o + e q) for q > 0; semi-global and dovetail: H[0][q] = 0.  E[0][.] is minus
 * infinity in every mode, F[0][.] outside global.  Column 0 needs no special case: the E recurrence produces it.
 *   Stored per cell, 4 bits.  hsrc (2 bits): the first of diagonal (0), E (1), F (2) that attains H.  closeE: H[i][q] - o >= E[i][q].
 * closeF: H[i][q] - o >= F[i][q].  A set close bit says that a gap arriving at this cell from below (closeE) or from the right (closeF)
 * is opened here, not extended; ties go to opening.
 *   The walk has a state in {H, E, F} and starts in H at the mode's end cell.  In H at (i, q): hsrc 0 emits '=' or 'X' and moves
 * diagonally; hsrc 1 switches to E without moving; hsrc 2 to F.  In E: emit 'I', i <- i - 1, then H if closeE of the new cell is set,
 * else E.  In F: emit 'D', q <- q - 1, then H if closeF of the new cell is set, else F.  In row 0 (global only) it emits 'D' leftwards
 * to (0, 0), in column 0 with i > 0 'I' upwards, whatever its state.  The clamp into the band and TOUCHED are the section above's: any
 * visited cell with p <= 0 or p >= B - 1 in a row >= 1, in any state, or an end that no path reaches.
 *   BELLA_ALIGN_STATUS_TOO_LARGE: (n + m) max(a, b, o + e) >= 2^27 (with (1, 1, 0, 1): n + m >= 2^27), or the pair's direction bytes
 * n * B / 2 at the band it is to run with exceed one batch.
 *   With (1, 1, 0, 1) the results and the runs are bella_hip_align_sequences', from other kernels. */
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_align_scoring) of the caller's header (the struct may grow)               */
    uint32_t match;               /* a: 1 .. 255                                                                           */
    uint32_t mismatch;            /* b: 0 .. 255, subtracted                                                               */
    uint32_t gap_open;            /* o: 0 .. 255, subtracted once per gap                                                  */
    uint32_t gap_extend;          /* e: 1 .. 255, subtracted per base of a gap                                             */
    uint32_t reserved;            /* 0                                                                                     */
} bella_align_scoring;
/* bella_hip_align_sequences under `scoring`; scoring == NULL: (1, 1, 0, 1), through the affine kernels.  Every check of that call applies;
 * BELLA_ERR_BAD_ARG on top, with nothing written or launched, for a score outside its range, reserved != 0, a struct_size too small. */
int bella_hip_align_sequences_affine(bella_ctx* ctx, const uint8_t* bases, uint64_t nbases, const bella_align_pair* pairs, uint64_t npairs, const bella_align_params* params,
                                     const bella_align_scoring* scoring, bella_align_result* out, uint64_t* nops);

/* ---- read correction rounds: the partners' raw clips aligned against the corrected read, one more consensus (no
 * counterpart in the reference) ------------------------------------------------------------------------------------------------------
 * One ROUND aligns, for every accumulated overlap record, each of the two reads' RAW clips against the CURRENT corrected sequence of the
 * other read, votes into a nine-counter table in corrected coordinates and applies bella_hip_consensus's rule to every current sequence
 * as if it were a read.  Round 1 is bella_hip_consensus; round k reads round k - 1.  Everything is an integer; the tests hold a numpy
 * statement (bella_testkit/recorrect_mirror.py), and the device result equals it.
 *   Coordinate map.  bella_hip_consensus keeps, per read r of L_r bases, the anchors a_r[j], j = 0 .. ceil(L_r / 256): the offset inside
 * the corrected read at which raw base min(256 j, L_r) was emitted (its emit scan), so the last anchor is the corrected length; 8 bytes per
 * 256 bases.  P_r(x), 0 <= x <= L_r, is section 18's P over the segments pos = 256 j, nb = min(256, L_r - 256 j), cpos = a_r[j],
 * cnb = a_r[j + 1] - a_r[j]: P_r(x) = a_r[j] + (x - 256 j) cnb / nb (floor) with j = floor(x / 256), and P_r(L_r) = the current length.  A
 * round's new anchor j is its own emit scan at the old anchor j: the anchors stay exact, the interpolation between them is approximate.
 *   Jobs.  Record x (V = cid, H = rid, strand, [begV, endV) on V, [begH, endH) on H') gives job 2 x (side 0, target V) and 2 x + 1
 * (side 1, target H):
 *     2 x,     strand 0: rows H[begH, endH);                              raw window on V [begV, endV)
 *     2 x,     strand 1: rows the reverse complement of H[L_H - endH, L_H - begH);   raw window on V [begV, endV)
 *     2 x + 1, strand 0: rows V[begV, endV);                              raw window on H [begH, endH)
 *     2 x + 1, strand 1: rows the reverse complement of V[begV, endV);    raw window on H [L_H - endH, L_H - begH)
 * Every record votes, whatever class the graph would give it, two records of one read pair both; the clips of bella_hip_graph_trim are
 * ignored.  n = the rows, s = P_t(window begin), e = P_t(window end), plen = the target's current length; plen == 0: status NONE.
 *   Alignment, band rule, statuses (BAND_CAPPED, LOW_IDENTITY, VOTED: the BELLA_REALIGN_* values), votes and consensus: section 18's,
 * with the target as the voted side -- c = s + floor(((e - s) - n) / 2), cell (i, q) iff -B/2 <= q - i - c < B/2 and 0 <= q <= plen, B from
 * band0 doubling up to band_max while the walk touches the band's first or last diagonal.  The consensus takes the current sequence's own
 * bases as b[p] (with their + 1 vote); a read nobody voted on comes out as it went in.
 *   Limits: one inserted base per junction, plain majority, a fixed centre diagonal, the interpolation between anchors, all current bases
 * together fewer than 2^31. */
#define BELLA_RECORRECT_DEFAULT_BAND 512
#define BELLA_RECORRECT_DEFAULT_BAND_MAX 4096
#define BELLA_RECORRECT_DEFAULT_MIN_IDENTITY 700
#define BELLA_RECORRECT_ANCHOR_STEP 256
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_recorrect_params) of the caller's header (the struct may grow)            */
    uint32_t band0;               /* a power of two in [256, band_max]; the documented default is 512                      */
    uint32_t band_max;            /* a power of two <= 262144; 4096                                                        */
    uint32_t min_identity;        /* permille of '=' among the alignment's columns below which a job does not vote; 700    */
    uint32_t min_depth;           /* >= 1; 3                                                                               */
    uint32_t keep_ops;            /* tests: != 0 keeps the voters' runs and the table for bella_hip_get_recorrect_ops      */
} bella_recorrect_params;
typedef struct {
    uint32_t record, side;        /* job 2 record + side; side 0: the target is V, 1: the target is H                      */
    uint32_t target, query;       /* reads                                                                                 */
    uint32_t orient;              /* 1: the rows are the query clip reverse-complemented (the record's strand)             */
    uint32_t status;              /* BELLA_REALIGN_NONE, _VOTED, _BAND_CAPPED or _LOW_IDENTITY                             */
    uint32_t qbeg, qend;          /* the query clip, on the query read as given                                            */
    int64_t s, e;                 /* the window expected for the clip on the target's current sequence                     */
    uint32_t band;                /* the last band the job was aligned with (0: never aligned)                             */
    uint32_t n_eq, n_x, n_ins, n_del;
    int32_t score;
    int64_t q_begin, q_end;       /* the junctions of the target's current sequence the alignment spans                    */
    uint64_t op_off;              /* keep_ops: first run among the kept runs                                               */
    uint32_t nops, pad;
} bella_recorrect_job;
/* What the last round did.  A sized struct: bella_hip_get_recorrect_stats writes at most struct_size bytes. */
typedef struct {
    uint32_t round;               /* 2 = the first round after bella_hip_consensus                                         */
    uint32_t batches;             /* DP launches' batches                                                                  */
    uint64_t jobs, none, band_capped, low_identity, voted;
    uint64_t dp_cells;            /* rows x band summed over every DP that ran                                             */
    uint64_t dir_bytes_peak;      /* the largest batch's direction bytes                                                   */
    uint64_t votes;
    uint64_t bases_before, bases_after;
    uint64_t substituted, deleted, inserted;
    double place_ms, dp_ms, walk_ms, vote_ms, decide_ms;      /* device time between events                               */
} bella_recorrect_stats;
/* One round on the device, over the records accumulated at the time of the call.  params == NULL: the defaults.  BELLA_ERR_STATE without a
 * consensus; BELLA_ERR_BAD_ARG for a band that is no power of two or out of range, min_depth < 1, min_identity > 1000, a struct_size too
 * small; BELLA_ERR_NOMEM when the table (36 bytes per current base) does not fit.  The result replaces the last round's; a failed round
 * leaves the round before; whatever drops the consensus (a new consensus, a change of the table, new reads) drops the rounds.
 * bella_hip_get_consensus keeps returning round 1.  Zero records launch nothing and return the input.  total_bases may be NULL. */
int bella_hip_recorrect(bella_ctx* ctx, const bella_recorrect_params* params, uint64_t* total_bases);
/* offsets[nreads + 1] into bases[total_bases] (upper-case ASCII); stats[nreads] relative to the round's input.  Any pointer may be NULL. */
int bella_hip_get_recorrected(bella_ctx* ctx, uint64_t* offsets, uint8_t* bases, bella_consensus_read* stats);
/* *njobs = 2 x the records of the last round; out (nullable) receives them. */
int bella_hip_get_recorrect_jobs(bella_ctx* ctx, uint64_t* njobs, bella_recorrect_job* out);
/* tests: *nops = the kept runs; ops (nullable) receives them, table (nullable) the round's counters (9 uint32 per base of the round's
 * input).  Both are empty unless the round ran with keep_ops. */
int bella_hip_get_recorrect_ops(bella_ctx* ctx, uint64_t* nops, uint32_t* ops, uint32_t* table);
int bella_hip_get_recorrect_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* tests: the anchors of the newest sequences (the last round's, or the consensus's): offsets[nreads + 1] into anchors[]; either may be
 * NULL.  BELLA_ERR_STATE without a consensus. */
int bella_hip_get_recorrect_anchors(bella_ctx* ctx, uint64_t* offsets, uint64_t* anchors);

/* ---- coverage trimming: clip every read to its longest well-covered stretch before the graph (no counterpart in
 * the reference; the stage is miniasm's ma_hit_sub / ma_hit_cut) ---------------------------------------------------------------------
 * Notation of the string graph section.  A record whose e1 - b1 or e2 - b2 is below min_span gives nothing.  Every other record gives
 * one interval [b, e) to each of its two reads in that read's OWN coordinates (length l): (b1, e1) to V; (b2, e2) to H for strand 0 and
 * (l2 - e2, l2 - b2) for strand 1.  The interval is shrunk to [s, t): s = b if b <= end_clip else b + end_clip; t = e if l - e <= end_clip
 * else e - end_clip (an interval that reaches a read end keeps that end); it is dropped when t <= s.  depth(p) = the shrunk intervals
 * that contain p; a region is a maximal run of positions with depth >= min_depth (two regions that abut are one: depth is judged after
 * all events of a position).  The clip of a read is its longest region, the leftmost on ties; without a region, or with the longest
 * shorter than min_span, the read is UNCOVERED and its clip is (0, 0).
 * While clips exist bella_hip_graph_build CUTS every record first: cs1, ce1 = V's clip; c2s, c2e = H's clip in H' coordinates (mirrored
 * by l2 for strand 1).  A record with an uncovered read is OUTSIDE.  Otherwise db = max(0, cs1 - b1, c2s - b2), de = max(0, e1 - ce1,
 * e2 - c2e), the ends become b1 + db, e1 - de, b2 + db, e2 - de (both sides move by the same amount: a record carries no path); a record
 * with an empty interval is OUTSIDE; otherwise cs1 is subtracted from V's coordinates, c2s from H''s, and the lengths are ce1 - cs1 and
 * c2e - c2s.  The six rules then run unchanged.  OUTSIDE records give no candidates.  An uncovered read is dead everywhere downstream
 * (bella_hip_graph_get's contained[] holds 2 for it); edge len / ovl, unitig pos / nbases / len and the unitig bases are in clipped
 * coordinates: a vertex of read r contributes read[beg + i] (orientation 0) or the complement of read[end - 1 - i] (orientation 1).
 * bella_hip_graph_polish_unitigs takes its decision at the ORIGINAL position beg + i (resp. end - 1 - i). */
typedef struct {
    uint32_t struct_size;         /* sizeof(bella_graph_trim_params) of the caller's header (the struct may grow)           */
    uint32_t min_depth;           /* documented default 3; >= 1                                                            */
    uint32_t end_clip;            /* 500                                                                                   */
    uint32_t min_span;            /* 1000                                                                                  */
} bella_graph_trim_params;
typedef struct {
    uint32_t beg, end;            /* the clip [beg, end) in the read's own coordinates; (0, 0) = uncovered                 */
    uint32_t nregions;            /* regions of the read (2 and more: the signature of a chimera)                          */
    uint32_t max_depth;           /* the largest depth on the read                                                         */
} bella_read_clip;
/* What the last bella_hip_graph_trim did.  A sized struct: bella_hip_graph_get_trim_stats writes at most struct_size bytes. */
typedef struct {
    uint64_t intervals;           /* shrunk intervals that entered the sweep                                               */
    uint64_t reads_clipped;       /* covered reads whose clip is not the whole read                                        */
    uint64_t reads_uncovered;
    uint64_t reads_multi;         /* reads with two or more regions                                                        */
    uint64_t bases_before, bases_after;
    uint64_t records_outside;     /* filled by the next bella_hip_graph_build (0 until then)                               */
    double events_ms, sort_ms, sweep_ms;      /* between two events on the stream; sort_ms includes the per-read offsets       */
    double host_ms;               /* the whole call on the host clock                                                      */
} bella_trim_stats;
/* Computes the clips from the accumulated records, on the device.  params == NULL: the defaults.  BELLA_ERR_BAD_ARG for a struct_size
 * too small or min_depth < 1; BELLA_ERR_STATE without reads.  Drops any built graph and any unitigs.  The clips stay until
 * bella_hip_graph_untrim, until records are added, bella_hip_graph_reset, or reads are loaded; bella_hip_graph_build uses them while
 * they exist.  Without a trim every entry point behaves as if this section did not exist. */
int bella_hip_graph_trim(bella_ctx* ctx, const bella_graph_trim_params* params);
/* out[nreads].  BELLA_ERR_STATE without a trim. */
int bella_hip_graph_get_trim(bella_ctx* ctx, bella_read_clip* out);
int bella_hip_graph_get_trim_stats(bella_ctx* ctx, void* out, uint64_t struct_size);
/* Drops the clips, and with them the built graph and the unitigs, which were made with them.  Without a trim nothing happens. */
int bella_hip_graph_untrim(bella_ctx* ctx);

/* ---- multi-GPU: one context per GPU, RCCL over xGMI ------------------------------------------------
 * The reference's multi-GPU path hands alignment batches to the devices inside one call (loganGPU/functions.cuh:441-443,
 * 498-637; include/align.hpp:226-229) and has no collective.  Here reads are 1D row-block partitioned: context r assembles the
 * rows of B of its read block (bella_hip_assemble_panel / _counted_panel), bella_hip_allgather_panels exchanges the panels with
 * ONE grouped point-to-point all-gather (every peer pair uses its own xGMI link; the blocks land directly at their offsets of
 * the full arrays, no padding, no staging) and builds the device layout; bella_hip_set_partition then gives every context its
 * output columns.  The communicator is RCCL's: rank 0 makes the 128-byte id (bella_hip_comm_id), the host program hands it to
 * every rank (MPI, torch.distributed, a file ...), every rank calls bella_hip_comm_init (collective). */
#define BELLA_HIP_COMM_ID_BYTES 128
int bella_hip_comm_id(uint8_t id[BELLA_HIP_COMM_ID_BYTES]);
int bella_hip_comm_init(bella_ctx* ctx, int nranks, int rank, const uint8_t id[BELLA_HIP_COMM_ID_BYTES]);
int bella_hip_comm_destroy(bella_ctx* ctx);
/* 1 if librccl can be loaded in this process (every rank can check this BEFORE the collective bella_hip_comm_init) */
int bella_hip_comm_available(void);
/* The same communicator interface over an in-process transport: the "ranks" are contexts of ONE process (each driven by its own
 * host thread, on one GPU or several), rendezvous on the host, bytes moved with device-to-device copies.  Runs the N > 1 logic of
 * the two collective entry points below without RCCL (tests on a single GPU; several contexts inside one host program). */
int bella_hip_comm_id_local(uint8_t id[BELLA_HIP_COMM_ID_BYTES]);
int bella_hip_comm_init_local(bella_ctx* ctx, int nranks, int rank, const uint8_t id[BELLA_HIP_COMM_ID_BYTES]);
/* collective: needs a panel (rank r: rows [first_r, first_r + rows_r), the blocks in rank order covering all reads) */
int bella_hip_allgather_panels(bella_ctx* ctx);
/* collective k-mer counting (kmercount.hpp:467-677 + main.cpp:393-416 across the ranks; the reference's relative is --split-count,
 * kmercount.hpp:534, which partitions the k-mer space into sequential passes): rank r counts the canonical k-mers of ITS range of
 * the code space over all reads, the partial dictionaries are exchanged once, tuples are made for the reads of the rank's own
 * block only (the block it will pass to bella_hip_assemble_counted_panel).  selector: 0 all k-mers, 1 syncmers (-s), 2 minimizers (-w). */
int bella_hip_count_kmers_dist(bella_ctx* ctx, uint16_t kmer_size, uint32_t lower, uint32_t upper, uint32_t selector, uint32_t window,
                               uint32_t first_read, uint32_t nreads_block, uint32_t* nkmers, uint64_t* ntuples, uint64_t* ndistinct);

/* ---- measurement --------------------------------------------------------------------------------- */
int bella_hip_get_timings(bella_ctx* ctx, bella_timings* t);
/* Device memory the context holds right now, by role (multi-GPU: what is replicated and what follows the partition). */
typedef struct {
    uint64_t reads_bytes;      /* packed reads + offsets: replicated                                                     */
    uint64_t matrix_bytes;     /* B in the reference's layout (colptr / rowids / values): what the all-gather delivers     */
    uint64_t layout_A_bytes;   /* A' (k-mer -> reads lists): whole on every context                                        */
    uint64_t layout_B_bytes;   /* B' entries + the rows' product counts + row pointers: owned columns only                 */
    uint64_t rowlist_bytes;    /* row lists (BELLA_TUNE_ROW_LISTS) + row pointers: owned columns only                      */
    uint64_t pass_bytes;       /* buffers of the passes (records, product lists, workspaces): follow the pass's products   */
    uint64_t other_bytes;      /* counting / assembly / alignment buffers still held, and released ones kept for reuse      */
    uint64_t owned_nnz;        /* nnz of the owned columns (B' keeps those of them that have a later read: BELLA_TUNE_COMPACT_B) */
    uint64_t layout_shared;    /* 1: the current layout was formed shared over the ranks (BELLA_TUNE_DIST_LAYOUT), else 0  */
    uint64_t live_nnz;         /* B' entries the layout holds: those of the owned columns that have a later read (ABI 6)  */
} bella_memory;
int bella_hip_get_memory(bella_ctx* ctx, bella_memory* m);
/* the same, writing at most struct_size bytes (pass sizeof(bella_memory) of the header the caller was built against: the struct has
 * grown between ABI versions -- 64 bytes in version 4, 72 in 5, 80 in 6 -- and will again) */
int bella_hip_get_memory_sized(bella_ctx* ctx, void* m, uint64_t struct_size);
/* 0 = default; bit0 = force the global-memory row path (tests); bit1 = no pair_ext output; bit2 = tests: treat every fifth
 * column as if its product lists had come out of order (the LDS tiers verify the order and fall back to the repairing path);
 * bit3 = tests: 512-thread workgroups in every LDS class (default: 1024 threads where a CU holds one or two columns);
 * bit4 = tests: key tables of cap/2 slots (the layout of pair-rich inputs) on any input; bit5 = tests: every column above the
 * LDS tiers takes the sort-based path of the wide columns (default: from 16 such columns in a pass on); bit6 = tests: that path
 * sorts on 64-bit keys on any input (default: 32-bit keys when column bits + read-id bits fit); bit8 = tests: the exact X-drop mode
 * launches its extensions in chunks of 1,000 (default 2^24: grid x block stays below 2^32 threads); bit10 (read when the operands are
 * assembled) = tests: the lists of A' in order of first appearance in B' (default: k-mer order), no row lists; bit11 (same moment) =
 * tests: as if the row lists BELLA_TUNE_ROW_LISTS asks for, and the per-product B' of BELLA_TUNE_PRODUCT_ENTRIES, did not fit in memory
 * (the layout stands without them);
 * bit12 = tests: the columns above the LDS tiers are grouped by the radix sort also when the row lists would allow grouping in LDS;
 * bit13 = tests: the symbolic phase (bella_hip_count_pairs) keeps its bitmaps in global memory also when they fit in LDS;
 * bit14 = tests: k-mer counting looks every position up in a hash table over the dictionary (the path of syncmer mode, of k-mers too
 * long to share a 64-bit sort key with their position, and of the distributed count) also where the sorted words carry their positions;
 * bit15 (read when the operands are assembled) = tests: every entry of B' in the plain form (default, when A' is larger than the last-level
 * cache: an entry whose k-mer has exactly one later read carries that read instead of an index into A'; the plain form is also that of
 * inputs with 2^30 reads or 2^31 nonzeros and more); bit16 (same moment) = tests: that inline form on inputs of any size;
 * bit18 = tests: inside bella_hip_allgather_panels this rank fails after the ranks agreed on the shared formation of A' and before its own
 * share begins (every rank must leave the call with an error, none may wait); bit19 = tests: bella_hip_graph_build reduces every vertex
 * on the global-memory path of the vertices whose neighbours do not fit the LDS table */
int bella_hip_set_debug(bella_ctx* ctx, uint32_t flags);
/* Reserve device memory up front: ONE slab of `bytes` taken from the driver (and touched) now, from which the stages' buffers are cut
 * afterwards.  The reference has no counterpart (its vectors grow on the host); here the first hipMalloc of a multi-GB buffer costs
 * tens of ms per GB (the driver maps and wipes the pages), which a process that runs the pipeline should pay once, not inside its first
 * k-mer count, assembly and pass.  *ms (optional) = what the reservation took.  bytes == 0 gives an unused slab back.  What does not fit
 * the slab later is allocated as before; the slab goes with the context. */
int bella_hip_reserve(bella_ctx* ctx, uint64_t bytes, double* ms);
/* Device buffers of >= 128 MB that a stage released stay with the context for the next stage that fits them (a hipMalloc right after a
 * hipFree of tens of GB waits for the driver to wipe the pages); they are counted as free wherever the library sizes something by free
 * memory and are given up when one of its own allocations fails.  bella_hip_trim gives them back to the driver NOW: for hosts whose
 * other allocators (another context, RCCL, a framework) need the memory. */
int bella_hip_trim(bella_ctx* ctx);
/* Per-context tuning parameters (tests and A/B measurements; nothing here changes results).  what:
 *   BELLA_TUNE_LDS_TIERS      values = ascending product capacities of the row kernels' LDS tiers, each in [64, 11008] (n = 0: defaults)
 *   BELLA_TUNE_KCOUNT_BUDGET  values[0] = k-mers per pass of the counting sort (default 2^30)
 *   BELLA_TUNE_WIDE_BUDGET    values[0] = products per batch of the sort-based path of the wide columns (default 2^30)
 *   BELLA_TUNE_XDROP_VARIANT  values[0] = 0 one launch in length-sorted order, 1 (default; n = 0) slices of 512 steps with compaction of
 *                             the live extensions between launches, 2 packed kernel in pair order, 3 the scalar statement of xavier.h.
 *                             Same results in every variant.
 *   BELLA_TUNE_ROW_LISTS      values[0] = 1: operands installed from now on also get ROW LISTS -- the two operand entries of every product
 *                             of the owned columns side by side in product order (10 bytes per product, written once at assembly time)
 *                             -- when they fit next to what a pass needs; the numeric phase then streams its products instead of
 *                             expanding B' x A'.  For callers that run SEVERAL passes over the same columns (parameter sweeps): the
 *                             expansion is paid once instead of per pass.  Default 0 (n = 0): a one-shot call is faster without them
 *                             (layout + first pass); bella_timings.expand_ms reports the expansion when they are built.
 *   BELLA_TUNE_XDROP_CLASS_MIN values[0] = extensions of a batch from which on the slices of variant 1 run the batch as four classes by step
 *                             estimate, the three classes of long extensions on streams of their own at a higher priority (default 2^20:
 *                             four times the wavefronts the device holds at once; tests set it low, UINT64_MAX = never)
 *   BELLA_TUNE_LAYOUT_ORDER   values[0] = 0 (default): the lists of A' in k-mer order; 1: in order of first appearance in B' (the owner row of a
 *                             list streams it; three more random-access passes at layout time).  Read when operands are installed.
 *   BELLA_TUNE_INLINE_ENTRIES values[0] = 0 (default): an entry of B' whose k-mer has exactly one later read carries that read (util.hpp)
 *                             when A' is larger than BELLA_TUNE_CACHE_BYTES; 1: never (plain entries); 2: always.  Read at layout time.
 *   BELLA_TUNE_ROW_PATH       values[0] = 0 (default): columns in the LDS tiers; 1: every column on the global-workspace path (the
 *                             repairing path a device that fails the lane-order self-test gets)
 *   BELLA_TUNE_CACHE_BYTES    values[0] = size of A' from which on it counts as larger than the last-level cache (default 192 MB: three
 *                             quarters of the 256 MB Infinity Cache of an MI355X; the HIP runtime does not report that cache)
 *   BELLA_TUNE_DIST_LAYOUT    values[0] = 0: bella_hip_allgather_panels forms A' on every rank (each sorts ALL entries by k-mer).  1: the
 *                             formation is SHARED over the ranks of the communicator (2 = default: shared on the in-process transport, where
 *                             it is measured; replicated over RCCL until a run on several devices has shown the win) -- rank g sorts the entries whose k-mer id lies in the
 *                             g-th N-th of the id space, emits its slice of A' and the B' entries of all rows for those k-mers; slices and
 *                             entries travel in one more grouped exchange.  The same layout entry for entry.  Taken when EVERY rank can: the
 *                             partition (first, stride) = (rank, ranks) set by bella_hip_set_partition before the call, at most 64 ranks,
 *                             BELLA_TUNE_LAYOUT_ORDER 0 (the call asks all ranks and falls back to the replicated formation on all of them).
 *   BELLA_TUNE_COMPACT_B      values[0] = 0 (default): the device layout drops the entries of B' whose k-mer has no later read (they have
 *                             no product in the strict lower triangle, overlap.hpp:157-202); 1: every entry stays.  Read at layout time.
 *   BELLA_TUNE_PRODUCT_ENTRIES values[0] = 0 (default): the compacting layout writes B' with one entry per PRODUCT (a plain entry with c
 *                             later reads becomes c entries of count 1 pointing at consecutive places of its list in A'; row i of B' is then
 *                             the product list of column i and the LDS-tier row kernels skip the expansion) when the row lists are not
 *                             asked for, A' is larger than BELLA_TUNE_CACHE_BYTES, the products fit 32-bit row pointers and 8 bytes per product stay within 12 bytes per owned
 *                             nonzero; 1: never (one entry per live nonzero); 2: whenever the compaction runs and the products fit.  If
 *                             the buffer cannot be had (bella_hip_set_debug bit 11: tests, as if) the per-entry layout stands.
 *                             BELLA_TUNE_COMPACT_B 1 implies the per-entry form.  Read at layout time.
 *   BELLA_TUNE_ORDER_SPLIT    values[0] = owned columns of a pass above which the slot-order pass runs as TWO launches, one per table
 *                             size class (order.hpp), instead of one launch for all tables of up to 1,024 slots (default, n = 0: 32,768;
 *                             0: always two launches -- tests run both instances on small inputs).  Read by every pass.
 *   BELLA_TUNE_ROUND_BUDGET   values[0] = direction bytes of one batch of a realignment or correction round, taken as given (no 64 MB
 *                             floor; a batch always takes at least one job, so 1 means one job per batch -- tests run many batches on
 *                             small inputs).  Default (n = 0 or 0): half of the free device memory, 64 MB .. 8 GB.  Read at the start of
 *                             each round.  The trace's budget is not touched.  bella_hip_graph_align_links and bella_hip_align_sequences
 *                             batch by it too; in the latter a pair whose own direction bytes exceed it is TOO_LARGE.
 *   BELLA_TUNE_XDROP_BATCH    values[0] = extensions (two per pair) of one batch of the sliced X-drop kernels (variant 1, and variant 0's
 *                             fall-back), taken as given: neither the free-memory rule nor the floor of 65,536 extensions applies -- tests
 *                             run several batches, full and partial, on small inputs.  Default (n = 0 or 0): at most 16 M extensions, at
 *                             most a quarter of the free device memory, at least 65,536.  Read by every call.
 * (bella_hip_set_debug bits 0, 10, 15 and 16 of earlier rounds still select the same things: aliases, no longer needed)
 */
enum { BELLA_TUNE_LDS_TIERS = 0, BELLA_TUNE_KCOUNT_BUDGET = 1, BELLA_TUNE_WIDE_BUDGET = 2, BELLA_TUNE_XDROP_VARIANT = 3, BELLA_TUNE_ROW_LISTS = 4,
       BELLA_TUNE_XDROP_CLASS_MIN = 5, BELLA_TUNE_LAYOUT_ORDER = 6, BELLA_TUNE_INLINE_ENTRIES = 7, BELLA_TUNE_ROW_PATH = 8, BELLA_TUNE_CACHE_BYTES = 9, BELLA_TUNE_DIST_LAYOUT = 10, BELLA_TUNE_COMPACT_B = 11,
       BELLA_TUNE_PRODUCT_ENTRIES = 12, BELLA_TUNE_ORDER_SPLIT = 13, BELLA_TUNE_ROUND_BUDGET = 14, BELLA_TUNE_XDROP_BATCH = 15 };
int bella_hip_set_tuning(bella_ctx* ctx, uint32_t what, const uint64_t* values, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* BELLA_HIP_H */
