// bella_hip_main.cpp -> bella_amd/bin/bella-hip: BELLA's command line with the WHOLE pipeline on the MI355X.
//
// The flags, the output file and the stdout protocol are those of the reference's src/main.cpp (:65-175 options, :130 output name,
// :472-473 nkmer, src/CSC.cpp:405 nnz(A), include/overlap.hpp:686 nnz(C), :771 lines written, main.cpp:532 run time); nothing of the
// reference runs: FASTQ list -> bella_hip_load_fastq_list (replaces ParallelFASTQ, main.cpp:339-360) -> bella_hip_count_kmers /
// _syncmers / _minimizers (SplitCount / SyncmerCount / MinimizerCount, include/kmercount.hpp:467-986, and the tuple loop,
// main.cpp:363-416) -> bella_hip_assemble_counted (CSC constructor + Transpose, main.cpp:476-489) -> the stage plan, HashSpGEMM,
// RunPairWiseAlignments and the writer of include/overlap.hpp:650-789 (bella_hip_driver.hpp).  One host thread and one context per
// GPU (-g): reads replicated, the dictionary counted across the contexts, B assembled by row blocks and exchanged device to device,
// output columns i % N == g per context.
//
// K-mer ids are labels: the reference numbers the reliable k-mers in libcuckoo's iteration order, this program in ascending order of
// the canonical word.  The ids decide the order of a column's products and through it the order of the output lines and, for pairs
// with several shared k-mers, count / seed (the reference's own output changes the same way with its thread
// count).  --tuples FILE takes the reference's `readbykmers.mtx` dump (include/common/bellaio.h:2-47: "nreads nkmers ntuples", then
// "read+1 kmer+1 pos" per line) instead of counting: same ids as that reference run, same output file byte for byte.
//
// --paf --cigar: true PAF: every stage traces its passed pairs on the device before it writes them.
// --correct FILE: read correction: every stage's traced pairs vote into a per-read pileup on the device, the
// consensus of every read goes to FILE as FASTA after the last stage; the main output file is what it is without the option.
// --correct-rounds N: N - 1 correction rounds follow the consensus, each aligning the raw partners of every traced
// pair against the corrected reads of the round before; FILE then holds the last round.
//
// --normalize-gaps: with --correct / --polish, every gap run votes at its canonical position.
// --clip-ends: every traced alignment of the run is cut to its maximum-scoring segment at --clip-identity
// permille before anything reads it (records, pileup votes, the true PAF); the -o file does not change.
// --polish: unitig consensus: every stage's traced pairs vote as with --correct, the unitigs are polished from
// the pileup on the device after the last stage; --unitigs / --unitigs-fasta then carry the polished sequences and coordinates.
// --polish-rounds N: N - 1 realignment rounds follow, each aligning the reads against the unitigs of the round before.
// --realign-circular: those rounds place the reads of a circular unitig on the unrolled circle, across its origin too.
// --align-links: the ends of the two unitigs of every link are aligned against each other on the device, on the
// sequences the --unitigs file carries; an aligned link's L line takes the CIGAR of that alignment, NM:i: and ol:i: (the raw overlap).
//
// --trim: coverage trimming: after the last stage every read is clipped, on the device, to its longest stretch that
// --trim-depth overlap records cover; the graph is built from the records cut to the clips, and --gfa / --unitigs / --unitigs-fasta are in
// clipped coordinates; --trimmed-reads FILE: the clipped reads as FASTA.
//
// Not built (rejected loudly): --hopc, --estimate, --split-count > 1.
#include <sys/stat.h>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "bella_hip.h"
#include "bella_hip_driver.hpp"

namespace {

struct Options {
    std::string fastq_list, output, tuples, correct, gfa, unitigs, unitigs_fasta;
    int kmer = 17, xdrop = 7, memory = 8000, bin_size = 500, gpus = 1, split_count = 1, window = 0, upper = 8, lower = 2;
    double error = 0.15, deviation = 0.1;
    bool estimate = false, skip_alignment = false, paf = false, hopc = false, syncmer = false, help = false, exact = false, cigar = false;
    int trace_band = 0, min_depth = 3;
    bool min_depth_given = false;
    int correct_rounds = 1, correct_band = 512, correct_min_identity = 700;
    bool correct_param_given = false;
    int gfa_fuzz = 1000, gfa_max_overhang = 1000, gfa_min_overlap = 1000;
    bool gfa_no_seq = false, gfa_param_given = false;
    int tip_reads = 4, tip_rounds = 3;
    bool gfa_clean = false, tip_param_given = false;
    int bubble_reads = 64, bubble_dist = 50000, bubble_rounds = 3;
    bool pop_bubbles = false, bubble_param_given = false;
    int polish_min_depth = 3;
    bool polish = false, polish_param_given = false;
    int polish_rounds = 1, realign_band = 512, realign_min_identity = 700;
    bool realign_param_given = false, realign_circular = false;
    int link_band = 512, link_min_identity = 700;
    bool align_links = false, link_param_given = false;
    int trim_depth = 3, trim_end_clip = 500;
    std::string trimmed_reads;
    bool trim = false, trim_param_given = false;
    int weak_min = 500, weak_max = 700, weak_steps = 2;
    bool cut_weak = false, weak_param_given = false;
    bool normalize_gaps = false;
    bool clip_ends = false, clip_param_given = false;
    int clip_identity = BELLA_CLIP_DEFAULT_IDENTITY;
    bool graph() const { return !gfa.empty() || !unitigs.empty() || !unitigs_fasta.empty(); }
};

const char* kHelp =
    "Long Read to Long Read Aligner and Overlapper (MI355X)\n"
    "Usage:\n"
    "  bella-hip [OPTION...]\n\n"
    "  -f, --fastq arg            List of Fastq(s) (required)\n"
    "  -o, --output arg           Output Filename (required)\n"
    "  -k, --kmer arg             K-mer Length (default: 17)\n"
    "  -x, --xdrop arg            X-Drop (default: 7)\n"
    "  -e, --error arg            Error Rate (default: 0.15)\n"
    "      --estimate             Estimate Error Rate from Data (not built)\n"
    "      --skip-alignment       Overlap Only\n"
    "  -m, --memory arg           Total RAM of the System in MB (default: 8000)\n"
    "      --score-deviation arg  Deviation from the Mean Alignment Score [0,1] (default: 0.1)\n"
    "  -b, --bin-size arg         Bin Size for Binning Algorithm (default: 500)\n"
    "      --paf                  Output in PAF format\n"
    "  -g, --gpus arg             GPUs Available (default: 1)\n"
    "      --split-count arg      K-mer Counting Split Count (only 1)\n"
    "      --hopc                 Use HOPC representation (not built)\n"
    "  -w, --window arg           Window Size for Minimizer Selection (default: 0)\n"
    "  -s, --syncmer              Enable Syncmer Selection\n"
    "  -u, --upper-freq arg       K-mer Frequency Upper Bound (default: 8)\n"
    "  -l, --lower-freq arg       K-mer Frequency Lower Bound (default: 2)\n"
    "      --tuples arg           readbykmers.mtx of a reference run: its k-mer ids instead of counting\n"
    "      --exact-xdrop          the exact (growing band) X-drop of the reference's GPU build instead of Xavier\n"
    "      --cigar                with --paf: true PAF -- base-level alignment of every line (residue matches, block length, NM, cg:Z:)\n"
    "      --trace-band arg       first band of the base-level alignments, in diagonals (default: 256; doubled where a path touches it)\n"
    "      --correct arg          corrected reads (FASTA): per-read pileup of the base-level alignments on the device, majority consensus\n"
    "      --min-depth arg        with --correct: votes a position needs before it is changed (default: 3)\n"
    "      --correct-rounds arg   with --correct: correction rounds (default: 1; at most 4); every round after the first aligns the raw partners of every\n"
    "                             overlap against the corrected reads of the round before, on the device, and takes the consensus of those alignments\n"
    "      --correct-band arg     with --correct: the first band of those alignments, a power of two from 256 to 4096 (default: 512)\n"
    "      --correct-min-identity arg  with --correct: permille of matches below which an alignment does not vote (default: 700)\n"
    "      --normalize-gaps       with --correct / --polish: every gap of the base-level alignments votes at a canonical position (moved towards the start\n"
    "                             of the read it votes on, inside the neighbouring run of matches), so equal indels seen from either side add up\n"
    "      --clip-ends            with an option that traces (--cigar, --correct, --gfa, --unitigs, --unitigs-fasta, --polish): every base-level alignment is\n"
    "                             cut to its maximum-scoring segment under an identity threshold, so junk ends and chimeric halves leave the records and votes\n"
    "      --clip-identity arg    with --clip-ends: that threshold in permille, 1 to 999 (default: 650)\n"
    "      --gfa arg              string graph (GFA 1): overlap classes, contained reads dropped, transitive reduction, on the device\n"
    "      --gfa-min-overlap arg  with --gfa: shortest overlap that counts (default: 1000)\n"
    "      --gfa-max-overhang arg with --gfa: longest unaligned end of a dovetail or containment (default: 1000)\n"
    "      --gfa-fuzz arg         with --gfa: slack of the transitive reduction, in bases (default: 1000)\n"
    "      --gfa-no-seq           with --gfa / --unitigs: '*' instead of the bases in the S lines\n"
    "      --unitigs arg          unitigs of the string graph (GFA 1: S, a and L lines): tips clipped, maximal non-branching paths compacted, on the device\n"
    "      --unitigs-fasta arg    the unitigs' sequences (FASTA); both build the graph (the --gfa-* parameters apply), --gfa is not required\n"
    "      --tip-reads arg        with --unitigs / --unitigs-fasta / --gfa-clean: longest tip that is clipped, in reads (default: 4; 0: no clipping)\n"
    "      --tip-rounds arg       ... and the number of clipping rounds (default: 3)\n"
    "      --gfa-clean            with --gfa: the file shows the graph after tip clipping (and bubble popping)\n"
    "      --pop-bubbles          with --unitigs / --unitigs-fasta / --gfa-clean: pop bubbles after the tip clipping, on the device\n"
    "      --bubble-reads arg     with --pop-bubbles: largest bubble that is popped, in reads (default: 64; at most 255; 0: no popping)\n"
    "      --bubble-dist arg      ... its largest distance from the source, in bases (default: 50000)\n"
    "      --bubble-rounds arg    ... and the number of popping rounds (default: 3)\n"
    "      --cut-weak             with --unitigs / --unitigs-fasta / --gfa-clean: remove weak overlaps after the tip clipping and the bubble popping, on the device:\n"
    "                             an edge goes when its overlap is below a fraction of the best overlap of its vertex; tips and bubbles again after every cut\n"
    "      --weak-min arg         with --cut-weak: the fraction of the first cut, in permille (default: 500)\n"
    "      --weak-max arg         ... the fraction of the last cut (default: 700)\n"
    "      --weak-steps arg       ... and the steps from the first to the last: steps + 1 cuts (default: 2; at most 16)\n"
    "      --polish               with --unitigs / --unitigs-fasta: unitig consensus from the pileup of the base-level alignments, on the device\n"
    "      --polish-min-depth arg with --polish: votes a position needs before it is changed (default: 3)\n"
    "      --polish-rounds arg    with --polish: consensus rounds (default: 1; at most 4); every round after the first aligns the reads against the\n"
    "                             unitigs of the round before, on the device, and takes the consensus of those alignments\n"
    "      --realign-band arg     with --polish: the first band of those alignments, a power of two from 256 to 4096 (default: 512)\n"
    "      --realign-min-identity arg  with --polish: permille of matches below which a read's alignment does not vote (default: 700)\n"
    "      --realign-circular     with --polish: those alignments treat a circular unitig as a circle, so the reads across its origin vote too\n"
    "      --align-links          with --unitigs: align the ends of the two unitigs of every link against each other, on the device; an aligned link's L line\n"
    "                             carries the CIGAR of that alignment (M / I / D, `from` is the reference), NM:i: and ol:i:, the overlap the graph had\n"
    "      --link-band arg        with --align-links: the first band of those alignments, a power of two from 256 to 4096 (default: 512)\n"
    "      --link-min-identity arg  with --align-links: permille of matches below which a link keeps its <ovl>M line (default: 700)\n"
    "      --trim                 with --gfa / --unitigs / --unitigs-fasta: clip every read to its longest stretch that --trim-depth overlaps cover, on the\n"
    "                             device, before the graph is built (shortest stretch: --gfa-min-overlap); the graph files are in clipped coordinates\n"
    "      --trim-depth arg       with --trim: overlaps a position needs to count as covered (default: 3)\n"
    "      --trim-end-clip arg    with --trim: bases an overlap's inner ends are shortened by before it is counted (default: 500)\n"
    "      --trimmed-reads arg    with --trim: the clipped reads (FASTA), in input order, without the uncovered ones\n"
    "  -h, --help                 Usage\n";

[[noreturn]] void die(const std::string& msg) {
    std::cerr << "bella-hip: " << msg << std::endl;
    std::exit(1);
}

// cxxopts' forms (the reference's parser): --name value, --name=value, -n value, -nvalue; booleans take no value
Options parse(int argc, char** argv) {
    Options o;
    struct Spec { const char* lng; char sht; int kind; void* dst; };   // kind 0 bool, 1 int, 2 double, 3 string
    const Spec specs[] = {
        {"fastq", 'f', 3, &o.fastq_list}, {"output", 'o', 3, &o.output}, {"kmer", 'k', 1, &o.kmer}, {"xdrop", 'x', 1, &o.xdrop},
        {"error", 'e', 2, &o.error}, {"estimate", 0, 0, &o.estimate}, {"skip-alignment", 0, 0, &o.skip_alignment}, {"memory", 'm', 1, &o.memory},
        {"score-deviation", 0, 2, &o.deviation}, {"bin-size", 'b', 1, &o.bin_size}, {"paf", 0, 0, &o.paf}, {"gpus", 'g', 1, &o.gpus},
        {"split-count", 0, 1, &o.split_count}, {"hopc", 0, 0, &o.hopc}, {"window", 'w', 1, &o.window}, {"syncmer", 's', 0, &o.syncmer},
        {"upper-freq", 'u', 1, &o.upper}, {"lower-freq", 'l', 1, &o.lower}, {"tuples", 0, 3, &o.tuples}, {"exact-xdrop", 0, 0, &o.exact}, {"cigar", 0, 0, &o.cigar}, {"trace-band", 0, 1, &o.trace_band},
        {"correct", 0, 3, &o.correct}, {"min-depth", 0, 1, &o.min_depth},
        {"correct-rounds", 0, 1, &o.correct_rounds}, {"correct-band", 0, 1, &o.correct_band}, {"correct-min-identity", 0, 1, &o.correct_min_identity},
        {"normalize-gaps", 0, 0, &o.normalize_gaps}, {"clip-ends", 0, 0, &o.clip_ends}, {"clip-identity", 0, 1, &o.clip_identity},
        {"gfa", 0, 3, &o.gfa}, {"gfa-fuzz", 0, 1, &o.gfa_fuzz}, {"gfa-max-overhang", 0, 1, &o.gfa_max_overhang}, {"gfa-min-overlap", 0, 1, &o.gfa_min_overlap},
        {"gfa-no-seq", 0, 0, &o.gfa_no_seq},
        {"unitigs", 0, 3, &o.unitigs}, {"unitigs-fasta", 0, 3, &o.unitigs_fasta}, {"tip-reads", 0, 1, &o.tip_reads}, {"tip-rounds", 0, 1, &o.tip_rounds}, {"gfa-clean", 0, 0, &o.gfa_clean},
        {"pop-bubbles", 0, 0, &o.pop_bubbles}, {"bubble-reads", 0, 1, &o.bubble_reads}, {"bubble-dist", 0, 1, &o.bubble_dist}, {"bubble-rounds", 0, 1, &o.bubble_rounds},
        {"cut-weak", 0, 0, &o.cut_weak}, {"weak-min", 0, 1, &o.weak_min}, {"weak-max", 0, 1, &o.weak_max}, {"weak-steps", 0, 1, &o.weak_steps},
        {"polish", 0, 0, &o.polish}, {"polish-min-depth", 0, 1, &o.polish_min_depth},
        {"polish-rounds", 0, 1, &o.polish_rounds}, {"realign-band", 0, 1, &o.realign_band}, {"realign-min-identity", 0, 1, &o.realign_min_identity},
        {"realign-circular", 0, 0, &o.realign_circular},
        {"align-links", 0, 0, &o.align_links}, {"link-band", 0, 1, &o.link_band}, {"link-min-identity", 0, 1, &o.link_min_identity},
        {"trim", 0, 0, &o.trim}, {"trim-depth", 0, 1, &o.trim_depth}, {"trim-end-clip", 0, 1, &o.trim_end_clip}, {"trimmed-reads", 0, 3, &o.trimmed_reads},
        {"help", 'h', 0, &o.help}};
    auto assign = [&](const Spec& s, const char* v, const std::string& shown) {
        char* end = nullptr;
        if (s.kind == 1) { const long x = std::strtol(v, &end, 10); if (!*v || *end) die("option " + shown + ": '" + v + "' is not an integer"); *(int*)s.dst = (int)x; }
        else if (s.kind == 2) { const double x = std::strtod(v, &end); if (!*v || *end) die("option " + shown + ": '" + v + "' is not a number"); *(double*)s.dst = x; }
        else *(std::string*)s.dst = v;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const Spec* sp = nullptr;
        const char* val = nullptr;
        std::string holder;
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') {
            const size_t eq = a.find('=');
            const std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            for (const Spec& s : specs) if (name == s.lng) sp = &s;
            if (!sp) die("option '" + a + "' does not exist");
            if (eq != std::string::npos) { holder = a.substr(eq + 1); val = holder.c_str(); }
        } else if (a.size() >= 2 && a[0] == '-') {
            for (const Spec& s : specs) if (s.sht && a[1] == s.sht) sp = &s;
            if (!sp) die("option '" + a + "' does not exist");
            if (a.size() > 2) { holder = a.substr(2); val = holder.c_str(); }
        } else die("unexpected argument '" + a + "'");
        if (sp->kind == 0) {
            if (val) die("option " + a + " takes no value");
            *(bool*)sp->dst = true;
            if (sp->dst == &o.gfa_no_seq) o.gfa_param_given = true;
            if (sp->dst == &o.realign_circular) o.realign_param_given = true;
            continue;
        }
        if (!val) {
            if (i + 1 >= argc) die("option " + a + " is missing an argument");
            val = argv[++i];
        }
        assign(*sp, val, a);
        if (sp->dst == &o.min_depth) o.min_depth_given = true;
        if (sp->dst == &o.correct_rounds || sp->dst == &o.correct_band || sp->dst == &o.correct_min_identity) o.correct_param_given = true;
        if (sp->dst == &o.gfa_fuzz || sp->dst == &o.gfa_max_overhang || sp->dst == &o.gfa_min_overlap) o.gfa_param_given = true;
        if (sp->dst == &o.tip_reads || sp->dst == &o.tip_rounds) o.tip_param_given = true;
        if (sp->dst == &o.bubble_reads || sp->dst == &o.bubble_dist || sp->dst == &o.bubble_rounds) o.bubble_param_given = true;
        if (sp->dst == &o.weak_min || sp->dst == &o.weak_max || sp->dst == &o.weak_steps) o.weak_param_given = true;
        if (sp->dst == &o.polish_min_depth) o.polish_param_given = true;
        if (sp->dst == &o.polish_rounds || sp->dst == &o.realign_band || sp->dst == &o.realign_min_identity) o.realign_param_given = true;
        if (sp->dst == &o.link_band || sp->dst == &o.link_min_identity) o.link_param_given = true;
        if (sp->dst == &o.trim_depth || sp->dst == &o.trim_end_clip || sp->dst == &o.trimmed_reads) o.trim_param_given = true;
        if (sp->dst == &o.clip_identity) o.clip_param_given = true;
    }
    return o;
}

// GetFiles (include/kmercount.hpp:82-105): one path per line; a last line without '\n' is not read by the reference either
std::vector<std::string> read_list(const std::string& path) {
    std::ifstream f(path);
    if (!f.is_open()) die("Could not open " + path);
    std::vector<std::string> out;
    std::string line;
    while (std::getline(f, line)) {
        if (f.eof()) break;                                         // (no trailing newline: getline hit the end of the file in this line)
        if (!line.empty()) out.push_back(line);
    }
    return out;
}

struct MtxTuples { uint32_t nreads = 0, nkmers = 0; std::vector<uint32_t> kmer, read; std::vector<uint16_t> pos; };
MtxTuples read_mtx(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) die("Could not open " + path);
    MtxTuples t;
    unsigned long long nr = 0, nk = 0, nt = 0;
    if (std::fscanf(f, "%llu %llu %llu", &nr, &nk, &nt) != 3) die(path + ": not a readbykmers.mtx (header: nreads nkmers ntuples)");
    t.nreads = (uint32_t)nr; t.nkmers = (uint32_t)nk;
    t.kmer.reserve(nt); t.read.reserve(nt); t.pos.reserve(nt);
    unsigned long long r = 0, k = 0, p = 0;
    while (std::fscanf(f, "%llu %llu %llu", &r, &k, &p) == 3) {
        if (!r || !k || r > nr || k > nk || p > 65535) die(path + ": tuple out of range");
        t.read.push_back((uint32_t)(r - 1)); t.kmer.push_back((uint32_t)(k - 1)); t.pos.push_back((uint16_t)p);
    }
    std::fclose(f);
    if (t.kmer.size() != nt) die(path + ": " + std::to_string(t.kmer.size()) + " tuples, header says " + std::to_string(nt));
    for (size_t i = 1; i < t.read.size(); ++i)
        if (t.read[i] < t.read[i - 1]) die(path + ": tuples must be grouped by non-decreasing read (the reference's 1-thread dump is)");
    return t;
}

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

int main(int argc, char** argv) {
    using namespace bella_hip_detail;
    const Options o = parse(argc, argv);
    if (o.help || o.fastq_list.empty() || o.output.empty()) { std::cout << kHelp << std::endl; return 0; }     // main.cpp:97-145
    if (o.deviation > 1.0 || o.deviation < 0.0) { std::cout << kHelp << std::endl; return 0; }                 // main.cpp:159-163
    if (o.hopc) die("--hopc is not built (the HOPC representation, include/kmercount.hpp: outside this engine's parity contract)");
    if (o.estimate) die("--estimate is not built (error-rate estimation from the quality strings): pass -e");
    if (o.split_count != 1) die("--split-count > 1 is not built: the device counter takes the whole k-mer space in one call (or in passes of its own)");
    if (o.cigar && !o.paf) die("--cigar needs --paf (the base-level alignment is written as PAF columns 10-11 and the cg:Z: tag)");
    if (o.cigar && o.skip_alignment) die("--cigar cannot be combined with --skip-alignment (there is no alignment to trace)");
    if (o.trace_band < 0 || o.trace_band > (1 << 18)) die("--trace-band must be in [0, 262144]");
    if (o.trace_band && !o.cigar && o.correct.empty() && !o.graph()) die("--trace-band needs --cigar, --correct, --gfa, --unitigs or --unitigs-fasta");
    if (o.graph() && o.skip_alignment) die("--gfa, --unitigs and --unitigs-fasta cannot be combined with --skip-alignment (the graph is made of base-level alignments)");
    if (o.gfa_param_given && !o.graph()) die("--gfa-fuzz, --gfa-max-overhang, --gfa-min-overlap and --gfa-no-seq need --gfa or --unitigs or --unitigs-fasta");
    if (o.gfa_clean && o.gfa.empty()) die("--gfa-clean needs --gfa");
    if (o.tip_param_given && o.unitigs.empty() && o.unitigs_fasta.empty() && !o.gfa_clean) die("--tip-reads and --tip-rounds need --unitigs, --unitigs-fasta or --gfa-clean");
    if (o.tip_reads < 0 || o.tip_rounds < 0 || o.tip_rounds > BELLA_MAX_TIP_ROUNDS) die("--tip-reads must not be negative and --tip-rounds must be in [0, " + std::to_string(BELLA_MAX_TIP_ROUNDS) + "]");
    if (o.bubble_param_given && !o.pop_bubbles) die("--bubble-reads, --bubble-dist and --bubble-rounds need --pop-bubbles");
    if (o.pop_bubbles && o.unitigs.empty() && o.unitigs_fasta.empty() && !o.gfa_clean) die("--pop-bubbles needs --unitigs, --unitigs-fasta or --gfa-clean");
    if (o.bubble_reads < 0 || o.bubble_reads > BELLA_MAX_BUBBLE_READS || o.bubble_dist < 0 || o.bubble_rounds < 0 || o.bubble_rounds > BELLA_MAX_BUBBLE_ROUNDS)
        die("--bubble-reads must be in [0, " + std::to_string(BELLA_MAX_BUBBLE_READS) + "], --bubble-dist must not be negative and --bubble-rounds must be in [0, " +
            std::to_string(BELLA_MAX_BUBBLE_ROUNDS) + "]");
    if (o.weak_param_given && !o.cut_weak) die("--weak-min, --weak-max and --weak-steps need --cut-weak");
    if (o.cut_weak && o.unitigs.empty() && o.unitigs_fasta.empty() && !o.gfa_clean) die("--cut-weak needs --unitigs, --unitigs-fasta or --gfa-clean");
    if (o.weak_min <= 0 || o.weak_min > o.weak_max || o.weak_max > 1000 || o.weak_steps < 0 || o.weak_steps > 16)
        die("--weak-min and --weak-max must be in [1, 1000] with --weak-min not above --weak-max, and --weak-steps must be in [0, 16]");
    if (o.polish_param_given && !o.polish) die("--polish-min-depth needs --polish");
    if (o.polish && o.unitigs.empty() && o.unitigs_fasta.empty()) die("--polish needs --unitigs or --unitigs-fasta");
    if (o.polish && o.gfa_no_seq && o.unitigs_fasta.empty()) die("--polish with --gfa-no-seq needs --unitigs-fasta (there is no sequence to polish into)");
    if (o.polish && o.polish_min_depth < 1) die("--polish-min-depth must be at least 1");
    if (o.realign_circular && !o.polish) die("--realign-circular needs --polish");
    if (o.realign_param_given && !o.polish) die("--polish-rounds, --realign-band and --realign-min-identity need --polish");
    if (o.polish_rounds < 1 || o.polish_rounds > 4) die("--polish-rounds must be in [1, 4]");
    if (o.realign_band < 256 || o.realign_band > 4096 || (o.realign_band & (o.realign_band - 1))) die("--realign-band must be a power of two in [256, 4096]");
    if (o.realign_min_identity < 0 || o.realign_min_identity > 1000) die("--realign-min-identity is in permille: [0, 1000]");
    if (o.align_links && o.unitigs.empty()) die("--align-links needs --unitigs (the alignments go into the L lines of that file)");
    if (o.link_param_given && !o.align_links) die("--link-band and --link-min-identity need --align-links");
    if (o.link_band < 256 || o.link_band > 4096 || (o.link_band & (o.link_band - 1))) die("--link-band must be a power of two in [256, 4096]");
    if (o.link_min_identity < 0 || o.link_min_identity > 1000) die("--link-min-identity is in permille: [0, 1000]");
    if (o.trim_param_given && !o.trim) die("--trim-depth, --trim-end-clip and --trimmed-reads need --trim");
    if (o.trim && !o.graph()) die("--trim needs --gfa, --unitigs or --unitigs-fasta");
    if (o.trim && (o.trim_depth < 1 || o.trim_end_clip < 0)) die("--trim-depth must be at least 1 and --trim-end-clip must not be negative");
    if (o.gfa_fuzz < 0 || o.gfa_max_overhang < 0 || o.gfa_min_overlap < 0) die("--gfa-fuzz, --gfa-max-overhang and --gfa-min-overlap must not be negative");
    if (!o.correct.empty() && o.skip_alignment) die("--correct cannot be combined with --skip-alignment (the pileup is made of base-level alignments)");
    if (o.min_depth_given && o.min_depth < 1) die("--min-depth must be at least 1");
    if (o.min_depth_given && o.correct.empty()) die("--min-depth needs --correct");
    if (o.correct_param_given && o.correct.empty()) die("--correct-rounds, --correct-band and --correct-min-identity need --correct");
    if (o.correct_rounds < 1 || o.correct_rounds > 4) die("--correct-rounds must be in [1, 4]");
    if (o.correct_band < 256 || o.correct_band > 4096 || (o.correct_band & (o.correct_band - 1))) die("--correct-band must be a power of two in [256, 4096]");
    if (o.correct_min_identity < 0 || o.correct_min_identity > 1000) die("--correct-min-identity is in permille: [0, 1000]");
    if (o.normalize_gaps && o.correct.empty() && !o.polish) die("--normalize-gaps needs --correct or --polish (it changes where the gaps of the pileup vote)");
    if (o.clip_ends && !o.cigar && o.correct.empty() && !o.graph() && !o.polish)
        die("--clip-ends needs an option that traces: --cigar, --correct, --gfa, --unitigs, --unitigs-fasta or --polish (it clips the base-level alignments)");
    if (o.clip_param_given && !o.clip_ends) die("--clip-identity needs --clip-ends");
    if (o.clip_identity < 1 || o.clip_identity > 999) die("--clip-identity is in permille: [1, 999]");
    if (o.kmer < 1 || o.kmer > 32) die("-k must be in [1,32] (one 64-bit word per k-mer, Kmer.hpp:27-28)");
    const std::string outfile = o.output + ".out";                  // main.cpp:113-130
    std::remove(outfile.c_str());
    const char* const tag = "bella_hip_main.cpp";
    const double all = now_s();

    const std::vector<std::string> files = read_list(o.fastq_list);
    if (files.empty()) die("no FASTQ file in " + o.fastq_list + " (every line must end in a newline, kmercount.hpp:96)");
    uint64_t file_bytes = 0;
    for (const std::string& f : files) {
        struct stat st;
        if (stat(f.c_str(), &st) != 0) die("Could not open " + f);
        file_bytes += (uint64_t)st.st_size;
        const std::string InputFile = f;
        BELLA_HIP_LOGT(tag, InputFile);
    }
    const int ndev = bella_hip_device_count();
    if (ndev <= 0) check(nullptr, BELLA_ERR_NO_DEVICE, "bella_hip_device_count");
    int N = o.gpus > 1 ? o.gpus : 1;
    if (N > ndev && !std::getenv("BELLA_HIP_OVERSUBSCRIBE")) N = ndev;   // (tests on a one-GPU box: contexts share the device)
    const int GPUs = N;
    BELLA_HIP_LOGT(tag, GPUs);

    // selector of the k-mers that make tuples: syncmers win over minimizers as in main.cpp:170-176
    const bool use_sync = o.syncmer, use_min = !o.syncmer && o.window != 0;
    MtxTuples mtx;
    if (!o.tuples.empty()) mtx = read_mtx(o.tuples);

    std::vector<Worker> W((size_t)N);
    std::vector<const char*> cpaths;
    for (const std::string& f : files) cpaths.push_back(f.c_str());
    uint8_t comm_id[BELLA_HIP_COMM_ID_BYTES];
    if (N > 1) check(nullptr, bella_hip_comm_id_local(comm_id), "bella_hip_comm_id_local");
    std::vector<uint32_t> nk_of((size_t)N, 0), nreads_of((size_t)N, 0);
    std::vector<double> t_ingest((size_t)N, 0), t_count((size_t)N, 0), t_asm((size_t)N, 0), t_init((size_t)N, 0);
    on_all(N, [&](int g) {
        Worker& w = W[(size_t)g];
        double t0 = now_s();
        check(nullptr, bella_hip_init(g % ndev, &w.ctx), "bella_hip_init");
        reserve_for(w.ctx, file_bytes / 2, (N + ndev - 1) / ndev);   // (a FASTQ file is half bases, half qualities)
        if (const char* e = std::getenv("BELLA_HIP_KCOUNT_BUDGET")) {
            const uint64_t v = std::strtoull(e, nullptr, 10);
            check(w.ctx, bella_hip_set_tuning(w.ctx, BELLA_TUNE_KCOUNT_BUDGET, &v, 1), "bella_hip_set_tuning");
        }
        t_init[(size_t)g] = now_s() - t0;
        t0 = now_s();
        uint32_t nreads = 0;
        uint64_t nbases = 0;
        check(w.ctx, bella_hip_load_fastq_list(w.ctx, cpaths.data(), (uint32_t)cpaths.size(), &nreads, &nbases), "bella_hip_load_fastq_list");
        nreads_of[(size_t)g] = nreads;
        t_ingest[(size_t)g] = now_s() - t0;
        t0 = now_s();
        const uint32_t lo = (uint32_t)((uint64_t)nreads * (uint64_t)g / (uint64_t)N), hi = (uint32_t)((uint64_t)nreads * (uint64_t)(g + 1) / (uint64_t)N);
        uint32_t nk = 0;
        if (N > 1) {
            check(w.ctx, bella_hip_set_partition(w.ctx, (uint32_t)g, (uint32_t)N), "bella_hip_set_partition");
            check(w.ctx, bella_hip_comm_init_local(w.ctx, N, g, comm_id), "bella_hip_comm_init_local");
        }
        if (!o.tuples.empty()) {
            if (mtx.nreads != nreads) die("--tuples: the dump holds " + std::to_string(mtx.nreads) + " reads, the FASTQ list " + std::to_string(nreads));
            nk = mtx.nkmers;
            t_count[(size_t)g] = 0;
            t0 = now_s();
            if (N == 1) {
                check(w.ctx, bella_hip_assemble_tuples(w.ctx, (uint16_t)o.kmer, nk, mtx.kmer.size(), mtx.kmer.data(), mtx.read.data(), mtx.pos.data()), "bella_hip_assemble_tuples");
            } else {
                const size_t a = (size_t)(std::lower_bound(mtx.read.begin(), mtx.read.end(), lo) - mtx.read.begin());
                const size_t b = (size_t)(std::lower_bound(mtx.read.begin(), mtx.read.end(), hi) - mtx.read.begin());
                check(w.ctx, bella_hip_assemble_panel(w.ctx, (uint16_t)o.kmer, nk, lo, hi - lo, b - a, mtx.kmer.data() + a, mtx.read.data() + a, mtx.pos.data() + a), "bella_hip_assemble_panel");
                check(w.ctx, bella_hip_allgather_panels(w.ctx), "bella_hip_allgather_panels");
            }
        } else {
            uint64_t nt = 0, nd = 0;
            if (N > 1)
                check(w.ctx, bella_hip_count_kmers_dist(w.ctx, (uint16_t)o.kmer, (uint32_t)o.lower, (uint32_t)o.upper, use_sync ? 1u : use_min ? 2u : 0u,
                                                        (uint32_t)o.window, lo, hi - lo, &nk, &nt, &nd), "bella_hip_count_kmers_dist");
            else if (use_sync) check(w.ctx, bella_hip_count_syncmers(w.ctx, (uint16_t)o.kmer, (uint32_t)o.lower, (uint32_t)o.upper, &nk, &nt, &nd), "bella_hip_count_syncmers");
            else if (use_min) check(w.ctx, bella_hip_count_minimizers(w.ctx, (uint16_t)o.kmer, (uint32_t)o.window, (uint32_t)o.lower, (uint32_t)o.upper, &nk, &nt, &nd), "bella_hip_count_minimizers");
            else check(w.ctx, bella_hip_count_kmers(w.ctx, (uint16_t)o.kmer, (uint32_t)o.lower, (uint32_t)o.upper, &nk, &nt, &nd), "bella_hip_count_kmers");
            t_count[(size_t)g] = now_s() - t0;
            t0 = now_s();
            if (N == 1) check(w.ctx, bella_hip_assemble_counted(w.ctx), "bella_hip_assemble_counted");
            else {
                check(w.ctx, bella_hip_assemble_counted_panel(w.ctx, lo, hi - lo), "bella_hip_assemble_counted_panel");
                check(w.ctx, bella_hip_allgather_panels(w.ctx), "bella_hip_allgather_panels");
            }
        }
        t_asm[(size_t)g] = now_s() - t0;
        nk_of[(size_t)g] = nk;
    });
    const uint32_t nreads = nreads_of[0];
    const std::string ContextAndReservationTime = std::to_string(t_init[0]) + " seconds";
    BELLA_HIP_LOGT(tag, ContextAndReservationTime);
    const std::string fastqParsingTime = std::to_string(t_ingest[0]) + " seconds";
    BELLA_HIP_LOGT(tag, fastqParsingTime);
    const uint32_t numReads = nreads;
    BELLA_HIP_LOGT(tag, numReads);
    const std::string KmerCountingTime = std::to_string(t_count[0]) + " seconds";
    BELLA_HIP_LOGT(tag, KmerCountingTime);
    std::cout << nk_of[0] << std::endl;                              // main.cpp:472-473 ("to help the parsing script")
    uint64_t nnzA = 0;
    check(W[0].ctx, bella_hip_get_B(W[0].ctx, &nnzA, nullptr, nullptr, nullptr), "bella_hip_get_B");
    std::cout << nnzA << std::endl;                                  // src/CSC.cpp:405 (nnz after MergeDuplicates)
    const std::string SparseMatrixCreationTime = std::to_string(t_asm[0]) + " seconds";
    BELLA_HIP_LOGT(tag, SparseMatrixCreationTime);

    // names and lengths for the writer
    uint64_t need = 0;
    check(W[0].ctx, bella_hip_get_read_names(W[0].ctx, nullptr, 0, nullptr, &need), "bella_hip_get_read_names");
    std::vector<char> namebuf((size_t)need + 1);
    std::vector<uint64_t> noffs((size_t)nreads + 1, 0);
    check(W[0].ctx, bella_hip_get_read_names(W[0].ctx, namebuf.data(), need, noffs.data(), &need), "bella_hip_get_read_names");
    std::vector<const char*> names(nreads);
    for (uint32_t r = 0; r < nreads; ++r) names[r] = namebuf.data() + noffs[r];
    std::vector<uint32_t> lens(nreads);
    if (nreads) check(W[0].ctx, bella_hip_get_read_lengths(W[0].ctx, lens.data()), "bella_hip_get_read_lengths");

    StageOpts so;
    so.N = N;
    so.nreads = nreads;
    so.p.kmer_size = (uint16_t)o.kmer;
    so.p.bin_size = (uint16_t)o.bin_size;
    so.p.xdrop = (uint16_t)o.xdrop;
    so.p.skip_alignment = o.skip_alignment ? 1 : 0;
    so.p.error_rate = o.error;
    so.p.delta_chernoff = o.deviation;
    so.paf = o.paf ? 1 : 0;
    so.total_memory_mb = (double)o.memory;
    so.per_nnz = 20.0;                                               // sizeof(spmatPtr_) + sizeof(uint32_t) in the reference (overlap.hpp:365-404)
    so.filename = outfile.c_str();
    so.tag = tag;
    so.exact = o.exact ? 1 : 0;
    so.cigar = o.cigar ? 1 : 0;
    so.trace_band = (uint32_t)o.trace_band;
    so.correct = o.correct.empty() ? nullptr : o.correct.c_str();
    so.min_depth = (uint32_t)o.min_depth;
    so.gfa = o.gfa.empty() ? nullptr : o.gfa.c_str();
    so.gfa_fuzz = (uint32_t)o.gfa_fuzz;
    so.gfa_max_overhang = (uint32_t)o.gfa_max_overhang;
    so.gfa_min_overlap = (uint32_t)o.gfa_min_overlap;
    so.gfa_no_seq = o.gfa_no_seq ? 1 : 0;
    so.unitigs = o.unitigs.empty() ? nullptr : o.unitigs.c_str();
    so.unitigs_fasta = o.unitigs_fasta.empty() ? nullptr : o.unitigs_fasta.c_str();
    so.tip_reads = (uint32_t)o.tip_reads; so.tip_rounds = (uint32_t)o.tip_rounds;
    so.gfa_clean = o.gfa_clean ? 1 : 0;
    so.pop_bubbles = o.pop_bubbles ? 1 : 0;
    so.bubble_reads = (uint32_t)o.bubble_reads; so.bubble_dist = (uint32_t)o.bubble_dist; so.bubble_rounds = (uint32_t)o.bubble_rounds;
    so.cut_weak = o.cut_weak ? 1 : 0;
    so.weak_min = (uint32_t)o.weak_min; so.weak_max = (uint32_t)o.weak_max; so.weak_steps = (uint32_t)o.weak_steps;
    so.polish = o.polish ? 1 : 0;
    so.polish_min_depth = (uint32_t)o.polish_min_depth;
    so.polish_rounds = (uint32_t)o.polish_rounds; so.realign_band = (uint32_t)o.realign_band; so.realign_min_identity = (uint32_t)o.realign_min_identity; so.realign_circular = o.realign_circular;
    so.align_links = o.align_links ? 1 : 0; so.link_band = (uint32_t)o.link_band; so.link_min_identity = (uint32_t)o.link_min_identity;
    so.correct_rounds = (uint32_t)o.correct_rounds; so.correct_band = (uint32_t)o.correct_band; so.correct_min_identity = (uint32_t)o.correct_min_identity;
    so.normalize_gaps = o.normalize_gaps ? 1 : 0;
    so.clip_ends = o.clip_ends ? 1 : 0; so.clip_identity = (uint32_t)o.clip_identity;
    so.trim = o.trim ? 1 : 0;
    so.trim_depth = (uint32_t)o.trim_depth; so.trim_end_clip = (uint32_t)o.trim_end_clip;
    so.trimmed_reads = o.trimmed_reads.empty() ? nullptr : o.trimmed_reads.c_str();
    const double t_stages = now_s();
    run_stages(W, so, names.data(), lens.data());
    {
        const CallStats& cs = last_call_stats();
        const std::string OverlapTime = std::to_string(cs.overlap_seconds) + " seconds";            // (overlap.hpp:714-727's bracket)
        BELLA_HIP_LOGT(tag, OverlapTime);
        const std::string RecordsAndAlignmentTime = std::to_string(cs.align_seconds) + " seconds";    // records to the host (+ X-drop + alignments to the host)
        BELLA_HIP_LOGT(tag, RecordsAndAlignmentTime);
        const std::string WriterTime = std::to_string(cs.write_seconds) + " seconds";
        BELLA_HIP_LOGT(tag, WriterTime);
        const std::string StagesTime = std::to_string(now_s() - t_stages) + " seconds";
        BELLA_HIP_LOGT(tag, StagesTime);
    }
    const double t_close = now_s();
    for (auto& w : W) bella_hip_destroy(w.ctx);
    const std::string TeardownTime = std::to_string(now_s() - t_close) + " seconds";
    BELLA_HIP_LOGT(tag, TeardownTime);

    const double totaltime = now_s() - all;
    const std::string TotalRuntime = std::to_string(totaltime) + " seconds";
    BELLA_HIP_LOGT(tag, TotalRuntime);
    std::cout << totaltime << std::endl;                             // main.cpp:532
    return 0;
}
