"""GPU tests of tip clipping, unitig compaction and unitig sequences: the device result EQUALS the mirror
(bella_testkit/unitig_mirror.py) -- cleaned CSR, removed flags, per-round counts, every unitig array, the links, the bases -- on the
golden sets, on reads cut from a known genome (the unitig is the genome), on a tip, a circle, segments shorter than the gather's
16-base groups and a graph full of forks; state and errors; bella-hip --unitigs end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from bella_amd import Engine, _lib, api
from bella_testkit import graph_mirror as G
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import aligned as _aligned, hub_and_band as _hub_and_band, records as _records, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

LOOSE = dict(min_overlap=0, fuzz=10)
ARRAYS = ("voff", "verts", "pos", "nbases", "len", "circular", "links")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _same(eng, m, lens, seqs, clean=None):
    """after eng.graph_build: clean (clean = None: no clean call) -> unitigs -> bases on the device, every array and count against the
    mirror's; -> (mirror clean, mirror unitigs, device stats, bases)"""
    off, e, cont = eng.graph()
    assert np.array_equal(off, m["offsets"]) and e.tobytes() == m["edges"].tobytes() and np.array_equal(cont, m["contained"])
    if clean is None:
        c = dict(offsets=m["offsets"], edges=m["edges"], removed=np.zeros(len(lens), np.uint8), rounds=[])
    else:
        c = U.clean(m["offsets"], m["edges"], m["contained"], **clean)
        eng.graph_clean(**clean)
    off, e, cont = eng.graph()
    assert np.array_equal(off, c["offsets"]) and e.tobytes() == c["edges"].tobytes() and np.array_equal(cont, m["contained"])
    assert np.array_equal(eng.graph_removed(), c["removed"])
    st = eng.unitig_stats()
    assert list(zip(st["tips_per_round"], st["reads_per_round"])) == c["rounds"] and st["rounds"] == len(c["rounds"])
    assert st["reads_removed"] == int(c["removed"].sum()) and st["edges_removed"] == len(m["edges"]) - len(c["edges"])
    mu = U.unitigs(c["offsets"], c["edges"], m["contained"], c["removed"], lens)
    U.check_invariants(mu, c["offsets"], c["edges"], m["contained"], c["removed"], lens)
    du = eng.graph_unitigs()
    for k in ARRAYS:
        assert du[k].dtype == mu[k].dtype and du[k].tobytes() == mu[k].tobytes(), k
    st = eng.unitig_stats()
    want = dict(unitigs=len(mu["len"]), vertices=len(mu["verts"]), links=len(mu["links"]), total_bases=mu["total_bases"], circular=int(mu["circular"].sum()),
                largest=mu["largest"], n50=mu["n50"])
    assert {k: st[k] for k in want} == want and du["total_bases"] == mu["total_bases"]
    moffs, mb = U.unitig_bases(mu, seqs)
    offs, bases = eng.unitig_bases()
    assert np.array_equal(offs, moffs) and bases.tobytes() == mb
    return c, mu, st, mb


def test_golden_sets_equal_the_mirror(eng, golden):
    """align -> trace -> graph_add_traced -> graph_build (loose and default) -> graph_clean with max_tip_reads 0, 1, 4 -> unitigs ->
    bases.  sanity3 and the default setting are the empty and near-empty cases (no edges; all reads contained or single)."""
    g = golden
    pars, pairs, alns = _aligned(eng, g)
    tr = eng.trace_pairs_records(pars)
    eng.graph_reset()
    eng.graph_add_traced()
    recs = _records(pairs, alns, tr)
    lens = g.rs.lengths
    for params in (LOOSE, {}):
        m = G.build(recs, lens, **params)
        for mt in (0, 1, 4):
            eng.graph_build(**params)
            c, mu, st, _ = _same(eng, m, lens, g.seqs, clean=dict(max_tip_reads=mt))
            print("UNITIG %s %s tips<=%d: rounds %s, %d unitigs, %d links, %d bases, n50 %d" % (g.name, params or "defaults", mt, c["rounds"], len(mu["len"]), len(mu["links"]),
                                                                                                mu["total_bases"], mu["n50"]))


def _genome_reads(eng, starts, lens, strands, seed):
    genome = U.random_genome(int((np.asarray(starts) + np.asarray(lens)).max()), seed)
    seqs = U.reads_from_genome(genome, starts, lens, strands)
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    return genome, seqs


def _is_substring(bases, genome, lo, hi):
    return bases == genome[lo:hi] or bases == U.revcomp(genome[lo:hi])


def test_reads_cut_from_a_genome_give_the_genome_back(eng):
    """500 reads at truth_chain's starts, lengths and strands cut from a random genome, exact records: one unitig, whose bases are the
    genome from the first non-contained read's start to the last one's end (or its reverse complement).  The genome is as long as
    truth_chain's reads reach, ~166 kb (reads of 9 to 11 kb every ~240 bases; ~550 kb would need them ~1.1 kb apart): the case is the
    one truth_chain's starts and lengths define."""
    starts, lens, strands, recs = G.truth_chain()
    genome, seqs = _genome_reads(eng, starts, lens, strands, 31)
    eng.graph_add_overlaps(recs)
    eng.graph_build()
    m = G.build(recs, lens)
    c, mu, st, bases = _same(eng, m, lens, seqs, clean={})
    live = np.flatnonzero(m["contained"] == 0)
    lo, hi = int(starts[live].min()), int((starts[live] + lens[live]).max())
    assert len(mu["len"]) == 1 and int(mu["len"][0]) == hi - lo and _is_substring(bases, genome, lo, hi)
    print("GENOME 500: %d reads in the unitig, %d bases, rank rounds %d, rank %.3f ms, gather %.3f ms" % (len(mu["verts"]), hi - lo, st["rank_rounds"], st["rank_ms"], st["gather_ms"]))


def test_a_chain_of_4000_reads_ranks_in_more_than_ten_rounds(eng):
    """the same with truth_chain(nreads=4000) (a genome of ~1.2 Mb): the ranking runs ceil(log2(8000)) = 13 jumping rounds.  The graph
    itself is the device's (held to the mirror above and in tests/test_graph_gpu.py); what is checked is the genome."""
    starts, lens, strands, recs = G.truth_chain(nreads=4000)
    genome, seqs = _genome_reads(eng, starts, lens, strands, 32)
    eng.graph_add_overlaps(recs)
    eng.graph_build()
    eng.graph_clean()
    off, e, cont = eng.graph()
    assert not eng.graph_removed().any()
    u = eng.graph_unitigs()
    st = eng.unitig_stats()
    offs, bases = eng.unitig_bases()
    live = np.flatnonzero(cont == 0)
    lo, hi = int(starts[live].min()), int((starts[live] + lens[live]).max())
    assert st["rank_rounds"] > 10 and len(u["len"]) == 1 and len(u["verts"]) == len(live) and int(u["len"][0]) == hi - lo
    assert np.all(np.diff(u["pos"].astype(np.int64)) > 0)
    assert _is_substring(bases.tobytes(), genome, lo, hi)
    print("GENOME 4000: %d reads in the unitig, %d bases, rank rounds %d, rank %.3f ms, gather %.3f ms" % (len(u["verts"]), hi - lo, st["rank_rounds"], st["rank_ms"], st["gather_ms"]))


def test_tip_input_with_real_bases(eng):
    starts, lens, strands, recs = U.tip_input()
    genome, seqs = _genome_reads(eng, starts, lens, strands, 33)
    eng.graph_add_overlaps(recs)
    m = G.build(recs, lens)
    eng.graph_build()
    c, mu, st, bases = _same(eng, m, lens, seqs, clean={})
    assert np.flatnonzero(c["removed"]).tolist() == [40, 41] and len(mu["len"]) == 1 and _is_substring(bases, genome, 0, 88000)
    eng.graph_build()
    c1, mu1, _, _ = _same(eng, m, lens, seqs, clean=dict(max_tip_reads=1))
    assert not c1["removed"].any() and len(mu1["len"]) == 3 and len(mu1["links"]) == 4
    eng.graph_build()                                                 # and without any clean call
    _same(eng, m, lens, seqs, clean=None)


def test_two_rounds(eng):
    lens, recs = U.two_round_input()
    seqs = [U.random_genome(int(n), 40 + i) for i, n in enumerate(lens)]
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    m = G.build(recs, lens)
    for rounds, want in ((3, [(2, 2), (1, 1), (0, 0)]), (1, [(2, 2)]), (2, [(2, 2), (1, 1)])):
        eng.graph_build()
        c, mu, st, _ = _same(eng, m, lens, seqs, clean=dict(tip_rounds=rounds))
        assert c["rounds"] == want


def test_circle(eng):
    genome, seqs, strands, recs = U.circle_input()
    lens = np.array([len(s) for s in seqs])
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    m = G.build(recs, lens)
    eng.graph_build()
    c, mu, st, bases = _same(eng, m, lens, seqs, clean={})
    assert mu["circular"].tolist() == [1] and mu["len"].tolist() == [120000] and len(mu["verts"]) == 60 and st["cycle_vertices"] == 120
    assert bases in genome + genome or U.revcomp(bases) in genome + genome


def test_segments_shorter_than_the_gathers_groups(eng):
    """reads of 40 to 70 bases every 1 to 20 bases: segments of 1 to 20 bases, most lanes of the gather straddle several"""
    rng = np.random.default_rng(17)
    n = 400
    starts = np.cumsum(rng.integers(1, 21, n))
    lens = rng.integers(40, 71, n)
    strands = rng.integers(0, 2, n)
    genome, seqs = _genome_reads(eng, starts, lens, strands, 34)
    recs = G.truth_records(starts, lens, strands, min_overlap=1)
    eng.graph_add_overlaps(recs)
    params = dict(min_overlap=0, fuzz=0)
    m = G.build(recs, lens, **params)
    eng.graph_build(**params)
    c, mu, st, bases = _same(eng, m, lens, seqs, clean=dict(max_tip_reads=0))
    live = np.flatnonzero(m["contained"] == 0)
    lo, hi = int(starts[live].min()), int((starts[live] + lens[live]).max())
    assert len(mu["len"]) == 1 and mu["nbases"].min() == 1 and np.median(mu["nbases"]) < 16 and _is_substring(bases, genome, lo, hi)


@pytest.fixture(scope="module")
def hub():
    recs, lens = _hub_and_band()
    rng = np.random.default_rng(5)
    seqs = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(n))].tobytes() for n in lens]
    return recs, lens, seqs, {fuzz: G.build(recs, lens, fuzz=fuzz) for fuzz in (1000, 0)}


@pytest.mark.parametrize("fuzz", [1000, 0])
def test_hub_and_band_forks_and_links(eng, hub, fuzz):
    """a 700-way fork and an eight-wide band: unclipped, forks everywhere (2,004 unitigs joined by 6,246 links, for either fuzz); with
    the defaults every arm is a tip, two rounds clip 890 + 119 reads and one unitig without links is left"""
    recs, lens, seqs, built = hub
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    for clean, want in ((dict(max_tip_reads=0), ([], 2004, 6246)), ({}, ([(890, 890), (117, 119), (0, 0)], 1, 0))):
        eng.graph_build(fuzz=fuzz)
        c, mu, st, _ = _same(eng, built[fuzz], lens, seqs, clean=clean)
        print("HUB fuzz %d %s: rounds %s, %d unitigs, %d links" % (fuzz, clean, c["rounds"], len(mu["len"]), len(mu["links"])))
        assert (c["rounds"], len(mu["len"]), len(mu["links"])) == want


def test_state_and_errors(eng):
    g = load_golden("toy120")
    eng.set_reads(g.rs)
    for call in (eng.graph_clean, eng.graph_unitigs, eng.graph_removed, eng.unitig_stats):
        with pytest.raises(api.BellaHipError) as ex:
            call()
        assert ex.value.code == -7, call
    eng.graph_build()                                                 # no records: an empty graph, every read a unitig of its own
    with pytest.raises(api.BellaHipError) as ex:
        eng.unitig_bases()
    assert ex.value.code == -7
    u = eng.graph_unitigs()
    assert len(u["len"]) == g.rs.nreads and np.array_equal(u["len"], g.rs.lengths.astype(np.uint64)) and len(u["links"]) == 0
    offs, bases = eng.unitig_bases()
    assert bases.tobytes() == b"".join(g.seqs)
    small = _lib.GraphCleanParams(C.sizeof(_lib.GraphCleanParams) - 4, 4, 3)
    assert eng.lib.bella_hip_graph_clean(eng.h, C.byref(small)) == -3
    many = _lib.GraphCleanParams(C.sizeof(_lib.GraphCleanParams), 4, _lib.MAX_TIP_ROUNDS + 1)
    assert eng.lib.bella_hip_graph_clean(eng.h, C.byref(many)) == -3
    assert eng.lib.bella_hip_graph_clean(eng.h, None) == 0             # NULL: the defaults
    with pytest.raises(api.BellaHipError) as ex:                     # a clean drops the unitigs
        eng.unitig_bases()
    assert ex.value.code == -7
    eng.graph_unitigs()
    eng.set_reads(g.rs)                                               # other reads drop graph and unitigs
    for call in (eng.graph_unitigs, eng.unitig_bases, eng.graph_removed):
        with pytest.raises(api.BellaHipError) as ex:
            call()
        assert ex.value.code == -7
    two = synth.ReadSet.from_strings([b"ACGTACGTAC", b"ACGTACGTAC"])
    eng.set_reads(two)                                                # one read contained in the other: one live read, no edges
    eng.graph_add_overlaps(np.array([(0, 1, 0, 10, 0, 10, 0, 0, (0, 0, 0))], G.OVL_DT))
    eng.graph_build(min_overlap=0)
    m = G.build(np.array([(0, 1, 0, 10, 0, 10, 0, 0, (0, 0, 0))], G.OVL_DT), [10, 10], min_overlap=0)
    c, mu, st, bases = _same(eng, m, [10, 10], [b"ACGTACGTAC"] * 2, clean={})
    assert int(m["contained"].sum()) == 1 and len(mu["len"]) == 1 and bases == b"ACGTACGTAC"
    one = synth.ReadSet.from_strings([b"ACGTTGCAAC"])               # nreads == 1
    eng.set_reads(one)
    eng.graph_build()
    eng.graph_clean()
    u = eng.graph_unitigs()
    assert u["verts"].tolist() == [0] and eng.unitig_bases()[1].tobytes() == b"ACGTTGCAAC"


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return tuple(files.get(n) for n in ("out.out", "g.gfa", "u.gfa", "u.fa"))


def test_cli_unitigs_end_to_end(eng, tmp_path):
    """bella-hip --unitigs / --unitigs-fasta on a golden set: the files are the mirror's text of the Python path's records; the -o file
    and the --gfa file (without --gfa-clean) are what they are without the new options; -m 1, -g 2 and both give the same files;
    --gfa-clean, --gfa-no-seq, --tip-reads 0"""
    g = load_golden("toy120")
    pars, pairs, alns = _aligned(eng, g)
    recs = _records(pairs, alns, eng.trace_pairs_records(pars))
    lens = g.rs.lengths
    m = G.build(recs, lens, **LOOSE)

    def texts(**clean):
        c = U.clean(m["offsets"], m["edges"], m["contained"], **clean)
        u = U.unitigs(c["offsets"], c["edges"], m["contained"], c["removed"], lens)
        offs, b = U.unitig_bases(u, g.seqs)
        return c, U.unitig_gfa_text(g.names, u, offs, b), U.unitig_gfa_text(g.names, u), U.fasta_text(u, offs, b)
    c, want, want_noseq, want_fa = texts()
    c0, want0, _, want_fa0 = texts(max_tip_reads=0)
    gfa_plain = G.gfa_text(g.names, lens, g.seqs, m["offsets"], m["edges"], m["contained"])
    gfa_clean = G.gfa_text(g.names, lens, g.seqs, c["offsets"], c["edges"], m["contained"] | c["removed"])
    assert want.count(b"\nS\t") >= 1
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx]
    loose = ["--gfa-min-overlap", "0", "--gfa-fuzz", "10"]
    gfa = ["--gfa", "g.gfa"]
    utg = ["--unitigs", "u.gfa", "--unitigs-fasta", "u.fa"]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    out0, gfa0, none, none2 = _run([fq], base + gfa + loose, str(tmp_path / "plain"))
    assert out0 == g.out["align"] and gfa0 == gfa_plain and none is None and none2 is None
    assert _run([fq], base + utg + loose, str(tmp_path / "utg")) == (out0, None, want, want_fa)                 # --gfa is not required
    assert _run([fq], base + ["--unitigs", "u.gfa"] + loose, str(tmp_path / "only")) == (out0, None, want, None)
    assert _run([fq], base + gfa + utg + loose, str(tmp_path / "both")) == (out0, gfa_plain, want, want_fa)
    assert _run([fq], base + gfa + utg + loose + ["--gfa-clean"], str(tmp_path / "clean")) == (out0, gfa_clean, want, want_fa)
    assert _run([fq], base + utg + loose + ["--gfa-no-seq"], str(tmp_path / "noseq")) == (out0, None, want_noseq, want_fa)
    assert _run([fq], base + utg + loose + ["--tip-reads", "0"], str(tmp_path / "tip0")) == (out0, None, want0, want_fa0)
    assert _run([fq], base + gfa + utg + loose + ["-m", "1"], str(tmp_path / "m1")) == (out0, gfa_plain, want, want_fa)
    assert _run([fq], base + gfa + utg + loose + ["-g", "2"], str(tmp_path / "g2"), over) == (out0, gfa_plain, want, want_fa)
    assert _run([fq], base + gfa + utg + loose + ["-m", "1", "-g", "2"], str(tmp_path / "m1g2"), over) == (out0, gfa_plain, want, want_fa)
