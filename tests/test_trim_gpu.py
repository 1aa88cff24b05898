"""GPU tests of the coverage trimming: the device result EQUALS the mirror (bella_testkit/trim_mirror.py) -- the
clips and their statistics, the graph built from the cut records, the unitigs and their bases in clipped coordinates, the polished
unitigs -- on hand-worked cases, junk ends, chimeras, a read whose sweep crosses many chunks, reads around the 64-event chunk size;
state and errors; bella-hip --trim end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import bubble_mirror as B
from bella_testkit import graph_mirror as G
from bella_testkit import synth
from bella_testkit import trim_mirror as T
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import aligned as _aligned, raises, records as _records, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

ARRAYS = ("voff", "verts", "pos", "nbases", "len", "circular", "links")
STATE, BAD = -7, -3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _load(eng, lens, seqs=None):
    eng.set_reads(synth.ReadSet.from_strings(seqs if seqs is not None else B.dummy_seqs(lens)))


def _trim(eng, lens, recs, **tp):
    """records in, graph_trim: the clips and the statistics against the mirror; -> the mirror's clips"""
    eng.graph_reset()
    eng.graph_add_overlaps(recs)
    eng.graph_trim(**tp)
    mc = T.clips(recs, lens, **tp)
    c = eng.graph_clips()
    assert c.dtype == mc.dtype and c.tobytes() == mc.tobytes(), np.flatnonzero(c != mc)[:10]
    st = eng.trim_stats()
    want = T.trim_stats(recs, lens, mc, **tp)
    assert {k: st[k] for k in want} == want and st["records_outside"] == 0
    return mc


def _build(eng, lens, recs, mc, **gp):
    """graph_build while the clips exist: CSR, edges, flags and statistics against the mirror; -> the mirror's graph"""
    m = T.build(recs, lens, mc, **gp)
    for debug in (0, 1 << 19):
        eng.set_debug(debug)
        try:
            eng.graph_build(**gp)
        finally:
            eng.set_debug(0)
        off, e, cont = eng.graph()
        assert np.array_equal(off, m["offsets"]) and e.tobytes() == m["edges"].tobytes() and np.array_equal(cont, m["contained"])
        st = eng.graph_stats()
        assert {k: st[k] for k in m["stats"]} == m["stats"]
        assert eng.trim_stats()["records_outside"] == m["records_outside"]
    return m


def _unitigs(eng, m, seqs, mc, clean):
    """after _build: clean -> unitigs -> bases on the device against the mirrors called with the clipped lengths and seq[beg:end];
    -> (mirror clean, mirror unitigs, bases)"""
    dead = (m["contained"] != 0).astype(np.uint8)
    c = U.clean(m["offsets"], m["edges"], dead, **clean)
    eng.graph_clean(**clean)
    off, e, cont = eng.graph()
    assert np.array_equal(off, c["offsets"]) and e.tobytes() == c["edges"].tobytes() and np.array_equal(cont, m["contained"])
    assert np.array_equal(eng.graph_removed(), c["removed"])
    mu = U.unitigs(c["offsets"], c["edges"], dead, c["removed"], m["lens"])
    U.check_invariants(mu, c["offsets"], c["edges"], dead, c["removed"], m["lens"])
    du = eng.graph_unitigs()
    for k in ARRAYS:
        assert du[k].dtype == mu[k].dtype and du[k].tobytes() == mu[k].tobytes(), k
    moffs, mb = U.unitig_bases(mu, T.clip_seqs(seqs, mc))
    offs, bases = eng.unitig_bases()
    assert np.array_equal(offs, moffs) and bases.tobytes() == mb
    return c, mu, mb


def test_hand_cases(eng):
    for name, lens, recs, tp, want in T.hand_cases():
        _load(eng, lens)
        mc = _trim(eng, lens, recs, **tp)
        assert [tuple(int(x) for x in row) for row in mc.tolist()] == want, name
        _build(eng, lens, recs, mc)


def test_junk_ends_and_chimeras(eng):
    """junk_ends(truth_chain(150)) and truth_chain(500) with 40 chimeras: clips, then the graph of the cut records"""
    starts, lens, strands, recs = G.truth_chain(150)
    jl, jr, head, tail = T.junk_ends(starts, lens, strands, recs, 0.3, 1200, 3000)
    _load(eng, jl)
    for tp in ({}, dict(end_clip=0), dict(min_depth=5, end_clip=100, min_span=2000)):
        mc = _trim(eng, jl, jr, **tp)
        m = _build(eng, jl, jr, mc)
    starts, lens, strands, recs = G.truth_chain(500)
    cl, cr, ids, _ = T.chimeras(starts, lens, strands, recs, count=40)
    _load(eng, cl)
    mc = _trim(eng, cl, cr)
    assert np.all(mc["nregions"][ids] >= 2)
    m = _build(eng, cl, cr, mc)
    assert m["records_outside"] > 0
    mc = _trim(eng, cl, cr, end_clip=0)
    assert not np.any(mc["nregions"][ids] >= 2)


def test_a_sweep_over_many_chunks(eng):
    """the hub input: read 0 has 700 records, so ~1,400 events in 22 chunks of 64; every region decision crosses chunk borders"""
    lens, recs = B.existing_inputs()["hub"][:2]
    _load(eng, lens)
    for tp in ({}, dict(min_depth=100, end_clip=0), dict(min_depth=650, end_clip=37, min_span=1)):
        mc = _trim(eng, lens, recs, **tp)
        assert mc["max_depth"][0] >= 600
    _build(eng, lens, recs, _trim(eng, lens, recs))


def _fan(nints, seed):
    """read 0 with `nints` intervals (2 nints events) at seeded positions, many of them equal, so that groups of equal positions straddle
    the 64-event chunk borders: -> (lens, recs)"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 12, nints) * 500
    e = b + 1000 + rng.integers(0, 12, nints) * 500
    out = [T._record(0, (int(x), int(y)), k + 1, (0, int(y - x)), 15000, int(k & 1), 0) for k, (x, y) in enumerate(zip(b, e))]
    return np.full(nints + 1, 15000, np.int64), np.array(out, G.OVL_DT)


@pytest.mark.parametrize("nints", [31, 32, 33, 63, 64, 65])
def test_reads_around_the_chunk_size(eng, nints):
    """a read with 62, 64 (one full chunk), 66, 126, 128 (two full chunks) and 130 events.  Events come in pairs, so an odd count such as
    65 cannot occur; 64 + 2 is the smallest count past one chunk"""
    for seed in range(4):
        lens, recs = _fan(nints, seed)
        _load(eng, lens)
        for tp in (dict(min_depth=3, end_clip=0, min_span=500), dict(min_depth=2, end_clip=500, min_span=1000), dict(min_depth=nints // 4, end_clip=250, min_span=1)):
            mc = _trim(eng, lens, recs, **tp)
    assert int(mc["max_depth"][0]) > 3


def test_no_records_and_one_read(eng):
    lens = np.array([5000], np.int64)
    _load(eng, lens)
    mc = _trim(eng, lens, np.zeros(0, G.OVL_DT))
    assert mc.tolist() == [(0, 0, 0, 0)]
    m = _build(eng, lens, np.zeros(0, G.OVL_DT), mc)
    assert m["contained"].tolist() == [T.UNCOVERED]
    u = eng.graph_unitigs()
    assert len(u["len"]) == 0 and u["total_bases"] == 0


def _junk_genome(n, seed):
    """truth_chain(n) cut from a random genome, junk ends of random bases added: -> (genome, seqs, lens, recs)"""
    starts, lens, strands, recs = G.truth_chain(n)
    genome = U.random_genome(int((starts + lens).max()), seed)
    jl, jr, head, tail = T.junk_ends(starts, lens, strands, recs, 0.4, 1200, 3000, seed=seed)
    seqs = T.junk_seqs(U.reads_from_genome(genome, starts, lens, strands), head, tail, seed)
    assert [len(s) for s in seqs] == jl.tolist()
    return genome, seqs, jl, jr


def test_unitigs_of_trimmed_reads_are_the_genome(eng):
    """real bases with junk ends: after the trim there is one unitig, a substring of the genome or of its reverse complement (untrimmed
    the junk is in the unitigs); the clipped gather in both orientations"""
    genome, seqs, lens, recs = _junk_genome(120, 41)
    _load(eng, lens, seqs)
    mc = _trim(eng, lens, recs)
    m = _build(eng, lens, recs, mc)
    assert m["stats"]["n_internal"] == 0
    c, mu, mb = _unitigs(eng, m, seqs, mc, {})
    assert len(mu["len"]) == 1 and (mb in genome or mb in U.revcomp(genome)) and len(mb) > 30000
    st = eng.unitig_stats()
    assert st["unitigs"] == 1 and st["total_bases"] == len(mb)


def test_short_segments_with_clips(eng):
    """short_segment_input with 3 to 12 junk bases on 40 % of the ends and loose trim parameters: segments shorter than the gather's 16-base
    groups from clipped, unaligned spans in both orientations; every unitig is a substring of the genome or its reverse complement"""
    starts, lens, strands, recs = U.short_segment_input()
    genome = U.random_genome(int((starts + lens).max()), 34)
    jl, jr, head, tail = T.junk_ends(starts, lens, strands, recs, 0.4, 3, 12, seed=5)
    seqs = T.junk_seqs(U.reads_from_genome(genome, starts, lens, strands), head, tail, 6)
    _load(eng, jl, seqs)
    mc = _trim(eng, jl, jr, min_depth=2, end_clip=2, min_span=10)
    assert (mc["beg"] > 0).sum() > 50 and ((mc["end"] > mc["beg"]) & (mc["end"] < jl)).sum() > 50
    m = _build(eng, jl, jr, mc, min_overlap=0, fuzz=0)
    c, mu, mb = _unitigs(eng, m, seqs, mc, dict(max_tip_reads=0))
    assert int(mu["nbases"].min()) < 16 and len(mu["verts"]) > 100 and (mu["verts"] & 1).sum() > 20
    rc = U.revcomp(genome)
    offs = np.concatenate([[0], np.cumsum(mu["len"].astype(np.int64))])
    for k in range(len(mu["len"])):
        s = mb[offs[k]:offs[k + 1]]
        assert s in genome or s in rc, k


@pytest.mark.parametrize("case", ["junk", "short"])
def test_polish_of_trimmed_unitigs(eng, case):
    """graph_polish_unitigs on random_table while clips exist, against the trimmed polish mirror: the decisions are those of the ORIGINAL
    positions"""
    if case == "junk":
        genome, seqs, lens, recs = _junk_genome(40, 43)
        tp, gp, cp = {}, {}, {}
    else:
        starts, l0, strands, r0 = U.short_segment_input(200)
        genome = U.random_genome(int((starts + l0).max()), 35)
        lens, recs, head, tail = T.junk_ends(starts, l0, strands, r0, 0.4, 3, 12, seed=7)
        seqs = T.junk_seqs(U.reads_from_genome(genome, starts, l0, strands), head, tail, 8)
        tp, gp, cp = dict(min_depth=2, end_clip=2, min_span=10), dict(min_overlap=0, fuzz=0), dict(max_tip_reads=0)
    _load(eng, lens, seqs)
    mc = _trim(eng, lens, recs, **tp)
    m = _build(eng, lens, recs, mc, **gp)
    c, mu, mb = _unitigs(eng, m, seqs, mc, cp)
    for seed, md in ((0, 3), (1, 1)):
        table = U.random_table(lens, seed, md)
        eng.pileup_reset()
        eng.add_pileup(0, eng.nreads, table)
        want = T.polished(mu, seqs, table, mc, md)
        p = eng.graph_polish_unitigs(md)
        assert np.array_equal(p["offsets"], want["offsets"]) and p["bases"].tobytes() == want["bases"]
        assert np.array_equal(p["pos"], want["pos"]) and np.array_equal(p["nbases"], want["nbases"]) and p["stats"].tobytes() == want["stats"].tobytes()
        assert p["bases"].tobytes() != mb
    eng.pileup_reset()                                                  # an all-zero table: the raw, clipped unitigs
    assert eng.graph_polish_unitigs()["bases"].tobytes() == mb


def test_state_and_errors():
    starts, lens, strands, recs = G.truth_chain(60)
    jl, jr, _, _ = T.junk_ends(starts, lens, strands, recs, 0.3, 1200, 3000)
    e = Engine(0)
    try:
        raises(STATE, e.graph_trim)                                   # no reads
        _load(e, jl)
        raises(STATE, e.graph_clips)                                    # no trim
        raises(STATE, e.trim_stats)
        e.graph_untrim()                                                # nothing to drop: no error
        e.graph_add_overlaps(jr)
        plain = G.build(jr, jl)

        def is_plain():
            e.graph_build()
            off, ed, cont = e.graph()
            assert np.array_equal(off, plain["offsets"]) and ed.tobytes() == plain["edges"].tobytes() and np.array_equal(cont, plain["contained"])
            st = e.graph_stats()
            assert {k: st[k] for k in plain["stats"]} == plain["stats"]
        is_plain()
        small = _lib.GraphTrimParams(C.sizeof(_lib.GraphTrimParams) - 4, 3, 500, 1000)
        assert e.lib.bella_hip_graph_trim(e.h, C.byref(small)) == BAD
        raises(BAD, e.graph_trim, min_depth=0)
        raises(STATE, e.graph_clips)                                    # the refused calls left no clips
        e.graph()                                                       # ... and the graph alone
        assert e.lib.bella_hip_graph_trim(e.h, None) == 0               # NULL: the defaults
        mc = T.clips(jr, jl)
        assert e.graph_clips().tobytes() == mc.tobytes()
        raises(STATE, e.graph)                                          # the trim dropped the graph
        big = (C.c_uint8 * 256)()
        C.memset(big, 0xEE, 256)
        assert e.lib.bella_hip_graph_get_trim_stats(e.h, big, 16) == 0  # a sized struct: at most struct_size bytes
        assert bytes(big[16:32]) == b"\xee" * 16 and int.from_bytes(bytes(big[0:8]), "little") == e.trim_stats()["intervals"]
        _build(e, jl, jr, mc)
        e.graph_unitigs()
        e.graph_untrim()
        raises(STATE, e.graph_clips)
        raises(STATE, e.graph)                                          # made with the clips: gone with them
        is_plain()                                                      # exactly the untrimmed mirror again
        e.graph_trim()
        e.graph_add_overlaps(np.zeros(0, G.OVL_DT))                     # adding records drops the clips
        raises(STATE, e.graph_clips)
        is_plain()
        e.graph_trim()
        e.graph_reset()
        raises(STATE, e.graph_clips)
        e.graph_add_overlaps(jr)
        e.graph_trim()
        _load(e, jl)                                                    # loading reads drops them too
        raises(STATE, e.graph_clips)
    finally:
        e.close()


def _run(*args):
    files = run_cli(*args)
    return tuple(files.get(n) for n in ("out.out", "g.gfa", "u.gfa", "u.fa", "t.fa")), files["stderr"]


@pytest.mark.parametrize("name", ["toy120", "toyjunk220"])
def test_cli_trim_end_to_end(eng, tmp_path, name):
    """bella-hip --trim on a golden set: the --gfa, --unitigs, --unitigs-fasta and --trimmed-reads files are the mirror's text of the
    Python path's records; -m 1, -g 2 and both give the same files; without --trim the files are what they are today.  The toy reads are
    short, so the trim parameters are loose"""
    g = load_golden(name)
    pars, pairs, alns = _aligned(eng, g)
    recs = _records(pairs, alns, eng.trace_pairs_records(pars))
    lens = np.asarray(g.rs.lengths, np.int64)
    loose = dict(min_overlap=0, fuzz=10)

    def texts(m, ulens, seqs, slens):
        dead = (m["contained"] != 0).astype(np.uint8)
        c = U.clean(m["offsets"], m["edges"], dead)
        u = U.unitigs(c["offsets"], c["edges"], dead, c["removed"], ulens)
        offs, b = U.unitig_bases(u, seqs)
        return G.gfa_text(g.names, slens, seqs, m["offsets"], m["edges"], dead), U.unitig_gfa_text(g.names, u, offs, b), U.fasta_text(u, offs, b)
    plain = texts(G.build(recs, lens, **loose), lens, g.seqs, lens)
    mc = T.clips(recs, lens, min_depth=2, end_clip=20, min_span=0)
    m = T.build(recs, lens, mc, **loose)
    cseqs = T.clip_seqs(g.seqs, mc)
    trimmed = texts(m, m["lens"], cseqs, m["lens"]) + (T.trimmed_fasta_text(g.names, g.seqs, mc),)
    assert trimmed[:3] != plain
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx, "--gfa", "g.gfa", "--unitigs", "u.gfa", "--unitigs-fasta", "u.fa", "--gfa-min-overlap", "0", "--gfa-fuzz", "10"]
    trim = ["--trim", "--trim-depth", "2", "--trim-end-clip", "20", "--trimmed-reads", "t.fa"]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    files, _ = _run([fq], base, str(tmp_path / "plain"))
    assert files == (g.out["align"],) + plain + (None,)
    files, err = _run([fq], base + trim, str(tmp_path / "trim"))
    assert files == (g.out["align"],) + trimmed
    st = T.trim_stats(recs, lens, mc, min_depth=2, end_clip=20, min_span=0)
    log = [ln for ln in err.decode().splitlines() if "Trim = " in ln]
    assert len(log) == 1 and ("%d intervals, %d reads clipped, %d uncovered" % (st["intervals"], st["reads_clipped"], st["reads_uncovered"])) in log[0]
    assert ("%d records outside" % m["records_outside"]) in log[0]
    assert _run([fq], base + trim + ["-m", "1"], str(tmp_path / "m1"))[0] == files
    assert _run([fq], base + trim + ["-g", "2"], str(tmp_path / "g2"), over)[0] == files
    assert _run([fq], base + trim + ["-m", "1", "-g", "2"], str(tmp_path / "m1g2"), over)[0] == files
    assert _run([fq], base + ["-m", "1", "-g", "2"], str(tmp_path / "plain_m1g2"), over)[0] == (g.out["align"],) + plain + (None,)
    print("TRIM cli %s: %s" % (name, log[0].split("Trim = ")[1]))
