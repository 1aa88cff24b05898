"""GPU tests of the unitig consensus: the device result EQUALS the mirror (bella_testkit/unitig_mirror.py:
polished) -- offsets, bases, pos, nbases, every field of the per-unitig records, the totals -- on synthetic tables that take every
branch of the rule, on edge shapes of the tiles, on the tables of real traces; state and errors; bella-hip --polish end to end; and the
measured effect on 2,000 reads of 10 kb at 15 % error."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import graph_mirror as G
from bella_testkit import pileup_mirror as P
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import aligned as _aligned, raises, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

LOOSE = dict(min_overlap=0, fuzz=10)
TILE = 4096
CASES = {c[0]: c for c in U.polish_cases()}
SEEN = dict(rc=False, short=False, boundary=False, odd_total=False)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _install(eng, seqs, recs, graph, clean):
    """reads, records, graph, clean (None: no clean call), unitigs: -> the device's unitigs (pinned to the mirror by test_unitig_gpu.py)"""
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    if len(recs):
        eng.graph_add_overlaps(recs)
    eng.graph_build(**graph)
    if clean is not None:
        eng.graph_clean(**clean)
    return eng.graph_unitigs()


def _table(eng, table):
    eng.pileup_reset()
    eng.add_pileup(0, eng.nreads, table)


def _same(eng, u, seqs, table, md):
    """polish on the device against the mirror: every array, every record, the totals; -> (device result, stats)"""
    p = eng.graph_polish_unitigs(md)
    m = U.polished(u, seqs, table, md)
    assert p["offsets"].dtype == np.uint64 and np.array_equal(p["offsets"], m["offsets"])
    assert p["bases"].tobytes() == m["bases"]
    assert p["pos"].dtype == np.uint64 and np.array_equal(p["pos"], m["pos"])
    assert p["nbases"].dtype == np.uint32 and np.array_equal(p["nbases"], m["nbases"])
    assert p["stats"].dtype == _lib.POLISH_DT == U.POLISH_DT
    for f in U.POLISH_DT.names:
        assert np.array_equal(p["stats"][f], m["stats"][f]), f
    st = eng.polish_stats()
    want = dict(unitigs=len(u["len"]), vertices=len(u["verts"]), bases_before=int(u["len"].sum()), bases_after=len(m["bases"]), min_depth=md,
                tiles=(int(u["len"].sum()) + TILE - 1) // TILE, table_bytes=36 * int(u["len"].sum()))
    for f in ("substituted", "deleted", "inserted", "covered", "depth_sum"):
        want[f] = int(m["stats"][f].sum())
    assert {k: st[k] for k in want} == want
    return p, st


@pytest.mark.parametrize("name", list(CASES))
def test_synthetic_tables_equal_the_mirror(eng, name):
    """the tip input (88,000 positions: 22 tiles; unclipped, three unitigs whose boundaries lie inside tiles), the circle, the two-round
    input and the short segments, each with random_table seeds 0-2 and min_depth 1, 3, 50"""
    _, seqs, recs, graph, clean = CASES[name]
    u = _install(eng, seqs, recs, graph, clean)
    lens = [len(s) for s in seqs]
    for seed in range(3):
        t = U.random_table(lens, seed)
        _table(eng, t)
        for md in (1, 3, 50):
            p, st = _same(eng, u, seqs, t, md)
            SEEN["odd_total"] |= len(p["bases"]) % 16 != 0
            if seed == 0:
                print("POLISH %s min_depth %d: %d unitigs, %d vertices, %d -> %d bases, substituted %d, deleted %d, inserted %d, decide %.3f ms, write %.3f ms"
                      % (name, md, st["unitigs"], st["vertices"], st["bases_before"], st["bases_after"], st["substituted"], st["deleted"], st["inserted"],
                         st["decide_ms"], st["write_ms"]))
    SEEN["rc"] |= bool((u["verts"] & 1).any())
    SEEN["short"] |= bool((u["nbases"] < 16).any())
    raw_offs = np.concatenate([[0], np.cumsum(u["len"])])
    SEEN["boundary"] |= bool((raw_offs[1:-1] % TILE != 0).any())


def test_the_synthetic_set_covers_what_it_should():
    """over the cases above: orientation-1 segments, segments shorter than 16 positions, a tile that holds a unitig boundary, outputs
    whose total is not a multiple of 16 (runs after them: pytest keeps file order)"""
    assert all(SEEN.values()), SEEN


def test_all_zero_table_gives_the_raw_unitigs(eng):
    for name in ("tip3", "short", "circle"):
        _, seqs, recs, graph, clean = CASES[name]
        u = _install(eng, seqs, recs, graph, clean)
        eng.pileup_reset()
        p = eng.graph_polish_unitigs()
        offs, bases = eng.unitig_bases()
        assert np.array_equal(p["offsets"], offs) and p["bases"].tobytes() == bases.tobytes() and np.array_equal(p["pos"], u["pos"]) and np.array_equal(p["nbases"], u["nbases"])
        assert np.array_equal(p["stats"]["len_after"], u["len"]) and not p["stats"]["covered"].any()
        _same(eng, u, seqs, np.zeros((sum(len(s) for s in seqs), 9), np.uint32), 3)


def test_a_unitig_deleted_whole_and_a_base_inserted_at_every_junction(eng):
    _, seqs, recs, graph, clean = CASES["tip3"]
    u = _install(eng, seqs, recs, graph, clean)
    assert len(u["len"]) == 3
    lens = np.array([len(s) for s in seqs])
    roff = np.concatenate([[0], np.cumsum(lens)])
    t = np.zeros((int(roff[-1]), 9), np.uint32)
    for v in u["verts"][int(u["voff"][1]):int(u["voff"][2])].tolist():                    # every position of the middle unitig's reads: deleted
        t[roff[v >> 1]:roff[(v >> 1) + 1], 4] = 10
    _table(eng, t)
    p, st = _same(eng, u, seqs, t, 3)
    assert p["stats"]["len_after"].tolist() == [int(u["len"][0]), 0, int(u["len"][2])] and p["offsets"].tolist() == [0, int(u["len"][0]), int(u["len"][0]), int(u["len"][0] + u["len"][2])]
    offs, bases = eng.unitig_bases()
    assert p["bases"].tobytes() == bases.tobytes()[:int(offs[1])] + bases.tobytes()[int(offs[2]):]
    t[:] = 0                                                          # depth 5 everywhere, ten votes for an inserted C: every junction fires
    t[:, 0] = 5
    t[:, 6] = 10
    _table(eng, t)
    p, st = _same(eng, u, seqs, t, 3)
    nfirst = int(sum(1 for v, n in zip(u["verts"].tolist(), u["nbases"].tolist()) if not v & 1 or n == lens[v >> 1]))      # segments that hold their read's position 0
    assert st["bases_after"] == 2 * st["bases_before"] - nfirst and st["inserted"] == st["bases_before"] - nfirst


@pytest.mark.parametrize("total", [TILE, TILE + 1])
def test_exactly_one_tile_and_one_more_position(eng, total):
    seqs = [U.random_genome(1000, 70), U.random_genome(total - 1000, 71)]
    u = _install(eng, seqs, np.zeros(0, G.OVL_DT), {}, None)              # no edges: every read a unitig of its own
    assert int(u["len"].sum()) == total and len(u["len"]) == 2
    for seed in (0, 1):
        t = U.random_table([len(s) for s in seqs], seed)
        _table(eng, t)
        p, st = _same(eng, u, seqs, t, 3)
        assert st["tiles"] == (1 if total == TILE else 2)


def test_one_vertex_unitigs_are_the_reads_consensus(eng):
    """A graph without edges: every read is a one-vertex unitig of orientation 0 and its polished sequence is Engine.consensus's, the
    statistics too.  The compaction never emits a one-vertex unitig of orientation 1 (a path v is emitted iff v <= v ^ 1), so
    orientation 1 is held to the same fact where the device can produce it: the last vertex of a path contributes its whole read, and
    with a strand-1 dovetail that vertex has orientation 1 -- its segment is the reverse complement of the read's consensus."""
    seqs = [U.random_genome(n, 80 + i) for i, n in enumerate((1, 15, 16, 17, 1000, 5000, 10000))]
    lens = [len(s) for s in seqs]
    u = _install(eng, seqs, np.zeros(0, G.OVL_DT), {}, None)
    assert u["verts"].tolist() == [2 * r for r in range(len(seqs))]
    t = U.random_table(lens, 4)
    _table(eng, t)
    for md in (1, 3):
        p, _ = _same(eng, u, seqs, t, md)
        offs, bases, stats = eng.consensus(md)
        assert np.array_equal(p["offsets"], offs) and p["bases"].tobytes() == bases.tobytes()
        for f in _lib.CONS_DT.names:
            assert np.array_equal(p["stats"][f].astype(np.uint64), stats[f].astype(np.uint64)), f
    seqs = [U.random_genome(10000, 90), U.random_genome(10000, 91)]
    rec = np.array([(0, 1, 4000, 10000, 0, 6000, 0, 1, (0, 0, 0))], G.OVL_DT)
    u = _install(eng, seqs, rec, {}, {})
    assert u["verts"].tolist() == [0, 3] and u["nbases"].tolist() == [4000, 10000]
    t = U.random_table([10000, 10000], 5)
    _table(eng, t)
    p, _ = _same(eng, u, seqs, t, 3)
    offs, bases, stats = eng.consensus(3)
    raw = p["bases"].tobytes()
    assert raw[int(p["pos"][1]):] == U.revcomp(bases.tobytes()[int(offs[1]):int(offs[2])]) and int(p["nbases"][1]) == int(stats[1]["len_after"])
    assert raw[:int(p["pos"][1])] == P.consensus(seqs[0][:4000], t[:4000], 3)[0]


@pytest.mark.parametrize("name", ["toy120", "toylen80", "sanity3"])
def test_real_traces_equal_the_mirror(eng, name):
    """align -> trace with votes, runs kept -> graph_add_traced -> graph_build (loose and default) -> clean -> unitigs -> polish, against
    the mirror fed with pileup_mirror.pileup of the same traces"""
    g = load_golden(name)
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    tr, ops = eng.trace_pairs(pars, pileup=True, keep_ops=True)
    table, _ = P.pileup(g.seqs, pairs, alns, tr, ops)
    eng.graph_reset()
    eng.graph_add_traced()
    for params in (LOOSE, {}):
        eng.graph_build(**params)
        eng.graph_clean()
        u = eng.graph_unitigs()
        for md in (1, 3):
            p, st = _same(eng, u, g.seqs, table, md)
            print("POLISH %s %s min_depth %d: %d unitigs of %d reads, %d -> %d bases, covered %d, substituted %d, deleted %d, inserted %d"
                  % (name, params or "defaults", md, st["unitigs"], st["vertices"], st["bases_before"], st["bases_after"], st["covered"], st["substituted"],
                     st["deleted"], st["inserted"]))


def test_zero_unitigs_launch_nothing(eng):
    """two reads that contain each other: no live read, no unitig; the polish returns empties"""
    eng.set_reads(synth.ReadSet.from_strings([b"ACGTACGTAC", b"ACGTACGTAC"]))
    eng.graph_add_overlaps(np.array([(0, 1, 0, 10, 0, 10, 0, 0, (0, 0, 0)), (1, 0, 0, 10, 0, 10, 0, 0, (0, 0, 0))], G.OVL_DT))
    eng.graph_build(min_overlap=0)
    u = eng.graph_unitigs()
    assert len(u["len"]) == 0 and len(u["verts"]) == 0
    eng.pileup_reset()
    p = eng.graph_polish_unitigs()
    assert p["offsets"].tolist() == [0] and len(p["bases"]) == 0 and len(p["pos"]) == 0 and len(p["nbases"]) == 0 and len(p["stats"]) == 0
    st = eng.polish_stats()
    assert st["bases_after"] == 0 and st["tiles"] == 0 and st["decide_ms"] == 0 and st["write_ms"] == 0


def test_state_and_errors():
    e = Engine(0)
    try:
        _, seqs, recs, graph, clean = CASES["two_round"]
        STATE, BAD = -7, -3
        e.set_reads(synth.ReadSet.from_strings(seqs))
        e.pileup_reset()
        raises(STATE, e.graph_polish_unitigs)                           # no graph, no unitigs
        e.graph_add_overlaps(recs)
        e.graph_build()
        raises(STATE, e.graph_polish_unitigs)
        raises(STATE, e.polish_stats)
        e.set_reads(synth.ReadSet.from_strings(seqs))                   # (loading reads drops the table)
        e.graph_add_overlaps(recs)
        e.graph_build()
        e.graph_unitigs()
        raises(STATE, e.graph_polish_unitigs)                           # unitigs, no table
        e.pileup_reset()
        raises(BAD, e.graph_polish_unitigs, 0)
        small = _lib.PolishParams(C.sizeof(_lib.PolishParams) - 4, 3)
        assert e.lib.bella_hip_graph_polish_unitigs(e.h, C.byref(small), None) == BAD
        assert e.lib.bella_hip_graph_polish_unitigs(e.h, None, None) == BAD
        ok = _lib.PolishParams(C.sizeof(_lib.PolishParams), 3)
        assert e.lib.bella_hip_graph_polish_unitigs(e.h, C.byref(ok), None) == 0              # total_bases may be NULL
        assert e.lib.bella_hip_graph_get_polished(e.h, None, None, None, None, None) == 0      # any pointer may be NULL
        table = U.random_table([len(s) for s in seqs], 0)
        for drop in (lambda: e.graph_clean(), lambda: e.graph_pop_bubbles(), lambda: e.add_pileup(0, e.nreads, table), lambda: e.pileup_reset(),
                     lambda: e.graph_unitigs()):
            e.graph_unitigs()
            e.graph_polish_unitigs()
            assert e.polish_stats()["unitigs"] >= 1
            drop()
            raises(STATE, e.polish_stats)
            assert e.lib.bella_hip_graph_get_polished(e.h, None, None, None, None, None) == STATE
        e.graph_unitigs()
        e.graph_polish_unitigs()
        e.set_reads(synth.ReadSet.from_strings(seqs))
        raises(STATE, e.polish_stats)
    finally:
        e.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return tuple(files.get(n) for n in ("out.out", "u.gfa", "u.fa", "c.fasta")), files["stderr"]


def test_cli_polish_end_to_end(eng, tmp_path):
    """bella-hip --unitigs --unitigs-fasta --polish on toy120: the files are the mirror's text of the Python path's records and table;
    without --polish they are the raw text; --correct writes the same file with and without --polish; -m 1 and -g 2 give the same files;
    the Unitigs log line says "polished N -> M bases" only with the option"""
    g = load_golden("toy120")
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    tr, ops = eng.trace_pairs(pars, pileup=True, keep_ops=True)
    table, _ = P.pileup(g.seqs, pairs, alns, tr, ops)
    m = (alns["passed"] == 1) & (tr["nops"] > 0)
    recs = np.zeros(int(m.sum()), G.OVL_DT)
    recs["cid"], recs["rid"] = pairs["cid"][m], pairs["rid"][m]
    for f, t in (("begV", "tbegV"), ("endV", "tendV"), ("begH", "tbegH"), ("endH", "tendH")):
        recs[f] = tr[t][m]
    recs["score"], recs["strand"] = alns["score"][m], alns["strand"][m]
    _, _, u = U.case_unitigs(g.seqs, recs, LOOSE, {})
    offs, bases = U.unitig_bases(u, g.seqs)
    raw_gfa, raw_fa = U.unitig_gfa_text(g.names, u, offs, bases), U.fasta_text(u, offs, bases)

    def texts(md):
        p = U.polished(u, g.seqs, table, md)
        q = U.polished_unitigs(u, p)
        return U.unitig_gfa_text(g.names, q, p["offsets"], p["bases"]), U.unitig_gfa_text(g.names, q), U.fasta_text(q, p["offsets"], p["bases"]), p
    pol_gfa, pol_noseq, pol_fa, p3 = texts(3)
    pol_gfa1, _, pol_fa1, _ = texts(1)
    assert pol_gfa != raw_gfa and pol_fa != raw_fa and pol_gfa1 != pol_gfa
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    plain = g.meta["flags"] + ["--tuples", mtx]
    base = plain + ["--gfa-min-overlap", "0", "--gfa-fuzz", "10"]
    utg = ["--unitigs", "u.gfa", "--unitigs-fasta", "u.fa"]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    out0 = g.out["align"]
    got, err = _run([fq], base + utg, str(tmp_path / "raw"))
    assert got == (out0, raw_gfa, raw_fa, None) and b"polished" not in err
    got, err = _run([fq], base + utg + ["--polish"], str(tmp_path / "pol"))
    assert got == (out0, pol_gfa, pol_fa, None)
    assert b"polished %d -> %d bases" % (int(u["len"].sum()), len(p3["bases"])) in err
    assert _run([fq], base + utg + ["--polish", "--polish-min-depth", "1"], str(tmp_path / "md1"))[0] == (out0, pol_gfa1, pol_fa1, None)
    assert _run([fq], base + utg + ["--polish", "--gfa-no-seq"], str(tmp_path / "noseq"))[0] == (out0, pol_noseq, pol_fa, None)
    assert _run([fq], base + ["--unitigs-fasta", "u.fa", "--polish"], str(tmp_path / "fa"))[0] == (out0, None, pol_fa, None)
    cor = _run([fq], plain + ["--correct", "c.fasta"], str(tmp_path / "cor"))[0][3]
    assert cor is not None and cor.count(b">") == g.rs.nreads
    assert _run([fq], base + utg + ["--polish", "--correct", "c.fasta"], str(tmp_path / "polcor"))[0] == (out0, pol_gfa, pol_fa, cor)
    assert _run([fq], base + utg + ["--polish", "-m", "1"], str(tmp_path / "m1"))[0] == (out0, pol_gfa, pol_fa, None)
    assert _run([fq], base + utg + ["--polish", "--correct", "c.fasta", "-g", "2"], str(tmp_path / "g2"), over)[0] == (out0, pol_gfa, pol_fa, cor)


# ---- does it polish? ---------------------------------------------------------------------------------------------------------------
def test_it_polishes_unitigs_of_10kb_reads_at_15_percent_error(eng):
    """The 2,000 x 10 kb, 15 % error, seed-21 set of tests/test_pileup_gpu.py, the same pipeline, then graph (defaults), clean, unitigs,
    polish with min_depth 3.  A fixed-seed sample of 40 vertices among those whose read is interior (start at least one read length from
    either genome end) and whose window of W = 2,000 bases from the segment's start fits inside the unitig, raw and polished.  Each
    window against its template -- with d = strand XOR orientation, genome[s : s + 5W/4] for d = 0, the reverse complement of
    genome[s + L - 5W/4 : s + L] for d = 1 -- by Levenshtein distance with the window consumed whole and the template's end free.
    Condition: the polished sum is BELOW the raw sum (it holds on an MI355X); the test prints both sums, the ratio, the total length raw
    and polished next to the genome span, and the timers -- the line for DESIGN.md section 14."""
    nreads, read_len, seed, md, W = 2000, 10000, 21, 3, 2000
    rs = synth.make_reads(nreads, read_len=read_len, err=0.15, seed=seed)
    glen = max(read_len + 1, round(nreads * read_len / 30.0))
    genome = synth.BASES[np.random.default_rng(seed).integers(0, 4, size=glen, dtype=np.uint8)].tobytes()
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    assert eng.align_pairs(pars) > 2000
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    eng.graph_reset()
    eng.graph_add_traced()
    eng.graph_build()
    eng.graph_clean()
    u = eng.graph_unitigs()
    offs, bases = eng.unitig_bases()
    p = eng.graph_polish_unitigs(md)
    st, ust = eng.polish_stats(), eng.unitig_stats()
    meta = [tuple(int(x) for x in n.split("_")[1:]) for n in rs.names]                   # (start, length, strand)
    slot_utg = np.repeat(np.arange(len(u["len"])), np.diff(u["voff"].astype(np.int64)))
    ok = []
    for i, v in enumerate(u["verts"].tolist()):
        s, L, _ = meta[v >> 1]
        k = int(slot_utg[i])
        if s >= read_len and s + L <= glen - read_len and int(u["pos"][i]) + W <= int(u["len"][k]) and int(p["pos"][i]) + W <= int(p["stats"][k]["len_after"]):
            ok.append(i)
    assert len(ok) >= 40, len(ok)
    drawn = sorted(np.random.default_rng(41).choice(ok, 40, replace=False).tolist())
    raw, pol = bases.tobytes(), p["bases"].tobytes()
    d_raw = d_pol = 0
    for i in drawn:
        v, k = int(u["verts"][i]), int(slot_utg[i])
        s, L, strand = meta[v >> 1]
        t = genome[s:s + 5 * W // 4] if not (strand ^ (v & 1)) else U.revcomp(genome[s + L - 5 * W // 4:s + L])
        a, b = int(offs[k]) + int(u["pos"][i]), int(p["offsets"][k]) + int(p["pos"][i])
        d_raw += U.window_distance(raw[a:a + W], t)
        d_pol += U.window_distance(pol[b:b + W], t)
    span = max(s + L for s, L, _ in meta) - min(s for s, _, _ in meta)
    print("POLISH 2000 x 10 kb, 15 %% error, min_depth %d: %d unitigs, %d qualifying vertices, 40 windows of %d: distance to the template raw %d (%.2f %%), "
          "polished %d (%.2f %%), ratio %.3f; total length raw %d, polished %d, genome span %d; substituted %d, deleted %d, inserted %d; decide %.3f ms, write %.3f ms, "
          "gather %.3f ms" % (md, len(u["len"]), len(ok), W, d_raw, 100.0 * d_raw / (40 * W), d_pol, 100.0 * d_pol / (40 * W), d_pol / max(d_raw, 1), st["bases_before"],
                              st["bases_after"], span, st["substituted"], st["deleted"], st["inserted"], st["decide_ms"], st["write_ms"], ust["gather_ms"]))
    assert d_pol < d_raw, (d_pol, d_raw)
