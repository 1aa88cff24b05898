"""GPU tests of the realignment round: the device result EQUALS the mirror (bella_testkit/realign_mirror.py) --
placements, alignment records, runs, table, bases, pos / nbases, counts -- on the synthetic layouts of bella_testkit/realign_cases.py,
over two rounds, on real traces; the same round in many batches (BELLA_TUNE_ROUND_BUDGET); state and errors; and the measured effect
on 2,000 reads of 10 kb at 15 % error."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib
from bella_testkit import graph_mirror as G
from bella_testkit import realign_cases as RC
from bella_testkit import realign_mirror as R
from bella_testkit import synth
from bella_testkit import unitig_mirror as U
from bella_testkit import pileup_mirror as P
from bella_testkit.pipeline import aligned as _aligned, dps_and_largest_job, raises, realign_getters, run_cli, same_but_for_the_batching, with_round_budget
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

SEEN = dict(first_base=False, last_base=False, orient1=False, anchor_v=False, anchor_h_strand1=False, tie=False, unplaced=False, outside=False, origin=False,
            doubled=False, capped=False, low_identity=False, wide=False, one_vertex=False, trim=False)
RUNS = {"doubling": dict(band0=256, band_max=2048), "capped": dict(band0=512, band_max=512), "wide": dict(band0=2048, band_max=4096)}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _install(eng, seqs, recs, graph, trim=None):
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    if trim is not None:
        eng.graph_trim(**trim)
    eng.graph_build(**graph)
    eng.graph_clean()
    return eng.graph_unitigs()


def _polish(eng, table, md=3):
    eng.pileup_reset()
    if table is not None:
        eng.add_pileup(0, eng.nreads, table)
    return eng.graph_polish_unitigs(md)


def _same(eng, u, cur, seqs, recs, clips=None, **params):
    """one round on the device against the mirror's round on `cur`: -> (device result, mirror result, placements)"""
    got = eng.graph_realign_unitigs(keep_ops=1, **params)
    cont, rem = eng.graph()[2], eng.graph_removed()
    m = R.realign_round(u, cur, seqs, recs, cont, rem, clips, **{**R.DEFAULTS, **params})
    pl = eng.realign_placements()
    assert pl.dtype == _lib.PLACE_DT == R.PLACE_DT
    for f in R.COMPARED:
        assert np.array_equal(pl[f], m["placements"][f]), (f, pl[f], m["placements"][f])
    ops, table = eng.realign_ops()
    for r in np.flatnonzero(pl["status"] == R.VOTED).tolist():
        assert np.array_equal(ops[int(pl[r]["op_off"]):int(pl[r]["op_off"]) + int(pl[r]["nops"])], m["ops"][r]), r
    assert len(ops) == sum(len(x) for x in m["ops"].values())
    assert np.array_equal(table, m["table"])
    assert got["offsets"].dtype == np.uint64 and np.array_equal(got["offsets"], m["offsets"])
    assert got["bases"].tobytes() == m["bases"]
    assert got["pos"].dtype == np.uint64 and np.array_equal(got["pos"], m["pos"])
    assert got["nbases"].dtype == np.uint32 and np.array_equal(got["nbases"], m["nbases"])
    for f in U.POLISH_DT.names:
        assert np.array_equal(got["stats"][f], m["stats"][f]), f
    st = eng.realign_stats()
    want = dict(m["counts"], bases_before=int(cur["offsets"][-1]), bases_after=len(m["bases"]))
    for f in ("substituted", "deleted", "inserted"):
        want[f] = int(m["stats"][f].sum())
    assert {k: st[k] for k in want} == want
    return got, m, pl


@pytest.mark.parametrize("run", list(RUNS))
def test_the_line_equals_the_mirror(eng, run):
    """the line of realign_cases.py, polished with its table, under three band settings: doubling from 256, capped at 512, and the wide
    kernel from 2,048"""
    seqs, recs = RC.line_case()
    u = _install(eng, seqs, recs, RC.GRAPH)
    assert u["len"].tolist() == [6800, 900]
    p = _polish(eng, RC.line_table(seqs))
    assert len(p["bases"]) != 7700
    got, m, pl = _same(eng, u, p, seqs, recs, **RUNS[run])
    st = eng.realign_stats()
    print("REALIGN line %s: %s; dp %.3f ms, walk %.3f ms, vote %.3f ms, decide %.3f ms, %d batches" % (run, m["counts"], st["dp_ms"], st["walk_ms"], st["vote_ms"], st["decide_ms"],
                                                                                                      st["batches"]))
    plen = int(p["offsets"][1])
    voted = pl["status"] == R.VOTED
    SEEN["first_base"] |= bool((voted & (pl["q_begin"] == 0) & (pl["unitig"] == 0)).any())
    SEEN["last_base"] |= bool((voted & (pl["q_end"] == plen) & (pl["unitig"] == 0)).any())
    SEEN["orient1"] |= bool((voted & (pl["orient"] == 1)).any())
    SEEN["unplaced"] |= bool((pl["status"] == R.UNPLACED).any())
    SEEN["outside"] |= bool((pl["status"] == R.OUTSIDE).any())
    SEEN["low_identity"] |= bool((pl["status"] == R.LOW_IDENTITY).any())
    SEEN["capped"] |= bool((pl["status"] == R.BAND_CAPPED).any()) and RUNS[run]["band_max"] == 512
    SEEN["doubled"] |= bool((voted & (pl["band"] == 512)).any()) and RUNS[run]["band0"] == 256
    SEEN["wide"] |= bool((voted & (pl["band"] == 2048)).any())
    SEEN["one_vertex"] |= bool(voted[14]) and int(u["voff"][2] - u["voff"][1]) == 1
    for r in np.flatnonzero(voted & (pl["anchor"] != R.NO)).tolist():
        rec = recs[int(pl[r]["anchor"])]
        SEEN["anchor_v"] |= int(rec["rid"]) == r
        SEEN["anchor_h_strand1"] |= int(rec["cid"]) == r and int(rec["strand"]) == 1
    both = [x for x, rec in enumerate(recs) if 2 in (int(rec["cid"]), int(rec["rid"])) and {int(rec["cid"]), int(rec["rid"])} & set(RC.BACKBONE)]
    SEEN["tie"] |= len(both) == 2 and int(pl[2]["anchor"]) == min(both) and int(recs[both[0]]["endH"] - recs[both[0]]["begH"]) == int(recs[both[1]]["endV"] - recs[both[1]]["begV"])


# ---- the line in many batches (BELLA_TUNE_ROUND_BUDGET) ----------------------------------------------------------------------------
DP_RAN = (R.VOTED, R.LOW_IDENTITY, R.BAND_CAPPED)
LINE_RUNS = {}                                                          # run -> the line's round under the default budget, made once


def _line_round(eng, run, budget=None):
    """the line polished with its table, one round of RUNS[run] under round_budget = budget (None: the default rule): -> realign_getters"""
    if budget is None and run in LINE_RUNS:
        return LINE_RUNS[run]
    seqs, recs = RC.line_case()
    _install(eng, seqs, recs, RC.GRAPH)
    _polish(eng, RC.line_table(seqs))
    out = with_round_budget(eng, budget, lambda: realign_getters(eng, keep_ops=1, **RUNS[run]))
    if budget is None:
        LINE_RUNS[run] = out
    return out


def _dps(x, band0):
    """of the reads whose DP ran (no trim: a job's n is its read's length)"""
    ran = np.isin(x["placements"]["status"], DP_RAN)
    return dps_and_largest_job(x["placements"]["band"][ran], np.array([len(s) for s in RC.line_case()[0]])[ran], band0)


@pytest.mark.parametrize("run", list(RUNS))
def test_the_line_in_one_job_per_batch(eng, run):
    """round_budget = 1: every batch takes exactly one job, so dir_off, op_off and the pending list carry over after every job"""
    one, many = _line_round(eng, run), _line_round(eng, run, 1)
    same_but_for_the_batching(one, many)
    ndp, largest = _dps(many, RUNS[run]["band0"])
    print("REALIGN line %s: %d batches by default, %d with one job per batch, peak %d -> %d direction bytes" % (run, one["st"]["batches"], many["st"]["batches"],
                                                                                                             one["st"]["dir_bytes_peak"], many["st"]["dir_bytes_peak"]))
    assert many["st"]["batches"] == ndp > one["st"]["batches"]
    assert many["st"]["dir_bytes_peak"] == largest


def test_a_budget_that_cuts_inside_a_band(eng):
    """`doubling` with room for two of the largest job at band0: a batch ends because the next job would not fit, the jobs of one band
    are spread over several batches and dir_off starts again in each"""
    one = _line_round(eng, "doubling")
    band0 = RUNS["doubling"]["band0"]
    ndp, largest = _dps(one, band0)
    ran = np.isin(one["placements"]["status"], DP_RAN)
    budget = 2 * max(len(s) for s, r in zip(RC.line_case()[0], ran) if r) * band0 // 4
    some = _line_round(eng, "doubling", budget)
    same_but_for_the_batching(one, some)
    print("REALIGN line doubling: budget %d: %d batches of %d DPs, peak %d" % (budget, some["st"]["batches"], ndp, some["st"]["dir_bytes_peak"]))
    assert 1 < some["st"]["batches"] < ndp
    assert some["st"]["dir_bytes_peak"] <= max(budget, largest)                     # (a job that does not fit runs alone)


def test_two_rounds_equal_the_mirrors_two_rounds(eng):
    seqs, recs = RC.line_case()
    u = _install(eng, seqs, recs, RC.GRAPH)
    p = _polish(eng, RC.line_table(seqs))
    got, m, _ = _same(eng, u, p, seqs, recs, band0=256)
    assert eng.realign_stats()["round"] == 1
    got2, m2, _ = _same(eng, u, m, seqs, recs, band0=256)
    assert eng.realign_stats()["round"] == 2 and eng.realign_stats()["bases_before"] == len(m["bases"])
    assert got2["bases"].tobytes() != p["bases"].tobytes()


def test_a_circular_unitig_skips_the_reads_across_its_origin(eng):
    seqs, recs = RC.circle_case()
    u = _install(eng, seqs, recs, RC.GRAPH)
    assert u["circular"].tolist() == [1] and u["len"].tolist() == [6000]
    p = _polish(eng, None)
    got, m, pl = _same(eng, u, p, seqs, recs, band0=256)
    assert (pl["status"] == R.OUTSIDE).sum() == 2 and (pl["e"][pl["status"] == R.OUTSIDE] > 6000 + 128).all()
    SEEN["origin"] = True


def test_a_trim_in_force(eng):
    """the line, trimmed with min_depth 2: the reads that vote are aligned clip by clip"""
    seqs, recs = RC.line_case()
    u = _install(eng, seqs, recs, RC.GRAPH, trim=dict(min_depth=2, end_clip=20, min_span=200))
    clips = eng.graph_clips()
    p = _polish(eng, RC.line_table(seqs))
    got, m, pl = _same(eng, u, p, seqs, recs, clips=(clips["beg"], clips["end"]), band0=256)
    lens = np.array([len(s) for s in seqs])
    voted = pl["status"] == R.VOTED
    SEEN["trim"] = bool((voted & ((clips["beg"] > 0) | (clips["end"] < lens))).any())


def test_the_synthetic_set_covers_what_it_should():
    """over the cases above (pytest keeps file order): a voter at the unitig's first base and one at its last, orientation 1, an anchor
    that is V and one that is H' with strand 1, the tie between two anchors of equal span, an unplaced and an outside read, the reads
    across a circle's origin, a doubled band, a capped read, a low-identity read, the wide kernel, a one-vertex unitig, a trim"""
    assert all(SEEN.values()), SEEN


def test_without_a_voter_the_result_is_the_input(eng):
    """one read, one unitig, polished with a random table; with min_identity 1000 the read no longer equals it and does not vote"""
    seqs = [U.random_genome(1500, 183)]
    u = _install(eng, seqs, np.zeros(0, G.OVL_DT), {})
    p = _polish(eng, U.random_table([1500], 1))
    got, m, pl = _same(eng, u, p, seqs, np.zeros(0, G.OVL_DT), band0=256, min_identity=1000)
    assert pl["status"].tolist() == [R.LOW_IDENTITY] and eng.realign_stats()["votes"] == 0
    assert got["bases"].tobytes() == p["bases"].tobytes() and np.array_equal(got["pos"], p["pos"]) and np.array_equal(got["nbases"], p["nbases"])


@pytest.mark.parametrize("name", ["toy120", "toylen80", "sanity3"])
def test_real_traces_equal_the_mirror(eng, name):
    g = load_golden(name)
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    eng.graph_reset()
    eng.graph_add_traced()
    recs = eng.graph_overlaps()
    eng.graph_build(min_overlap=0, fuzz=10)
    eng.graph_clean()
    u = eng.graph_unitigs()
    p = eng.graph_polish_unitigs(3)
    got, m, pl = _same(eng, u, p, g.seqs, recs, band0=256)
    print("REALIGN %s: %d unitigs, %d -> %d -> %d bases, %s" % (name, len(u["len"]), int(u["len"].sum()), len(p["bases"]), len(got["bases"]), m["counts"]))


def test_zero_unitigs_launch_nothing(eng):
    eng.set_reads(synth.ReadSet.from_strings([b"ACGTACGTAC", b"ACGTACGTAC"]))
    eng.graph_add_overlaps(np.array([(0, 1, 0, 10, 0, 10, 0, 0, (0, 0, 0)), (1, 0, 0, 10, 0, 10, 0, 0, (0, 0, 0))], G.OVL_DT))
    eng.graph_build(min_overlap=0)
    eng.graph_unitigs()
    eng.pileup_reset()
    eng.graph_polish_unitigs()
    r = eng.graph_realign_unitigs()
    assert r["offsets"].tolist() == [0] and len(r["bases"]) == 0 and len(r["pos"]) == 0
    st = eng.realign_stats()
    assert st["batches"] == 0 and st["dp_ms"] == 0 and st["voted"] == 0 and st["round"] == 1
    assert (eng.realign_placements()["status"] == R.NONE).all()


def test_state_and_errors():
    e = Engine(0)
    try:
        STATE, BAD = -7, -3
        seqs, recs = RC.circle_case()
        e.set_reads(synth.ReadSet.from_strings(seqs))
        e.graph_add_overlaps(recs)
        e.graph_build(**RC.GRAPH)
        e.graph_unitigs()
        e.pileup_reset()
        raises(STATE, e.graph_realign_unitigs)                          # before the polish
        raises(STATE, e.realign_stats)
        e.graph_polish_unitigs()
        raises(STATE, e.realign_placements)
        for bad in (dict(band0=300), dict(band0=128), dict(band0=1024, band_max=512), dict(band_max=1 << 19), dict(min_depth=0), dict(min_identity=1001)):
            raises(BAD, lambda: e.graph_realign_unitigs(**bad))
        small = _lib.RealignParams(C.sizeof(_lib.RealignParams) - 4, 512, 4096, 700, 3, 0)
        assert e.lib.bella_hip_graph_realign_unitigs(e.h, C.byref(small), None) == BAD
        assert e.lib.bella_hip_graph_realign_unitigs(e.h, None, None) == 0                  # the defaults; total_bases may be NULL
        assert e.lib.bella_hip_graph_get_realigned(e.h, None, None, None, None, None) == 0

        def batches():                                                  # of the first round after a polish
            e.graph_polish_unitigs()
            e.graph_realign_unitigs(band0=256)
            return e.realign_stats()["batches"]
        by_default = batches()
        e.set_tuning("round_budget", 1)
        assert batches() > by_default
        e.set_tuning("round_budget")                                    # no value: the default rule again
        assert batches() == by_default
        e.set_tuning("round_budget", 1)
        e.set_tuning("round_budget", 0)                                 # and so does 0
        assert batches() == by_default
        for drop in (lambda: e.graph_cut_weak(), lambda: e.pileup_reset(), lambda: e.graph_polish_unitigs(), lambda: e.graph_unitigs()):
            e.graph_unitigs()
            e.pileup_reset()
            e.graph_polish_unitigs()
            e.graph_realign_unitigs(band0=256)
            assert e.realign_stats()["round"] == 1
            drop()
            raises(STATE, e.realign_stats)
            assert e.lib.bella_hip_graph_get_realigned(e.h, None, None, None, None, None) == STATE
    finally:
        e.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return tuple(files.get(n) for n in ("out.out", "u.gfa", "u.fa")), files["stderr"]


def test_cli_polish_rounds_end_to_end(eng, tmp_path):
    """bella-hip --unitigs --unitigs-fasta --polish --polish-rounds 2 on toy120: the files are the mirror's text of a realignment round on
    the mirror's polish; with --polish-rounds 1 and without the option they are the --polish files byte for byte; -m 1 and -g 2 give the
    same files; the "Realigned" log line appears only with a second round"""
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
    gm, cm, u = U.case_unitigs(g.seqs, recs, dict(min_overlap=0, fuzz=10), {})
    p = U.polished(u, g.seqs, table, 3)
    r = R.realign_round(u, p, g.seqs, recs, gm["contained"], cm["removed"], None, band0=256)

    def texts(x):
        q = U.polished_unitigs(u, x)
        return U.unitig_gfa_text(g.names, q, x["offsets"], x["bases"]), U.fasta_text(q, x["offsets"], x["bases"])
    pol_gfa, pol_fa = texts(p)
    rea_gfa, rea_fa = texts(r)
    assert rea_gfa != pol_gfa and rea_fa != pol_fa
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r_ + 1, k + 1, q) for k, r_, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx, "--gfa-min-overlap", "0", "--gfa-fuzz", "10", "--unitigs", "u.gfa", "--unitigs-fasta", "u.fa", "--polish"]
    two = ["--polish-rounds", "2", "--realign-band", "256"]
    out0 = g.out["align"]
    got, err = _run([fq], base, str(tmp_path / "pol"))
    assert got == (out0, pol_gfa, pol_fa) and b"Realigned" not in err
    got, err = _run([fq], base + ["--polish-rounds", "1"], str(tmp_path / "one"))
    assert got == (out0, pol_gfa, pol_fa) and b"Realigned" not in err
    got, err = _run([fq], base + two, str(tmp_path / "two"))
    assert got == (out0, rea_gfa, rea_fa)
    c = r["counts"]
    assert b"Realigned = round 2: %d of %d reads realigned" % (c["voted"], c["backbone"] + c["contained"] + c["unplaced"]) in err
    assert b"%d -> %d bases" % (len(p["bases"]), len(r["bases"])) in err
    assert _run([fq], base + two + ["-m", "1"], str(tmp_path / "m1"))[0] == (out0, rea_gfa, rea_fa)
    assert _run([fq], base + two + ["-g", "2"], str(tmp_path / "g2"), {"BELLA_HIP_OVERSUBSCRIBE": "1"})[0] == (out0, rea_gfa, rea_fa)


# ---- does it help? -----------------------------------------------------------------------------------------------------------------
def test_a_second_round_improves_unitigs_of_10kb_reads_at_15_percent_error(eng):
    """The set, the pipeline and the 40 windows of tests/test_polish_gpu.py's last test; the windows are located through the new pos.
    Condition: the summed window distance after one realignment round is BELOW the polished one.  Prints the raw, polished, round-2 and
    round-3 sums, the lengths next to the genome span, the read counts by status and the timers."""
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
    trace_dp_ms = eng.trace_stats().dp_ms
    eng.graph_reset()
    eng.graph_add_traced()
    eng.graph_build()
    eng.graph_clean()
    u = eng.graph_unitigs()
    offs, bases = eng.unitig_bases()
    p = eng.graph_polish_unitigs(md)
    r2 = eng.graph_realign_unitigs()
    st2 = eng.realign_stats()
    r3 = eng.graph_realign_unitigs()
    st3 = eng.realign_stats()
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
    seq = [bases.tobytes()] + [x["bases"].tobytes() for x in (p, r2, r3)]
    where = [(offs, u["pos"])] + [(x["offsets"], x["pos"]) for x in (p, r2, r3)]
    d = [0, 0, 0, 0]
    for i in drawn:
        v, k = int(u["verts"][i]), int(slot_utg[i])
        s, L, strand = meta[v >> 1]
        t = genome[s:s + 5 * W // 4] if not (strand ^ (v & 1)) else U.revcomp(genome[s + L - 5 * W // 4:s + L])
        for j in range(4):
            a = int(where[j][0][k]) + int(where[j][1][i])
            d[j] += U.window_distance(seq[j][a:a + W], t)
    span = max(s + L for s, L, _ in meta) - min(s for s, _, _ in meta)
    by_status = {k: st2[k] for k in ("backbone", "contained", "unplaced", "outside", "band_capped", "low_identity", "voted", "repeated")}
    print("REALIGN 2000 x 10 kb, 15 %% error: 40 windows of %d: distance to the template raw %d (%.2f %%), polished %d (%.2f %%), round 2 %d (%.2f %%), round 3 %d (%.2f %%); "
          "total length raw %d, polished %d, round 2 %d, round 3 %d, genome span %d; round 2 reads %s; round 2 place %.3f ms, dp %.3f ms (the first trace's dp %.3f ms), walk %.3f ms, "
          "vote %.3f ms, decide %.3f ms, %d batches, %d dp cells, %d direction bytes at the peak; round 3 dp %.3f ms, voted %d"
          % (W, d[0], d[0] / (0.4 * W), d[1], d[1] / (0.4 * W), d[2], d[2] / (0.4 * W), d[3], d[3] / (0.4 * W), len(seq[0]), len(seq[1]), len(seq[2]), len(seq[3]), span, by_status,
             st2["place_ms"], st2["dp_ms"], trace_dp_ms, st2["walk_ms"], st2["vote_ms"], st2["decide_ms"], st2["batches"], st2["dp_cells"], st2["dir_bytes_peak"], st3["dp_ms"],
             st3["voted"]))
    assert d[2] < d[1], (d[2], d[1])
