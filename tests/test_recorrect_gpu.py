"""GPU tests of the read correction rounds: the device result EQUALS the mirror (bella_testkit/recorrect_mirror.py)
-- jobs, runs, table, offsets, bases, per-read statistics, anchors, counts -- on realign_cases.line_case, on the layout of
bella_testkit/recorrect_cases.py under three band settings, in many batches (BELLA_TUNE_ROUND_BUDGET), over two rounds, on real traces; state and errors; the command line; and
the measured effect on 2,000 reads of 10 kb at 15 % error."""
import ctypes as C
import gzip
import multiprocessing as mp
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import graph_mirror as G
from bella_testkit import pileup_mirror as P
from bella_testkit import realign_cases as LC
from bella_testkit import recorrect_cases as RC
from bella_testkit import recorrect_mirror as M
from bella_testkit import synth
from bella_testkit import trace_mirror as T
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import aligned as _aligned, dps_and_largest_job, raises, recorrect_getters, run_cli, same_but_for_the_batching, with_round_budget
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

SEEN = dict(side0_strand0=False, side0_strand1=False, side1_strand0=False, side1_strand1=False, first_base=False, last_base=False, short_target=False,
            two_steps_target=False, crosses_anchor=False, doubled=False, capped=False, low_identity=False, wide=False, pair_twice=False, no_record=False,
            empty_target=False)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _round1(eng, seqs, recs, table, md=3):
    """reads, records and the round-1 pileup on the device; the consensus EQUALS the mirror's round 1, anchors included: -> that round"""
    eng.set_reads(synth.ReadSet.from_strings(seqs))
    eng.graph_add_overlaps(recs)
    eng.pileup_reset()
    if table is not None:
        eng.add_pileup(0, eng.nreads, table)
    return _is_round1(eng, seqs, eng.get_pileup(0, eng.nreads).reshape(-1, 9) if table is None else table, md)


def _is_round1(eng, seqs, table, md=3):
    offs, bases, stats = eng.consensus(md)
    cur = M.first_round(seqs, table, md)
    assert np.array_equal(offs, cur["offsets"]) and bases.tobytes() == cur["bases"]
    _same_anchors(eng, cur)
    return cur


def _same_anchors(eng, m):
    aoff, anch = eng.recorrect_anchors()
    want_off, want = M.flat_anchors(m["anchors"])
    assert aoff.dtype == np.uint64 and np.array_equal(aoff, want_off) and np.array_equal(anch, want)


def _same(eng, cur, seqs, recs, **params):
    """one round on the device against the mirror's round on `cur`: -> (mirror result, device jobs)"""
    offs, bases, stats = eng.recorrect(keep_ops=1, **params)
    m = M.recorrect_round(cur, seqs, recs, **{**M.DEFAULTS, **params})
    J = eng.recorrect_jobs()
    assert J.dtype == _lib.RECJOB_DT == M.JOB_DT and len(J) == 2 * len(recs)
    for f in M.COMPARED:
        assert np.array_equal(J[f], m["jobs"][f]), (f, J[f], m["jobs"][f])
    ops, table = eng.recorrect_ops()
    for x in np.flatnonzero(J["status"] == M.VOTED).tolist():
        assert np.array_equal(ops[int(J[x]["op_off"]):int(J[x]["op_off"]) + int(J[x]["nops"])], m["ops"][x]), x
    assert len(ops) == sum(len(x) for x in m["ops"].values())
    assert np.array_equal(table, m["table"])
    assert offs.dtype == np.uint64 and np.array_equal(offs, m["offsets"])
    assert bases.tobytes() == m["bases"]
    assert stats.dtype == _lib.CONS_DT == M.CONS_DT
    for f in M.CONS_DT.names:
        assert np.array_equal(stats[f], m["stats"][f]), f
    _same_anchors(eng, m)
    st = eng.recorrect_stats()
    want = dict(m["counts"], bases_before=int(cur["offsets"][-1]), bases_after=len(m["bases"]))
    for f in ("substituted", "deleted", "inserted"):
        want[f] = int(m["stats"][f].sum())
    assert {k: st[k] for k in want} == want
    return m, J


def test_the_line_equals_the_mirror(eng):
    """realign_cases.line_case: its reads and records, the round-1 pileup from line_table -- pileup_reset, add_pileup, consensus(3), one round"""
    seqs, recs = LC.line_case()
    cur = _round1(eng, seqs, recs, LC.line_table(seqs))
    assert cur["bases"] != b"".join(seqs)
    m, J = _same(eng, cur, seqs, recs, band0=256)
    st = eng.recorrect_stats()
    assert st["round"] == 2 and st["jobs"] == 2 * len(recs)
    print("RECORRECT line: %s; place %.3f ms, dp %.3f ms, walk %.3f ms, vote %.3f ms, decide %.3f ms, %d batches"
          % (m["counts"], st["place_ms"], st["dp_ms"], st["walk_ms"], st["vote_ms"], st["decide_ms"], st["batches"]))


@pytest.mark.parametrize("run", list(RC.RUNS))
def test_the_mixed_case_equals_the_mirror(eng, run):
    """recorrect_cases.mixed_case under three band settings: doubling from 256, capped at 512, and the wide kernel from 2,048"""
    seqs, recs = RC.mixed_case()
    cur = _round1(eng, seqs, recs, RC.mixed_table(seqs))
    m, J = _same(eng, cur, seqs, recs, **RC.RUNS[run])
    st = eng.recorrect_stats()
    print("RECORRECT mixed %s: %s; dp %.3f ms, walk %.3f ms, vote %.3f ms, %d batches" % (run, m["counts"], st["dp_ms"], st["walk_ms"], st["vote_ms"], st["batches"]))
    lens = np.array([len(s) for s in seqs])
    plen = np.diff(cur["offsets"].astype(np.int64))
    voted = J["status"] == M.VOTED
    for side in (0, 1):
        for strand in (0, 1):
            SEEN["side%d_strand%d" % (side, strand)] |= bool((voted & (J["side"] == side) & (J["orient"] == strand)).any())
    _, W = M.jobs(recs, lens)
    SEEN["first_base"] |= bool((voted & (W[:, 0] == 0) & (J["q_begin"] == 0)).any())
    SEEN["last_base"] |= bool((voted & (W[:, 1] == lens[J["target"]]) & (J["q_end"] == plen[J["target"]])).any())
    SEEN["short_target"] |= bool((voted & (J["target"] == RC.SHORT)).any()) and lens[RC.SHORT] < M.STEP
    SEEN["two_steps_target"] |= bool((voted & (J["target"] == RC.TWO_STEPS)).any()) and lens[RC.TWO_STEPS] == 2 * M.STEP
    SEEN["crosses_anchor"] |= bool((voted & (W[:, 0] // M.STEP != (W[:, 1] - 1) // M.STEP)).any())
    SEEN["doubled"] |= bool((voted & (J["band"] == 512)).any()) and RC.RUNS[run]["band0"] == 256
    SEEN["capped"] |= bool((J["status"] == M.BAND_CAPPED).any()) and RC.RUNS[run]["band_max"] == 512
    SEEN["low_identity"] |= bool((J["status"] == M.LOW_IDENTITY).any())
    SEEN["wide"] |= bool((voted & (J["band"] == 2048)).any())
    twice = np.flatnonzero((recs["cid"] == RC.PAIR_TWICE[0]) & (recs["rid"] == RC.PAIR_TWICE[1]))
    SEEN["pair_twice"] |= len(twice) == 2 and bool(voted[2 * twice].all() and voted[2 * twice + 1].all())
    a, z = (int(x) for x in cur["offsets"][RC.NO_RECORD:RC.NO_RECORD + 2])
    b, y = (int(x) for x in m["offsets"][RC.NO_RECORD:RC.NO_RECORD + 2])
    SEEN["no_record"] |= not (set(recs["cid"].tolist()) | set(recs["rid"].tolist())) & {RC.NO_RECORD} and m["bases"][b:y] == cur["bases"][a:z] == seqs[RC.NO_RECORD]
    SEEN["empty_target"] |= plen[RC.EMPTY] == 0 and bool(((J["status"] == M.NONE) & (J["target"] == RC.EMPTY)).any())


@pytest.mark.parametrize("run", list(RC.RUNS))
def test_the_mixed_case_in_many_batches(eng, run):
    """BELLA_TUNE_ROUND_BUDGET: the mixed case with one job per batch (budget 1) and with room for two of the largest job at band0 (a
    batch ends because the next job would not fit) against the default budget -- sequences, offsets, per-read statistics, anchors, job
    records with op_off, kept runs, table and counts are the same; then a second round on top with one job per batch EQUALS the mirror's
    second round: the round's buffers are handed to the context as before"""
    seqs, recs = RC.mixed_case()
    cur = _round1(eng, seqs, recs, RC.mixed_table(seqs))
    params = RC.RUNS[run]

    def round2(budget):
        eng.consensus(3)                                               # (round 1 again: the round before goes)
        return with_round_budget(eng, budget, lambda: recorrect_getters(eng, keep_ops=1, **params))
    one = round2(None)
    J = one["jobs"]
    ran = np.isin(J["status"], (M.VOTED, M.LOW_IDENTITY, M.BAND_CAPPED))
    n = J["qend"][ran].astype(np.int64) - J["qbeg"][ran]               # (a job's rows: the query's clip)
    ndp, largest = dps_and_largest_job(J["band"][ran], n, params["band0"])
    two_jobs = 2 * int(n.max()) * params["band0"] // 4
    many, some = round2(1), round2(two_jobs)
    same_but_for_the_batching(one, many)
    same_but_for_the_batching(one, some)
    print("RECORRECT mixed %s: %d batches by default, %d with budget %d, %d with one job per batch (%d DPs)"
          % (run, one["st"]["batches"], some["st"]["batches"], two_jobs, many["st"]["batches"], ndp))
    assert many["st"]["batches"] == ndp > one["st"]["batches"] and many["st"]["dir_bytes_peak"] == largest
    assert 1 < some["st"]["batches"] < ndp and some["st"]["dir_bytes_peak"] <= max(two_jobs, largest)     # (a job that does not fit runs alone)
    eng.consensus(3)
    m, _ = with_round_budget(eng, 1, lambda: _same(eng, cur, seqs, recs, **params))
    with_round_budget(eng, 1, lambda: _same(eng, m, seqs, recs, **params))
    assert eng.recorrect_stats()["round"] == 3 and eng.recorrect_stats()["batches"] > one["st"]["batches"]


def test_the_synthetic_set_covers_what_it_should():
    """over the three runs above (pytest keeps file order): voters on both sides and both strands, a window at a target's first base and
    one at its last, a target shorter than one anchor step and one of exactly two, a window across an anchor, a doubled, a capped, a
    low-identity and a wide job, two records of one pair, a read without a record that comes out unchanged, a target whose round-1
    consensus is empty"""
    assert all(SEEN.values()), SEEN


def test_two_rounds_equal_the_mirrors_two_rounds(eng):
    """the anchors compose: round 3 on the device reads round 2's sequences and anchors, as the mirror's does"""
    seqs, recs = RC.mixed_case()
    cur = _round1(eng, seqs, recs, RC.mixed_table(seqs))
    m, _ = _same(eng, cur, seqs, recs, band0=256)
    assert eng.recorrect_stats()["round"] == 2
    m2, _ = _same(eng, m, seqs, recs, band0=256)
    st = eng.recorrect_stats()
    assert st["round"] == 3 and st["bases_before"] == len(m["bases"])
    assert m["bases"] != cur["bases"]
    offs, bases, _ = eng.consensus(3)                                  # (round 1 again: the rounds go)
    assert bases.tobytes() == cur["bases"]
    raises(-7, eng.recorrect_stats)


@pytest.mark.parametrize("name", ["toy120", "toylen80", "sanity3"])
def test_real_traces_equal_the_mirror(eng, name):
    """align, trace with pileup, graph_add_traced, consensus, one round.  The pileup and so round 1 are those of ALL traced pairs; the
    round itself runs on every n-th of their records (about 48 of them) so that the numpy mirror of two DPs per record stays within
    seconds"""
    g = load_golden(name)
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    eng.graph_reset()
    eng.graph_add_traced()
    recs = eng.graph_overlaps()
    recs = recs[::max(1, len(recs) // 48)]
    eng.graph_reset()
    eng.graph_add_overlaps(recs)
    assert name == "sanity3" or ((recs["strand"] == 1).any() and (recs["strand"] == 0).any())
    cur = _is_round1(eng, g.seqs, eng.get_pileup(0, eng.nreads).reshape(-1, 9))
    m, J = _same(eng, cur, g.seqs, recs, band0=256)
    print("RECORRECT %s: %d records, %d -> %d -> %d bases, %s" % (name, len(recs), sum(len(s) for s in g.seqs), len(cur["bases"]), len(m["bases"]), m["counts"]))


def test_zero_records_launch_nothing(eng):
    seqs = [U.random_genome(700, 5), U.random_genome(300, 6)]
    cur = _round1(eng, seqs, np.zeros(0, G.OVL_DT), U.random_table([700, 300], 2))
    offs, bases, stats = eng.recorrect()
    assert np.array_equal(offs, cur["offsets"]) and bases.tobytes() == cur["bases"]
    assert stats["len_before"].tolist() == stats["len_after"].tolist() == np.diff(cur["offsets"].astype(np.int64)).tolist() and not stats["substituted"].any()
    st = eng.recorrect_stats()
    assert st["batches"] == 0 and st["dp_ms"] == 0 and st["place_ms"] == 0 and st["voted"] == 0 and st["jobs"] == 0 and st["round"] == 2
    assert len(eng.recorrect_jobs()) == 0
    _same_anchors(eng, cur)
    m, _ = _same(eng, cur, seqs, np.zeros(0, G.OVL_DT))                # (and a second one: round 3 of nothing)
    assert eng.recorrect_stats()["round"] == 3


def test_every_current_sequence_empty(eng):
    """two reads whose round-1 table deletes every position: both jobs of their record are NONE, nothing is aligned, nothing comes out"""
    seqs = [U.random_genome(60, 8), U.random_genome(50, 9)]
    table = np.zeros((110, 9), np.uint32)
    table[:, 4] = 9
    recs = np.array([(0, 1, 5, 45, 0, 40, 0, 1, (0, 0, 0))], G.OVL_DT)
    cur = _round1(eng, seqs, recs, table)
    assert len(cur["bases"]) == 0
    m, J = _same(eng, cur, seqs, recs)
    st = eng.recorrect_stats()
    assert J["status"].tolist() == [M.NONE, M.NONE] and st["none"] == 2 and st["batches"] == 0 and st["bases_after"] == 0


def test_state_and_errors():
    e = Engine(0)
    try:
        STATE, BAD = -7, -3
        seqs, recs = RC.mixed_case()
        e.set_reads(synth.ReadSet.from_strings(seqs))
        e.graph_add_overlaps(recs)
        e.pileup_reset()
        raises(STATE, e.recorrect)                                     # before the consensus
        raises(STATE, e.recorrect_stats)
        raises(STATE, e.recorrect_anchors)
        e.consensus(3)
        raises(STATE, e.recorrected)                                   # the getters without a round
        raises(STATE, e.recorrect_jobs)
        raises(STATE, e.recorrect_ops)
        for bad in (dict(band0=300), dict(band0=128), dict(band0=1024, band_max=512), dict(band_max=1 << 19), dict(min_depth=0), dict(min_identity=1001)):
            raises(BAD, lambda: e.recorrect(**bad))
        with pytest.raises(TypeError):
            e.recorrect(band=512)
        small = _lib.RecorrectParams(C.sizeof(_lib.RecorrectParams) - 4, 512, 4096, 700, 3, 0)
        assert e.lib.bella_hip_recorrect(e.h, C.byref(small), None) == BAD
        raises(STATE, e.recorrect_stats)                               # (nothing of the refused calls stayed)
        assert e.lib.bella_hip_recorrect(e.h, None, None) == 0        # the defaults; total_bases may be NULL
        assert e.lib.bella_hip_get_recorrected(e.h, None, None, None) == 0
        first = e.recorrected()
        raises(BAD, lambda: e.recorrect(band0=300))                    # a failed round leaves the round before
        assert e.recorrect_stats()["round"] == 2 and e.recorrected()[1].tobytes() == first[1].tobytes()
        table = RC.mixed_table(seqs)
        for drop in (lambda: e.consensus(3), lambda: e.pileup_reset(), lambda: e.add_pileup(0, e.nreads, table), lambda: e.set_reads(synth.ReadSet.from_strings(seqs))):
            e.pileup_reset()
            e.add_pileup(0, e.nreads, table)
            c1 = e.consensus(3)
            r2 = e.recorrect(band0=256)
            assert e.recorrect_stats()["round"] == 2 and r2[1].tobytes() != c1[1].tobytes()
            got = np.zeros(len(c1[1]), np.uint8)
            e._chk(e.lib.bella_hip_get_consensus(e.h, None, got.ctypes.data, None))
            assert got.tobytes() == c1[1].tobytes()                    # bella_hip_get_consensus keeps returning round 1
            drop()
            raises(STATE, e.recorrect_stats)
            assert e.lib.bella_hip_get_recorrected(e.h, None, None, None) == STATE
    finally:
        e.close()


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return (files.get("out.out"), files.get("c.fasta")), files["stderr"]


def test_cli_correct_rounds_end_to_end(eng, tmp_path):
    """bella-hip --correct --correct-rounds 2 on toy120: the FASTA is the Python path's byte for byte; with --correct-rounds 1 and
    without the option the file and the log are the --correct run's; -m 1 and -g 2 give the same FASTA; the -o file is unchanged"""
    g = load_golden("toy120")
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    eng.trace_pairs(pars, pileup=True, keep_ops=False)
    eng.graph_reset()
    eng.graph_add_traced()
    want = {}
    offs, bases, _ = eng.consensus(3)
    api.write_fasta(str(tmp_path / "py1.fasta"), g.names, offs, bases)
    offs, bases, _ = eng.recorrect()
    st = eng.recorrect_stats()
    api.write_fasta(str(tmp_path / "py2.fasta"), g.names, offs, bases)
    want = [open(str(tmp_path / ("py%d.fasta" % k)), "rb").read() for k in (1, 2)]
    assert want[0] != want[1]
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx, "--correct", "c.fasta"]
    two = ["--correct-rounds", "2"]
    out0 = g.out["align"]
    timed = lambda ln: any(w in ln.split(b" = ")[0].lower() for w in (b"time", b"rate"))            # (the lines that carry a clock's reading)
    log = lambda err: [ln.split(b"\t", 2)[2] for ln in err.splitlines() if ln.startswith(b"INFO:") and not timed(ln.split(b"\t", 2)[2])]
    got, err0 = _run([fq], base, str(tmp_path / "cor"))
    assert got == (out0, want[0]) and b"Recorrected" not in err0
    got, err1 = _run([fq], base + ["--correct-rounds", "1"], str(tmp_path / "one"))
    assert got == (out0, want[0]) and log(err1) == log(err0)
    got, err = _run([fq], base + two, str(tmp_path / "two"))
    assert got == (out0, want[1])
    assert b"Recorrected = round 2: %d of %d alignments voted" % (st["voted"], st["jobs"]) in err and b"%d -> %d bases" % (st["bases_before"], st["bases_after"]) in err
    assert err.count(b"Recorrected") == 1 and _run([fq], base + ["--correct-rounds", "3"], str(tmp_path / "three"))[1].count(b"Recorrected") == 2
    assert _run([fq], base + two + ["-m", "1"], str(tmp_path / "m1"))[0] == (out0, want[1])
    assert _run([fq], base + two + ["-g", "2"], str(tmp_path / "g2"), {"BELLA_HIP_OVERSUBSCRIBE": "1"})[0] == (out0, want[1])


# ---- does it help? -----------------------------------------------------------------------------------------------------------------
def _dist(job):
    return P.edit_distance(job[0], job[1])


def test_a_second_round_improves_10kb_reads_at_15_percent_error(eng):
    """The set and pipeline of tests/test_pileup_gpu.py's last test (2,000 x 10 kb, seed 21, count_kmers(17, 2, 8), min_depth 3), with
    graph_add_traced after the trace.  A fixed-seed sample of 20 interior reads; a read is kept when at least half of it is covered, and
    at least half of the drawn reads must be kept.  Condition: the summed global edit distance to the templates after round 2 is BELOW
    round 1's, and round 1's is below the raw reads'.  Prints raw, round 1, round 2, the per-phase times and the job counts by status.
    Measured on an MI355X: 20 of 20 drawn reads kept; raw 27,643 (13.82 % of the template bases), round 1 7,540
    (3.77 %), round 2 906 (0.45 %); 57,011 records, 114,022 jobs, all voted at B = 512 in 10 batches; place 0.061 ms, dp 483.0 ms (the
    first trace's dp 135.7 ms), walk 315.6 ms, vote 15.2 ms, decide 0.71 ms."""
    nreads, read_len, seed, md = 2000, 10000, 21, 3
    rs = synth.make_reads(nreads, read_len=read_len, err=0.15, seed=seed)
    glen = max(read_len + 1, round(nreads * read_len / 30.0))
    genome = np.random.default_rng(seed).integers(0, 4, size=glen, dtype=np.uint8)
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
    nrec = eng.graph_add_traced()
    o1, b1, stats = eng.consensus(md)
    o2, b2, _ = eng.recorrect(min_depth=md)
    st = eng.recorrect_stats()
    seqs = rs.seqs()
    meta = [tuple(int(x) for x in n.split("_")[1:]) for n in rs.names]                   # (start, length, strand)
    interior = [r for r, (s, L, _) in enumerate(meta) if s >= read_len and s + L <= glen - read_len]
    drawn = sorted(np.random.default_rng(43).choice(interior, 20, replace=False).tolist())
    kept = [r for r in drawn if 2 * int(stats[r]["covered"]) >= int(stats[r]["len_before"])]
    assert 2 * len(kept) >= len(drawn), (len(kept), len(drawn))
    r1, r2 = b1.tobytes(), b2.tobytes()
    jobs = []
    for r in kept:
        s, L, strand = meta[r]
        t = synth.BASES[genome[s:s + L]].tobytes()
        if strand:
            t = T.revcomp(t)
        jobs += [(seqs[r], t), (r1[int(o1[r]):int(o1[r + 1])], t), (r2[int(o2[r]):int(o2[r + 1])], t)]
    # (forked workers inherit the parent's device file descriptors: 8 of them + the parent stay clear of a limit of 16 such processes)
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        d = pool.map(_dist, jobs, chunksize=1)
    d_raw, d_1, d_2 = sum(d[0::3]), sum(d[1::3]), sum(d[2::3])
    tlen = sum(len(j[1]) for j in jobs[0::3])
    print("RECORRECT 2000 x 10 kb, 15 %% error, min_depth %d: %d of %d drawn reads kept; edit distance to the template raw %d (%.2f %%), round 1 %d (%.2f %%), "
          "round 2 %d (%.2f %%); %d records, jobs %s; place %.3f ms, dp %.3f ms (the first trace's dp %.3f ms), walk %.3f ms, vote %.3f ms, decide %.3f ms, %d batches, "
          "%d dp cells, %d direction bytes at the peak, %d votes; %d -> %d bases"
          % (md, len(kept), len(drawn), d_raw, 100.0 * d_raw / tlen, d_1, 100.0 * d_1 / tlen, d_2, 100.0 * d_2 / tlen, nrec,
             {k: st[k] for k in ("jobs", "none", "band_capped", "low_identity", "voted")}, st["place_ms"], st["dp_ms"], trace_dp_ms, st["walk_ms"], st["vote_ms"],
             st["decide_ms"], st["batches"], st["dp_cells"], st["dir_bytes_peak"], st["votes"], st["bases_before"], st["bases_after"]))
    assert d_2 < d_1 < d_raw, (d_raw, d_1, d_2)
