"""GPU tests of the gap normalisation of the pileup votes: the table k_pile_vote_norm accumulates EQUALS the
numpy mirror (bella_testkit/normalize_mirror.py) applied to the device's own traces, on every golden set and on explicit pairs that put
a gap at an exact lane and chunk (bella_testkit/normalize_cases.py); bella-hip --normalize-gaps end to end; and what it buys."""
import gzip
import multiprocessing as mp
import os

import numpy as np
import pytest

from bella_amd import BellaPars, Engine, _lib, api
from bella_testkit import normalize_cases as NC
from bella_testkit import normalize_mirror as N
from bella_testkit import pileup_mirror as P
from bella_testkit import synth
from bella_testkit import trace_mirror as M
from bella_testkit import unitig_mirror as U
from bella_testkit.pipeline import aligned as _aligned, raises, run_cli
from conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu
BAD = -3
COUNTS = ("pairs", "runs", "gap_runs", "shifted_runs", "shifted_columns", "votes")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def test_table_equals_the_normalised_mirror_on_every_golden_set(eng, golden):
    """trace_pairs(pileup=True, normalize=True): the table is the normalised mirror's, from the device's own traces and runs, with the
    runs kept and without; records and runs are byte for byte the plain call's; vote_stats() are the mirror's counts; a plain call
    afterwards gives the plain mirror's table; on a set with more than 100 traced pairs the two tables differ; the consensus of the
    normalised table is the mirror's consensus of it."""
    g = golden
    pars, pairs, alns = _aligned(eng, g)
    eng.pileup_reset()
    tr, ops = eng.trace_pairs(pars, pileup=True, normalize=True, keep_ops=True)
    vs = eng.vote_stats()
    table = eng.get_pileup()
    want, st = N.pileup(g.seqs, pairs, alns, tr, ops)
    assert np.array_equal(table, want), (g.name, np.argwhere(table != want)[:5])
    assert {k: vs[k] for k in COUNTS} == st and vs["normalized"] == 1 and vs["vote_ms"] == eng.trace_stats().vote_ms
    assert st["votes"] == int(want.sum(dtype=np.int64)) == eng.trace_stats().votes
    off = np.concatenate([[0], np.cumsum([len(s) for s in g.seqs])]).astype(np.int64)
    offs, bases, stats = eng.consensus(3)
    raw = bases.tobytes()
    for r, s in enumerate(g.seqs):
        seq, cst = P.consensus(s, want[off[r]:off[r + 1]], 3)
        assert raw[int(offs[r]):int(offs[r + 1])] == seq and {f: int(stats[r][f]) for f in cst} == cst, (g.name, r)
    eng.pileup_reset()
    tr2, ops2 = eng.trace_pairs(pars, pileup=True, normalize=True, keep_ops=False)
    assert len(ops2) == 0 and tr2.tobytes() == tr.tobytes() and np.array_equal(eng.get_pileup(), want)
    assert {k: eng.vote_stats()[k] for k in COUNTS} == st
    # the plain call: same records and runs, the plain table, nothing counted as shifted
    eng.pileup_reset()
    tr0, ops0 = eng.trace_pairs(pars, pileup=True, keep_ops=True)
    assert tr0.tobytes() == tr.tobytes() and ops0.tobytes() == ops.tobytes()
    plain, _ = P.pileup(g.seqs, pairs, alns, tr0, ops0)
    assert np.array_equal(eng.get_pileup(), plain)
    vs0 = eng.vote_stats()
    assert vs0["normalized"] == 0 and vs0["shifted_runs"] == 0 and vs0["shifted_columns"] == 0 and vs0["gap_runs"] == 0
    assert vs0["pairs"] == st["pairs"] and vs0["runs"] == st["runs"] == len(ops) and vs0["votes"] == int(plain.sum(dtype=np.int64))
    if st["pairs"] > 100:
        assert not np.array_equal(plain, want) and st["shifted_runs"] > 0
    print("NORMALIZE %s: %s; plain votes %d; vote %.3f ms plain, %.3f ms normalised" % (g.name, st, vs0["votes"], vs0["vote_ms"], vs["vote_ms"]))


def test_flag_validation(eng):
    g = load_golden("sanity3")
    pars, _, _ = _aligned(eng, g)
    eng.pileup_reset()
    cp = pars.c()
    import ctypes as C
    call = lambda flags: eng.lib.bella_hip_trace_pairs_flags(eng.h, C.byref(cp), 0, flags, None, None)
    assert call(_lib.TRACE_NORMALIZE) == BAD and b"BELLA_TRACE_PILEUP" in eng.lib.bella_hip_last_error(eng.h)
    assert call(_lib.TRACE_NORMALIZE | _lib.TRACE_PASSED_ONLY) == BAD
    assert call(16) == BAD and call(16 | 15) == BAD
    assert call(_lib.TRACE_NORMALIZE | _lib.TRACE_PILEUP) == BAD          # (the pileup takes the passed pairs only, as before)
    assert int(eng.get_pileup().sum(dtype=np.int64)) == 0
    assert call(_lib.TRACE_NORMALIZE | _lib.TRACE_PILEUP | _lib.TRACE_PASSED_ONLY) == 0
    with pytest.raises(ValueError):
        eng.trace_pairs(pars, normalize=True)


# ---- explicit pairs ------------------------------------------------------------------------------------------------------------------
ROLES = [(0, True), (1, True), (0, False), (1, False)]      # (strand, cid < rid)


def _vote(eng, reads, pairs, ops, normalize):
    eng.set_reads(synth.ReadSet.from_strings(reads))
    eng.pileup_reset()
    eng.pileup_vote(pairs, ops, normalize=normalize)
    return eng.get_pileup(), eng.vote_stats()


@pytest.mark.parametrize("normalize", [False, True])
def test_explicit_pairs_at_every_place_the_kernel_can_go_wrong(eng, normalize):
    """every case of normalize_cases (each asserted to have the run index and shift it is meant to have), on both strands and in both
    role orders, in one batch: table == mirror, vote stats == the mirror's counts"""
    cases = NC.all_cases()
    for c in cases:
        NC.check_expect(c)
    assert [len(c["words"]) for c in cases[:7]] == [1, 63, 64, 65, 127, 128, 129]
    reads, pairs, ops = NC.build_batch([c for c in cases for _ in ROLES], ROLES)
    assert max(len(r) for r in reads) <= 320 and {(int(p["strand"]), int(p["rid"]) < int(p["cid"])) for p in pairs} == {(0, False), (0, True), (1, False), (1, True)}
    table, vs = _vote(eng, reads, pairs, ops, normalize)
    want, st = NC.mirror_table(reads, pairs, ops, normalize)
    assert np.array_equal(table, want), np.argwhere(table != want)[:8]
    assert {k: vs[k] for k in COUNTS} == st and vs["normalized"] == int(normalize)
    if normalize:
        plain, _ = NC.mirror_table(reads, pairs, ops, False)
        assert not np.array_equal(plain, want) and st["shifted_columns"] > 4 * (299 + 12)
        # the dropped junctions: plain loses an ins vote that the shift brings back inside the read
        assert int(want[:, P.INS:].sum()) > int(plain[:, P.INS:].sum())


@pytest.mark.parametrize("normalize", [False, True])
def test_explicit_empty_inputs(eng, normalize):
    c = NC.ends_case(np.random.default_rng(3))
    reads, pairs, ops = NC.build_batch([c, c], [(0, True), (1, False)])
    pairs["nops"][0] = 0                                      # a pair without runs votes nothing
    table, vs = _vote(eng, reads, pairs, ops, normalize)
    want, st = NC.mirror_table(reads, pairs, ops, normalize)
    assert np.array_equal(table, want) and vs["pairs"] == 1 == st["pairs"] and vs["votes"] == st["votes"] > 0
    eng.pileup_reset()
    eng.pileup_vote(pairs[:0], ops[:0], normalize=normalize)  # no pair at all
    vs = eng.vote_stats()
    assert int(eng.get_pileup().sum(dtype=np.int64)) == 0 and vs["pairs"] == 0 and vs["votes"] == 0 and vs["normalized"] == int(normalize)


def test_explicit_vote_validates_before_it_votes(eng):
    cases = [NC.between_x_case(np.random.default_rng(4)), NC.junction_v_case(np.random.default_rng(5))]
    reads, pairs, ops = NC.build_batch(cases, [(0, True), (1, True)])
    eng.set_reads(synth.ReadSet.from_strings(reads))
    eng.pileup_reset()
    eng.pileup_vote(pairs, ops, normalize=True)
    before = eng.get_pileup()
    assert before.sum() > 0

    def bad(field=None, value=None, pair=1, op_at=None, op_word=None, cut_ops=0):
        p, o = pairs.copy(), ops.copy()
        if field:
            p[field][pair] = value
        if op_at is not None:
            o[op_at] = op_word
        for nz in (False, True):
            raises(BAD, eng.pileup_vote, p, o[:len(o) - cut_ops], nz)
            assert np.array_equal(eng.get_pileup(), before)    # nothing was voted, not even the valid first pair
    bad("rid", len(reads))
    bad("cid", 2 ** 32 - 1)
    bad("strand", 2)
    bad("tbegV", -1)
    bad("tbegH", -1)
    bad("tbegV", 1)                                           # the runs now leave V
    bad("tbegH", 3)                                           # ... and H (two spare bases behind the alignment)
    bad("op_off", len(ops))                                   # op_off + nops outside ops
    bad("nops", int(pairs["nops"][1]) + 1)
    bad(cut_ops=1)
    last = len(ops) - 1
    bad(op_at=last, op_word=(1 << 4) | 4)                     # an op that is none of = X I D
    bad(op_at=last, op_word=(1 << 4) | 15)
    bad(op_at=last, op_word=0 | 3)                            # a run of length 0
    bad(op_at=int(pairs["op_off"][1]), op_word=(400 << 4) | 0)            # a run longer than the reads
    assert eng.lib.bella_hip_pileup_vote(eng.h, None, 1, None, 0, 0) == BAD
    assert eng.lib.bella_hip_pileup_vote(eng.h, pairs.ctypes.data, len(pairs), ops.ctypes.data, len(ops), 4) == BAD      # flags: 0 or 8
    assert np.array_equal(eng.get_pileup(), before)
    e2 = Engine(0)
    try:
        e2.set_reads(synth.ReadSet.from_strings(reads))
        raises(-7, e2.pileup_vote, pairs, ops)                # no table
    finally:
        e2.close()


# ---- command line --------------------------------------------------------------------------------------------------------------------
def _run(*args):
    files = run_cli(*args)
    return files["out.out"], files.get("c.fasta")


def test_cli_normalize_gaps_end_to_end(eng, tmp_path):
    """bella-hip --correct --normalize-gaps on toy120: the FASTA is the Python path's with normalize=True and differs from the one without
    the option; -m 1, -g 2 and both give the same files; the -o file is the golden one; --paf --cigar writes the PAF it writes without
    the option; the log sums the shifts"""
    g = load_golden("toy120")
    pars, pairs, alns = _aligned(eng, g)
    want = {}
    for nz in (False, True):
        eng.pileup_reset()
        eng.trace_pairs(pars, pileup=True, keep_ops=False, normalize=nz)
        vs = eng.vote_stats()
        offs, bases, _ = eng.consensus(3)
        f = str(tmp_path / ("py%d.fasta" % nz))
        api.write_fasta(f, g.names, offs, bases)
        want[nz] = open(f, "rb").read()
    assert want[True] != want[False] and vs["shifted_runs"] > 0
    fq = str(tmp_path / "reads.fastq")
    with gzip.open(os.path.join(GOLD, g.name, "reads.fastq.gz"), "rb") as src, open(fq, "wb") as dst:
        dst.write(src.read())
    mtx = str(tmp_path / "readbykmers.mtx")
    with open(mtx, "w") as f:
        f.write("%d\t%d\t%d\n" % (g.rs.nreads, g.nkmers, len(g.tk)))
        f.write("".join("%d\t%d\t%d\n" % (r + 1, k + 1, q) for k, r, q in zip(g.tk.tolist(), g.tr.tolist(), g.tp.tolist())))
    base = g.meta["flags"] + ["--tuples", mtx]
    over = {"BELLA_HIP_OVERSUBSCRIBE": "1"}
    cor = ["--correct", "c.fasta"]
    nrm = cor + ["--normalize-gaps"]
    out0 = g.out["align"]
    files = run_cli([fq], base + nrm, str(tmp_path / "nrm"))
    assert (files["out.out"], files["c.fasta"]) == (out0, want[True])
    assert b"NormalizedGaps = %d shifted_runs, %d shifted_columns" % (vs["shifted_runs"], vs["shifted_columns"]) in files["stderr"]
    files = run_cli([fq], base + cor, str(tmp_path / "cor"))
    assert (files["out.out"], files["c.fasta"]) == (out0, want[False]) and b"NormalizedGaps" not in files["stderr"]
    assert _run([fq], base + nrm + ["-m", "1"], str(tmp_path / "m1")) == (out0, want[True])
    files = run_cli([fq], base + nrm + ["-g", "2"], str(tmp_path / "g2"), over)
    assert (files["out.out"], files["c.fasta"]) == (out0, want[True])
    assert b"NormalizedGaps = %d shifted_runs, %d shifted_columns" % (vs["shifted_runs"], vs["shifted_columns"]) in files["stderr"]
    assert _run([fq], base + nrm + ["-m", "1", "-g", "2"], str(tmp_path / "m1g2"), over) == (out0, want[True])
    cg, _ = _run([fq], base + ["--paf", "--cigar"] + cor, str(tmp_path / "cigar"))
    assert _run([fq], base + ["--paf", "--cigar"] + nrm, str(tmp_path / "cigarnrm")) == (cg, want[True])


def test_cli_polish_with_normalize_gaps_agrees_with_the_python_path(eng, tmp_path):
    """120 synthetic reads of 3 kb at 15 % error: bella-hip --unitigs-fasta --polish --normalize-gaps writes the FASTA of the Python path
    (trace with normalize=True -> records -> build -> clean -> unitigs -> polish)"""
    rs = synth.make_reads(120, read_len=3000, err=0.15, seed=17)
    fq = str(tmp_path / "s.fastq")
    synth.write_fastq(fq, rs)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    assert eng.align_pairs(pars) > 100
    want = {}
    for nz in (False, True):
        eng.pileup_reset()
        eng.trace_pairs(pars, pileup=True, keep_ops=False, normalize=nz)
        eng.graph_reset()
        eng.graph_add_traced()
        eng.graph_build()
        eng.graph_clean()
        u = eng.graph_unitigs()
        p = eng.graph_polish_unitigs(3)
        want[nz] = U.fasta_text(u, p["offsets"], p["bases"].tobytes())
    assert len(u["len"]) >= 1 and want[True] != want[False]
    files = run_cli([fq], ["--unitigs-fasta", "u.fa", "--polish", "--normalize-gaps"], str(tmp_path / "pol"))
    assert files["u.fa"] == want[True] and b"NormalizedGaps = " in files["stderr"]


# ---- does it help? -------------------------------------------------------------------------------------------------------------------
def _dist(job):
    return P.edit_distance(job[0], job[1])


def test_normalised_consensus_is_closer_to_the_templates(eng):
    """300 synthetic reads of 3 kb at 15 % error, 30x; the pipeline's own pairs; a fixed-seed sample of 20 interior reads; edit distance to
    the templates raw, corrected plain, corrected with normalize=True (min_depth 3).  Condition: normalised < plain < raw.  The ratios
    and the same sample after one recorrect round from either start are printed, not asserted (the line for DESIGN.md section 21).
    Measured on an MI355X: raw 8,446 (14.08 % of the 60,000 template bases), plain 2,231 (3.72 %), normalised 899 (1.50 %), normalised /
    plain 0.403; after one recorrect round 241 from the plain start, 211 from the normalised one."""
    nreads, read_len, seed, md = 300, 3000, 23, 3
    rs = synth.make_reads(nreads, read_len=read_len, err=0.15, seed=seed)
    G = max(read_len + 1, round(nreads * read_len / 30.0))
    genome = np.random.default_rng(seed).integers(0, 4, size=G, dtype=np.uint8)
    eng.set_reads(rs)
    eng.count_kmers(17, 2, 8)
    eng.assemble_counted()
    pars = BellaPars()
    eng.overlap(pars)
    assert eng.align_pairs(pars) > 300
    seqs = rs.seqs()
    meta = [tuple(int(x) for x in n.split("_")[1:]) for n in rs.names]                   # (start, length, strand)
    interior = [r for r, (s, L, _) in enumerate(meta) if s >= read_len and s + L <= G - read_len]
    drawn = sorted(np.random.default_rng(33).choice(interior, 20, replace=False).tolist())
    tmpl = {}
    for r in drawn:
        s, L, strand = meta[r]
        t = synth.BASES[genome[s:s + L]].tobytes()
        tmpl[r] = M.revcomp(t) if strand else t
    jobs = [(seqs[r], tmpl[r]) for r in drawn]
    stats = {}
    for nz in (False, True):
        eng.pileup_reset()
        eng.trace_pairs(pars, pileup=True, keep_ops=False, normalize=nz)
        stats[nz] = eng.vote_stats()
        offs, bases, _ = eng.consensus(md)
        raw = bases.tobytes()
        jobs += [(raw[int(offs[r]):int(offs[r + 1])], tmpl[r]) for r in drawn]
        eng.graph_reset()
        eng.graph_add_traced()
        offs, bases, _ = eng.recorrect(min_depth=md)
        raw = bases.tobytes()
        jobs += [(raw[int(offs[r]):int(offs[r + 1])], tmpl[r]) for r in drawn]
    # (forked workers inherit the parent's device file descriptors: 8 of them + the parent stay clear of a limit of 16 such processes)
    with mp.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        d = pool.map(_dist, jobs, chunksize=1)
    d_raw, d_plain, d_plain2, d_norm, d_norm2 = (sum(d[20 * k:20 * k + 20]) for k in range(5))
    tlen = sum(len(t) for t in tmpl.values())
    print("NORMALIZE 300 x 3 kb, 15 %% error, min_depth %d, 20 interior reads, %d template bases: edit distance raw %d (%.2f %%), plain %d (%.2f %%), normalised %d (%.2f %%), "
          "normalised / plain %.3f; after one recorrect round: from plain %d, from normalised %d; shifted_runs %d of 2 x %d gap runs, shifted_columns %d; vote %.3f ms plain, %.3f ms normalised"
          % (md, tlen, d_raw, 100.0 * d_raw / tlen, d_plain, 100.0 * d_plain / tlen, d_norm, 100.0 * d_norm / tlen, d_norm / max(d_plain, 1), d_plain2, d_norm2,
             stats[True]["shifted_runs"], stats[True]["gap_runs"], stats[True]["shifted_columns"], stats[False]["vote_ms"], stats[True]["vote_ms"]))
    assert d_norm < d_plain < d_raw, (d_norm, d_plain, d_raw)
